// matrix row-split ELBO kernel with planar flows, fp32 rows gathered through row_index (see vibo_msplit_kernel.hpp)
#include "vibo_msplit_kernel.hpp"
#include "vibo_launch.hpp"
namespace vibo {
hipError_t launch_elbo_msplit_fg(const ElboParams& p, const SplitVariant& v, int grid, hipStream_t s) {
    return launch_msplit_rm<kRowsGathered, true>(p, v, grid, s);
}
}  // namespace vibo
