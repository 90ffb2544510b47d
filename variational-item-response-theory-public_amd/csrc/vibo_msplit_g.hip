// matrix row-split ELBO kernel, fp32 rows gathered through row_index (see vibo_msplit_kernel.hpp)
#include "vibo_msplit_kernel.hpp"
#include "vibo_launch.hpp"
namespace vibo {
hipError_t launch_elbo_msplit_g(const ElboParams& p, const SplitVariant& v, int grid, hipStream_t s) {
    return launch_msplit_rm<kRowsGathered, false>(p, v, grid, s);
}
}  // namespace vibo
