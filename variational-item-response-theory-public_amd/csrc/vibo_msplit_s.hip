// matrix row-split ELBO kernel, fp32 rows in order whose sign bit is the mask (VIBO_MASK_SIGN; see vibo_msplit_kernel.hpp, row
// mode 3): the plain model's twelve instantiations (XM 0, no flows; IRT 1/2/3 x GRAD x NW8)
#include "vibo_msplit_kernel.hpp"
#include "vibo_launch.hpp"
namespace vibo {
hipError_t launch_elbo_msplit_s(const ElboParams& p, const SplitVariant& v, int grid, hipStream_t s) {
    return launch_msplit_xm<kRowsSign, false, kHooksNone>(p, v, grid, s);
}
}  // namespace vibo
