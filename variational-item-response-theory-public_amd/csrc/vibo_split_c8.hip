// row-split ELBO kernel reading 1-byte cell codes (VIBO_MASK_CODES), template ability width 8
#include "vibo_split_kernel.hpp"
#include "vibo_launch.hpp"
namespace vibo {
hipError_t launch_elbo_split_c8(const ElboParams& p, const SplitVariant& v, int grid, hipStream_t s) {
    return launch_split_at<8, kRowsCodes>(p, v, grid, s);
}
}  // namespace vibo
