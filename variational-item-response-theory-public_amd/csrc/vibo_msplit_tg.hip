// matrix row-split ELBO kernel on a matrix' prepacked tile image under a caller-supplied posterior (VIBO_MASK_TILES with
// VIBO_POSTERIOR_GIVEN, include/vibo_hip_given_tiles.h; see vibo_msplit_kernel.hpp, row mode 4, hook mode 2): twelve instantiations
// (no flows; IRT 1/2/3 x GRAD x NW8), all on the two-barrier batch loop
#include "vibo_msplit_kernel.hpp"
#include "vibo_launch.hpp"
namespace vibo {
hipError_t launch_elbo_msplit_tg(const ElboParams& p, const SplitVariant& v, int grid, hipStream_t s) {
    return launch_msplit_xm<kRowsTiles, false, kHooksGiven>(p, v, grid, s);
}
}  // namespace vibo
