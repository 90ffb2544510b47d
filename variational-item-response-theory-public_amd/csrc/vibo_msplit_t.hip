// matrix row-split ELBO kernel on a matrix' prepacked tile image (VIBO_MASK_TILES, include/vibo_hip_tile_rows.h; see
// vibo_msplit_kernel.hpp, row mode 4): the plain model's twelve instantiations (XM 0, no flows; IRT 1/2/3 x GRAD x NW8)
#include "vibo_msplit_kernel.hpp"
#include "vibo_launch.hpp"
namespace vibo {
hipError_t launch_elbo_msplit_t(const ElboParams& p, const SplitVariant& v, int grid, hipStream_t s) {
    return launch_msplit_xm<kRowsTiles, false, kHooksNone>(p, v, grid, s);
}
}  // namespace vibo
#ifdef VIBO_MS_TIMING
extern "C" int vibo_debug_ms_timing_t(long long* host_out, int n) {
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_ms_timing), (size_t)n * sizeof(long long));
}
#endif
