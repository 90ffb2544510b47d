// matrix row-split ELBO kernel, 1-byte cell codes (VIBO_MASK_CODES) (see vibo_msplit_kernel.hpp)
#include "vibo_msplit_kernel.hpp"
#include "vibo_launch.hpp"
namespace vibo {
hipError_t launch_elbo_msplit_c(const ElboParams& p, const SplitVariant& v, int grid, hipStream_t s) {
    return launch_msplit_rm<kRowsCodes, false>(p, v, grid, s);
}
}  // namespace vibo
#ifdef VIBO_MS_TIMING
extern "C" int vibo_debug_ms_timing_c(long long* host_out, int n) {
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_ms_timing), (size_t)n * sizeof(long long));
}
#endif
