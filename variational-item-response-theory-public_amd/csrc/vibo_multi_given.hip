// multi-sample forward kernel, caller-supplied posterior (VIBO_POSTERIOR_GIVEN): its instantiations, in a unit of their own so
// that the build does not serialise on vibo_multi.o (see vibo_multi_kernel.hpp)
#include "vibo_multi_kernel.hpp"
#include "vibo_multi.hpp"
namespace vibo {
hipError_t launch_elbo_multi_given(const MultiParams& mp, int at, int irt, int sc, int nq, int grid, hipStream_t s) {
    if (at <= 2) return launch_multi_at<2, true>(mp, irt, sc, nq, grid, s);
    if (at == 4) return launch_multi_at<4, true>(mp, irt, sc, nq, grid, s);
    return launch_multi_at<8, true>(mp, irt, sc, nq, grid, s);
}
}  // namespace vibo
