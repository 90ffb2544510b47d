// matrix row-split ELBO kernel, fp32 rows in order whose sign bit is the mask (VIBO_MASK_SIGN; see vibo_msplit_kernel.hpp, row
// mode 3): the plain model's twelve instantiations (XM 0, no flows; IRT 1/2/3 x GRAD x NW8)
#include "vibo_msplit_kernel.hpp"
#include "vibo_launch.hpp"
namespace vibo {
hipError_t launch_elbo_msplit_s(const ElboParams& p, int irt, bool grad, int nw, int grid, hipStream_t s) {
    // (the caller has refused everything else with -8: vibo_capi.hip sends single-launch calls of the plain model only)
    if (p.cond_table || p.given_post || p.given_grad || p.row_cnt || p.pre_stats || p.post_coef || p.n_flows != 0 || p.row_index || p.mask ||
        !p.response) return hipErrorInvalidValue;
#define VIBO_MSS(IRT_, GRAD_) (nw == 8 ? launch_msplit_inst<IRT_, GRAD_, 3, false, true, 0>(p, nw, grid, s) : launch_msplit_inst<IRT_, GRAD_, 3, false, false, 0>(p, nw, grid, s))
    if (irt == 1) return grad ? VIBO_MSS(1, true) : VIBO_MSS(1, false);
    if (irt == 2) return grad ? VIBO_MSS(2, true) : VIBO_MSS(2, false);
    return grad ? VIBO_MSS(3, true) : VIBO_MSS(3, false);
#undef VIBO_MSS
}
}  // namespace vibo
