// vibo_launch.hpp -- per-ability-width launchers of the fused ELBO kernel.
// One translation unit per template ability width keeps hipcc compile times
// parallel (see Makefile); vibo_capi.hip dispatches to these (launch_split / run_single).
#pragma once
#include <hip/hip_runtime.h>
#include "vibo_params.hpp"
#include "vibo_variant.hpp"

namespace vibo {

// waves per workgroup: 2 (I <= 144), 4 (I <= 304), 8 (I <= 512), 16 (I <= 1024)
struct LaunchGeom {
    int waves, grid;
    size_t lds_bytes;
};

hipError_t launch_elbo_a1(const ElboParams& p, int irt, bool grad, const LaunchGeom& g, hipStream_t s);
hipError_t launch_elbo_a2(const ElboParams& p, int irt, bool grad, const LaunchGeom& g, hipStream_t s);
hipError_t launch_elbo_a4(const ElboParams& p, int irt, bool grad, const LaunchGeom& g, hipStream_t s);
hipError_t launch_elbo_a8(const ElboParams& p, int irt, bool grad, const LaunchGeom& g, hipStream_t s);

// wave-per-row kernel (vibo_row_kernel.hip): A in {1,2}, 1PL/2PL, I <= 1024, 16-byte aligned rows
hipError_t launch_elbo_rows(const ElboParams& p, int irt, bool grad, int grid, hipStream_t s);

// The row-split launchers, one per translation unit (parallel compiles, per-unit -mllvm options in the Makefile), ONE signature: the
// variant (split_variant in vibo_planner.hip) says which instantiation runs; launch_split in vibo_capi.hip picks the unit from it.
//   split_<r><at>: VALU kernel (vibo_split_kernel.hpp), template ability width 2 / 4 / 8; 1PL/2PL/3PL, optional planar flows
//   msplit_<r>, msplit_f<r>, msplit_x<r>: matrix kernel (vibo_msplit_kernel.hpp) plain / with flows / with the conditional posterior's
//       first pass folded in (hook mode 3); at most 1024 items per launch.  narrow: vibo_narrow.hip, 4..128 items, ability_dim <= 4
//   <r> = rows: a fp32 in order, g fp32 through row_index, c 1-byte cell codes, s fp32 in order with the sign bit as the mask,
//       t the matrix' prepacked tile image (msplit_tg: the same under a caller-supplied posterior, hook mode 2)
using SplitLauncher = hipError_t(const ElboParams& p, const SplitVariant& v, int grid, hipStream_t s);
SplitLauncher launch_elbo_split_a2, launch_elbo_split_a4, launch_elbo_split_a8, launch_elbo_split_g2, launch_elbo_split_g4,
    launch_elbo_split_g8, launch_elbo_split_c2, launch_elbo_split_c4, launch_elbo_split_c8, launch_elbo_msplit_a, launch_elbo_msplit_g,
    launch_elbo_msplit_c, launch_elbo_msplit_s, launch_elbo_msplit_t, launch_elbo_msplit_fa, launch_elbo_msplit_fg, launch_elbo_msplit_fc,
    launch_elbo_msplit_xa, launch_elbo_msplit_xg, launch_elbo_msplit_tg, launch_elbo_narrow;

// narrow-row kernel: waves per SIMD each instantiation is compiled for (registers: items x (parameters + gradient accumulators) + one
// unit of rows; 3PL with gradients at 8 items per lane: 128 registers were 4-12 short -- spilled, and a spill reload waits behind the
// row loads).  ONE definition for the kernel's launch bounds (vibo_narrow.hip) and the planner's grid (vibo_planner.hip: workgroups per
// CU = waves per SIMD): the grid has to match the occupancy the kernel was compiled for.
constexpr int narrow_waves_per_simd(int at, int il, bool g3 = false) {
    return at == 1 ? ((g3 && il == 8) ? 3 : 4) : at == 2 ? (il == 4 ? 4 : 3) : (il == 4 ? 3 : 2);
}

// the folded train step's epilogue (vibo_trainer.hip): finalize + loss + MLP / item backward + Adam + the next step's noise
hipError_t launch_train_epilogue_fused(const EpiParams& e, hipStream_t s);
int train_epilogue_item_blocks(int n_item_entries);

}  // namespace vibo
