// vibo_planner.hpp -- descriptor checks and the launch plan of an ELBO call (vibo_planner.hip).  Host-only code: it reads the
// descriptor and the number of compute units, launches nothing and keeps no state but the calling thread's last error string.
// The facts it shares with the dispatch -- the panel split, 256-byte rounding, the error string -- are in vibo_host.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/vibo_hip.h"
#include "vibo_host.hpp"
#include "vibo_launch.hpp"
#include "vibo_params.hpp"

namespace vibo {

// sign_rows: the entry point takes VIBO_MASK_SIGN rows (include/vibo_hip_sign_rows.h) and VIBO_MASK_TILES images
// (include/vibo_hip_tile_rows.h) where sign_rows_ok says so; every other one
// refuses them here (-8).  given_tiles: the entry point takes VIBO_MASK_TILES images under VIBO_POSTERIOR_GIVEN
// (include/vibo_hip_given_tiles.h) where given_tile_rows_ok says so, and no other VIBO_MASK_TILES descriptor
int check_desc(const vibo_desc* d, bool sign_rows = false, bool given_tiles = false);
// VIBO_MASK_TILES under VIBO_POSTERIOR_GIVEN: no flows, 4..1024 items (one panel, FirstPass::GivenDirect), the matrix kernel as the engine
bool given_tile_rows_ok(const vibo_desc* d);
// VIBO_MASK_SIGN: the shapes the format is implemented for -- what the planner sends to the single-launch matrix row-split kernel
// (unconditional posterior, no flows, 4..1024 items, chunkable rows)
bool sign_rows_ok(const vibo_desc* d);
int codes_unsupported();
// the pointer checks the entry points that read person rows share (after check_desc)
int require_rows(const vibo_desc* d, const float* response, const void* mask);

// min(num_cu * per_cu, ceil(persons / rows_per_wg)): a grid that fills the chip but gives every workgroup at least one batch of rows
inline int clamp_grid(int num_cu, int per_cu, int persons, int rows_per_wg) {
    const int n = num_cu * per_cu, cap = (persons + rows_per_wg - 1) / rows_per_wg;
    return n > cap ? cap : n;
}
bool rows_chunkable(const vibo_desc* d);
// rows can be read in aligned chunks of 4 cells (16 B of responses + 4 B of mask, or 4 B of cell codes)
bool rows_vec_ok(const vibo_desc* d, const float* response, const void* mask);

// What a call runs.  make_plan decides it once from the descriptor; resolve_path applies the one thing only the launch knows (whether
// the caller's rows are aligned for 16-byte loads).  Everything else -- vibo_plan_kernel, the folded step's queries, the multi-sample
// plan, the refusals and the dispatch of vibo_elbo_fwd_bwd -- reads these.
enum class Path {
    General,      // wave-per-person kernel (ability_dim 9..16; conditional posterior / flows / > 1024 items on rows no row-split kernel takes)
    Panels,       // a first pass, one row-split launch per panel of kPanelItems items, a gradient tail
    Split,        // one row-split launch (4..1024 items, unconditional posterior)
    Row,          // wave-per-row register kernel (int64 masks)
    Tiled         // tiled kernel
};
// (Engine -- which row-split kernel a Panels / Split call runs; Plan::split_nblk is the narrow-row kernel's grid too: vibo_variant.hpp)
enum class FirstPass {   // Panels: what supplies the whole-row statistics
    None,
    RowCount,     // unconditional posterior: packed counts of the whole row
    CondValu,     // conditional posterior: cond_pre_kernel per panel (vibo_cond.hip)
    CondMatrix,   // ... on the matrix pipe from the cell codes, all items at once (vibo_cmean.hip)
    CondFused,    // ... folded into the matrix row-split kernel (one panel, ability_dim 1, fp32 rows: its XM == 3)
    GivenDirect,  // VIBO_POSTERIOR_GIVEN, one panel: the kernel's slot lanes read / write the posterior themselves
    GivenPre      // VIBO_POSTERIOR_GIVEN, more panels: given_pre_kernel / given_post_kernel
};
enum class Tail {        // Panels with want_grad: what turns the per-person coefficients into the table gradient
    None,
    CondValu,     // cond_post_kernel per panel + cond_finalize
    CondMatrix,   // vibo_cmean.hip, all items at once
    Given         // given_post_kernel
};

struct Plan {
    Path path;
    Engine engine;
    FirstPass first;
    Tail tail;
    int row_nblk;             // Row: grid
    int split_nq, split_nblk; // Panels / Split: waves per workgroup (VALU kernel), grid (per panel)
    int cond_nblk;            // workgroups of the conditional posterior's cond_pre launches (2 per CU)
    int cond_post_nblk;       // ... of cond_post: 3 per CU when it reads cell codes at template width <= 2 (its launch bound there)
    int panels;               // Panels: panel_count(num_item)
    int cond_rec;             // floats per cond_post workgroup record
    int AT, D, DP, n_tiles, nblk, lds_stride, lds_main;
    LaunchGeom geom;          // Tiled (and the fallback of Split / Row for unaligned rows)
    PartialLayout lay;
    // workspace layout (bytes from its start); the prepped item rows are at 0
    size_t off_cnt;           // Panels: per-person packed counts of the whole row
    size_t off_partial;       // the ELBO kernel's partial records
    size_t off_pre, off_coef; // Panels: per-person statistics in / backward coefficients out
    size_t off_cpart;         // ... scratch of the matrix-pipe passes (images + records)
    size_t off_crec;          // ... the VALU post pass's records (behind that scratch, if any)
    size_t off_codes;         // fp32 rows read by more than one pass: the first pass's 1-byte cell codes [B][codes_stride] (0: not used)
    long long codes_stride;
    size_t total_bytes;

    bool row_split() const { return path == Path::Panels || path == Path::Split; }
    bool conditional() const { return first == FirstPass::CondValu || first == FirstPass::CondMatrix || first == FirstPass::CondFused; }
    bool given() const { return first == FirstPass::GivenDirect || first == FirstPass::GivenPre; }
};

// < 0: the descriptor has no plan (error string set).  allow_msplit = false: the VALU row-split kernel whatever the thresholds say
// (the multi-sample forward)
int make_plan(const vibo_desc* d, int num_cu, Plan* pl, bool allow_msplit = true);
// the path the launch takes: pl.path when the rows are aligned (vec), else its fallback
Path resolve_path(const Plan& pl, const vibo_desc* d, bool vec);
int plan_kernel_code(const Plan& pl);        // VIBO_KERNEL_* of resolve_path(vec = true)
int plan_cond_pass_bits(const Plan& pl);     // vibo_plan_cond_passes
// Which instantiation a row-split launch of this plan runs, every field derived once: from the descriptor and the plan, and from `p` what
// only the launch knows (its items, rows gathered / become cell codes).  false: there is none, or p's hook fields contradict the one named.
bool split_variant(const vibo_desc* d, const Plan& pl, const ElboParams& p, SplitVariant* v);
// The folded train step (vibo_elbo_fwd_bwd_step + vibo_train_epilogue_fused) covers single-launch row-split calls of the plain model.
// ok: the descriptor can take it (vibo_train_step_supported bit 0); fused_finalize: vibo_train_epilogue_fused sums in the stand-alone finalize's
// order (bit 1); draws_noise: the step's kernel may draw its ability noise and skip the posterior's mean / log-variance; sample_optional: and the sample
struct StepContract { bool ok, fused_finalize, draws_noise, sample_optional; };
StepContract step_contract(const vibo_desc* d, const Plan& pl, bool rows_gathered);
// plan of a multi-sample forward: the single-launch plan with want_grad = 0, restricted to the row-split paths.
// given_call: vibo_elbo_multi_forward_given (VIBO_POSTERIOR_GIVEN descriptors only; the plain call refuses those)
int multi_plan(const vibo_desc* d, int num_cu, vibo_desc* d0, Plan* pl, size_t* prep_bytes, bool given_call = false);

// bytes of `panels` blocks of per-person row statistics (2A sums + the observed count): the conditional posterior's `pre` block of an
// ELBO plan, and the head of the encode path's scratch (the matrix-pipe pass's own scratch lies right behind it)
inline size_t pre_block_bytes(int panels, long long persons, int A) { return up256((size_t)panels * persons * (2 * A + 1) * 4); }
bool encode_on_matrix_pipe(const vibo_desc* d);
// scratch the fast encode path needs (0: not applicable -> wave-per-person encode_kernel)
size_t encode_scratch_bytes(const vibo_desc* d);

}  // namespace vibo
