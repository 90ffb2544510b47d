// vibo_planner.hip -- which kernels an ELBO call runs, on how many workgroups, and where its workspace blocks lie (vibo_planner.hpp).
// make_plan works in stages: path (shape eligibility) -> engine (the measured thresholds) -> grids -> workspace layout.
#include "vibo_planner.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../../include/vibo_hip_sign_rows.h"
#include "../../include/vibo_hip_tile_rows.h"
#include "vibo_cond.hpp"

namespace vibo {

static thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
const char* last_error() { return g_err; }

int check_desc(const vibo_desc* d, bool sign_rows, bool given_tiles) {
    if (!d) return fail(-1, "null descriptor");
    if (d->abi_version != VIBO_ABI_VERSION) return fail(-2, "abi_version %d != %d", d->abi_version, VIBO_ABI_VERSION);
    if (d->num_person < 1) return fail(-3, "num_person must be >= 1");
    if (d->num_item < 1) return fail(-3, "num_item must be >= 1");
    if (d->ability_dim < 1 || d->ability_dim > VIBO_MAX_ABILITY_DIM_WIDE)
        return fail(-3, "ability_dim %d outside 1..%d", d->ability_dim, VIBO_MAX_ABILITY_DIM_WIDE);
    if (d->ability_dim > VIBO_MAX_ABILITY_DIM && d->posterior == VIBO_POSTERIOR_GIVEN)
        return fail(-8, "VIBO_POSTERIOR_GIVEN needs the row-split path: ability_dim <= %d", VIBO_MAX_ABILITY_DIM);
    if (d->ability_dim > VIBO_MAX_ABILITY_DIM && (d->mask_dtype == VIBO_MASK_CODES))
        return fail(-8, "cell codes (VIBO_MASK_CODES) need the row-split paths: ability_dim <= %d", VIBO_MAX_ABILITY_DIM);
    if (d->irt_model < 1 || d->irt_model > 3) return fail(-3, "irt_model must be 1, 2 or 3");
    if (d->posterior != VIBO_POSTERIOR_UNCONDITIONAL && d->posterior != VIBO_POSTERIOR_CONDITIONAL &&
        d->posterior != VIBO_POSTERIOR_GIVEN)
        return fail(-3, "bad posterior");
    if (d->missing_mode != VIBO_MISSING_PRIOR && d->missing_mode != VIBO_MISSING_DROP) return fail(-3, "bad missing_mode");
    if (d->mask_dtype < 0 || d->mask_dtype > VIBO_MASK_TILES || d->mask_dtype == 5) return fail(-3, "bad mask_dtype");
    if (d->mask_dtype == VIBO_MASK_SIGN && !sign_rows)
        return fail(-8, "VIBO_MASK_SIGN rows (the response's sign bit is the mask): taken by vibo_elbo_fwd_bwd and its _step forms only");
    if (d->mask_dtype == VIBO_MASK_TILES && !sign_rows && !given_tiles)
        return fail(-8, "VIBO_MASK_TILES rows (the matrix' prepacked tile image): taken by vibo_elbo_fwd_bwd and its _step forms only");
    if (d->reg_mode != VIBO_REG_KL && d->reg_mode != VIBO_REG_SAMPLED) return fail(-3, "bad reg_mode");
    if (d->n_flows < 0 || d->n_flows > VIBO_MAX_FLOWS) return fail(-3, "n_flows outside 0..%d", VIBO_MAX_FLOWS);
    if (d->n_flows > 0 && d->reg_mode != VIBO_REG_SAMPLED) return fail(-3, "flows need reg_mode SAMPLED");
    if (d->flags & ~(VIBO_FLAG_KERNEL_VALU | VIBO_FLAG_KERNEL_MATRIX | VIBO_FLAG_NO_EMIT_CODES | VIBO_FLAG_COND_VALU | VIBO_FLAG_COND_MATRIX |
                     VIBO_FLAG_COND_THREE_PASS)) return fail(-3, "unknown flags");
    if ((d->flags & VIBO_FLAG_KERNEL_VALU) && (d->flags & VIBO_FLAG_KERNEL_MATRIX)) return fail(-3, "flags pin two kernels");
    if ((d->flags & VIBO_FLAG_COND_VALU) && (d->flags & VIBO_FLAG_COND_MATRIX)) return fail(-3, "flags pin two forms of the conditional passes");
    if (d->mask_dtype == VIBO_MASK_SIGN && !sign_rows_ok(d))
        return fail(-8, "VIBO_MASK_SIGN rows (the response's sign bit is the mask): only calls the planner sends to the single-launch "
                        "matrix row-split kernel (unconditional posterior, no flows, 4..1024 items, chunkable rows, enough persons or "
                        "VIBO_FLAG_KERNEL_MATRIX)");
    if (d->mask_dtype == VIBO_MASK_TILES && given_tiles) {      // (vibo_elbo_fwd_bwd_given_tiles: this combination and no other)
        if (!given_tile_rows_ok(d))
            return fail(-8, "VIBO_MASK_TILES rows under VIBO_POSTERIOR_GIVEN: only calls the planner sends to the matrix row-split kernel "
                            "in one panel (no flows, 4..1024 items, enough persons or VIBO_FLAG_KERNEL_MATRIX)");
        return 0;
    }
    if (d->mask_dtype == VIBO_MASK_TILES && !sign_rows_ok(d))
        return fail(-8, "VIBO_MASK_TILES rows (the matrix' prepacked tile image): only calls the planner sends to the single-launch "
                        "matrix row-split kernel (unconditional posterior, no flows, 4..1024 items, enough persons or "
                        "VIBO_FLAG_KERNEL_MATRIX)");
    return 0;
}

bool sign_rows_ok(const vibo_desc* d) {
    if (d->posterior != VIBO_POSTERIOR_UNCONDITIONAL || d->n_flows != 0) return false;
    Plan pl;
    // (path and engine do not depend on the compute-unit count)
    return make_plan(d, 256, &pl) == 0 && pl.path == Path::Split && pl.engine == Engine::Matrix;
}

bool given_tile_rows_ok(const vibo_desc* d) {
    if (d->mask_dtype != VIBO_MASK_TILES || d->posterior != VIBO_POSTERIOR_GIVEN || d->n_flows != 0 || d->num_item < 4 || d->num_item > kPanelItems)
        return false;
    Plan pl;
    return make_plan(d, 256, &pl) == 0 && pl.path == Path::Panels && pl.first == FirstPass::GivenDirect && pl.engine == Engine::Matrix;
}

int codes_unsupported() {
    return fail(-8, "cell codes (VIBO_MASK_CODES) need the row-split paths: 4..32767 items, rows 4-byte aligned with a "
                    "stride that pads them to a multiple of 4 cells");
}

int require_rows(const vibo_desc* d, const float* response, const void* mask) {
    if (!response && d->mask_dtype != VIBO_MASK_CODES) return fail(-5, "null required pointer");
    const bool no_mask = d->mask_dtype == VIBO_MASK_NONE || d->mask_dtype == VIBO_MASK_SIGN || d->mask_dtype == VIBO_MASK_TILES;
    if (no_mask != (mask == nullptr)) return fail(-5, "mask pointer / mask_dtype mismatch");
    return 0;
}

// ---------------------------------------------------------------------------
// stage 1: shape eligibility -> Path
// ---------------------------------------------------------------------------
// 16-byte row chunks need I % 4 == 0, or row strides that pad every row to a multiple of 4 cells (the cells past
// the row's end are read but masked out in the kernels)
bool rows_chunkable(const vibo_desc* d) {
    const int I = d->num_item;
    if (I % 4 == 0 || d->mask_dtype == VIBO_MASK_TILES) return true;      // (a tile image has no rows: its strides are not read)
    const long long i4 = (I + 3) & ~3;
    if (d->mask_dtype != VIBO_MASK_CODES && d->response_row_stride < i4) return false;
    if ((d->mask_dtype == VIBO_MASK_U8 || d->mask_dtype == VIBO_MASK_CODES) && d->mask_row_stride < i4) return false;
    return true;
}

bool rows_vec_ok(const vibo_desc* d, const float* response, const void* mask) {
    bool vec = rows_chunkable(d);
    if (d->mask_dtype == VIBO_MASK_TILES) return ((uintptr_t)response & 15) == 0;
    if (d->mask_dtype != VIBO_MASK_CODES) vec = vec && (d->response_row_stride % 4 == 0) && (((uintptr_t)response & 15) == 0);
    if (d->mask_dtype == VIBO_MASK_U8 || d->mask_dtype == VIBO_MASK_CODES)
        vec = vec && (d->mask_row_stride % 4 == 0) && (((uintptr_t)mask & 3) == 0);
    if (d->mask_dtype == VIBO_MASK_I64) vec = vec && (d->mask_row_stride % 2 == 0) && (((uintptr_t)mask & 15) == 0);
    return vec;
}

// rows a row-split kernel can take: u8 / no mask / cell codes, readable in chunks of 4 cells
static bool row_split_shape(const vibo_desc* d, int max_items) {
    return d->num_item >= 4 && d->num_item <= max_items && rows_chunkable(d) && d->mask_dtype != VIBO_MASK_I64;
}

// wave-per-row kernel (A <= 2, 1PL/2PL, 192 <= I <= 1024): 4 workgroups of 4 waves per CU
static bool row_kernel_shape(const vibo_desc* d) {
    const int I = d->num_item;
    return d->ability_dim <= 2 && d->irt_model <= 2 && I >= 192 && I <= 1024 && (I % 4 == 0) && d->n_flows == 0;
}

static int choose_path(const vibo_desc* d, Path* path) {
    const int I = d->num_item, A = d->ability_dim;
    const bool is_cond = d->posterior == VIBO_POSTERIOR_CONDITIONAL, is_given = d->posterior == VIBO_POSTERIOR_GIVEN;
    // ability_dim 9..16: the wave-per-person kernel's wide instantiation (every row-split / tiled kernel holds 8 dims)
    if (A > VIBO_MAX_ABILITY_DIM) { *path = Path::General; return 0; }
    if (is_given && !row_split_shape(d, 32767))
        return fail(-8, "VIBO_POSTERIOR_GIVEN needs the row-split path: 4..32767 items, rows chunkable in 4 cells, no int64 mask");
    // panel mode (item counts up to 32767: the whole-row counts are packed as n_correct << 16 | n_observed in an
    // int): one row-split launch per kPanelItems items (the backward is linear in d LL/d theta, so the panels
    // backpropagate their partial sums independently).  Unconditional posterior: a row-count pass supplies the
    // whole-row counts.  Conditional posterior (any item count): cond_pre_kernel supplies the product-of-experts
    // sums, cond_post_kernel scatters the table gradient (vibo_cond.hip).  The wave-per-person kernel remains
    // the fallback for unaligned rows (decided at launch).
    if (row_split_shape(d, 32767) && (is_cond || is_given || I > kPanelItems)) { *path = Path::Panels; return 0; }
    // wave-per-person kernel: conditional posterior, > 1024 items; planar flows only when the row-split kernel
    // cannot take the launch (ragged / unaligned rows, int64 mask, < 192 items)
    if (is_cond || I > kPanelItems || (d->n_flows > 0 && !row_split_shape(d, kPanelItems))) { *path = Path::General; return 0; }
    // row-split kernel (192 <= I <= 1024, u8 / no mask): nq waves share a row, 8 waves per CU.
    // Preferred over the wave-per-row kernel (1.03 vs 1.10 ms at A = 1, 1.03 vs 1.49 ms at A = 2 on 1M x 1k),
    // which stays for int64 masks.
    if (row_split_shape(d, kPanelItems)) { *path = Path::Split; return 0; }
    *path = row_kernel_shape(d) ? Path::Row : Path::Tiled;
    return 0;
}

Path resolve_path(const Plan& pl, const vibo_desc* d, bool vec) {
    if (vec) return pl.path;
    // rows that cannot be read in aligned 16-byte chunks
    switch (pl.path) {
        case Path::General:
        case Path::Panels: return Path::General;
        case Path::Split: return d->n_flows > 0 ? Path::General : Path::Tiled;      // (the tiled kernel has no flows)
        default: return Path::Tiled;
    }
}

int plan_kernel_code(const Plan& pl) {
    switch (pl.path) {
        case Path::General: return VIBO_KERNEL_GENERAL;
        case Path::Row: return VIBO_KERNEL_ROW;
        case Path::Tiled: return VIBO_KERNEL_TILED;
        default: break;
    }
    return pl.engine == Engine::Matrix ? VIBO_KERNEL_MATRIX : pl.engine == Engine::Narrow ? VIBO_KERNEL_NARROW : VIBO_KERNEL_VALU;
}

int plan_cond_pass_bits(const Plan& pl) {
    if (!pl.conditional()) return 0;
    return (pl.first == FirstPass::CondMatrix ? 1 : 0) | (pl.tail == Tail::CondMatrix ? 2 : 0) | (pl.first == FirstPass::CondFused ? 4 : 0);
}

// the variant's fields that the descriptor and the plan fix, for a launch over `items` items whose rows reach the kernel as mask_dtype
static SplitVariant variant_of(const vibo_desc* d, const Plan& pl, int items, int mask_dtype, bool gathered) {
    SplitVariant v{};
    v.engine = pl.engine; v.irt = d->irt_model; v.grad = d->want_grad != 0; v.flows = d->n_flows > 0;
    v.rm = mask_dtype == VIBO_MASK_CODES ? kRowsCodes : mask_dtype == VIBO_MASK_SIGN ? kRowsSign : mask_dtype == VIBO_MASK_TILES ? kRowsTiles
           : gathered ? kRowsGathered : kRowsInOrder;
    v.xm = pl.path != Path::Panels ? kHooksNone
           : pl.first == FirstPass::CondFused ? kHooksCondFused : pl.first == FirstPass::GivenDirect ? kHooksGiven : kHooksPanel;
    v.at = pl.engine == Engine::Matrix ? 8 : pl.engine == Engine::Narrow ? (d->ability_dim <= 2 ? d->ability_dim : 4) : pl.AT <= 2 ? 2 : pl.AT == 4 ? 4 : 8;
    v.waves = pl.engine == Engine::Matrix ? (items + 127) / 128 : pl.engine == Engine::Narrow ? 4 : (items + 255) / 256;
    v.nw8 = pl.engine == Engine::Matrix && v.waves == 8;
    return v;
}

bool split_variant(const vibo_desc* d, const Plan& pl, const ElboParams& p, SplitVariant* out) {
    const SplitVariant v = *out = variant_of(d, pl, p.I, p.mask_dtype, p.row_index != nullptr);
    // the hook fields first_pass / launch_panels left in p against the mode the plan names (fused: one panel, ability_dim 1, fp32 rows)
    const bool panel = p.row_cnt || p.pre_stats || !p.primary || p.panel_count > 1, given = p.given_post || p.given_grad;
    const bool hooks_ok = v.xm == kHooksNone    ? !(panel || p.post_coef || given || p.cond_table)
                          : v.xm == kHooksPanel ? !(given || p.cond_table)
                          : v.xm == kHooksGiven ? p.given_post && !(panel || p.post_coef || p.cond_table)
                                                : p.cond_table && !(panel || given) && (p.post_coef || !v.grad) && p.A == 1 && !v.flows &&
                                                      v.rm <= kRowsGathered && v.engine == Engine::Matrix;
    // sign-as-mask rows and tile images: the matrix kernel's plain instantiations, rows in order without a mask; tile images also
    // under the caller-supplied posterior (vibo_msplit_tg.hip)
    const bool sign_xm = v.xm == kHooksNone || (v.rm == kRowsTiles && v.xm == kHooksGiven);
    const bool sign_ok = (v.rm != kRowsSign && v.rm != kRowsTiles) || (v.engine == Engine::Matrix && sign_xm && !v.flows && !p.row_index && !p.mask && p.response);
    // the narrow-row kernel: the plain model on 1-byte masks / cell codes
    const bool narrow_ok = v.engine != Engine::Narrow || (p.I >= 4 && p.I <= 128 && p.A <= 4 && !v.flows && v.xm == kHooksNone &&
                                                          (v.rm == kRowsCodes || p.mask_dtype != VIBO_MASK_I64));
    // eps may be null only where the instantiation draws the noise itself, and only in the folded step
    return hooks_ok && sign_ok && narrow_ok && (p.eps || (ms_draws_noise(v) && p.step_tick));
}

StepContract step_contract(const vibo_desc* d, const Plan& pl, bool rows_gathered) {
    StepContract c{};
    c.ok = d->posterior == VIBO_POSTERIOR_UNCONDITIONAL && d->n_flows == 0 && d->reg_mode == VIBO_REG_KL && d->want_grad && pl.path == Path::Split;
    if (!c.ok) return c;
    const SplitVariant v = variant_of(d, pl, d->num_item, d->mask_dtype, rows_gathered);
    // (vibo_train_epilogue_fused sums in groups of 64: where the stand-alone finalize picks 16, the step's two forms would differ in the last bits)
    c.fused_finalize = finalize_group(pl.split_nblk, 8 + 8 * d->ability_dim + d->num_item * pl.D) == 64;
    c.draws_noise = ms_draws_noise(v); c.sample_optional = ms_sample_optional(v);
    return c;
}

// ---------------------------------------------------------------------------
// stage 2: engine choice -- the measured thresholds
// ---------------------------------------------------------------------------
// cell-code rows leave room for a third wave per SIMD in the narrower row-split kernels (see split_kernel's launch bounds)
static bool codes_three_waves(const vibo_desc* d, int AT) {
    return d->mask_dtype == VIBO_MASK_CODES && (AT <= 2 || (AT == 4 && d->irt_model <= 2));
}

// Which row-split kernel: the matrix-pipe kernel (contractions as f16 hi/lo MFMAs) or the VALU kernel.  The descriptor's
// flags pin one of them (A/B measurements, tests of both paths); VIBO_FLAG_NO_EMIT_CODES: later passes re-read the fp32 rows.
static bool emit_codes_wanted(const vibo_desc* d) { return !(d->flags & VIBO_FLAG_NO_EMIT_CODES); }
// fp32 rows whose first pass leaves 1-byte cell codes behind for the passes that follow / rows that are or become cell codes
static bool rows_become_codes(const vibo_desc* d) {
    return emit_codes_wanted(d) && d->mask_dtype != VIBO_MASK_CODES && d->mask_dtype != VIBO_MASK_I64;
}
static bool rows_are_or_become_codes(const vibo_desc* d) { return d->mask_dtype == VIBO_MASK_CODES || rows_become_codes(d); }

static bool want_msplit(const vibo_desc* d) {
    if (d->flags & VIBO_FLAG_KERNEL_VALU) return false;
    // (32-bit row numbers and batch counters in the matrix kernel)
    if (d->num_person > 0x7fffffff - 0x10000) return false;
    if (d->flags & VIBO_FLAG_KERNEL_MATRIX) return true;
    // Thresholds from tools/calibrate_planner.py (hipGraph replays of both kernels over persons x items x ability_dim on an
    // MI355X, profiles/r03_planner_calibration.txt):
    //  * small minibatches (the reference CLI's default is 16 persons): the matrix kernel's fixed cost -- operand images,
    //    512-thread workgroups, one batch of 32 rows per workgroup -- loses to the VALU kernel's 8-row batches: 1 000 items,
    //    ability_dim 8: 17 vs 22 us at 256 persons, 24 vs 24 at 2 048, 33 vs 27 at 4 096
    //  * narrow matrices: a workgroup of the matrix kernel is ceil(I / 128) waves on one CU, so with few items the chip holds
    //    few waves; the VALU kernel's 256-item waves and 2 workgroups per CU do better there
    //  * ability_dim <= 4: the contractions are a small part of the VALU kernel's work, the matrix kernel only wins once every
    //    workgroup streams several batches (65 536 x 1 000: 80 vs 91 us; 16 384 x 1 000: 36 vs 33)
    // Conditional posterior at ability_dim 1 on fp32 rows: the matrix kernel also replaces the first pass there (its XM == 3), which
    // moves the break-even down (tools/calibrate_planner.py-style hipGraph replays, round 6: 8 192 x 1 000 49 vs 57 us, 16 384 x 1 000
    // 59 vs 72, 65 536 x 512 111 vs 165, 65 536 x 256 102 vs 148; 4 096 persons: 42 vs 45 at 1 000 items, 41 vs 40 at 768, 35 vs 31 at 256)
    if (d->posterior == VIBO_POSTERIOR_CONDITIONAL && d->ability_dim == 1 && d->n_flows == 0 && d->num_item <= kPanelItems && d->num_item >= 256 &&
        d->mask_dtype != VIBO_MASK_CODES && d->mask_dtype != VIBO_MASK_I64 && !(d->flags & (VIBO_FLAG_COND_THREE_PASS | VIBO_FLAG_COND_VALU)) &&
        (!d->want_grad || emit_codes_wanted(d)))
        return d->num_person >= (d->num_item >= 896 ? 4096 : 8192);
    const int width = panel_span(d->num_item, 0).items;
    // (round 6, profiles/r06_planner_calibration.txt: the kernel's launch got ~9 us shorter -- 2 048 x 1 000 at ability_dim 8 19.4 vs 22.6 us,
    //  and the 385..512-item exclusion of round 3 -- "2 workgroups per CU with one batch each at 16 384 persons: 48 vs 42 us" -- now
    //  measures 18.2 vs 21.9 us at 4 096 persons, 36.4 vs 38.8 at 16 384: dropped)
    if (d->ability_dim >= 5 && width >= 896 && d->num_person >= 2048) return true;
    if (d->num_person < 4096) return false;
    const bool many = d->num_person >= 32768;
    if (d->ability_dim <= 4) return many && width >= 640;
    if (width < 320) return false;
    return true;
}
// Narrow rows (4..128 items: BASELINE configs[0] and [3]) of the plain model: the kernel that gives a row to 16 lanes instead of a
// whole wave (vibo_narrow.hip).  Either pinning flag keeps the row-split kernels (tests and A/B runs of those paths).
static bool want_narrow(const vibo_desc* d) {
    if (d->flags & (VIBO_FLAG_KERNEL_VALU | VIBO_FLAG_KERNEL_MATRIX)) return false;
    return d->num_item >= 4 && d->num_item <= 128 && d->ability_dim <= 4 && d->n_flows == 0 &&
           d->posterior == VIBO_POSTERIOR_UNCONDITIONAL && d->mask_dtype != VIBO_MASK_I64;
}

// Conditional posterior (Panels): which form its first pass and its gradient tail take.
static void choose_cond_passes(const vibo_desc* d, Plan* pl) {
    const int I = d->num_item, A = d->ability_dim;
    // the conditional posterior's passes on the matrix pipe need the rows as cell codes: the caller's, or the ones the
    // first pass over fp32 rows leaves behind
    // Where they win was measured with hipGraph replays of both forms over persons x items x ability_dim
    // (tools/calibrate_planner.py --cond: VIBO_FLAG_COND_MATRIX against VIBO_FLAG_COND_VALU; profiles/r03_cond_calibration.txt):
    //   rows = cell codes:  5+ dims always (16 x 1 000: 47 vs 67 us -- the VALU passes take two launches each there),
    //                       3-4 dims from 1 024 persons, 2 dims from 4 096, 1 dim from ~16 M cells (16 384 x 1 000: 74 vs 76 us)
    //   rows = fp32:        the VALU pre pass reads the rows AND leaves the codes behind (1M x 1k: 1.22 ms = the 5 B/cell
    //                       stream); a count-and-emit pass in front of the matrix-pipe pre pass costs the same 1.25 ms
    //                       again, so the VALU pre pass stays up to 4 ability dims (one launch: 1M x 1k at 3 / 4 dims
    //                       2.60 -> 2.39 / 2.41 ms) and only the gradient pass moves: 3+ dims always, else from 2 048 persons
    long long min_persons = (d->flags & VIBO_FLAG_COND_MATRIX) ? 1 : -1;
    if (min_persons < 0) {
        if (d->mask_dtype == VIBO_MASK_CODES) {
            const long long by_cells = 16000000LL / (I > 0 ? I : 1);
            min_persons = A >= 5 ? 1 : A >= 3 ? 1024 : A == 2 ? 4096 : (by_cells > 16384 ? by_cells : 16384);
        } else {
            min_persons = A >= 3 ? 1 : 2048;
        }
    }
    const bool cmat_ok = !(d->flags & VIBO_FLAG_COND_VALU) && rows_are_or_become_codes(d) && d->num_person >= min_persons;
    const bool cmat_pre = cmat_ok && (d->mask_dtype == VIBO_MASK_CODES || A >= 5);
    // Conditional posterior, one panel, ability_dim 1, fp32 rows: the matrix kernel gathers the experts itself while it packs the
    // cells (its XM == 3) and leaves the rows' cell codes behind for the table-gradient pass -- one 5 B/cell stream where
    // cond_pre read 5 + wrote 1 and the matrix kernel read 1 (1M x 1k: 2.28 -> see DESIGN 8.1).  VIBO_FLAG_COND_THREE_PASS /
    // VIBO_FLAG_COND_VALU / VIBO_FLAG_NO_EMIT_CODES keep the three passes.
    const bool cond_fused = pl->panels == 1 && A == 1 && pl->engine == Engine::Matrix && d->n_flows == 0 && d->mask_dtype != VIBO_MASK_CODES &&
                            !(d->flags & (VIBO_FLAG_COND_THREE_PASS | VIBO_FLAG_COND_VALU)) && (!d->want_grad || emit_codes_wanted(d));
    pl->first = cond_fused ? FirstPass::CondFused : cmat_pre ? FirstPass::CondMatrix : FirstPass::CondValu;
    pl->tail = !d->want_grad ? Tail::None : cmat_ok ? Tail::CondMatrix : Tail::CondValu;
}

// ---------------------------------------------------------------------------
// stage 3: grid sizes
// ---------------------------------------------------------------------------
static int narrow_blocks(int num_cu, const vibo_desc* d) {
    // a workgroup = 4 waves = one per SIMD; workgroups per CU = the waves per SIMD the instantiation is compiled for
    // (narrow_waves_per_simd in vibo_narrow.hip); under 1024 records so that the fused train epilogue can finalize them
    const int il = d->num_item <= 64 ? 4 : 8, at = d->ability_dim <= 1 ? 1 : d->ability_dim <= 2 ? 2 : 4;
    const bool g3 = d->irt_model == 3 && d->want_grad;
    const int wps = narrow_waves_per_simd(at, il, g3);      // (vibo_launch.hpp: the kernel's launch bounds use the same function)
    long long nblk = (long long)num_cu * wps;
    if (nblk > 1020) nblk = 1020;
    const long long need = (d->num_person + 15) / 16;          // 4 rows per wave and round
    return (int)(nblk < need ? nblk : (need > 0 ? need : 1));
}
static int msplit_blocks(int num_cu, int items, long long persons) {
    const int nw = (items + 127) / 128;
    // workgroups per CU = what is resident at once: 2 waves per SIMD (the kernel's register budget) = 8 waves per CU, and the
    // 17.6 KB of LDS per wave stay under 160 KB with them.  (Round 2 launched 2 per CU at 5..7 waves and 4 at 3 waves: the
    // surplus workgroups queued behind the resident ones -- with one 32-row batch each that doubled the call:
    // 16 384 x 768 at ability_dim 8 57 us against the VALU kernel's 45, tools/calibrate_planner.py)
    long long nblk = (long long)num_cu * (8 / nw > 1 ? 8 / nw : 1);
    const long long nb = (persons + 31) / 32;
    return (int)(nblk < nb ? nblk : nb);
}

// Engine, template width and grid of the row-split launches: `width` items and nq VALU-kernel waves per launch
static void plan_row_split(const vibo_desc* d, int num_cu, int width, int nq, bool allow_msplit, Plan* pl) {
    if (pl->AT < 2) pl->AT = 2;       // the row-split kernel's narrowest template is 2 wide
    pl->split_nq = nq;
    // 8 waves per CU; forward-only fits 3 waves per SIMD
    pl->split_nblk = clamp_grid(num_cu, ((d->want_grad && !codes_three_waves(d, pl->AT)) ? 8 : 12) / nq, d->num_person, 8);
    pl->engine = Engine::Valu;
    if (allow_msplit && want_msplit(d)) {
        pl->engine = Engine::Matrix;
        pl->AT = 8;
        pl->split_nblk = msplit_blocks(num_cu, width, d->num_person);
    } else if (allow_msplit && want_narrow(d)) {
        pl->engine = Engine::Narrow;
        pl->split_nblk = narrow_blocks(num_cu, d);
    }
    pl->DP = prepped_item_width(d->irt_model, pl->AT);
}

// Tiled kernel (also what Split / Row fall back to on unaligned rows): waves per workgroup, LDS, grid
static void plan_tiled(const vibo_desc* d, int num_cu, Plan* pl) {
    const int I = d->num_item;
    // waves per workgroup (each wave owns <= SB 16-item blocks, see vibo_elbo_kernel.hpp geometry table);
    // the code tile is double-buffered in LDS, 16/waves workgroups share a CU
    const int waves = I <= 144 ? 2 : I <= 304 ? 4 : I <= 512 ? 8 : 16;
    pl->lds_stride = code_tile_stride(waves);
    size_t main_b = (size_t)kTilePersons * pl->lds_stride;            // one fp8 code tile
    const size_t red = (size_t)waves * pl->AT * 65 * 4;               // per-wave dLL/dtheta partials (aliased)
    if (main_b < red) main_b = red;
    if (main_b < (size_t)waves * 32) main_b = (size_t)waves * 32;
    main_b = (main_b + 15) & ~(size_t)15;
    size_t lds = 2 * main_b                                            // double-buffered code tile
                 + 2 * (size_t)(pl->AT + 1) * 65 * 4                   // [theta|valid] share, double-buffered
                 + (size_t)waves * 16 * 20 * 4                         // per-wave G-tile transpose slab
                 + 2 * kTilePersons * 4 + 4 * 2 * pl->AT * 4;          // counts, encoder-table constants
    lds = up256(lds);
    const size_t lds_cu = 160 * 1024;
    int per_cu = (int)(lds_cu / lds);
    const int wave_cap = 16 / waves;             // 4 waves per SIMD (launch bound) = 16 per CU
    if (per_cu > wave_cap) per_cu = wave_cap;
    if (per_cu < 1) per_cu = 1;
    pl->nblk = num_cu * per_cu;
    if (pl->nblk > pl->n_tiles) pl->nblk = pl->n_tiles;
    pl->lds_main = (int)main_b;
    pl->geom.waves = waves;
    pl->geom.grid = pl->nblk;
    pl->geom.lds_bytes = lds;
}

static void plan_panel_grids(const vibo_desc* d, int num_cu, bool allow_msplit, Plan* pl) {
    const int I = d->num_item;
    plan_row_split(d, num_cu, panel_span(I, 0).items, 4, allow_msplit, pl);
    if (pl->engine == Engine::Matrix && pl->panels > 1) {
        // all panels in ONE launch (ElboParams::panel_count): the chip's workgroup slots are shared out over the panels
        int per = num_cu / pl->panels;
        if (per < 1) per = 1;
        if (pl->split_nblk > per) pl->split_nblk = per;
    }
    pl->cond_nblk = clamp_grid(num_cu, 2, d->num_person, 8);      // (4 per CU for one ability dim was tried: the fp32-row variants spill 35-46 registers, 2x slower)
    pl->cond_post_nblk = pl->cond_nblk;
    pl->cond_rec = 8 * d->ability_dim * kPanelItems;
}
// cond_post on cell codes (the caller's, or the ones cond_pre leaves behind) has no fp32 row registers: 3 waves per SIMD
static void raise_cond_post_grid(const vibo_desc* d, int num_cu, Plan* pl) {
    if (pl->conditional() && pl->tail != Tail::CondMatrix && rows_are_or_become_codes(d) && d->ability_dim <= 2)
        pl->cond_post_nblk = clamp_grid(num_cu, 3, d->num_person, 8);
}

// ---------------------------------------------------------------------------
// stage 4: workspace layout
// ---------------------------------------------------------------------------
// the prepped item rows (the head of every workspace; the multi-sample forward keeps up to 4 of them)
static size_t prepped_item_bytes(int I, int DP) { return up256((size_t)((I + 15) & ~15) * DP * 4); }

static void layout_workspace(const vibo_desc* d, Plan* pl) {
    const int I = d->num_item, A = d->ability_dim;
    if (pl->path == Path::General) {
        pl->total_bytes = 256;            // 8 scalar accumulators
        return;
    }
    size_t off = prepped_item_bytes(I, pl->DP);
    if (pl->path != Path::Panels) {
        // one launch: the records of whichever kernel the launch resolves to
        int max_blk = pl->nblk;
        if (pl->row_nblk > max_blk) max_blk = pl->row_nblk;
        if (pl->split_nblk > max_blk) max_blk = pl->split_nblk;
        pl->off_partial = off;
        pl->total_bytes = off + (size_t)max_blk * pl->lay.stride * 4 + 256;
        return;
    }
    pl->off_cnt = off;
    off += up256((size_t)d->num_person * 4);
    pl->off_partial = off;
    off += up256((size_t)pl->panels * pl->split_nblk * pl->lay.stride * 4);
    pl->off_pre = pl->off_coef = pl->off_cpart = pl->off_crec = off;
    if (pl->conditional()) {
        pl->off_pre = off;
        off += pre_block_bytes(pl->panels, d->num_person, A);
        pl->off_coef = off;
        off += up256((size_t)pl->panels * d->num_person * 4 * A * 4);
        pl->off_cpart = off;
        if (pl->first == FirstPass::CondMatrix || pl->tail == Tail::CondMatrix) off += up256(cond_mfma_scratch_bytes(d->num_person, I, A));
        pl->off_crec = off;
        if (pl->tail != Tail::CondMatrix) off += up256((size_t)pl->panels * pl->cond_post_nblk * pl->cond_rec * 4);
    } else if (pl->given()) {
        pl->off_pre = off;
        off += pre_block_bytes(1, d->num_person, A);
        pl->off_coef = off;
        off += up256((size_t)pl->panels * d->num_person * 4 * A * 4);
    }
    // fp32 rows of the conditional posterior (three passes, five at ability_dim > 4): cond_pre also writes the rows' 1-byte
    // cell codes, the later passes read those: 8 instead of 15 B/term of HBM traffic.  (For the two passes of the
    // unconditional posterior with more than 1024 items the extra write costs more than the cheaper panels win:
    // 100k x 10k 2.32 vs 2.23 ms, so row_count_kernel's code output stays unused there.)
    pl->codes_stride = ((long long)I + 255) / 256 * 256;      // whole 128-byte lines per wave store (4 B per lane x 64 lanes)
    if (pl->conditional() && rows_become_codes(d)) {
        pl->off_codes = off;
        off += up256((size_t)d->num_person * pl->codes_stride);
    }
    pl->total_bytes = off + 256;
}

// ---------------------------------------------------------------------------
int make_plan(const vibo_desc* d, int num_cu, Plan* pl, bool allow_msplit) {
    const int I = d->num_item, A = d->ability_dim;
    memset(pl, 0, sizeof(*pl));
    const int rc = choose_path(d, &pl->path);
    if (rc < 0) return rc;
    pl->AT = A > VIBO_MAX_ABILITY_DIM ? 8 : padded_ability_dim(A);
    pl->D = item_feat_dim(d->irt_model, A);
    pl->DP = prepped_item_width(d->irt_model, pl->AT);
    pl->n_tiles = (d->num_person + kTilePersons - 1) / kTilePersons;
    pl->lds_stride = 16;
    pl->lay = partial_layout(A, pl->D, pl->path == Path::Panels ? kPanelItems : I, d->n_flows);
    if (pl->path == Path::Panels) {
        pl->panels = panel_count(I);
        plan_panel_grids(d, num_cu, allow_msplit, pl);
        if (d->posterior == VIBO_POSTERIOR_CONDITIONAL) {
            choose_cond_passes(d, pl);
            raise_cond_post_grid(d, num_cu, pl);
        } else if (d->posterior == VIBO_POSTERIOR_GIVEN) {
            pl->first = pl->panels == 1 ? FirstPass::GivenDirect : FirstPass::GivenPre;
            pl->tail = (d->want_grad && pl->panels > 1) ? Tail::Given : Tail::None;
        } else {
            pl->first = FirstPass::RowCount;
        }
    } else if (pl->path != Path::General) {
        plan_tiled(d, num_cu, pl);        // (at the ability width of the posterior itself: before the row-split kernels widen AT)
        // wave-per-row kernel: 16 items x (params + grads) per lane: 2 workgroups (8 waves) per CU.  (Its records are reserved
        // wherever the shape fits it, also where the row-split kernel runs instead.)
        if (row_kernel_shape(d)) pl->row_nblk = clamp_grid(num_cu, 2, d->num_person, 4);
        if (pl->path == Path::Split) plan_row_split(d, num_cu, I, (I + 255) / 256, allow_msplit, pl);
    }
    layout_workspace(d, pl);
    return 0;
}

int multi_plan(const vibo_desc* d, int num_cu, vibo_desc* d0, Plan* pl, size_t* prep_bytes, bool given_call) {
    *d0 = *d;
    d0->want_grad = 0;
    if (given_call && d->posterior != VIBO_POSTERIOR_GIVEN)
        return fail(-3, "vibo_elbo_multi_forward_given: the descriptor's posterior must be VIBO_POSTERIOR_GIVEN");
    // (GIVEN outside the row-split shapes -- 4..32767 items, rows chunkable in 4 cells, no int64 mask, ability_dim <= 8 -- has no plan: -8)
    const int rc = make_plan(d0, num_cu, pl, false);
    if (rc < 0) return rc;
    // conditional posterior: the expert table itself depends on the item sample; its call stacks the samples' tables and comes back
    // here with the posteriors as given
    if (d->posterior == VIBO_POSTERIOR_CONDITIONAL)
        return fail(-8, "multi-sample forward: conditional posterior, one table per sample (use vibo_elbo_multi_forward_cond)");
    if (d->posterior == VIBO_POSTERIOR_GIVEN && !given_call)
        return fail(-8, "multi-sample forward: caller-supplied posterior (use vibo_elbo_multi_forward_given)");
    if (!pl->row_split()) return fail(-8, "multi-sample forward: shape is not on the row-split path");
    *prep_bytes = prepped_item_bytes(d->num_item, pl->DP);
    return 0;
}

// conditional posterior on cell codes, 4 096 persons or more: the experts' sums on the matrix pipe (launch_cond_pre_mfma), as in the
// ELBO call
bool encode_on_matrix_pipe(const vibo_desc* d) {
    return d->posterior == VIBO_POSTERIOR_CONDITIONAL && d->mask_dtype == VIBO_MASK_CODES && !(d->flags & VIBO_FLAG_COND_VALU) &&
           (d->num_person >= 4096 || d->ability_dim >= 5 || (d->flags & VIBO_FLAG_COND_MATRIX));
}
size_t encode_scratch_bytes(const vibo_desc* d) {
    const int I = d->num_item, A = d->ability_dim;
    if (A > VIBO_MAX_ABILITY_DIM) return 0;      // (wave-per-person encode kernel)
    if (!row_split_shape(d, 32767)) return 0;
    if (d->posterior == VIBO_POSTERIOR_CONDITIONAL) {
        size_t pre = pre_block_bytes(panel_count(I), d->num_person, A);
        if (encode_on_matrix_pipe(d)) pre += cond_mfma_scratch_bytes(d->num_person, I, A);      // (only its table image is used)
        return pre + 256;
    }
    return (size_t)d->num_person * 4 + 256;
}

}  // namespace vibo
