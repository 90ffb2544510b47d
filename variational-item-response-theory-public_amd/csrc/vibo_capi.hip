// vibo_capi.hip -- C ABI of libvibo_hip.so (see include/vibo_hip.h): the extern "C" surface and the drivers that turn a plan
// (vibo_planner.hpp) into launches.  The small kernels around the fused ELBO kernels are in vibo_helpers.hip.
// vibo_host.hpp: what they share with the planner and the other units' entry points (panel split, workspace check, failed-launch path).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/vibo_hip.h"
#include "../../include/vibo_hip_sign_rows.h"
#include "../../include/vibo_hip_tile_rows.h"
#include "../../include/vibo_hip_given_tiles.h"
#include "vibo_cond.hpp"
#include "vibo_general.hpp"
#include "vibo_helpers.hpp"
#include "vibo_launch.hpp"
#include "vibo_multi.hpp"
#include "vibo_params.hpp"
#include "vibo_planner.hpp"
#include "vibo_train_hook.hpp"

namespace vibo {

// measurement hook (vibo_set_insitu_timer): the timer block the matrix row-split launches of THIS host thread stamp; null = none
static thread_local unsigned long long* g_insitu = nullptr;

// descriptor check + plan of the exports that launch nothing: 0, or the refusal's code (error string set)
static int plan_for(const vibo_desc* d, Plan* pl, bool sign_rows = false) {
    const int rc = check_desc(d, sign_rows);
    return rc ? rc : make_plan(d, device_cus(), pl);
}

// One row-split launch: split_variant (vibo_planner.hip) names the instantiation or refuses; the variant alone picks the unit.
static hipError_t launch_split(const vibo_desc* d, const Plan& pl, const ElboParams& p, int grid, hipStream_t s) {
    static SplitLauncher* const valu[3][3] = {{launch_elbo_split_a2, launch_elbo_split_a4, launch_elbo_split_a8},
                                              {launch_elbo_split_g2, launch_elbo_split_g4, launch_elbo_split_g8},
                                              {launch_elbo_split_c2, launch_elbo_split_c4, launch_elbo_split_c8}};
    static SplitLauncher* const matrix[3][5] = {{launch_elbo_msplit_a, launch_elbo_msplit_g, launch_elbo_msplit_c, launch_elbo_msplit_s, launch_elbo_msplit_t},
                                                {launch_elbo_msplit_fa, launch_elbo_msplit_fg, launch_elbo_msplit_fc, nullptr, nullptr},
                                                {launch_elbo_msplit_xa, launch_elbo_msplit_xg, nullptr, nullptr, nullptr}};      // plain | flows | fused
    SplitVariant v;
    if (!split_variant(d, pl, p, &v)) return hipErrorInvalidValue;      // (also: none of the table's empty cells)
    // (a tile image under the caller-supplied posterior has a unit of its own: launch_elbo_msplit_t holds hook mode 0 alone)
    SplitLauncher* const unit = v.engine == Engine::Narrow ? launch_elbo_narrow
                                : v.engine == Engine::Valu ? valu[v.rm][v.at == 2 ? 0 : v.at == 4 ? 1 : 2]
                                : (v.rm == kRowsTiles && v.xm == kHooksGiven) ? launch_elbo_msplit_tg
                                                           : matrix[v.xm == kHooksCondFused ? 2 : v.flows ? 1 : 0][v.rm];
    return unit(p, v, grid, s);
}

// the pointers of one ELBO call (vibo_elbo_fwd_bwd and its variants)
struct ElboArgs {
    const float* response;
    const void* mask;
    const int64_t* row_index;
    const float *table, *item, *eps, *flow;
    float *out_scalars, *ability_mu, *ability_logvar, *ability, *ability_k, *ability_ladj;
    float *grad_table, *grad_item, *grad_flow;
    void* workspace;
    size_t workspace_bytes;
    hipStream_t stream;
    const int32_t* row_counts = nullptr;      // vibo_elbo_fwd_bwd_counts: the caller's whole-row counts
    int32_t* step_count = nullptr;            // vibo_elbo_fwd_bwd_step: the train step's Adam counter
    int skip_finalize = 0;
    uint64_t noise_seed = 0;                  // vibo_elbo_fwd_bwd_step_noise
    uint32_t noise_stream = 0;
    bool given_tiles = false;                 // vibo_elbo_fwd_bwd_given_tiles: a VIBO_MASK_TILES image under VIBO_POSTERIOR_GIVEN, and nothing else
};

// the panel passes' blocks of the workspace
struct PanelBufs {
    float *pre, *coef;
    void* mscratch;           // matrix-pipe passes: images + records
    float* crec;              // the VALU post pass's records
    uint8_t* code_rows;       // fp32 rows + more than one pass: the first pass (cond_pre / the fused matrix kernel) leaves 1-byte cell codes
                              // of the minibatch's rows here (already gathered), every later pass reads those; null: not used
};

// the row description of a call, the same fields in every params struct (the item count is the struct's own: I, I_total or both)
template <typename Params>
static void fill_rows(Params& p, const vibo_desc* d, const float* response, const void* mask, const int64_t* row_index) {
    p.response = response; p.mask = mask; p.row_index = row_index;
    p.resp_stride = d->response_row_stride; p.mask_stride = d->mask_row_stride;
    p.B = d->num_person; p.A = d->ability_dim; p.mask_dtype = d->mask_dtype;
}
// from here on the rows are the cell codes just written (in minibatch order)
template <typename Params>
static void read_emitted_codes(Params& p, const uint8_t* code_rows, long long codes_stride) {
    p.response = nullptr; p.mask = code_rows; p.row_index = nullptr;
    p.mask_stride = codes_stride; p.mask_dtype = VIBO_MASK_CODES;
}

static int run_general(const vibo_desc* d, const Plan& pl, const ElboArgs& a, int num_cu) {
    const int I = d->num_item, A = d->ability_dim;
    hipStream_t s = a.stream;
    const size_t n_table = (size_t)(d->posterior == VIBO_POSTERIOR_CONDITIONAL ? 2 * I * 2 * A : 2 * 2 * A);
    const size_t n_flow = (size_t)d->n_flows * (2 * A + 1);
    hipError_t ge = hipMemsetAsync(a.workspace, 0, 256, s);
    if (ge == hipSuccess && d->want_grad) {
        ge = hipMemsetAsync(a.grad_table, 0, 2 * n_table * sizeof(float), s);
        if (ge == hipSuccess) ge = hipMemsetAsync(a.grad_item, 0, (size_t)I * pl.D * sizeof(float), s);
        if (ge == hipSuccess && n_flow) ge = hipMemsetAsync(a.grad_flow, 0, 2 * n_flow * sizeof(float), s);
    }
    if (ge != hipSuccess) return hip_fail(ge, "memset");
    GeneralParams g;
    memset(&g, 0, sizeof(g));
    fill_rows(g, d, a.response, a.mask, a.row_index);
    g.table = a.table; g.item = a.item; g.eps = a.eps;
    g.flow = a.flow; g.ability_mu = a.ability_mu; g.ability_logvar = a.ability_logvar; g.ability = a.ability;
    g.ability_k = a.ability_k; g.ability_ladj = a.ability_ladj;
    g.grad_table = a.grad_table; g.grad_item = a.grad_item; g.grad_flow = a.grad_flow;
    g.acc_scalars = static_cast<float*>(a.workspace); g.out_scalars = a.out_scalars;
    g.I = I; g.D = pl.D; g.irt = d->irt_model;
    g.conditional = d->posterior == VIBO_POSTERIOR_CONDITIONAL; g.missing_mode = d->missing_mode;
    g.reg_mode = d->reg_mode; g.n_flows = d->n_flows; g.want_grad = d->want_grad;
    return hip_rc(launch_elbo_general(g, num_cu, s), "general elbo kernel launch");
}

// what every ELBO launch's params take from the descriptor and the plan: the rows, the model's shape, one whole-row panel
static void elbo_shape(ElboParams& p, const vibo_desc* d, const Plan& pl, const float* response, const void* mask, const int64_t* row_index,
                       const float* table, const float* flow) {
    fill_rows(p, d, response, mask, row_index);
    p.table = table; p.flow = flow;
    p.I = p.I_total = d->num_item; p.D = pl.D; p.DP = pl.DP;
    p.missing_mode = d->missing_mode; p.reg_mode = d->reg_mode; p.n_flows = d->n_flows;
    p.lay = pl.lay; p.primary = 1;
}

static ElboParams elbo_params(const vibo_desc* d, const Plan& pl, const ElboArgs& a, bool vec) {
    ElboParams p;
    memset(&p, 0, sizeof(p));
    elbo_shape(p, d, pl, a.response, a.mask, a.row_index, a.table, a.flow);
    p.item_prep = static_cast<float*>(a.workspace); p.item_raw = a.item; p.eps = a.eps;
    p.ability_mu = a.ability_mu; p.ability_logvar = a.ability_logvar; p.ability = a.ability;
    p.partial = reinterpret_cast<float*>(static_cast<char*>(a.workspace) + pl.off_partial);
    p.n_tiles = pl.n_tiles; p.lds_stride = pl.lds_stride; p.lds_main = pl.lds_main;
    p.ability_k = a.ability_k; p.ability_ladj = a.ability_ladj;
    p.vec_ok = (vec && p.I % 4 == 0) ? 1 : 0;      // the tiled / wave-per-row kernels' vector loads assume whole chunks
    p.step_tick = a.step_count;
    p.insitu = g_insitu;
    p.noise_seed_lo = (uint32_t)a.noise_seed; p.noise_seed_hi = (uint32_t)(a.noise_seed >> 32); p.noise_stream = a.noise_stream;
    return p;
}

// the row fields and the expert table of the conditional passes
static CondParams cond_params(const vibo_desc* d, const float* response, const void* mask, const int64_t* row_index, const float* table) {
    CondParams cp;
    memset(&cp, 0, sizeof(cp));
    fill_rows(cp, d, response, mask, row_index);
    cp.table = table; cp.I_total = d->num_item;
    return cp;
}

// cond_pre_kernel over the items [cp.item0, + cp.I) into cp.pre_out: 4 ability dims per launch.  code_rows: the first launch leaves the
// rows' cell codes there, and dims 4..7 read those instead of the caller's rows
static hipError_t cond_pre_span(CondParams cp, uint8_t* code_rows, long long codes_stride, int grid, hipStream_t s) {
    const CondPassShape sh = cond_pass_shape(cp.A, cp.I);
    hipError_t e = hipSuccess;
    for (cp.a0 = 0; cp.a0 < cp.A && e == hipSuccess; cp.a0 += 4) {
        cp.codes_out = cp.a0 == 0 ? code_rows : nullptr;
        if (code_rows && cp.a0 > 0) read_emitted_codes(cp, code_rows, codes_stride);
        e = launch_cond_pre(cp, sh.at, sh.waves, grid, s);
    }
    return e;
}

// conditional posterior, VALU first pass
static hipError_t cond_pre_valu(const vibo_desc* d, const Plan& pl, CondParams cp, const PanelBufs& b, hipStream_t s) {
    cp.item0 = 0; cp.I = d->num_item; cp.pre_out = b.pre;
    if (pl.panels == 1) return cond_pre_span(cp, b.code_rows, pl.codes_stride, pl.cond_nblk, s);
    // more than one panel: ALL of them in one launch per 4 ability dims (CondParams::panel_count), the chip's workgroup
    // slots shared out over the panels; their statistics summed into panel 0's block
    const int per = pl.cond_nblk / pl.panels;
    cp.I = kPanelItems; cp.panel_count = pl.panels;
    const hipError_t e = cond_pre_span(cp, b.code_rows, pl.codes_stride, (per < 1 ? 1 : per) * pl.panels, s);
    return e != hipSuccess ? e : launch_panel_sum(b.pre, (long long)d->num_person * (2 * d->ability_dim + 1), pl.panels, s);
}

// unconditional posterior over more than 1024 items: the whole-row counts
static hipError_t first_pass_counts(const vibo_desc* d, const Plan& pl, const ElboArgs& a, int num_cu, ElboParams& p) {
    int* cnt = reinterpret_cast<int*>(static_cast<char*>(a.workspace) + pl.off_cnt);
    p.row_cnt = cnt;
    if (a.row_counts && !a.row_index) {
        // the caller's whole-row counts (vibo_row_counts of the same rows, kept with its resident data: they depend on the
        // data alone): no count pass -- half of the call on rows of more than 1024 items (100k x 10k: 1.64 -> 0.85 ms)
        p.row_cnt = a.row_counts;
        return hipSuccess;
    }
    if (a.row_counts) return launch_gather_counts(a.row_counts, a.row_index, cnt, d->num_person, a.stream);
    return launch_row_counts(d, num_cu, a.response, a.mask, a.row_index, cnt, nullptr, pl.codes_stride, a.stream);
}

// Panels: whatever supplies the whole-row statistics, and the ElboParams fields through which the row-split kernel reads them
static hipError_t first_pass(const vibo_desc* d, const Plan& pl, const ElboArgs& a, int num_cu, const CondParams& cp, const PanelBufs& b,
                             ElboParams& p) {
    const int I = d->num_item, A = d->ability_dim;
    hipStream_t s = a.stream;
    switch (pl.first) {
        case FirstPass::CondFused:
            // no first pass: the matrix kernel gathers the experts itself (XM == 3) and writes the cell codes the gradient pass reads
            p.cond_table = a.table;
            p.codes_out = d->want_grad ? b.code_rows : nullptr;
            p.codes_stride = pl.codes_stride;
            return hipSuccess;
        case FirstPass::GivenDirect:
            p.given_post = a.table;
            p.given_grad = d->want_grad ? a.grad_table : nullptr;
            p.table = a.item;             // the 2-row expert table is not used in this mode: any finite floats (>= 4 A of them)
            return hipSuccess;
        case FirstPass::GivenPre:
            p.pre_stats = b.pre;
            p.pre_panels = 1;
            p.table = a.item;             // the 2-row expert table is not used in this mode: any finite floats (>= 4 A of them)
            return launch_given_pre(a.table, b.pre, (long long)d->num_person, A, I, s);
        case FirstPass::CondMatrix:
            // matrix-pipe pre pass.  fp32 rows: the contraction kernel reads them itself and leaves the rows' cell codes behind for
            // the passes that follow (minibatch order) -- round 3 ran a re-pack stream (row_count_kernel) in front of it
            p.pre_stats = b.pre;
            p.pre_panels = 1;
            if (b.code_rows)
                return launch_cond_pre_mfma_fp32(a.response, d->mask_dtype == VIBO_MASK_U8 ? a.mask : nullptr, (long long)d->response_row_stride,
                                                 (long long)d->mask_row_stride, a.row_index, d->num_person, I, A, a.table, b.pre, b.code_rows,
                                                 (long long)pl.codes_stride, b.mscratch, s);
            return launch_cond_pre_mfma(static_cast<const uint8_t*>(a.mask), d->mask_row_stride, a.row_index, d->num_person, I, A, a.table,
                                        b.pre, b.mscratch, s);
        case FirstPass::CondValu:
            p.pre_stats = b.pre;
            p.pre_panels = 1;             // (more panels: summed into panel 0's block)
            return cond_pre_valu(d, pl, cp, b, s);
        default:
            return first_pass_counts(d, pl, a, num_cu, p);
    }
}

// Panels: the row-split launches
static hipError_t launch_panels(const vibo_desc* d, const Plan& pl, ElboParams& p, float* coef, hipStream_t s) {
    const int I = d->num_item, A = d->ability_dim;
    float* partial = p.partial;
    if (pl.tail == Tail::None) coef = nullptr;      // (no pass reads the per-person backward coefficients)
    if (pl.engine == Engine::Matrix && pl.panels > 1) {
        // the matrix kernel takes all panels in one launch: workgroup = (panel, slot), see ElboParams::panel_count
        p.item0 = 0; p.I = kPanelItems; p.primary = 1; p.panel_count = pl.panels;
        p.post_coef = coef;
        return launch_split(d, pl, p, pl.panels * pl.split_nblk, s);
    }
    hipError_t e = hipSuccess;
    for (int pn = 0; pn < pl.panels && e == hipSuccess; ++pn) {
        const PanelSpan sp = panel_span(I, pn);
        p.item0 = sp.item0; p.I = sp.items;
        p.primary = pn == 0 ? 1 : 0;
        p.partial = partial + (size_t)pn * pl.split_nblk * pl.lay.stride;
        p.post_coef = coef ? coef + (size_t)pn * d->num_person * 4 * A : nullptr;
        e = launch_split(d, pl, p, pl.split_nblk, s);
    }
    p.partial = partial;
    return e;
}

// Panels with gradients: the per-person backward coefficients -> the gradient of the expert table / the caller's posterior
static hipError_t gradient_tail(const vibo_desc* d, const Plan& pl, const ElboArgs& a, CondParams cp, const PanelBufs& b, CondFinTail* tail) {
    const int I = d->num_item, A = d->ability_dim;
    hipStream_t s = a.stream;
    if (pl.tail == Tail::None) return hipSuccess;
    if (pl.tail == Tail::Given) return launch_given_post(a.table, b.coef, pl.panels, a.grad_table, (long long)d->num_person, A, s);
    hipError_t e = hipSuccess;
    if (pl.panels > 1) {       // the panels' backward coefficients summed once (cond_post reads 1 block, not `panels`)
        e = launch_panel_sum(b.coef, (long long)d->num_person * 4 * A, pl.panels, s);
        cp.coef_panels = 1;
    }
    if (pl.tail == Tail::CondMatrix) {
        if (e == hipSuccess)
            e = launch_cond_post_mfma(static_cast<const uint8_t*>(cp.mask), cp.mask_stride, cp.row_index, d->num_person, I, A, a.table,
                                      b.coef, a.grad_table, b.mscratch, s, tail);
        return e;
    }
    for (int pn = 0; pn < pl.panels && e == hipSuccess; ++pn) {
        const PanelSpan sp = panel_span(I, pn);
        const CondPassShape sh = cond_pass_shape(A, sp.items);
        cp.item0 = sp.item0; cp.I = sp.items;
        cp.partial = b.crec + (size_t)pn * pl.cond_post_nblk * pl.cond_rec;
        for (cp.a0 = 0; cp.a0 < A && e == hipSuccess; cp.a0 += 4) e = launch_cond_post(cp, sh.at, sh.waves, pl.cond_post_nblk, s);
    }
    if (e == hipSuccess) e = launch_cond_finalize(b.crec, a.grad_table, I, A, pl.panels, pl.cond_post_nblk, pl.cond_rec, s, tail);
    return e;
}

static hipError_t run_panels(const vibo_desc* d, const Plan& pl, const ElboArgs& a, int num_cu, ElboParams& p, CondFinTail* tail) {
    char* wsb = static_cast<char*>(a.workspace);
    PanelBufs b;
    b.pre = reinterpret_cast<float*>(wsb + pl.off_pre);
    b.coef = reinterpret_cast<float*>(wsb + pl.off_coef);
    b.mscratch = wsb + pl.off_cpart;
    b.crec = reinterpret_cast<float*>(wsb + pl.off_crec);
    b.code_rows = pl.off_codes ? reinterpret_cast<uint8_t*>(wsb + pl.off_codes) : nullptr;
    CondParams cp = cond_params(d, a.response, a.mask, a.row_index, a.table);
    cp.codes_stride = pl.codes_stride;
    cp.coef_panels = pl.panels; cp.rec_stride = pl.cond_rec; cp.coef_in = b.coef;

    hipError_t e = first_pass(d, pl, a, num_cu, cp, b, p);
    if (e != hipSuccess) return e;
    if (b.code_rows) {
        read_emitted_codes(cp, b.code_rows, pl.codes_stride);
        // (CondFused: the matrix kernel reads the fp32 rows; the gradient pass the codes it leaves behind)
        if (pl.first != FirstPass::CondFused) read_emitted_codes(p, b.code_rows, pl.codes_stride);
    }
    e = launch_panels(d, pl, p, b.coef, a.stream);
    if (e != hipSuccess) return e;
    return gradient_tail(d, pl, a, cp, b, tail);
}

// Split / Row / Tiled: one launch
static hipError_t run_single(const vibo_desc* d, const Plan& pl, Path path, const ElboParams& p, hipStream_t s) {
    const bool grad = d->want_grad != 0;
    if (path == Path::Split) return launch_split(d, pl, p, pl.split_nblk, s);
    if (path == Path::Row) return launch_elbo_rows(p, d->irt_model, grad, pl.row_nblk, s);
    switch (pl.AT) {
        case 1: return launch_elbo_a1(p, d->irt_model, grad, pl.geom, s);
        case 2: return launch_elbo_a2(p, d->irt_model, grad, pl.geom, s);
        case 4: return launch_elbo_a4(p, d->irt_model, grad, pl.geom, s);
        default: return launch_elbo_a8(p, d->irt_model, grad, pl.geom, s);
    }
}

// the fixed-order sum of the launch's partial records (and, in the same launch, the conditional posterior's last stage)
static int run_finalize(const vibo_desc* d, const Plan& pl, Path path, const ElboArgs& a, const float* partial, const CondFinTail& tail) {
    FinalizeParams f;
    memset(&f, 0, sizeof(f));
    f.partial = partial; f.out_scalars = a.out_scalars; f.grad_item = a.grad_item; f.grad_flow = a.grad_flow;
    f.grad_table = (pl.conditional() || pl.given()) ? nullptr : a.grad_table;      // (theirs comes from the gradient tail)
    f.nblk = path == Path::Panels ? pl.panels * pl.split_nblk : path == Path::Split ? pl.split_nblk : path == Path::Row ? pl.row_nblk : pl.nblk;
    f.I = d->num_item; f.A = d->ability_dim; f.D = pl.D; f.n_flows = d->n_flows; f.reg_mode = d->reg_mode;
    f.irt = d->irt_model; f.want_grad = d->want_grad ? 1 : 0; f.lay = pl.lay;
    f.panel_items = path == Path::Panels ? kPanelItems : 1 << 30;
    f.bpp = path == Path::Panels ? pl.split_nblk : f.nblk;
    f.tail = tail;
    return hip_rc(launch_finalize(f, a.stream), "finalize launch");
}

static int elbo_fwd_bwd_impl(const vibo_desc* d, const ElboArgs& a) {
    const int num_cu = device_cus();
    int rc = check_desc(d, !a.given_tiles, a.given_tiles);
    if (rc) return rc;
    const bool tile_rows = d->mask_dtype == VIBO_MASK_TILES;
    const bool sign_rows = d->mask_dtype == VIBO_MASK_SIGN || tile_rows;      // (the row formats of this call alone)
    if (sign_rows && (a.row_index || a.row_counts))
        return fail(-8, "%s rows: rows in order only (row_index must be NULL), without caller-supplied row counts",
                    tile_rows ? "VIBO_MASK_TILES" : "VIBO_MASK_SIGN");
    if ((!a.response && d->mask_dtype != VIBO_MASK_CODES) || !a.table || !a.item || !a.out_scalars)
        return fail(-5, "null required pointer");
    // (null eps / ability_mu / ability_logvar / ability: the folded step on the matrix kernel only, checked once the plan is known)
    const bool own_post = a.eps && a.ability_mu && a.ability_logvar && a.ability;
    if (!own_post && !a.step_count) return fail(-5, "null required pointer");
    if ((a.ability_mu == nullptr) != (a.ability_logvar == nullptr)) return fail(-5, "ability_mu / ability_logvar: both or neither");    if ((rc = require_rows(d, a.response, a.mask)) != 0) return rc;
    if (d->want_grad && (!a.grad_table || !a.grad_item)) return fail(-5, "want_grad needs grad_table and grad_item");
    if (d->n_flows > 0 && (!a.flow || !a.ability_k || !a.ability_ladj)) return fail(-5, "flows need flow, ability_k, ability_ladj");
    if (d->n_flows > 0 && d->want_grad && !a.grad_flow) return fail(-5, "want_grad with flows needs grad_flow");
    Plan pl;
    if ((rc = make_plan(d, num_cu, &pl)) < 0) return rc;
    if ((rc = check_workspace(a.workspace, a.workspace_bytes, pl.total_bytes)) != 0) return rc;
    // 16-byte row loads need aligned rows
    const bool vec = rows_vec_ok(d, a.response, a.mask);
    const Path path = resolve_path(pl, d, vec);
    const bool row_split = path == Path::Panels || path == Path::Split;
    if (d->mask_dtype == VIBO_MASK_CODES && !row_split) return codes_unsupported();
    const bool image_path = a.given_tiles ? path == Path::Panels && pl.first == FirstPass::GivenDirect : path == Path::Split;
    if (sign_rows && !(image_path && pl.engine == Engine::Matrix))
        return tile_rows ? fail(-8, "VIBO_MASK_TILES rows: the tile image must be 16-byte aligned")
                         : fail(-8, "VIBO_MASK_SIGN rows: the response rows must be 16-byte aligned with a stride that is a multiple of 4");
    if (pl.given() && path != Path::Panels)
        return fail(-8, "VIBO_POSTERIOR_GIVEN: rows must be aligned for 4-cell chunks (see vibo_amd.ops.pad_rows)");
    const StepContract step = step_contract(d, pl, a.row_index != nullptr);
    if ((a.step_count || a.skip_finalize) && !(step.ok && path == Path::Split))
        return fail(-8, "vibo_elbo_fwd_bwd_step: single-launch row-split calls of the plain model only (unconditional posterior, no "
                        "flows, KL regulariser, gradients, 4..1024 items, aligned rows): use vibo_train_prologue + vibo_elbo_fwd_bwd");
    if (!own_post && !step.draws_noise)
        return fail(-5, "null eps / ability_mu / ability_logvar / ability: only where the folded step runs the matrix kernel "
                        "(vibo_train_step_draws_noise)");
    if (!a.ability && !step.sample_optional)      // (ms_sample_optional, vibo_variant.hpp)
        return fail(-5, "null ability: not for fp32 rows gathered through row_index at fewer than 897 items");
    if (path == Path::General) return run_general(d, pl, a, num_cu);

    ElboParams p = elbo_params(d, pl, a, vec);
    if (!row_split &&            // (the row-split kernels read the item sample themselves)
        (rc = hip_rc(launch_item_prep(a.item, static_cast<float*>(a.workspace), d->num_item, d->ability_dim, pl.AT, pl.D, pl.DP, d->irt_model,
                                      a.stream), "item_prep launch")) != 0) return rc;
    CondFinTail tail;                  // the conditional posterior's last stage, launched with the ELBO finalize
    memset(&tail, 0, sizeof(tail));
    const hipError_t e = path == Path::Panels ? run_panels(d, pl, a, num_cu, p, &tail) : run_single(d, pl, path, p, a.stream);
    if (e != hipSuccess) return hip_fail(e, "elbo kernel launch");
    if (a.skip_finalize) return 0;      // the partial records stay in the workspace for vibo_train_epilogue_fused
    return run_finalize(d, pl, path, a, p.partial, tail);
}

}  // namespace vibo

using namespace vibo;

extern "C" {

int vibo_version(void) { return VIBO_ABI_VERSION; }

const char* vibo_last_error_string(void) { return last_error(); }

int vibo_plan_cond_passes(const vibo_desc* d) {
    Plan pl;
    const int rc = plan_for(d, &pl);
    return rc ? rc : plan_cond_pass_bits(pl);
}

// The kernel the plan names: resolve_path for aligned rows.  The answer depends on the descriptor alone, so it is the same for a call
// whose launch later falls back because the caller's rows are not aligned for 16-byte loads (Panels / flows -> the wave-per-person
// kernel, Split / Row -> the tiled kernel).
int vibo_plan_kernel(const vibo_desc* d) {
    Plan pl;
    const int rc = plan_for(d, &pl, true);
    return rc ? rc : plan_kernel_code(pl);
}

int vibo_selftest_lane_swaps(const float* in, float* out, void* stream) {
    if (!in || !out) return fail(-5, "null required pointer");
    return hip_rc(launch_lane_swap_selftest(in, out, (hipStream_t)stream), "lane swap selftest launch");
}

int vibo_set_insitu_timer(uint64_t* block) {
    if ((uintptr_t)block & 7) return fail(-5, "vibo_set_insitu_timer: the block must be 8-byte aligned");
    g_insitu = reinterpret_cast<unsigned long long*>(block);
    return 0;
}
int vibo_insitu_timer_reset(uint64_t* block, void* stream) {
    if (!block || ((uintptr_t)block & 7)) return fail(-5, "vibo_insitu_timer_reset: null / unaligned block");
    // words 0 (earliest entry) and 5 (shortest launch) start at all-ones, the rest at zero: two byte-fills, no kernel
    hipError_t e = hipMemsetAsync(block, 0, 8 * sizeof(uint64_t), (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(block, 0xff, sizeof(uint64_t), (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(block + 5, 0xff, sizeof(uint64_t), (hipStream_t)stream);
    return hip_rc(e, "insitu timer reset");
}

size_t vibo_workspace_bytes(const vibo_desc* d) {
    Plan pl;
    if (plan_for(d, &pl, true) != 0) return 0;
    const size_t enc = encode_scratch_bytes(d);
    return pl.total_bytes > enc ? pl.total_bytes : enc;
}

int vibo_elbo_fwd_bwd(const vibo_desc* d, const float* response, const void* mask, const int64_t* row_index,
                      const float* table, const float* item, const float* eps, const float* flow,
                      float* out_scalars, float* ability_mu, float* ability_logvar, float* ability,
                      float* ability_k, float* ability_ladj, float* grad_table, float* grad_item,
                      float* grad_flow, void* workspace, size_t workspace_bytes, void* stream) {
    return elbo_fwd_bwd_impl(d, ElboArgs{response, mask, row_index, table, item, eps, flow, out_scalars, ability_mu, ability_logvar, ability,
                                         ability_k, ability_ladj, grad_table, grad_item, grad_flow, workspace, workspace_bytes,
                                         (hipStream_t)stream});
}

int vibo_elbo_fwd_bwd_counts(const vibo_desc* d, const float* response, const void* mask, const int64_t* row_index, const int32_t* row_counts,
                             const float* table, const float* item, const float* eps, const float* flow,
                             float* out_scalars, float* ability_mu, float* ability_logvar, float* ability,
                             float* ability_k, float* ability_ladj, float* grad_table, float* grad_item,
                             float* grad_flow, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_desc(d);               // (refuses VIBO_MASK_SIGN rows)
    if (rc) return rc;
    if (!row_counts) return fail(-5, "null row_counts");
    ElboArgs a{response, mask, row_index, table, item, eps, flow, out_scalars, ability_mu, ability_logvar, ability,
               ability_k, ability_ladj, grad_table, grad_item, grad_flow, workspace, workspace_bytes, (hipStream_t)stream};
    a.row_counts = row_counts;
    return elbo_fwd_bwd_impl(d, a);
}

int vibo_sign_rows_supported(const vibo_desc* d) {
    return (d && d->mask_dtype == VIBO_MASK_SIGN && check_desc(d, true) == 0) ? 1 : 0;
}

int vibo_rows_sign_is_mask(const vibo_desc* d, const float* response, const void* mask, int32_t* differs, void* stream) {
    const int rc = check_desc(d);
    if (rc) return rc;
    if (d->mask_dtype != VIBO_MASK_U8) return fail(-8, "vibo_rows_sign_is_mask: fp32 rows with a VIBO_MASK_U8 mask");
    if (!response || !mask || !differs) return fail(-5, "null required pointer");
    return hip_rc(launch_sign_is_mask(d, response, mask, rows_vec_ok(d, response, mask), differs, (hipStream_t)stream), "rows_sign_is_mask launch");
}

int vibo_tile_rows_supported(const vibo_desc* d) {
    return (d && d->mask_dtype == VIBO_MASK_TILES && check_desc(d, true) == 0) ? 1 : 0;
}

size_t vibo_tile_rows_bytes(const vibo_desc* d) {
    if (!vibo_tile_rows_supported(d)) return 0;
    return (size_t)(((long long)d->num_person + 31) / 32) * (size_t)((d->num_item + 127) / 128) * kTileWaveBytes;
}

int vibo_tile_rows_build(const vibo_desc* src, const void* response, const void* mask, void* image, size_t image_bytes, void* stream) {
    if (!src) return fail(-1, "null descriptor");
    const int fmt = src->mask_dtype;
    vibo_desc t = *src;                      // the launches that will read the image
    t.mask_dtype = VIBO_MASK_TILES;
    const int rc = check_desc(&t, true);
    if (rc) return rc;
    if (fmt != VIBO_MASK_U8 && fmt != VIBO_MASK_NONE && fmt != VIBO_MASK_SIGN && fmt != VIBO_MASK_CODES)
        return fail(-8, "vibo_tile_rows_build: source rows as fp32 with VIBO_MASK_U8 / VIBO_MASK_NONE / VIBO_MASK_SIGN, or VIBO_MASK_CODES");
    if (!image || (fmt != VIBO_MASK_CODES && !response)) return fail(-5, "null required pointer");
    if ((fmt == VIBO_MASK_U8 || fmt == VIBO_MASK_CODES) != (mask != nullptr)) return fail(-5, "mask pointer / mask_dtype mismatch");
    if (image_bytes < vibo_tile_rows_bytes(&t)) return fail(-7, "tile image too small: %zu < %zu", image_bytes, vibo_tile_rows_bytes(&t));
    if ((uintptr_t)image & 15) return fail(-7, "the tile image must be 16-byte aligned");
    const float* resp = fmt == VIBO_MASK_CODES ? nullptr : static_cast<const float*>(response);
    return hip_rc(launch_tile_rows_build(src, resp, mask, rows_vec_ok(src, resp, mask), image, (hipStream_t)stream), "tile_rows_build launch");
}

int vibo_given_tile_rows_supported(const vibo_desc* d) {
    return (d && d->mask_dtype == VIBO_MASK_TILES && check_desc(d, false, true) == 0) ? 1 : 0;
}

// a tile image plans like the same matrix as padded rows under a u8 mask
static vibo_desc tiles_as_padded_rows(vibo_desc u) {
    u.mask_dtype = VIBO_MASK_U8;
    u.response_row_stride = u.mask_row_stride = (u.num_item + 3) & ~3;
    return u;
}

size_t vibo_given_tiles_workspace_bytes(const vibo_desc* d) {
    if (!vibo_given_tile_rows_supported(d)) return 0;
    const vibo_desc u = tiles_as_padded_rows(*d);
    return vibo_workspace_bytes(&u);
}

int vibo_elbo_fwd_bwd_given_tiles(const vibo_desc* d, const float* response, const void* mask, const int64_t* row_index,
                                  const float* table, const float* item, const float* eps, const float* flow,
                                  float* out_scalars, float* ability_mu, float* ability_logvar, float* ability,
                                  float* ability_k, float* ability_ladj, float* grad_table, float* grad_item,
                                  float* grad_flow, void* workspace, size_t workspace_bytes, void* stream) {
    if (!vibo_given_tile_rows_supported(d)) {
        const int rc = check_desc(d, false, true);      // (its code and error string; a descriptor of another format: -8)
        return rc ? rc : fail(-8, "vibo_elbo_fwd_bwd_given_tiles: a VIBO_MASK_TILES descriptor with VIBO_POSTERIOR_GIVEN only");
    }
    if (row_index) return fail(-8, "vibo_elbo_fwd_bwd_given_tiles: rows in order only (row_index must be NULL)");
    if (mask || flow || ability_k || ability_ladj || grad_flow)
        return fail(-5, "vibo_elbo_fwd_bwd_given_tiles: mask, flow, ability_k, ability_ladj and grad_flow must be NULL");
    ElboArgs a{response, nullptr, nullptr, table, item, eps, nullptr, out_scalars, ability_mu, ability_logvar, ability,
               nullptr, nullptr, grad_table, grad_item, nullptr, workspace, workspace_bytes, (hipStream_t)stream};
    a.given_tiles = true;
    return elbo_fwd_bwd_impl(d, a);
}

// The folded step's contract as the step queries ask it: none for a refused descriptor.  (VIBO_MASK_SIGN rows answer as the same rows
// under a u8 mask: row modes 0 and 3 agree on every rule of the contract.)
static StepContract step_query(const vibo_desc* d, bool rows_gathered) {
    vibo_desc u = d ? *d : vibo_desc{};      // (null: refused by the descriptor check like any zeroed descriptor)
    if (u.mask_dtype == VIBO_MASK_SIGN) u.mask_dtype = VIBO_MASK_U8;
    if (u.mask_dtype == VIBO_MASK_TILES) u = tiles_as_padded_rows(u);
    Plan pl;
    return plan_for(&u, &pl) == 0 ? step_contract(&u, pl, rows_gathered) : StepContract{};
}

int vibo_train_step_supported(const vibo_desc* d) {
    const StepContract c = step_query(d, false);
    return c.ok ? 1 | (c.fused_finalize ? 2 : 0) : 0;
}
int vibo_train_step_draws_noise(const vibo_desc* d) { return step_query(d, false).draws_noise ? 1 : 0; }
int vibo_train_step_sample_optional(const vibo_desc* d, int rows_gathered) { return step_query(d, rows_gathered != 0).sample_optional ? 1 : 0; }

int vibo_elbo_fwd_bwd_step_noise(const vibo_desc* d, int32_t* step_count, int skip_finalize, const float* response, const void* mask,
                                 const int64_t* row_index, const float* table, const float* item, const float* eps, uint64_t seed,
                                 uint32_t ability_stream_id, float* out_scalars, float* ability_mu, float* ability_logvar, float* ability,
                                 float* grad_table, float* grad_item, void* workspace, size_t workspace_bytes, void* stream) {
    if (!step_count) return fail(-5, "null step_count");
    ElboArgs a{response, mask, row_index, table, item, eps, nullptr, out_scalars, ability_mu, ability_logvar, ability,
               nullptr, nullptr, grad_table, grad_item, nullptr, workspace, workspace_bytes, (hipStream_t)stream};
    a.step_count = step_count;
    a.skip_finalize = skip_finalize;
    a.noise_seed = seed;
    a.noise_stream = ability_stream_id;
    return elbo_fwd_bwd_impl(d, a);
}

int vibo_elbo_fwd_bwd_step(const vibo_desc* d, int32_t* step_count, int skip_finalize, const float* response, const void* mask,
                           const int64_t* row_index, const float* table, const float* item, const float* eps, float* out_scalars,
                           float* ability_mu, float* ability_logvar, float* ability, float* grad_table, float* grad_item,
                           void* workspace, size_t workspace_bytes, void* stream) {
    return vibo_elbo_fwd_bwd_step_noise(d, step_count, skip_finalize, response, mask, row_index, table, item, eps, 0, 0, out_scalars,
                                        ability_mu, ability_logvar, ability, grad_table, grad_item, workspace, workspace_bytes, stream);
}

int vibo_train_epilogue_fused(const vibo_desc* d, int hidden_dim, const void* workspace, float* flat, float* saved_h,
                              float* kl_parts, float* eps_item, const float* beta, const float* lr, int32_t* step_count,
                              float* mlp_params, float* mlp_m, float* mlp_v, float* item_mu, float* item_logvar, float* item_m,
                              float* item_v, float* loss_out, uint64_t seed, float* item_feat, float* table, float* eps_ability,
                              int64_t n_eps_ability, uint32_t ability_stream_id, void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (hidden_dim < 1 || hidden_dim > kMaxHidden) return fail(-6, "hidden_dim outside 1..%d", kMaxHidden);
    if (d->posterior != VIBO_POSTERIOR_UNCONDITIONAL || d->n_flows != 0 || d->reg_mode != VIBO_REG_KL)
        return fail(-6, "vibo_train_epilogue_fused: plain model only (unconditional posterior, no flows, KL regulariser)");
    if (!flat || !saved_h || !kl_parts || !eps_item || !beta || !lr || !step_count || !mlp_params || !mlp_m || !mlp_v || !item_mu ||
        !item_logvar || !item_m || !item_v || !loss_out || !item_feat || !table || (!eps_ability && n_eps_ability != 0) || n_eps_ability < 0)
        return fail(-5, "null required pointer");
    EpiParams e;
    memset(&e, 0, sizeof(e));
    const int I = d->num_item, A = d->ability_dim, D = item_feat_dim(d->irt_model, A);
    e.H = hidden_dim; e.O = 2 * A; e.n_item_entries = I * D; e.I = I; e.D = D;
    e.flat_in = flat; e.flat_out = flat; e.saved_h = saved_h; e.kl_parts = kl_parts; e.eps_item = eps_item; e.beta = beta; e.lr = lr;
    e.step_count = step_count; e.P = mlp_params; e.M = mlp_m; e.V = mlp_v; e.mu = item_mu; e.lv = item_logvar; e.im = item_m;
    e.iv = item_v; e.loss_out = loss_out; e.item_feat = item_feat; e.table = table;
    if (workspace) {
        // the partial records vibo_elbo_fwd_bwd_step(skip_finalize) left behind: same descriptor -> same plan
        Plan pl;
        if (make_plan(d, device_cus(), &pl) < 0) return fail(-8, "no plan for this descriptor");
        if (!step_contract(d, pl, false).ok) return fail(-8, "vibo_train_epilogue_fused: the descriptor is not a vibo_elbo_fwd_bwd_step call");
        if ((rc = check_workspace(workspace, 0, 0)) != 0) return rc;      // (its size is not an argument of this call)
        e.partial = reinterpret_cast<const float*>(static_cast<const char*>(workspace) + pl.off_partial);
        e.nblk = pl.split_nblk;
        e.lay = pl.lay;
        // (the record count alone: whatever the outputs, the stand-alone finalize would sum this many in groups of 16)
        if (finalize_group(e.nblk, 1 << 30) != 64) return fail(-8, "vibo_train_epilogue_fused: %d partial records (finalize order of many small records): "
                                            "call vibo_elbo_fwd_bwd_step without skip_finalize", e.nblk);
    }
    e.seed_lo = (uint32_t)seed; e.seed_hi = (uint32_t)(seed >> 32);
    e.eps_ab = eps_ability; e.n_ab = (long long)n_eps_ability; e.ab_stream = ability_stream_id;
    e.n_item_blocks = train_epilogue_item_blocks(e.n_item_entries);
    return hip_rc(launch_train_epilogue_fused(e, (hipStream_t)stream), "train_epilogue_fused launch");
}

static size_t multi_workspace_bytes(const vibo_desc* d, int num_samples, bool given) {
    if (check_desc(d) != 0 || num_samples < 1) return 0;
    vibo_desc d0;
    Plan pl;
    size_t prep = 0;
    if (multi_plan(d, device_cus(), &d0, &pl, &prep, given) != 0) return 0;
    return pl.total_bytes + 4 * prep;
}

size_t vibo_multi_workspace_bytes(const vibo_desc* d, int num_samples) { return multi_workspace_bytes(d, num_samples, false); }

size_t vibo_multi_given_workspace_bytes(const vibo_desc* d, int num_samples) { return multi_workspace_bytes(d, num_samples, true); }

// The argument checks that the multi-sample calls share, in their one order of precedence.  plan_rc / need: what the call's plan
// answered (its refusal is reported behind the pointer, row and flow checks) and the workspace bytes it asks for.
static int multi_check_args(const vibo_desc* d, bool have_pointers, const float* response, const void* mask, const float* flow,
                            int plan_rc, size_t need, void* workspace, size_t workspace_bytes) {
    int rc;
    if (!have_pointers) return fail(-5, "null required pointer");
    if ((rc = require_rows(d, response, mask)) != 0) return rc;
    if (d->n_flows > 0 && !flow) return fail(-5, "flows need flow");
    if (plan_rc) return plan_rc;
    if ((rc = check_workspace(workspace, workspace_bytes, need)) != 0) return rc;
    if (!rows_vec_ok(d, response, mask)) return fail(-8, "multi-sample forward: rows are not 16-byte chunkable");
    return 0;
}

// both multi-sample calls: `table` is the 2-row expert table, or (given) the caller's posterior with post_sstride floats between the samples'
static int multi_forward_impl(const vibo_desc* d, bool given, int num_samples, const float* response, const void* mask,
                              const int64_t* row_index, const float* table, long long post_sstride, const float* item, const float* eps,
                              const float* flow, float* out_scalars, void* workspace, size_t workspace_bytes, void* stream) {
    const int num_cu = device_cus();
    int rc = check_desc(d);
    if (rc) return rc;
    if (num_samples < 1) return fail(-3, "num_samples must be >= 1");
    vibo_desc d0;
    Plan pl;
    size_t prep = 0;
    int plan_rc = multi_plan(d, num_cu, &d0, &pl, &prep, given);
    if (plan_rc == 0 && given && post_sstride != 0 && post_sstride != (long long)d->num_person * 2 * d->ability_dim)
        plan_rc = fail(-3, "posterior_sample_stride must be 0 (one posterior for all samples) or num_person * 2 * ability_dim");
    rc = multi_check_args(d, table && item && eps && out_scalars, response, mask, flow, plan_rc, plan_rc ? 0 : pl.total_bytes + 4 * prep,
                          workspace, workspace_bytes);
    if (rc) return rc;
    const int I = d->num_item, A = d->ability_dim;
    hipStream_t s = (hipStream_t)stream;
    char* wsb = static_cast<char*>(workspace);
    float* partial = reinterpret_cast<float*>(wsb + pl.off_partial);
    float* item_prep = reinterpret_cast<float*>(wsb + pl.total_bytes);       // up to 4 prepped tables
    const int panels = pl.panels > 0 ? pl.panels : 1;
    const int nblk = pl.split_nblk;

    MultiParams mp;
    memset(&mp, 0, sizeof(mp));
    ElboParams& p = mp.e;
    elbo_shape(p, d, pl, response, mask, row_index, table, flow);
    p.item_prep = item_prep;
    mp.item_sstride = (long long)(prep / 4);
    mp.eps_sstride = (long long)d->num_person * A;
    mp.post_sstride = given ? post_sstride : 0;
    hipError_t e = hipSuccess;
    if (pl.path == Path::Panels && !given) {   // sample-independent: whole-row counts (given: the slot lanes read the posterior themselves)
        int* cnt = reinterpret_cast<int*>(wsb + pl.off_cnt);
        e = launch_row_counts(d, num_cu, response, mask, row_index, cnt, nullptr, 0, s);
        p.row_cnt = cnt;
    }
    if (e != hipSuccess) return hip_fail(e, "multi-sample forward: pre-pass launch");
    const int sc_max = pl.AT <= 4 ? 4 : 2;
    for (int s0 = 0; s0 < num_samples;) {
        const int rem = num_samples - s0;
        const int sc = rem >= 4 && sc_max >= 4 ? 4 : rem >= 2 ? 2 : 1;
        for (int k = 0; k < sc; ++k)
            (void)launch_item_prep(item + (size_t)(s0 + k) * I * pl.D, item_prep + (size_t)k * (prep / 4), I, A, pl.AT, pl.D, pl.DP,
                                   d->irt_model, s);      // (a failed launch shows at the next check)
        p.eps = eps + (size_t)s0 * d->num_person * A;
        if (given) p.given_post = table + (size_t)s0 * post_sstride;
        for (int pn = 0; pn < panels && e == hipSuccess; ++pn) {
            const PanelSpan sp = pl.panels > 0 ? panel_span(I, pn) : PanelSpan{0, I};
            p.item0 = sp.item0; p.I = sp.items;
            p.primary = pn == 0 ? 1 : 0;
            p.partial = partial + (size_t)pn * nblk * pl.lay.stride;
            e = (given ? launch_elbo_multi_given : launch_elbo_multi)(mp, pl.AT, d->irt_model, sc, (p.I + 255) / 256, nblk, s);
        }
        if (e != hipSuccess) return hip_fail(e, "multi-sample forward launch");
        if ((rc = hip_rc(launch_multi_finalize(partial, out_scalars + (size_t)s0 * VIBO_NUM_SCALARS, panels * nblk, pl.lay.stride, sc, d->reg_mode, s),
                         "multi-sample finalize launch")) != 0) return rc;
        s0 += sc;
    }
    return 0;
}

int vibo_elbo_multi_forward(const vibo_desc* d, int num_samples, const float* response, const void* mask,
                            const int64_t* row_index, const float* table, const float* item, const float* eps,
                            const float* flow, float* out_scalars, void* workspace, size_t workspace_bytes, void* stream) {
    return multi_forward_impl(d, false, num_samples, response, mask, row_index, table, 0, item, eps, flow, out_scalars, workspace,
                              workspace_bytes, stream);
}

int vibo_elbo_multi_forward_given(const vibo_desc* d, int num_samples, const float* response, const void* mask,
                                  const int64_t* row_index, const float* posterior, int64_t posterior_sample_stride,
                                  const float* item, const float* eps, const float* flow, float* out_scalars,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    return multi_forward_impl(d, true, num_samples, response, mask, row_index, posterior, (long long)posterior_sample_stride, item, eps,
                              flow, out_scalars, workspace, workspace_bytes, stream);
}

// vibo_elbo_multi_forward_cond: the GIVEN pass's descriptor and plan, and the blocks behind that plan's own workspace
struct MultiCondPlan {
    vibo_desc dg;              // the rows as the GIVEN pass reads them: the caller's cell codes, or the ones packed into the workspace
    size_t given_bytes;        // vibo_multi_given_workspace_bytes(&dg)
    size_t off_image, off_sums, off_post, off_codes, total_bytes;
    long long codes_stride;    // 0: the caller's rows are cell codes already
    int group, ldc;            // samples per contraction pass; floats per row of the sums (group * 2A + the count)
};
static int multi_cond_plan(const vibo_desc* d, int num_samples, int num_cu, MultiCondPlan* m) {
    if (d->posterior != VIBO_POSTERIOR_CONDITIONAL)
        return fail(-3, "vibo_elbo_multi_forward_cond: the descriptor's posterior must be VIBO_POSTERIOR_CONDITIONAL");
    if (num_samples < 1) return fail(-3, "num_samples must be >= 1");
    // the shapes of VIBO_POSTERIOR_GIVEN, asked of the caller's own rows first
    vibo_desc dq = *d;
    dq.posterior = VIBO_POSTERIOR_GIVEN;
    Plan pl;
    size_t prep = 0;
    int rc = check_desc(&dq);
    if (rc == 0) rc = multi_plan(&dq, num_cu, &m->dg, &pl, &prep, true);
    if (rc) return rc;
    const int I = d->num_item, A = d->ability_dim;
    // Measured against the loop (profiles/r09_multi_cond.txt, 1M x 1k, 16 samples): fp32 rows win at 1 and 8 dims (the loop re-reads
    // 5 B per cell and sample), cell codes at 1 and 2 dims (12.8 -> 11.2 / 12.9 -> 11.9 ms); from 3 dims the loop's 16-column pass
    // per sample over the 1-byte codes beats this call's share of a 64-column pass (13.0 -> 13.8 ms at 3 dims, 13.5 -> 18.5 at 8):
    // those callers keep looping.  VIBO_FLAG_COND_MATRIX pins the stacked form (tests, A/B runs)
    if (d->mask_dtype == VIBO_MASK_CODES && A >= 3 && !(d->flags & VIBO_FLAG_COND_MATRIX))
        return fail(-8, "multi-sample forward: cell codes at ability_dim >= 3 -- one launch per sample is faster (VIBO_FLAG_COND_MATRIX pins this call)");
    m->dg = dq;
    m->codes_stride = 0;
    if (d->mask_dtype != VIBO_MASK_CODES) {      // packed once, minibatch order, rows of whole 64-byte steps
        m->codes_stride = ((long long)I + 63) / 64 * 64;
        m->dg.mask_dtype = VIBO_MASK_CODES;
        m->dg.mask_row_stride = m->codes_stride;
        m->dg.response_row_stride = 0;
        vibo_desc d0;
        if ((rc = multi_plan(&m->dg, num_cu, &d0, &pl, &prep, true)) != 0) return rc;
    }
    m->given_bytes = up256(pl.total_bytes + 4 * prep);
    m->group = cond_stack_group(A);
    m->ldc = m->group * 2 * A + 1;
    const size_t B = (size_t)d->num_person;
    size_t off = m->given_bytes;
    m->off_image = off; off += up256(cond_stack_image_bytes(I));
    m->off_sums = off;  off += up256(B * m->ldc * 4);
    m->off_post = off;  off += up256((size_t)num_samples * B * 2 * A * 4);
    m->off_codes = off; off += up256(B * (size_t)m->codes_stride);
    m->total_bytes = off;
    return 0;
}

size_t vibo_multi_cond_workspace_bytes(const vibo_desc* d, int num_samples) {
    MultiCondPlan m;
    if (check_desc(d) != 0 || multi_cond_plan(d, num_samples, device_cus(), &m) != 0) return 0;
    return m.total_bytes;
}

int vibo_elbo_multi_forward_cond(const vibo_desc* d, int num_samples, const float* response, const void* mask, const int64_t* row_index,
                                 const float* tables, const float* item, const float* eps, const float* flow, float* out_scalars,
                                 float* posterior_out, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    MultiCondPlan m;
    if ((rc = multi_cond_plan(d, num_samples, device_cus(), &m)) != 0) return rc;
    rc = multi_check_args(d, tables && item && eps && out_scalars, response, mask, flow, 0, m.total_bytes, workspace, workspace_bytes);
    if (rc) return rc;
    const int I = d->num_item, A = d->ability_dim;
    const long long B = d->num_person;
    hipStream_t s = (hipStream_t)stream;
    char* wsb = static_cast<char*>(workspace);
    float* sums = reinterpret_cast<float*>(wsb + m.off_sums);
    float* post = posterior_out ? posterior_out : reinterpret_cast<float*>(wsb + m.off_post);
    // 1. the minibatch's cell codes
    const uint8_t* codes = static_cast<const uint8_t*>(mask);
    long long stride = d->mask_row_stride;
    const int64_t* ridx = row_index;
    if (m.codes_stride) {
        uint8_t* packed = reinterpret_cast<uint8_t*>(wsb + m.off_codes);
        if ((rc = hip_rc(launch_pack_codes(d, response, mask, packed, m.codes_stride, true, s, row_index), "multi-sample forward: pack_codes launch")) != 0) return rc;
        codes = packed; stride = m.codes_stride; ridx = nullptr;
    }
    // 2.-4. per group of samples: stacked table image, one contraction pass over the codes, the per-person finish.  The first
    // group's pass leaves the rows' observed counts in the sums' last column, which no later (never wider) group writes
    const size_t n_table = (size_t)2 * I * 2 * A;
    const int cnt_col = (num_samples < m.group ? num_samples : m.group) * 2 * A;
    for (int s0 = 0; s0 < num_samples; s0 += m.group) {
        const int G = num_samples - s0 < m.group ? num_samples - s0 : m.group;
        if ((rc = hip_rc(launch_cond_stack_sums(codes, stride, ridx, B, I, A, tables + (size_t)s0 * n_table, (long long)n_table, G, s0 == 0, sums,
                                                m.ldc, wsb + m.off_image, s), "multi-sample forward: experts' sums launch")) != 0) return rc;
        if ((rc = hip_rc(launch_cond_stack_finish(sums, m.ldc, cnt_col, post + (size_t)s0 * B * 2 * A, B, I, A, G, d->missing_mode, s),
                         "multi-sample forward: posterior finish launch")) != 0) return rc;
    }
    // 5. the GIVEN multi-sample pass on the codes
    return multi_forward_impl(&m.dg, true, num_samples, nullptr, codes, ridx, post, B * 2 * A, item, eps, flow, out_scalars, workspace,
                              m.given_bytes, stream);
}

int vibo_decode_mean(const vibo_desc* d, int num_samples, const float* ability, const float* item,
                     float* response_mu_mean, void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (num_samples < 1) return fail(-3, "num_samples must be >= 1");
    if (!ability || !item || !response_mu_mean) return fail(-5, "null required pointer");
    const int A = d->ability_dim;
    if (((long long)d->num_person + 7) / 8 > 65535LL * 32768) return fail(-3, "num_person too large");
    return hip_rc(launch_decode_mean(num_samples, ability, item, response_mu_mean, d->num_person, d->num_item, A,
                                     item_feat_dim(d->irt_model, A), d->irt_model, (hipStream_t)stream), "decode_mean launch");
}

// vibo_encode's fast path: the row statistics of the row-split pipeline (16-byte row chunks at HBM speed) + a per-person finish
static hipError_t encode_fast(const vibo_desc* d, int num_cu, const float* response, const void* mask, const int64_t* row_index,
                              const float* table, float* ability_mu, float* ability_logvar, void* workspace, hipStream_t s) {
    const int I = d->num_item, A = d->ability_dim;
    const long long B = d->num_person;
    if (d->posterior != VIBO_POSTERIOR_CONDITIONAL) {
        int* cnt = static_cast<int*>(workspace);
        (void)launch_row_counts(d, num_cu, response, mask, row_index, cnt, nullptr, 0, s);      // (a failed launch shows at the next check)
        return launch_encode_finish(cnt, nullptr, 0, table, ability_mu, ability_logvar, B, I, A, d->missing_mode, s);
    }
    float* pre = static_cast<float*>(workspace);
    const int panels = panel_count(I);
    const bool mfma = encode_on_matrix_pipe(d);
    hipError_t e = hipSuccess;
    if (mfma) {
        e = launch_cond_pre_mfma(static_cast<const uint8_t*>(mask), d->mask_row_stride, row_index, d->num_person, I, A, table, pre,
                                 static_cast<char*>(workspace) + pre_block_bytes(panels, B, A), s);
    } else {
        CondParams cp = cond_params(d, response, mask, row_index, table);
        const int grid = clamp_grid(num_cu, 3, d->num_person, 8);
        for (int pn = 0; pn < panels && e == hipSuccess; ++pn) {
            const PanelSpan sp = panel_span(I, pn);
            cp.item0 = sp.item0; cp.I = sp.items;
            cp.pre_out = pre + (size_t)pn * d->num_person * (2 * A + 1);
            e = cond_pre_span(cp, nullptr, 0, grid, s);
        }
    }
    if (e != hipSuccess) return e;
    return launch_encode_finish(nullptr, pre, mfma ? 1 : panels, table, ability_mu, ability_logvar, B, I, A, d->missing_mode, s);
}

int vibo_encode(const vibo_desc* d, const float* response, const void* mask, const int64_t* row_index,
                const float* table, float* ability_mu, float* ability_logvar, void* workspace,
                size_t workspace_bytes, void* stream) {
    const int num_cu = device_cus();
    int rc = check_desc(d);
    if (rc) return rc;
    if (d->posterior == VIBO_POSTERIOR_GIVEN) return fail(-3, "vibo_encode: the posterior is the caller's own with VIBO_POSTERIOR_GIVEN");
    if (!table || !ability_mu || !ability_logvar) return fail(-5, "null required pointer");
    if ((rc = require_rows(d, response, mask)) != 0) return rc;
    const size_t need = encode_scratch_bytes(d);
    if (need > 0 && rows_vec_ok(d, response, mask) && workspace && workspace_bytes >= need && (((uintptr_t)workspace & 255) == 0)) {
        return hip_rc(encode_fast(d, num_cu, response, mask, row_index, table, ability_mu, ability_logvar, workspace, (hipStream_t)stream),
                      "encode (fast path) launch");
    }
    if (d->mask_dtype == VIBO_MASK_CODES) return codes_unsupported();      // (or the workspace is missing / too small)
    EncodeParams p;
    memset(&p, 0, sizeof(p));
    fill_rows(p, d, response, mask, row_index);
    p.table = table; p.ability_mu = ability_mu; p.ability_logvar = ability_logvar;
    p.I = d->num_item; p.missing_mode = d->missing_mode;
    p.conditional = d->posterior == VIBO_POSTERIOR_CONDITIONAL;
    return hip_rc(launch_encode(p, (hipStream_t)stream), "encode launch");
}

int vibo_row_counts(const vibo_desc* d, const float* response, const void* mask, const int64_t* row_index, int32_t* counts,
                    void* stream) {
    const int num_cu = device_cus();
    int rc = check_desc(d);
    if (rc) return rc;
    if (!counts) return fail(-5, "null required pointer");
    if ((rc = require_rows(d, response, mask)) != 0) return rc;
    if (d->num_item > 32767) return fail(-3, "vibo_row_counts: the packed counts hold up to 32767 items");
    hipStream_t s = (hipStream_t)stream;
    const bool chunks = d->num_item >= 4 && d->mask_dtype != VIBO_MASK_I64 && rows_vec_ok(d, response, mask);
    const hipError_t e = chunks ? launch_row_counts(d, num_cu, response, mask, row_index, counts, nullptr, 0, s)
                                : launch_row_counts_scalar(d, response, mask, row_index, counts, s);
    return hip_rc(e, "row_counts launch");
}

int vibo_pack_codes(const vibo_desc* d, const float* response, const void* mask, uint8_t* codes, int64_t codes_row_stride,
                    void* stream) {
    // fast path: aligned rows, 4 cells per thread (16 B of responses + 4 B of mask -> one code word)
    const bool chunks = check_desc(d) == 0 && response && codes && d->mask_dtype != VIBO_MASK_CODES && d->mask_dtype != VIBO_MASK_I64 &&
                        (d->mask_dtype == VIBO_MASK_NONE) == (mask == nullptr) && codes_row_stride % 4 == 0 &&
                        codes_row_stride >= ((d->num_item + 3) & ~3) && (((uintptr_t)codes & 3) == 0) && rows_vec_ok(d, response, mask);
    if (!chunks) {
        int rc = check_desc(d);
        if (rc) return rc;
        if (d->mask_dtype == VIBO_MASK_CODES) return fail(-3, "vibo_pack_codes: the source rows are already cell codes");
        if (!response || !codes) return fail(-5, "null required pointer");
        if ((d->mask_dtype == VIBO_MASK_NONE) != (mask == nullptr)) return fail(-5, "mask pointer / mask_dtype mismatch");
        if (codes_row_stride < d->num_item) return fail(-3, "codes_row_stride %lld < num_item", (long long)codes_row_stride);
    }
    return hip_rc(launch_pack_codes(d, response, mask, codes, (long long)codes_row_stride, chunks, (hipStream_t)stream), "pack_codes launch");
}

int vibo_decode(const vibo_desc* d, const float* ability, const float* item, float* response_mu, void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!ability || !item || !response_mu) return fail(-5, "null required pointer");
    if (d->num_person > 65535 * 1024) return fail(-3, "num_person too large for decode grid");
    const int A = d->ability_dim;
    return hip_rc(launch_decode(ability, item, response_mu, d->num_person, d->num_item, A, item_feat_dim(d->irt_model, A), d->irt_model,
                                (hipStream_t)stream), "decode launch");
}

}  // extern "C"
