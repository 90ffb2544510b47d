// vibo_dtrainer.hip -- the whole train step of an MLP-decoder model (--generative-model link | deep | residual, product-of-experts
// encoder, unconditional posterior, no flows, analytic KL) around vibo_decoder_fwd_bwd, as native kernels: what vibo_trainer.hip is
// for the IRT decoder.  Reference: vibo.py:243-268 with models.py:337-443, 596-629, 769-919.
//
//   dt_prologue_kernel     block 0: step_count[0] += 1, the 2-row encoder table (vibo_train_hook.hpp), the decoder kernel's
//                          64-wide zero-padded copies of its second / third layer; item blocks: item sample, item KL parts,
//                          3PL guess (+ optionally the Philox noise): item_prologue_block / ability_noise_block
//   dt_item_fwd_kernel     deep / residual: mlp_item_feat over the I item rows (activations kept) and U = . mlp_concat[0].weight[:, :H]^T
//   dt_person_fwd_kernel   product of experts from the packed row counts, the ability sample, mlp_ability (activations kept) and
//                          V = . mlp_concat[0].weight[:, H:]^T + bias (link: V = link[0].bias), link / residual: the IRT logit L [B][I]
//   vibo_decoder_fwd_bwd   unchanged
//   dt_person_bwd_kernel   fixed-order sum of the d V records, mlp_ability backward, d ability += d L . (-a_i), reparameterisation and
//                          KL gradients, product-of-experts backward: ONE record per workgroup
//   dt_ditem_kernel        link / residual: the item gradient from d L, one record per person slice
//   dt_reduce_kernel       fixed-order fp64 sums of every record set (one launch)
//   dt_item_bwd_kernel     deep / residual: mlp_item_feat backward from d U: one record per workgroup + d item_feat
//   dt_epilogue_kernel     block 0: loss, the 2-row encoder backward + Adam (epi_mlp_block); then Adam on every decoder parameter and
//                          the item backward + Adam (epi_item_update); step_count[1] += 1
// Every dense layer runs 64 wide on zero-padded weights (as decoder._pad_hidden states it: padded units see zero weights and a zero
// bias, elu(0) = 0, so they contribute nothing and receive no gradient), one layer at a time: the layer's weights staged in LDS
// (row stride 65: "lane j walks row j" and "lane k walks column k" are both conflict-free), 16 rows per tile, a workgroup keeps
// its tiles through all layers.  Every sum over persons / items / records has a fixed order: bitwise reproducible, no atomics.
// Minibatches above `person_chunk` persons run the person kernels and the decoder once per chunk against per-chunk record slots.
//
// The conditional posterior q(ability | responses, items) (vibo_dtrain_*_cond; models.py:695-710, utils.py:105-113) runs beside that:
//   dt_prologue_cond_kernel    the prologue without the 2-row table
//   dt_table_fwd_kernel        the encoder MLP [1 + D -> H -> H -> 2A] over the 2 I rows [c, item_feat_i] (activations kept) and the
//                              operand of the experts' contraction, feature[c][i] = tau | mu tau | 0 ... (64 columns)
//   vibo_code_table_sum_forward    [lambda | s | 0] [B][64] = one-hot(codes) [B, 2I] x feature [2I, 64] (vibo_cmean.hip)
//   dt_person_fwd_cond_kernel / dt_person_bwd_cond_kernel   the unconditional kernels' bodies with the posterior read from those
//                              sums; the backward leaves d [lambda | s] of d LL (columns 0 .. 2A) and of d KL (2A .. 4A) per person
//   vibo_code_table_sum_backward   d feature [2][I][64] (fixed-order sum over the persons)
//   dt_table_bwd_kernel        d loss = -d LL + beta d KL -> d (mu, logvar) of the table, the encoder MLP backward: one record per
//                              workgroup (summed by dt_reduce_kernel) + the gradient of the rows' inputs, whose item columns the
//                              epilogue adds to d item_feat
//   dt_epilogue_cond_kernel    block 0: the loss; Adam on the encoder parameters from the reduced records with the decoder's
// The four kernels that exist once per posterior (prologue, person forward / backward, epilogue) are one body each, a template
// over the posterior (`if constexpr (kCond)` around what only one of them needs), instantiated under both kernel names.
// The two code-table calls run ONCE per step over the whole minibatch, whatever the person chunks: they keep no per-chunk state
// (the sums of all persons are formed before the first chunk, d [lambda | s] of all persons is complete after the last).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/vibo_hip.h"
#include "../../include/vibo_hip_tile_rows.h"
#include "vibo_device.hpp"
#include "vibo_finalize.hpp"
#include "vibo_host.hpp"
#include "vibo_philox.hpp"
#include "vibo_train_hook.hpp"

namespace vibo {

constexpr int kDW = 64;             // width every dense layer runs at
constexpr int kDLd = kDW + 1;       // LDS row stride of a staged weight matrix
constexpr int kDRows = 16;          // rows per tile
constexpr int kDThreads = 256;
constexpr int kDMaxGroups = 256;    // workgroups (= records) per row kernel
constexpr int kDMaxSlices = 64;     // person slices (= records) of dt_ditem_kernel

// a Linear -> ELU -> Linear -> ELU -> Linear stack [in -> H -> H -> out] in state_dict order (offsets into the flat parameters);
// out < 0: H
struct Mlp3 {
    int w0, b0, w1, b1, w2, b2, total;
};
__host__ __device__ inline Mlp3 mlp3_at(const int base, const int in, const int H, const int out = -1) {
    Mlp3 m;
    const int O = out < 0 ? H : out;
    m.w0 = base; m.b0 = m.w0 + H * in; m.w1 = m.b0 + H; m.b1 = m.w1 + H * H; m.w2 = m.b1 + H; m.b2 = m.w2 + O * H;
    m.total = m.b2 + O - base;
    return m;
}

// The flat parameter layout (include/vibo_hip.h).  The last stack -- link, or mlp_concat -- is the per-term network the decoder
// kernel runs: first layer t0w | t0b, second t2w | t2b, third t4w | t4b.
struct DParams {
    int kind, H, A, D, enc, dec;              // dec: first decoder parameter (= encoder floats)
    Mlp3 fi, fa;                              // mlp_item_feat / mlp_ability (deep, residual)
    int t0w, t0b, t2w, t2b, t4w, t4b, total;
};
// xin: the encoder's input width, 1 (unconditional posterior) or 1 + D (conditional: the rows [c, item_feat_i])
__host__ __device__ inline DParams dparams(const int kind, const int H, const int A, const int D, const int xin = 1) {
    DParams p;
    p.kind = kind; p.H = H; p.A = A; p.D = D;
    p.enc = mlp3_at(0, xin, H, 2 * A).total;
    p.dec = p.enc;
    int o = p.enc;
    if (kind == VIBO_DECODER_LINK) {
        p.fi = mlp3_at(o, 0, 0); p.fa = p.fi;
        p.t0w = o; p.t0b = p.t0w + H;                                   // link[0]: Linear(1, H)
    } else {
        p.fi = mlp3_at(o, D, H); o += p.fi.total;
        p.fa = mlp3_at(o, A, H); o += p.fa.total;
        p.t0w = o; p.t0b = p.t0w + H * 2 * H;                           // mlp_concat[0]: Linear(2H, H)
    }
    p.t2w = p.t0b + H; p.t2b = p.t2w + H * H; p.t4w = p.t2b + H; p.t4b = p.t4w + H; p.total = p.t4b + 1;
    return p;
}

// One record of dt_person_bwd_kernel:  tab [2 sets][2][2A] | kl | vb [H] (d mlp_concat[0].bias / d link[0].bias) | mlp_ability
// in its parameter layout | wcp [H][H] (d mlp_concat[0].weight[:, H:]);  of dt_item_bwd_kernel: mlp_item_feat | wci [H][H].
struct DRec {
    int tab, kl, vb, fa, wcp, ptotal, fi, wci, itotal;
};
__host__ __device__ inline DRec drec(const DParams& p) {
    DRec r;
    r.tab = 0; r.kl = 8 * p.A; r.vb = r.kl + 1; r.fa = r.vb + p.H;
    const bool mlp = p.kind != VIBO_DECODER_LINK;
    r.wcp = r.fa + (mlp ? p.fa.total : 0);
    r.ptotal = r.wcp + (mlp ? p.H * p.H : 0);
    r.fi = 0; r.wci = mlp ? p.fi.total : 0; r.itotal = mlp ? r.wci + p.H * p.H : 0;
    return r;
}

// Scratch layout (floats; every offset a multiple of 4: the decoder kernel wants U and V 16-byte aligned)
struct DLayout {
    int B, I, A, D, H, kind, irt;
    int n_chunk, bc, dc, n_ib, n_wave, gp, gi, ns;      // chunks, persons per chunk, decoder person_chunks, ..., person / item groups, slices
    bool has_l, has_g, mlp, cond;
    int xin, gt;                                        // conditional posterior: encoder input width, table workgroups (= records)
    size_t cx, th1, th2, tout, feat, sums, dsum, dfeat, tda, tdb, tgx, trec, s_enc, ct, ct_bytes;
    size_t flat8, table, saved_h, kl_parts, w2p, b2p, w3p, w1p, b3p, guess, ih1, ih2, ihid, U, post, ability, ah1, ah2, ahid, V, L,
        dL, da, db, gab, ida, idb, gx, ll_part, dW2, dvec, dU, dguess, dV, prec, drec_item, irec, s_dW2, s_dvec, s_dU, s_dguess,
        s_p, s_ditem, total;
};
static inline size_t up4(const size_t n) { return (n + 3) & ~(size_t)3; }
// The decoder launch's person_chunks for a chunk of b persons.  Asked of the decoder unit (which reads the device's CU count) once
// per shape and thread and kept: the three calls of a step and every later step lay their records out alike without a device query.
static int decoder_chunks_for(const int b, const int I) {
    thread_local int kb = 0, ki = 0, kdc = 0;
    if (kb != b || ki != I || kdc < 1) {
        kdc = vibo_decoder_person_chunks(b, I);
        kb = b; ki = I;
    }
    return kdc < 1 ? 1 : kdc;
}
static DLayout dlayout(const vibo_desc* d, const int kind, const int H, int person_chunk) {
    DLayout y;
    memset(&y, 0, sizeof(y));
    const int B = d->num_person, I = d->num_item, A = d->ability_dim, D = item_feat_dim(d->irt_model, A);
    y.B = B; y.I = I; y.A = A; y.D = D; y.H = H; y.kind = kind; y.irt = d->irt_model;
    y.mlp = kind != VIBO_DECODER_LINK;
    y.has_l = kind != VIBO_DECODER_DEEP;
    y.has_g = y.has_l && d->irt_model == VIBO_IRT_3PL;
    if (person_chunk < 1 || person_chunk > B) person_chunk = B;
    y.n_chunk = (B + person_chunk - 1) / person_chunk;
    y.bc = (B + y.n_chunk - 1) / y.n_chunk;            // nearly equal chunks
    y.n_chunk = (B + y.bc - 1) / y.bc;
    const int b_last = B - (y.n_chunk - 1) * y.bc;
    y.dc = decoder_chunks_for(b_last, I);               // one value for every chunk: uniform record slots
    y.n_ib = (I + 63) / 64;
    y.n_wave = 4 * y.n_ib * y.dc;
    y.gp = (y.bc + kDRows - 1) / kDRows; if (y.gp > kDMaxGroups) y.gp = kDMaxGroups;
    y.gi = (I + kDRows - 1) / kDRows; if (y.gi > kDMaxGroups) y.gi = kDMaxGroups;
    y.ns = (y.bc + 63) / 64; if (y.ns > kDMaxSlices) y.ns = kDMaxSlices;
    y.cond = d->posterior == VIBO_POSTERIOR_CONDITIONAL;
    y.xin = y.cond ? 1 + D : 1;
    y.gt = (2 * I + kDRows - 1) / kDRows; if (y.gt > kDMaxGroups) y.gt = kDMaxGroups;
    const DParams p = dparams(kind, H, A, D, y.xin);
    const DRec r = drec(p);
    size_t o = 0;
    auto take = [&](size_t& field, const size_t n) { field = o; o += up4(n); };
    const size_t sB = (size_t)B, sI = (size_t)I, sbc = (size_t)y.bc, nc = (size_t)y.n_chunk;
    take(y.flat8, VIBO_NUM_SCALARS);
    take(y.table, 4 * A);
    take(y.saved_h, 4 * H);
    take(y.kl_parts, kl_part_count(I * D));
    take(y.w2p, kDW * kDW); take(y.b2p, kDW); take(y.w3p, kDW); take(y.w1p, kDW); take(y.b3p, 4);
    take(y.guess, y.has_g ? sI : 0);
    take(y.ih1, y.mlp ? sI * kDW : 0); take(y.ih2, y.mlp ? sI * kDW : 0); take(y.ihid, y.mlp ? sI * kDW : 0);
    take(y.U, y.mlp ? sI * kDW : 0);
    take(y.post, sB * 2 * A); take(y.ability, sB * A);
    take(y.ah1, y.mlp ? sB * kDW : 0); take(y.ah2, y.mlp ? sB * kDW : 0); take(y.ahid, y.mlp ? sB * kDW : 0);
    take(y.V, sB * kDW);
    take(y.L, y.has_l ? sB * sI : 0); take(y.dL, y.has_l ? sB * sI : 0);
    take(y.da, sbc * kDW); take(y.db, y.mlp ? sbc * kDW : 0); take(y.gab, y.mlp ? sbc * A : 0);
    take(y.ida, y.mlp ? sI * kDW : 0); take(y.idb, y.mlp ? sI * kDW : 0); take(y.gx, y.mlp ? sI * D : 0);
    take(y.ll_part, nc * y.n_wave); take(y.dW2, nc * y.n_wave * kDW * kDW); take(y.dvec, nc * y.n_wave * 4 * kDW);
    take(y.dU, y.mlp ? nc * y.dc * sI * kDW : 0); take(y.dguess, y.has_g ? nc * y.dc * sI : 0);
    take(y.dV, (size_t)4 * y.n_ib * sbc * kDW);
    take(y.prec, nc * y.gp * r.ptotal);
    take(y.drec_item, y.has_l ? nc * y.ns * sI * D : 0);
    take(y.irec, y.mlp ? (size_t)y.gi * r.itotal : 0);
    take(y.s_dW2, kDW * kDW); take(y.s_dvec, 4 * kDW); take(y.s_dU, y.mlp ? sI * kDW : 0); take(y.s_dguess, y.has_g ? sI : 0);
    take(y.s_p, r.ptotal); take(y.s_ditem, y.has_l ? sI * D : 0);
    if (y.cond) {                                       // (behind everything else: the unconditional layout is a prefix)
        const size_t rows = 2 * sI;
        take(y.cx, rows * y.xin); take(y.th1, rows * kDW); take(y.th2, rows * kDW); take(y.tout, rows * kDW); take(y.feat, rows * kDW);
        take(y.sums, sB * kDW); take(y.dsum, sB * kDW); take(y.dfeat, rows * kDW);
        take(y.tda, rows * kDW); take(y.tdb, rows * kDW); take(y.tgx, rows * y.xin);
        take(y.trec, (size_t)y.gt * p.enc); take(y.s_enc, p.enc);
        y.ct_bytes = vibo_code_table_scratch_bytes(B, I, kDW);
        take(y.ct, y.ct_bytes / 4 + 64);                // (the code-table calls want 256-byte alignment: found inside this slot)
    }
    y.total = o;
    return y;
}

// ---- the dense layers ----------------------------------------------------------------------------------------------------------
// Stage W [n_out][n_in] (global, row stride w_ld) into Ws [64][kDLd], zero-padded to 64 x kin.
__device__ __forceinline__ void stage_weights(float* Ws, const float* __restrict__ Wg, const int w_ld, const int n_out, const int n_in,
                                              const int kin) {
    for (int e = threadIdx.x; e < kDW * kin; e += kDThreads) {
        const int j = e / kin, k = e % kin;
        Ws[j * kDLd + k] = (j < n_out && k < n_in) ? Wg[j * w_ld + k] : 0.f;
    }
}

// out[r][j] = act(bias[j] + sum_k W[j][k] in[r][k]) over the rows of this workgroup's tiles (wg, wg + nwg, ...); out rows are 64 wide
__device__ void fwd_layer(float* Ws, float* Ts, const float* __restrict__ Wg, const int w_ld, const int n_out, const int n_in,
                          const float* __restrict__ bias, const float* in, const int in_stride, const int kin, float* out,
                          const int n_rows, const bool act, const int wg, const int nwg) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    __syncthreads();
    stage_weights(Ws, Wg, w_ld, n_out, n_in, kin);
    const float bj = (bias != nullptr && lane < n_out) ? bias[lane] : 0.f;
    for (int t = wg; t * kDRows < n_rows; t += nwg) {
        __syncthreads();
        for (int e = tid; e < kDRows * kin; e += kDThreads) {
            const int r = e / kin, k = e % kin, row = t * kDRows + r;
            Ts[r * kDW + k] = row < n_rows ? in[(size_t)row * in_stride + k] : 0.f;
        }
        __syncthreads();
        float acc[4] = {bj, bj, bj, bj};
#pragma unroll 8
        for (int k = 0; k < kin; ++k) {
            const float wv = Ws[lane * kDLd + k];
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] = fmaf(wv, Ts[(w + 4 * m) * kDW + k], acc[m]);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = t * kDRows + w + 4 * m;
            if (row < n_rows) out[(size_t)row * kDW + lane] = act ? elu(acc[m]) : acc[m];
        }
    }
}

// The backward of one layer over this workgroup's tiles.  d_out [rows][64]: the gradient at the layer's linear output; in: the
// layer's input (in_elu: an ELU's output, whose derivative multiplies the gradient handed on).  Writes d_in[row][k < kin] (row
// stride d_stride; nullptr: not wanted) and this workgroup's record d W [n_out][n_in] (row stride rw_ld) | d bias [n_out].
__device__ void bwd_layer(float* Ws, float* Tin, float* Td, const float* __restrict__ Wg, const int w_ld, const int n_out, const int n_in,
                          const float* d_out, const float* in, const int in_stride, const int kin, const bool in_elu, float* d_in,
                          const int d_stride, const int n_rows, float* rec_w, const int rw_ld, float* rec_b, const int wg,
                          const int nwg) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    __syncthreads();
    stage_weights(Ws, Wg, w_ld, n_out, n_in, kin);
    float aw[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) aw[m] = 0.f;
    float ab = 0.f;
    for (int t = wg; t * kDRows < n_rows; t += nwg) {
        __syncthreads();
        for (int e = tid; e < kDRows * kDW; e += kDThreads) {
            const int r = e >> 6, c = e & 63, row = t * kDRows + r;
            const bool ok = row < n_rows;
            Td[e] = ok ? d_out[(size_t)row * kDW + c] : 0.f;
            Tin[e] = (ok && c < kin) ? in[(size_t)row * in_stride + c] : 0.f;
        }
        __syncthreads();
        for (int r = 0; r < kDRows; ++r) {              // d W[j][k] += d_out[r][j] in[r][k]: j = w + 4 m, k = lane
            const float x = Tin[r * kDW + lane];
#pragma unroll
            for (int m = 0; m < 16; ++m) aw[m] = fmaf(Td[r * kDW + w + 4 * m], x, aw[m]);
        }
        if (tid < kDW) {
            for (int r = 0; r < kDRows; ++r) ab += Td[r * kDW + tid];
        }
        if (d_in != nullptr) {                          // d in[r][k] = sum_j d_out[r][j] W[j][k]: k = lane
            float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
            for (int j = 0; j < kDW; ++j) {
                const float wv = Ws[j * kDLd + lane];
#pragma unroll
                for (int m = 0; m < 4; ++m) s[m] = fmaf(Td[(w + 4 * m) * kDW + j], wv, s[m]);
            }
            if (lane < kin) {
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int r = w + 4 * m, row = t * kDRows + r;
                    if (row < n_rows) {
                        const float h = Tin[r * kDW + lane];
                        d_in[(size_t)row * d_stride + lane] = in_elu ? s[m] * (h > 0.f ? 1.0f : h + 1.0f) : s[m];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const int j = w + 4 * m;
        if (j < n_out && lane < n_in) rec_w[j * rw_ld + lane] = aw[m];
    }
    if (rec_b != nullptr && tid < n_out) rec_b[tid] = ab;
}

// ---- the conditional posterior's side argument -------------------------------------------------------------------------------------
// What the *_cond kernels get beside the unconditional kernels' argument: the encoder stack e [xin -> H -> H -> 2A] over the
// n = 2 I table rows and where its pieces live.
struct DCond {
    Mlp3 e;
    int H, A, I, xin, nwg;
    const float *P, *item_feat, *beta;
    float *x, *h1, *h2, *out, *feat;          // table forward: input rows [2I][xin], activations / (mu | logvar) / feature [2I][64]
    const float* sums;                        // person kernels: [lambda | s | 0] [nb][64] of this chunk
    float* dsum;                              // ... d [lambda | s] of d LL | of d KL | 0 [nb][64]
    const float* dfeat;                       // table backward: d feature [2I][64]
    float *da, *db, *gx, *rec;                // ... [2I][64] x 2, d x [2I][xin], records [nwg][e.total]
    const float* s_enc;                       // epilogue: the reduced records (d loss / d encoder parameters)
};

// ---- prologue --------------------------------------------------------------------------------------------------------------------
struct DPrologue {
    DParams p;
    int I, gen, n_item_blocks;
    const float *P, *mu, *lv, *eps;
    float *eps_w, *item_feat, *table, *saved_h, *kl_parts, *w2p, *b2p, *w3p, *w1p, *b3p, *guess, *eps_ab;
    int32_t* step_count;
    uint32_t seed_lo, seed_hi, ab_stream;
    long long n_ab;
};

// ---- item side -------------------------------------------------------------------------------------------------------------------
struct DItem {
    DParams p;
    int I, nwg;
    const float* P;
    const float* item_feat;
    float *h1, *h2, *hid, *U;
    // backward
    const float* s_dU;
    float *da, *db, *gx, *rec;
    int rec_stride, r_fi, r_wci;
};
__global__ __launch_bounds__(kDThreads) void dt_item_fwd_kernel(const DItem a) {
    __shared__ float Ws[kDW * kDLd], Ts[kDRows * kDW];
    const DParams& p = a.p;
    const int H = p.H, wg = blockIdx.x;
    fwd_layer(Ws, Ts, a.P + p.fi.w0, p.D, H, p.D, a.P + p.fi.b0, a.item_feat, p.D, p.D, a.h1, a.I, true, wg, a.nwg);
    fwd_layer(Ws, Ts, a.P + p.fi.w1, H, H, H, a.P + p.fi.b1, a.h1, kDW, kDW, a.h2, a.I, true, wg, a.nwg);
    fwd_layer(Ws, Ts, a.P + p.fi.w2, H, H, H, a.P + p.fi.b2, a.h2, kDW, kDW, a.hid, a.I, false, wg, a.nwg);
    fwd_layer(Ws, Ts, a.P + p.t0w, 2 * H, H, H, nullptr, a.hid, kDW, kDW, a.U, a.I, false, wg, a.nwg);
}
__global__ __launch_bounds__(kDThreads) void dt_item_bwd_kernel(const DItem a) {
    __shared__ float Ws[kDW * kDLd], Tin[kDRows * kDW], Td[kDRows * kDW];
    const DParams& p = a.p;
    const int H = p.H, wg = blockIdx.x;
    float* rec = a.rec + (size_t)wg * a.rec_stride;
    float* rf = rec + a.r_fi - p.fi.w0;               // (mlp_item_feat in its parameter layout)
    bwd_layer(Ws, Tin, Td, a.P + p.t0w, 2 * H, H, H, a.s_dU, a.hid, kDW, kDW, false, a.da, kDW, a.I, rec + a.r_wci, H, nullptr, wg, a.nwg);
    bwd_layer(Ws, Tin, Td, a.P + p.fi.w2, H, H, H, a.da, a.h2, kDW, kDW, true, a.db, kDW, a.I, rf + p.fi.w2, H, rf + p.fi.b2, wg, a.nwg);
    bwd_layer(Ws, Tin, Td, a.P + p.fi.w1, H, H, H, a.db, a.h1, kDW, kDW, true, a.da, kDW, a.I, rf + p.fi.w1, H, rf + p.fi.b1, wg, a.nwg);
    bwd_layer(Ws, Tin, Td, a.P + p.fi.w0, p.D, H, p.D, a.da, a.item_feat, p.D, p.D, false, a.gx, p.D, a.I, rf + p.fi.w0, p.D, rf + p.fi.b0, wg,
              a.nwg);
}

// ---- person side -----------------------------------------------------------------------------------------------------------------
struct DPerson {
    DParams p;
    int I, irt, nb, nwg, prior, n_dv;         // nb: persons of this chunk; n_dv: d V records (4 ceil(I / 64))
    const float* P;
    const int32_t* counts;
    const float *table, *eps, *item_feat;
    float *post, *ability, *h1, *h2, *hid, *V, *L;
    // backward
    const float *dV, *dL;
    float *da, *db, *gab, *rec;
    int rec_stride, r_tab, r_kl, r_vb, r_fa, r_wcp;
};

// the product of experts of person row `c` (packed counts), dimension a: models._posterior_from_counts
struct Poe {
    float n0, n1, tau0, tau1, m0, m1, e0, e1, lam, smu;
};
__device__ __forceinline__ Poe poe_forward(const int c, const float* __restrict__ table, const int A, const int a, const int I,
                                           const int prior) {
    Poe q;
    const float nobs = (float)(c & 0xffff);
    q.n1 = (float)(c >> 16);
    q.n0 = nobs - q.n1;
    q.m0 = table[a]; q.m1 = table[2 * A + a];
    q.e0 = expf(table[A + a]); q.e1 = expf(table[3 * A + a]);
    q.tau0 = 1.0f / (q.e0 + kPoeEps);
    q.tau1 = 1.0f / (q.e1 + kPoeEps);
    q.lam = fmaf(q.n1, q.tau1, q.n0 * q.tau0);
    q.smu = fmaf(q.n1, q.m1 * q.tau1, q.n0 * (q.m0 * q.tau0));
    if (prior) q.lam += ((float)I - nobs) * (1.0f / (1.0f + kPoeEps));
    return q;
}


// the conditional product of experts of person row `row`, dimension a, from the experts' sums: lambda (with the prior experts of
// the missing cells) and s  (models._conditional_posterior_poe); the per-code fields stay unset
__device__ __forceinline__ Poe cpoe_forward(const DCond& c, const int row, const int a, const int count, const int I, const int prior) {
    Poe q;
    q.lam = c.sums[(size_t)row * kDW + a];
    q.smu = c.sums[(size_t)row * kDW + c.A + a];
    if (prior) q.lam += ((float)I - (float)(count & 0xffff)) * (1.0f / (1.0f + kPoeEps));
    return q;
}

// ---- the conditional posterior's expert table ---------------------------------------------------------------------------------
// row = c I + i of the 2 I table rows: input [c, item_feat_i] -> (mu | logvar) [2A] -> feature = tau | mu tau | 0 ... [64],
// tau = 1 / (exp(logvar) + 1e-8)  (utils.py:105-113)
__global__ __launch_bounds__(kDThreads) void dt_table_fwd_kernel(const DCond c) {
    __shared__ float Ws[kDW * kDLd], Ts[kDRows * kDW];
    const int tid = threadIdx.x, wg = blockIdx.x;
    const int H = c.H, A = c.A, I = c.I, xin = c.xin, n = 2 * c.I;
    for (int t = wg; t * kDRows < n; t += c.nwg) {
        for (int e = tid; e < kDRows * xin; e += kDThreads) {
            const int row = t * kDRows + e / xin, k = e % xin;
            if (row >= n) continue;
            const int cc = row >= I ? 1 : 0, i = row - cc * I;
            c.x[(size_t)row * xin + k] = k == 0 ? (float)cc : c.item_feat[(size_t)i * (xin - 1) + (k - 1)];
        }
    }
    // (fwd_layer starts with a barrier: this workgroup's input rows are visible to all of its threads)
    fwd_layer(Ws, Ts, c.P + c.e.w0, xin, H, xin, c.P + c.e.b0, c.x, xin, xin, c.h1, n, true, wg, c.nwg);
    fwd_layer(Ws, Ts, c.P + c.e.w1, H, H, H, c.P + c.e.b1, c.h1, kDW, kDW, c.h2, n, true, wg, c.nwg);
    fwd_layer(Ws, Ts, c.P + c.e.w2, H, 2 * A, H, c.P + c.e.b2, c.h2, kDW, kDW, c.out, n, false, wg, c.nwg);
    __syncthreads();
    for (int t = wg; t * kDRows < n; t += c.nwg) {
        for (int e = tid; e < kDRows * kDW; e += kDThreads) {
            const int row = t * kDRows + (e >> 6), j = e & 63;
            if (row >= n) continue;
            float v = 0.f;
            if (j < 2 * A) {
                const int q = j < A ? j : j - A;
                const float tau = 1.0f / (expf(c.out[(size_t)row * kDW + A + q]) + kPoeEps);
                v = j < A ? tau : c.out[(size_t)row * kDW + q] * tau;
            }
            c.feat[(size_t)row * kDW + j] = v;
        }
    }
}
// d feature [2I][64] (columns 0 .. 2A: of d LL, 2A .. 4A: of d KL) -> d loss / d (mu | logvar) of the table -> the encoder MLP
// backward: this workgroup's record in the encoder's parameter layout, and d x [2I][xin]
__global__ __launch_bounds__(kDThreads) void dt_table_bwd_kernel(const DCond c) {
    __shared__ float Ws[kDW * kDLd], Tin[kDRows * kDW], Td[kDRows * kDW];
    const int tid = threadIdx.x, wg = blockIdx.x;
    const int H = c.H, A = c.A, xin = c.xin, n = 2 * c.I;
    const float beta = *c.beta;
    for (int t = wg; t * kDRows < n; t += c.nwg) {
        for (int e = tid; e < kDRows * kDW; e += kDThreads) {
            const int row = t * kDRows + (e >> 6), j = e & 63;
            if (row >= n) continue;
            float v = 0.f;
            if (j < 2 * A) {
                const int q = j < A ? j : j - A;
                const float* g = c.dfeat + (size_t)row * kDW;
                const float gt = fmaf(beta, g[2 * A + q], -g[q]);              // d loss / d tau
                const float gm = fmaf(beta, g[3 * A + q], -g[A + q]);          // d loss / d (mu tau)
                const float mu = c.out[(size_t)row * kDW + q], ev = expf(c.out[(size_t)row * kDW + A + q]);
                const float tau = 1.0f / (ev + kPoeEps);
                v = j < A ? gm * tau : fmaf(gm, mu, gt) * (-ev * tau * tau);
            }
            c.da[(size_t)row * kDW + j] = v;
        }
    }
    float* rec = c.rec + (size_t)wg * c.e.total;
    bwd_layer(Ws, Tin, Td, c.P + c.e.w2, H, 2 * A, H, c.da, c.h2, kDW, kDW, true, c.db, kDW, n, rec + c.e.w2, H, rec + c.e.b2, wg, c.nwg);
    bwd_layer(Ws, Tin, Td, c.P + c.e.w1, H, H, H, c.db, c.h1, kDW, kDW, true, c.da, kDW, n, rec + c.e.w1, H, rec + c.e.b1, wg, c.nwg);
    bwd_layer(Ws, Tin, Td, c.P + c.e.w0, xin, H, xin, c.da, c.x, xin, xin, false, c.gx, xin, n, rec + c.e.w0, xin, rec + c.e.b0, wg, c.nwg);
}

// link / residual: d LL / d item_feat through the IRT logit, one record per person slice (grid: entries / 256 x slices)
__global__ __launch_bounds__(256) void dt_ditem_kernel(int I, int A, int D, int irt, int nb, int per_slice, const float* __restrict__ dL,
                                                       const float* __restrict__ ability, float* __restrict__ rec) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= I * D) return;
    const int i = idx / D, q = idx % D;
    const int p0 = blockIdx.y * per_slice, p1 = min(nb, p0 + per_slice);
    float s = 0.f;
    if (irt == VIBO_IRT_1PL || q == A) {
        for (int pp = p0; pp < p1; ++pp) s += dL[(size_t)pp * I + i];
    } else if (q < A) {
        for (int pp = p0; pp < p1; ++pp) s = fmaf(dL[(size_t)pp * I + i], -ability[(size_t)pp * A + q], s);
    }
    rec[(size_t)blockIdx.y * I * D + idx] = s;
}

// ---- record sums -----------------------------------------------------------------------------------------------------------------
constexpr int kDSegs = 9;
struct DSeg {
    const float* src;
    float* dst;
    int n_rec, n_out, blk0;
    size_t stride;
};
struct DReduce {
    DSeg s[kDSegs];
    int n;
};
// dst[e] = sum over the records of src[r * stride + e], fixed order (16 slices, fp64): 64 outputs per workgroup
__global__ __launch_bounds__(1024) void dt_reduce_kernel(const DReduce a) {
    __shared__ double sl[16][64];
    int k = 0;
    for (int q = 1; q < a.n; ++q)
        if ((int)blockIdx.x >= a.s[q].blk0) k = q;
    const DSeg& g = a.s[k];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int e = ((int)blockIdx.x - g.blk0) * 64 + lane;
    sl[slice][lane] = e < g.n_out ? record_slice_sum<16>(g.src, g.stride, e, 0, g.n_rec, slice) : 0.0;
    __syncthreads();
    if (slice == 0 && e < g.n_out) {
        double t = 0.0;
#pragma unroll
        for (int s = 0; s < 16; ++s) t += sl[s][lane];
        g.dst[e] = (float)t;
    }
}

// ---- epilogue --------------------------------------------------------------------------------------------------------------------
struct DEpilogue {
    DParams p;
    DRec r;
    int I, n_item_entries, n_dec_blocks, n_irec, has_l, has_g;
    const float *flat8, *s_p, *s_dW2, *s_dvec, *s_ditem, *s_dguess, *guess, *gx, *irec, *saved_h, *kl_parts, *eps, *beta, *lr;
    int32_t* step_count;
    float *P, *M, *V, *mu, *lv, *im, *iv, *loss;
};

// ---- the four kernels that exist once per posterior -------------------------------------------------------------------------------
// prologue, person forward / backward, epilogue: each body is written once as <kCond>, and dt_*_kernel (unconditional posterior) /
// dt_*_cond_kernel (conditional) behind the bodies are its two instantiations under their own names.  c: the conditional
// posterior's side argument, nullptr in the unconditional kernels, which never read it.
template <bool kCond>
__device__ __forceinline__ void prologue_body(const DPrologue& a) {
    const int tid = threadIdx.x;
    const DParams& p = a.p;
    if (blockIdx.x == 0) {
        if (tid == 0) a.step_count[0] += 1;
        const int H = p.H;
        if constexpr (!kCond) {                       // the 2-row encoder table (conditional: 2 I rows, dt_table_fwd_kernel)
            __shared__ float h1[2 * kDW], h2[2 * kDW];
            const int O = 2 * p.A;
            const MlpOffsets o = mlp_offsets(H, O);
            mlp2_layer0(a.P, o, H, O, h1, tid, kDThreads);
            __syncthreads();
            mlp2_layer1(a.P, o, H, O, h1, h2, tid, kDThreads);
            __syncthreads();
            mlp2_layer2(a.P, o, H, O, h1, h2, tid, kDThreads, a.table, a.saved_h);
        }
        // the per-term network's second and third layer, 64 wide (decoder._pad_hidden)
        for (int e = tid; e < kDW * kDW; e += kDThreads) {
            const int j = e >> 6, k = e & 63;
            a.w2p[e] = (j < H && k < H) ? a.P[p.t2w + j * H + k] : 0.f;
        }
        if (tid < kDW) {
            const bool in = tid < H;
            a.b2p[tid] = in ? a.P[p.t2b + tid] : 0.f;
            a.w3p[tid] = in ? a.P[p.t4w + tid] : 0.f;
            a.w1p[tid] = (in && p.kind == VIBO_DECODER_LINK) ? a.P[p.t0w + tid] : 0.f;
            if (tid == 0) a.b3p[0] = a.P[p.t4b];
        }
        return;
    }
    if ((int)blockIdx.x > a.n_item_blocks) {          // ability noise (stream ab_stream)
        ability_noise_block(blockIdx.x - 1 - a.n_item_blocks, kDThreads, tid, a.eps_ab, a.n_ab, (uint32_t)a.step_count[1], a.ab_stream,
                            a.seed_lo, a.seed_hi);
        return;
    }
    item_prologue_block(blockIdx.x - 1, tid, a.I, p.D, a.mu, a.lv, a.eps, a.eps_w, a.gen, a.step_count + 1, a.seed_lo, a.seed_hi,
                        a.item_feat, a.kl_parts);
    if (a.guess != nullptr) {                         // 3PL: guess = sigmoid(item_feat[:, A + 1]) (this thread's own store)
        const int k = (blockIdx.x - 1) * 256 + tid;
        if (k < a.I * p.D) {
            const int idx = item_entry_index(k, a.I, p.D);
            if (idx % p.D == p.A + 1) a.guess[idx / p.D] = 1.0f / (1.0f + expf(-a.item_feat[idx]));
        }
    }
}

// the product of experts of person `row` of the chunk, dimension a16: from the 2-row table, or from the conditional experts' sums
template <bool kCond>
__device__ __forceinline__ Poe person_poe(const DPerson& a, const DCond* c, const int row, const int a16) {
    if constexpr (kCond) return cpoe_forward(*c, row, a16, a.counts[row], a.I, a.prior);
    else return poe_forward(a.counts[row], a.table, a.p.A, a16, a.I, a.prior);
}

template <bool kCond>
__device__ __forceinline__ void person_fwd_body(const DPerson& a, const DCond* c) {
    __shared__ float Ws[kDW * kDLd], Ts[kDRows * kDW];
    const DParams& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int H = p.H, A = p.A, D = p.D, I = a.I, wg = blockIdx.x;
    const int r16 = tid >> 4, a16 = tid & 15;
    for (int t = wg; t * kDRows < a.nb; t += a.nwg) {
        const int row = t * kDRows + r16;
        if (row < a.nb && a16 < A) {
            const Poe q = person_poe<kCond>(a, c, row, a16);
            const float mu = q.smu / q.lam, lv = logf(1.0f / q.lam);
            a.post[(size_t)row * 2 * A + a16] = mu;
            a.post[(size_t)row * 2 * A + A + a16] = lv;
            a.ability[(size_t)row * A + a16] = fmaf(expf(0.5f * lv), a.eps[(size_t)row * A + a16], mu);
        }
    }
    if (p.kind == VIBO_DECODER_LINK) {
        for (int t = wg; t * kDRows < a.nb; t += a.nwg) {
            for (int e = tid; e < kDRows * kDW; e += kDThreads) {
                const int row = t * kDRows + (e >> 6), j = e & 63;
                if (row < a.nb) a.V[(size_t)row * kDW + j] = j < H ? a.P[p.t0b + j] : 0.f;
            }
        }
    } else {
        // (fwd_layer starts with a barrier: this workgroup's ability rows are visible to all of its threads)
        fwd_layer(Ws, Ts, a.P + p.fa.w0, A, H, A, a.P + p.fa.b0, a.ability, A, A, a.h1, a.nb, true, wg, a.nwg);
        fwd_layer(Ws, Ts, a.P + p.fa.w1, H, H, H, a.P + p.fa.b1, a.h1, kDW, kDW, a.h2, a.nb, true, wg, a.nwg);
        fwd_layer(Ws, Ts, a.P + p.fa.w2, H, H, H, a.P + p.fa.b2, a.h2, kDW, kDW, a.hid, a.nb, false, wg, a.nwg);
        fwd_layer(Ws, Ts, a.P + p.t0w + H, 2 * H, H, H, a.P + p.t0b, a.hid, kDW, kDW, a.V, a.nb, false, wg, a.nwg);
    }
    if (a.L != nullptr) {                             // decoder.irt_logit: a wave per row, lanes over the items
        __syncthreads();
        for (int t = wg; t * kDRows < a.nb; t += a.nwg) {
            for (int rr = 0; rr < 4; ++rr) {
                const int row = t * kDRows + 4 * w + rr;
                if (row >= a.nb) continue;
                const float* ab = a.ability + (size_t)row * A;
                for (int i = lane; i < I; i += 64) {
                    float s;
                    if (a.irt == VIBO_IRT_1PL) {
                        s = 0.f;
                        for (int q = 0; q < A; ++q) s += ab[q];
                        s += a.item_feat[i];
                    } else {
                        s = 0.f;
                        for (int q = 0; q < A; ++q) s = fmaf(ab[q], -a.item_feat[(size_t)i * D + q], s);
                        s += a.item_feat[(size_t)i * D + A];
                    }
                    a.L[(size_t)row * I + i] = s;
                }
            }
        }
    }
}

template <bool kCond>
__device__ __forceinline__ void person_bwd_body(const DPerson& a, const DCond* c) {
    __shared__ float Ws[kDW * kDLd], Tin[kDRows * kDW], Td[kDRows * kDW];
    __shared__ float gl[kDRows * 16], wsum[4];
    const DParams& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int H = p.H, A = p.A, D = p.D, I = a.I, wg = blockIdx.x;
    float* rec = a.rec + (size_t)wg * a.rec_stride;
    // d LL / d V = the fixed-order sum of the decoder kernel's records
    float vb = 0.f;                                   // link: d link[0].bias = sum over the persons (column tid & 63, rows w, w + 4, ...)
    for (int t = wg; t * kDRows < a.nb; t += a.nwg) {
        for (int e = tid; e < kDRows * kDW; e += kDThreads) {
            const int row = t * kDRows + (e >> 6), j = e & 63;
            if (row >= a.nb) continue;
            float s = 0.f;
            for (int k = 0; k < a.n_dv; ++k) s += a.dV[((size_t)k * a.nb + row) * kDW + j];
            a.da[(size_t)row * kDW + j] = s;
            vb += s;
        }
    }
    if (p.kind == VIBO_DECODER_LINK) {
        __syncthreads();
        Td[tid] = vb;
        __syncthreads();
        if (tid < H) rec[a.r_vb + tid] = (Td[tid] + Td[64 + tid]) + (Td[128 + tid] + Td[192 + tid]);
    } else {
        float* rf = rec + a.r_fa - p.fa.w0;           // (mlp_ability in its parameter layout)
        bwd_layer(Ws, Tin, Td, a.P + p.t0w + H, 2 * H, H, H, a.da, a.hid, kDW, kDW, false, a.db, kDW, a.nb, rec + a.r_wcp, H, rec + a.r_vb, wg,
                  a.nwg);
        bwd_layer(Ws, Tin, Td, a.P + p.fa.w2, H, H, H, a.db, a.h2, kDW, kDW, true, a.da, kDW, a.nb, rf + p.fa.w2, H, rf + p.fa.b2, wg, a.nwg);
        bwd_layer(Ws, Tin, Td, a.P + p.fa.w1, H, H, H, a.da, a.h1, kDW, kDW, true, a.db, kDW, a.nb, rf + p.fa.w1, H, rf + p.fa.b1, wg, a.nwg);
        bwd_layer(Ws, Tin, Td, a.P + p.fa.w0, A, H, A, a.db, a.ability, A, A, false, a.gab, A, a.nb, rf + p.fa.w0, A, rf + p.fa.b0, wg, a.nwg);
    }
    // d LL / d ability -> (mu, logvar) -> the 2-row table; KL and its gradient.  Thread (r16, a16) = (row of the tile, dimension).
    const int r16 = tid >> 4, a16 = tid & 15;
    float tg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // [set][c][mu | logvar] of dimension a16
    float kl = 0.f;
    for (int t = wg; t * kDRows < a.nb; t += a.nwg) {
        __syncthreads();
        if constexpr (kCond) {
            for (int e = tid; e < kDRows * kDW; e += kDThreads) {  // the columns of d [lambda | s] no dimension writes
                const int row = t * kDRows + (e >> 6), j = e & 63;
                if (row < a.nb && j >= 4 * A) c->dsum[(size_t)row * kDW + j] = 0.f;
            }
        }
        if (a.dL != nullptr) {                        // gl[r][q] = sum_i d L[row][i] (-item[i][q]): a wave per row, lanes over the items
            for (int rr = 0; rr < 4; ++rr) {
                const int r = 4 * w + rr, row = t * kDRows + r;
                float acc[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] = 0.f;
                if (row < a.nb) {
                    for (int i = lane; i < I; i += 64) {
                        const float g = a.dL[(size_t)row * I + i];
                        if (a.irt == VIBO_IRT_1PL) {
                            acc[0] += g;
                        } else {
#pragma unroll
                            for (int q = 0; q < 16; ++q)
                                if (q < A) acc[q] = fmaf(g, -a.item_feat[(size_t)i * D + q], acc[q]);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    if (q < A) {
                        const float s = wave_total(acc[a.irt == VIBO_IRT_1PL ? 0 : q]);
                        if (lane == 0) gl[r * 16 + q] = s;
                    }
                }
            }
        }
        __syncthreads();
        const int row = t * kDRows + r16;
        if (row < a.nb && a16 < A) {
            float g = p.kind == VIBO_DECODER_LINK ? 0.f : a.gab[(size_t)row * A + a16];
            if (a.dL != nullptr) g += gl[r16 * 16 + a16];
            const Poe q = person_poe<kCond>(a, c, row, a16);
            const float mu = a.post[(size_t)row * 2 * A + a16], lv = a.post[(size_t)row * 2 * A + A + a16];
            const float var = expf(lv);
            kl += -0.5f * (1.0f + lv - mu * mu - var);
            const float inv = 1.0f / q.lam;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                // set 0: d LL through the sample; set 1: d KL
                const float dmu = s == 0 ? g : mu;
                const float dlv = s == 0 ? g * a.eps[(size_t)row * A + a16] * (0.5f * expf(0.5f * lv)) : 0.5f * (var - 1.0f);
                const float dsmu = dmu * inv;
                const float dlam = -fmaf(dmu, mu, dlv) * inv;
                if constexpr (kCond) {
                    // mu = s / lambda, logvar = -log lambda: the table comes behind the sums (tg stays 0)
                    c->dsum[(size_t)row * kDW + 2 * A * s + a16] = dlam;
                    c->dsum[(size_t)row * kDW + 2 * A * s + A + a16] = dsmu;
                } else {
                    tg[4 * s + 0] += q.n0 * q.tau0 * dsmu;
                    tg[4 * s + 1] += q.n0 * fmaf(dsmu, q.m0, dlam) * (-q.e0 * q.tau0 * q.tau0);
                    tg[4 * s + 2] += q.n1 * q.tau1 * dsmu;
                    tg[4 * s + 3] += q.n1 * fmaf(dsmu, q.m1, dlam) * (-q.e1 * q.tau1 * q.tau1);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 8; ++v) Ws[tid * 8 + v] = tg[v];
    kl = wave_total(kl);
    if (lane == 0) wsum[w] = kl;
    __syncthreads();
    if (tid < 8 * A) {
        const int v = tid / A, q = tid % A;
        float s = 0.f;
        for (int r = 0; r < kDRows; ++r) s += Ws[(r * 16 + q) * 8 + v];
        // v = 4 set + 2 c + part -> grad_table layout [set][c][part A + q]
        rec[a.r_tab + (v >> 2) * 4 * A + ((v >> 1) & 1) * 2 * A + (v & 1) * A + q] = s;
    }
    if (tid == 0) rec[a.r_kl] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

template <bool kCond>
__device__ __forceinline__ void epilogue_body(const DEpilogue& a, const DCond* c) {
    const int tid = threadIdx.x;
    const DParams& p = a.p;
    const DRec& r = a.r;
    const float beta = *a.beta, lr = *a.lr;
    const AdamBias bc = adam_bias(a.step_count[0]);
    constexpr int BS = kEpiThreads;
    const int H = p.H;
    if (blockIdx.x == 0) {
        if (tid == 0) a.step_count[1] += 1;           // completed steps: the noise counter of the NEXT step
        if constexpr (kCond) {
            // the loss; the encoder's gradient is the reduced table records (c->s_enc), applied by the parameter blocks below
            item_kl_loss(tid, a.kl_parts, kl_part_count(a.n_item_entries), a.flat8, beta, a.loss);
        } else {
            // the 2-row encoder: sc = [LL, KL_ability, ...], gtab = d LL / d table then d KL / d table (the person records' sums)
            __shared__ EpiLds L;
            float pv[kEpiU], mv[kEpiU], vv[kEpiU];
            const MlpOffsets o = mlp_offsets(H, 2 * p.A);
            epi_mlp_prefetch(o.total, a.P, a.M, a.V, pv, mv, vv, tid);
            if (H == 64) epi_mlp_block<64>(L, H, 2 * p.A, kl_part_count(a.n_item_entries), a.flat8, a.s_p + r.tab, a.saved_h, a.kl_parts, beta, lr,
                                           bc, a.P, o, nullptr, a.P, a.M, a.V, pv, mv, vv, a.loss, tid);
            else epi_mlp_block<0>(L, H, 2 * p.A, kl_part_count(a.n_item_entries), a.flat8, a.s_p + r.tab, a.saved_h, a.kl_parts, beta, lr, bc,
                                  a.P, o, nullptr, a.P, a.M, a.V, pv, mv, vv, a.loss, tid);
        }
        return;
    }
    if ((int)blockIdx.x <= a.n_dec_blocks) {          // Adam on the decoder parameters (conditional: the encoder's too): d loss = -d LL
        const int k = (kCond ? 0 : p.dec) + ((int)blockIdx.x - 1) * BS + tid;
        if (k >= p.total) return;
        float g;
        if (kCond && k < p.enc) {
            g = -c->s_enc[k];                         // (records of d loss: adam_update below takes -g)
        } else if (k >= p.t2w) {                      // the per-term network's second and third layer: the decoder kernel's records
            if (k < p.t2b) {
                const int e = k - p.t2w;
                g = a.s_dW2[(e / H) * kDW + e % H];
            } else if (k < p.t4w) {
                g = a.s_dvec[k - p.t2b];
            } else if (k < p.t4b) {
                g = a.s_dvec[kDW + (k - p.t4w)];
            } else {
                g = a.s_dvec[3 * kDW];
            }
        } else if (p.kind == VIBO_DECODER_LINK) {
            g = k < p.t0b ? a.s_dvec[2 * kDW + (k - p.t0w)] : a.s_p[r.vb + (k - p.t0b)];
        } else if (k >= p.t0b) {
            g = a.s_p[r.vb + (k - p.t0b)];
        } else if (k >= p.fa.w0 && k < p.t0w) {
            g = a.s_p[r.fa + (k - p.fa.w0)];
        } else {
            // mlp_item_feat, or the item half of mlp_concat[0].weight: the item workgroups' records, in order
            int e;
            if (k < p.fa.w0) {
                e = r.fi + (k - p.fi.w0);
            } else {
                const int j = (k - p.t0w) / (2 * H), col = (k - p.t0w) % (2 * H);
                e = col < H ? r.wci + j * H + col : -1;
                if (e < 0) g = a.s_p[r.wcp + j * H + (col - H)];
            }
            if (e >= 0) {
                g = 0.f;
                for (int q = 0; q < a.n_irec; ++q) g += a.irec[(size_t)q * r.itotal + e];
            }
        }
        float pv = a.P[k], mv = a.M[k], vv = a.V[k];
        adam_update(pv, mv, vv, -g, lr, bc);
        a.P[k] = pv; a.M[k] = mv; a.V[k] = vv;
        return;
    }
    const int idx = ((int)blockIdx.x - 1 - a.n_dec_blocks) * BS + tid;
    if (idx < a.n_item_entries) {                     // d loss / d item_feat = -d LL / d item_feat
        float g = 0.f;
        if (a.has_l) g += a.s_ditem[idx];
        if (a.gx != nullptr) g += a.gx[idx];
        if (a.has_g && idx % p.D == p.A + 1) {
            const float gs = a.guess[idx / p.D];
            g += a.s_dguess[idx / p.D] * gs * (1.0f - gs);
        }
        if constexpr (kCond) {                        // the encoder reads the item sample: rows (0, i) and (1, i) of the table
            const int i = idx / p.D, q = idx % p.D, xin = p.D + 1;
            g -= c->gx[(size_t)i * xin + 1 + q] + c->gx[(size_t)(a.I + i) * xin + 1 + q];
        }
        float pm, pl;
        epi_item_update(idx, a.n_item_entries, -g, a.eps[idx], beta, lr, bc, a.mu, a.lv, a.im, a.iv, pm, pl);
    }
}

// The eight kernels: the unconditional posterior's four, then the conditional one's.  The code object keeps this order, and a step's
// kernels next to each other are worth 1 % of the 16-person step against each pair behind its body (profiles/r07_decoder_train_step.txt).
__global__ __launch_bounds__(kDThreads) void dt_prologue_kernel(const DPrologue a) { prologue_body<false>(a); }
__global__ __launch_bounds__(kDThreads) void dt_person_fwd_kernel(const DPerson a) { person_fwd_body<false>(a, nullptr); }
__global__ __launch_bounds__(kDThreads) void dt_person_bwd_kernel(const DPerson a) { person_bwd_body<false>(a, nullptr); }
__global__ __launch_bounds__(kEpiThreads) void dt_epilogue_kernel(const DEpilogue a) { epilogue_body<false>(a, nullptr); }
__global__ __launch_bounds__(kDThreads) void dt_prologue_cond_kernel(const DPrologue a) { prologue_body<true>(a); }
__global__ __launch_bounds__(kDThreads) void dt_person_fwd_cond_kernel(const DPerson a, const DCond c) { person_fwd_body<true>(a, &c); }
__global__ __launch_bounds__(kDThreads) void dt_person_bwd_cond_kernel(const DPerson a, const DCond c) { person_bwd_body<true>(a, &c); }
__global__ __launch_bounds__(kEpiThreads) void dt_epilogue_cond_kernel(const DEpilogue a, const DCond c) { epilogue_body<true>(a, &c); }

// which posterior an entry point serves: the vibo_dtrain_* calls the unconditional one, their *_cond twins the conditional one,
// the size queries either
enum { kPostUncond = 0, kPostCond = 1, kPostEither = 2 };
static int dt_check(const vibo_desc* d, const int kind, const int H, const int post = kPostUncond) {
    if (!d || d->abi_version != VIBO_ABI_VERSION) return -2;
    if (VIBO_MASK_IS_ELBO_ONLY(d->mask_dtype)) return -8;      // (VIBO_MASK_SIGN / _TILES: row formats of the ELBO call alone)
    if (d->ability_dim < 1 || d->ability_dim > VIBO_MAX_ABILITY_DIM_WIDE || d->num_item < 1 || d->num_person < 1) return -3;
    if (d->irt_model < VIBO_IRT_1PL || d->irt_model > VIBO_IRT_3PL) return -3;
    if (kind != VIBO_DECODER_LINK && kind != VIBO_DECODER_DEEP && kind != VIBO_DECODER_RESIDUAL) return -3;
    if (d->num_item > 65535) return -3;               // (the packed row counts)
    if (H < 1 || H > kDW) return -6;
    const bool uncond = d->posterior == VIBO_POSTERIOR_UNCONDITIONAL, cond = d->posterior == VIBO_POSTERIOR_CONDITIONAL;
    if (!((uncond && post != kPostCond) || (cond && post != kPostUncond)) || d->n_flows != 0 || d->reg_mode != VIBO_REG_KL) return -6;
    if (d->mask_dtype != VIBO_MASK_U8 && d->mask_dtype != VIBO_MASK_NONE) return -8;
    return 0;
}

}  // namespace vibo

using namespace vibo;

extern "C" int64_t vibo_dtrain_param_floats(const vibo_desc* d, int decoder, int hidden_dim) {
    if (!d || hidden_dim < 1 || d->ability_dim < 1 || d->irt_model < VIBO_IRT_1PL || d->irt_model > VIBO_IRT_3PL) return 0;
    if (VIBO_MASK_IS_ELBO_ONLY(d->mask_dtype)) return 0;      // (VIBO_MASK_SIGN / _TILES: row formats of the ELBO call alone)
    if (decoder != VIBO_DECODER_LINK && decoder != VIBO_DECODER_DEEP && decoder != VIBO_DECODER_RESIDUAL) return 0;
    const int D = item_feat_dim(d->irt_model, d->ability_dim);
    return dparams(decoder, hidden_dim, d->ability_dim, D, d->posterior == VIBO_POSTERIOR_CONDITIONAL ? 1 + D : 1).total;
}

extern "C" int64_t vibo_dtrain_scratch_floats(const vibo_desc* d, int decoder, int hidden_dim, int person_chunk) {
    if (dt_check(d, decoder, hidden_dim, kPostEither)) return 0;
    return (int64_t)dlayout(d, decoder, hidden_dim, person_chunk).total;
}

extern "C" int64_t vibo_dtrain_scratch_offset(const vibo_desc* d, int decoder, int hidden_dim, int person_chunk, int which) {
    if (dt_check(d, decoder, hidden_dim, kPostEither)) return -1;
    const DLayout y = dlayout(d, decoder, hidden_dim, person_chunk);
    switch (which) {
    case VIBO_DTRAIN_SCALARS: return (int64_t)y.flat8;
    case VIBO_DTRAIN_POSTERIOR: return (int64_t)y.post;
    case VIBO_DTRAIN_ABILITY: return (int64_t)y.ability;
    default: return -1;
    }
}

// the table's side argument of a step (every pointer but the per-chunk ones)
static DCond dcond(const DLayout& y, const DParams& p, const float* params, const float* item_feat, float* scratch) {
    DCond c;
    memset(&c, 0, sizeof(c));
    c.e = mlp3_at(0, y.xin, y.H, 2 * y.A);
    c.H = y.H; c.A = y.A; c.I = y.I; c.xin = y.xin; c.nwg = y.gt;
    c.P = params; c.item_feat = item_feat;
    c.x = scratch + y.cx; c.h1 = scratch + y.th1; c.h2 = scratch + y.th2; c.out = scratch + y.tout; c.feat = scratch + y.feat;
    c.sums = scratch + y.sums; c.dsum = scratch + y.dsum; c.dfeat = scratch + y.dfeat;
    c.da = scratch + y.tda; c.db = scratch + y.tdb; c.gx = scratch + y.tgx; c.rec = scratch + y.trec; c.s_enc = scratch + y.s_enc;
    return c;
}
static void* code_table_scratch(const DLayout& y, float* scratch) {
    return (void*)(((uintptr_t)(scratch + y.ct) + 255) & ~(uintptr_t)255);
}

// Launch the kernel of the step's posterior over `a`: the conditional one (c != nullptr) takes the table's side argument behind it.
template <class Arg>
static hipError_t launch_for_posterior(void (*uncond)(Arg), void (*cond)(Arg, DCond), const int grid, const int block, hipStream_t s,
                                       const Arg& a, const DCond* c) {
    if (c) hipLaunchKernelGGL(cond, dim3((unsigned)grid), dim3((unsigned)block), 0, s, a, *c);
    else hipLaunchKernelGGL(uncond, dim3((unsigned)grid), dim3((unsigned)block), 0, s, a);
    return hipGetLastError();
}

static int dt_prologue(const int post, const vibo_desc* d, int decoder, int hidden_dim, int person_chunk, const float* params,
                       const float* item_mu, const float* item_logvar, float* eps_item, uint64_t seed, int draw_noise,
                       float* eps_ability, uint32_t ability_stream_id, float* item_feat, float* scratch, int32_t* step_count,
                       void* stream) {
    const int rc = dt_check(d, decoder, hidden_dim, post);
    if (rc) return rc;
    if (!params || !item_mu || !item_logvar || !eps_item || !item_feat || !scratch || !step_count) return -5;
    if (draw_noise && !eps_ability) return -5;
    const DLayout y = dlayout(d, decoder, hidden_dim, person_chunk);
    hipStream_t s = (hipStream_t)stream;
    DPrologue a;
    memset(&a, 0, sizeof(a));
    a.p = dparams(decoder, hidden_dim, y.A, y.D, y.xin);
    a.I = y.I; a.gen = draw_noise ? 1 : 0;
    a.n_item_blocks = (y.I * y.D + 255) / 256;
    a.P = params; a.mu = item_mu; a.lv = item_logvar; a.eps = eps_item; a.eps_w = eps_item; a.item_feat = item_feat;
    a.table = scratch + y.table; a.saved_h = scratch + y.saved_h; a.kl_parts = scratch + y.kl_parts;
    a.w2p = scratch + y.w2p; a.b2p = scratch + y.b2p; a.w3p = scratch + y.w3p; a.w1p = scratch + y.w1p; a.b3p = scratch + y.b3p;
    a.guess = y.has_g ? scratch + y.guess : nullptr;
    a.eps_ab = eps_ability; a.step_count = step_count;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.ab_stream = ability_stream_id;
    a.n_ab = draw_noise ? (long long)y.B * y.A : 0;
    const long long ab_blocks = ((a.n_ab + 3) / 4 + kDThreads - 1) / kDThreads;
    hipLaunchKernelGGL(y.cond ? dt_prologue_cond_kernel : dt_prologue_kernel, dim3((unsigned)(1 + a.n_item_blocks + ab_blocks)),
                       dim3(kDThreads), 0, s, a);
    if (const int rc = launch_rc("vibo_dtrain_prologue launch")) return rc;
    if (y.mlp) {
        DItem it;
        memset(&it, 0, sizeof(it));
        it.p = a.p; it.I = y.I; it.nwg = y.gi; it.P = params; it.item_feat = item_feat;
        it.h1 = scratch + y.ih1; it.h2 = scratch + y.ih2; it.hid = scratch + y.ihid; it.U = scratch + y.U;
        hipLaunchKernelGGL(dt_item_fwd_kernel, dim3((unsigned)y.gi), dim3(kDThreads), 0, s, it);
        if (const int rc = launch_rc("vibo_dtrain_prologue: item forward launch")) return rc;
    }
    if (y.cond) {
        const DCond c = dcond(y, a.p, params, item_feat, scratch);
        hipLaunchKernelGGL(dt_table_fwd_kernel, dim3((unsigned)y.gt), dim3(kDThreads), 0, s, c);
        return launch_rc("vibo_dtrain_prologue: table forward launch");
    }
    return 0;
}
extern "C" int vibo_dtrain_prologue(const vibo_desc* d, int decoder, int hidden_dim, int person_chunk, const float* params,
                                    const float* item_mu, const float* item_logvar, float* eps_item, uint64_t seed, int draw_noise,
                                    float* eps_ability, uint32_t ability_stream_id, float* item_feat, float* scratch,
                                    int32_t* step_count, void* stream) {
    return dt_prologue(kPostUncond, d, decoder, hidden_dim, person_chunk, params, item_mu, item_logvar, eps_item, seed, draw_noise,
                       eps_ability, ability_stream_id, item_feat, scratch, step_count, stream);
}
extern "C" int vibo_dtrain_prologue_cond(const vibo_desc* d, int decoder, int hidden_dim, int person_chunk, const float* params,
                                         const float* item_mu, const float* item_logvar, float* eps_item, uint64_t seed, int draw_noise,
                                         float* eps_ability, uint32_t ability_stream_id, float* item_feat, float* scratch,
                                         int32_t* step_count, void* stream) {
    return dt_prologue(kPostCond, d, decoder, hidden_dim, person_chunk, params, item_mu, item_logvar, eps_item, seed, draw_noise,
                       eps_ability, ability_stream_id, item_feat, scratch, step_count, stream);
}

static int dt_forward_backward(const int post, const vibo_desc* d, int decoder, int hidden_dim, int person_chunk, const float* params,
                               const float* response, const uint8_t* mask, const int32_t* counts, const uint8_t* codes,
                               int64_t codes_row_stride, const float* eps_ability, const float* item_feat, float* scratch,
                               void* stream) {
    const int rc = dt_check(d, decoder, hidden_dim, post);
    if (rc) return rc;
    if (!params || !response || !counts || !eps_ability || !item_feat || !scratch) return -5;
    if (d->mask_dtype == VIBO_MASK_U8 && !mask) return -5;
    if (post == kPostCond) {
        if (!codes) return -5;
        if (codes_row_stride < d->num_item || codes_row_stride % 4 != 0 || ((uintptr_t)codes & 3)) return -8;
    }
    const DLayout y = dlayout(d, decoder, hidden_dim, person_chunk);
    const DParams p = dparams(decoder, hidden_dim, y.A, y.D, y.xin);
    const DRec r = drec(p);
    hipStream_t s = (hipStream_t)stream;
    const uint8_t* mk = d->mask_dtype == VIBO_MASK_U8 ? mask : nullptr;
    DCond cd;                                         // (set and passed on only for the conditional posterior)
    if (y.cond) {                                     // the experts' sums of every person of the minibatch, whatever the chunks
        cd = dcond(y, p, params, item_feat, scratch);
        const int crc = vibo_code_table_sum_forward(y.B, y.I, kDW, codes, codes_row_stride, scratch + y.feat, scratch + y.sums,
                                                    code_table_scratch(y, scratch), y.ct_bytes, stream);
        if (crc) return crc;
    }
    for (int c = 0; c < y.n_chunk; ++c) {
        const int p0 = c * y.bc;
        const int nb = (p0 + y.bc <= y.B ? y.bc : y.B - p0);
        const size_t sp = (size_t)p0;
        DPerson a;
        memset(&a, 0, sizeof(a));
        a.p = p; a.I = y.I; a.irt = y.irt; a.nb = nb; a.nwg = y.gp; a.prior = d->missing_mode == VIBO_MISSING_PRIOR ? 1 : 0;
        a.n_dv = 4 * y.n_ib;
        a.P = params; a.counts = counts + p0; a.table = scratch + y.table; a.eps = eps_ability + sp * y.A; a.item_feat = item_feat;
        a.post = scratch + y.post + sp * 2 * y.A; a.ability = scratch + y.ability + sp * y.A;
        if (y.mlp) {
            a.h1 = scratch + y.ah1 + sp * kDW; a.h2 = scratch + y.ah2 + sp * kDW; a.hid = scratch + y.ahid + sp * kDW;
            a.db = scratch + y.db; a.gab = scratch + y.gab;
        }
        a.V = scratch + y.V + sp * kDW;
        a.L = y.has_l ? scratch + y.L + sp * y.I : nullptr;
        a.dV = scratch + y.dV; a.dL = y.has_l ? scratch + y.dL + sp * y.I : nullptr;
        a.da = scratch + y.da;
        a.rec = scratch + y.prec + (size_t)c * y.gp * r.ptotal; a.rec_stride = r.ptotal;
        a.r_tab = r.tab; a.r_kl = r.kl; a.r_vb = r.vb; a.r_fa = r.fa; a.r_wcp = r.wcp;
        if (y.cond) {
            cd.sums = scratch + y.sums + sp * kDW; cd.dsum = scratch + y.dsum + sp * kDW;
        }
        if (const int rc = hip_rc(launch_for_posterior(dt_person_fwd_kernel, dt_person_fwd_cond_kernel, y.gp, kDThreads, s, a, y.cond ? &cd : nullptr),
                                  "vibo_dtrain_forward_backward: person forward launch")) return rc;
        vibo_decoder_desc dd;
        memset(&dd, 0, sizeof(dd));
        dd.num_person = nb; dd.num_item = y.I; dd.hidden_dim = kDW; dd.want_grad = 1; dd.person_chunks = y.dc;
        dd.resid = decoder == VIBO_DECODER_RESIDUAL ? 1.0f : 0.0f;
        dd.response_row_stride = d->response_row_stride; dd.mask_row_stride = d->mask_row_stride;
        const size_t cw = (size_t)c * y.n_wave;
        const int drc = vibo_decoder_fwd_bwd(
            &dd, response + sp * d->response_row_stride, mk ? mk + sp * d->mask_row_stride : nullptr, y.mlp ? scratch + y.U : nullptr, a.V,
            a.L, y.has_g ? scratch + y.guess : nullptr, decoder == VIBO_DECODER_LINK ? scratch + y.w1p : nullptr, scratch + y.w2p,
            scratch + y.b2p, scratch + y.w3p, scratch + y.b3p, scratch + y.ll_part + cw, y.mlp ? scratch + y.dU + (size_t)c * y.dc * y.I * kDW : nullptr,
            scratch + y.dV, y.has_l ? scratch + y.dL + sp * y.I : nullptr, y.has_g ? scratch + y.dguess + (size_t)c * y.dc * y.I : nullptr,
            scratch + y.dW2 + cw * kDW * kDW, scratch + y.dvec + cw * 4 * kDW, nullptr, stream);
        if (drc) return drc;
        if (const int rc = hip_rc(launch_for_posterior(dt_person_bwd_kernel, dt_person_bwd_cond_kernel, y.gp, kDThreads, s, a, y.cond ? &cd : nullptr),
                                  "vibo_dtrain_forward_backward: person backward launch")) return rc;
        if (y.has_l) {
            const int per = (nb + y.ns - 1) / y.ns;
            hipLaunchKernelGGL(dt_ditem_kernel, dim3((unsigned)((y.I * y.D + 255) / 256), (unsigned)y.ns), dim3(256), 0, s, y.I, y.A, y.D, y.irt,
                               nb, per, (const float*)a.dL, (const float*)a.ability, scratch + y.drec_item + (size_t)c * y.ns * y.I * y.D);
            if (const int rc = launch_rc("vibo_dtrain_forward_backward: item gradient launch")) return rc;
        }
    }
    if (y.cond)                                       // d [lambda | s] of every person is complete: its transpose onto the table rows
        return vibo_code_table_sum_backward(y.B, y.I, kDW, codes, codes_row_stride, scratch + y.dsum, scratch + y.dfeat,
                                            code_table_scratch(y, scratch), y.ct_bytes, stream);
    return 0;
}
extern "C" int vibo_dtrain_forward_backward(const vibo_desc* d, int decoder, int hidden_dim, int person_chunk, const float* params,
                                            const float* response, const uint8_t* mask, const int32_t* counts,
                                            const float* eps_ability, const float* item_feat, float* scratch, void* stream) {
    return dt_forward_backward(kPostUncond, d, decoder, hidden_dim, person_chunk, params, response, mask, counts, nullptr, 0, eps_ability,
                               item_feat, scratch, stream);
}
extern "C" int vibo_dtrain_forward_backward_cond(const vibo_desc* d, int decoder, int hidden_dim, int person_chunk, const float* params,
                                                 const float* response, const uint8_t* mask, const int32_t* counts,
                                                 const uint8_t* codes, int64_t codes_row_stride, const float* eps_ability,
                                                 const float* item_feat, float* scratch, void* stream) {
    return dt_forward_backward(kPostCond, d, decoder, hidden_dim, person_chunk, params, response, mask, counts, codes, codes_row_stride,
                               eps_ability, item_feat, scratch, stream);
}

static int dt_epilogue(const int post, const vibo_desc* d, int decoder, int hidden_dim, int person_chunk, float* scratch,
                       const float* eps_item, const float* item_feat, const float* beta, const float* lr, int32_t* step_count,
                       float* params, float* adam_m, float* adam_v, float* item_mu, float* item_logvar, float* item_m,
                       float* item_v, float* loss_out, void* stream) {
    const int rc = dt_check(d, decoder, hidden_dim, post);
    if (rc) return rc;
    if (!scratch || !eps_item || !item_feat || !beta || !lr || !step_count || !params || !adam_m || !adam_v || !item_mu || !item_logvar ||
        !item_m || !item_v || !loss_out)
        return -5;
    const DLayout y = dlayout(d, decoder, hidden_dim, person_chunk);
    const DParams p = dparams(decoder, hidden_dim, y.A, y.D, y.xin);
    const DRec r = drec(p);
    hipStream_t s = (hipStream_t)stream;
    DCond cd;                                         // (set and passed on only for the conditional posterior)
    if (y.cond) {                                     // the table backward: its records join the sums below
        cd = dcond(y, p, params, item_feat, scratch);
        cd.beta = beta;
        hipLaunchKernelGGL(dt_table_bwd_kernel, dim3((unsigned)y.gt), dim3(kDThreads), 0, s, cd);
        if (const int rc = launch_rc("vibo_dtrain_epilogue: table backward launch")) return rc;
    }
    DReduce q;
    memset(&q, 0, sizeof(q));
    int blk = 0;
    auto seg = [&](const size_t src, const size_t dst, const int n_rec, const size_t stride, const int n_out) {
        DSeg& g = q.s[q.n++];
        g.src = scratch + src; g.dst = scratch + dst; g.n_rec = n_rec; g.stride = stride; g.n_out = n_out; g.blk0 = blk;
        blk += (n_out + 63) / 64;
    };
    const int n_dec = y.n_chunk * y.n_wave;
    seg(y.ll_part, y.flat8 + VIBO_S_LL, n_dec, 1, 1);
    seg(y.prec + r.kl, y.flat8 + VIBO_S_REG, y.n_chunk * y.gp, r.ptotal, 1);
    seg(y.prec, y.s_p, y.n_chunk * y.gp, r.ptotal, r.ptotal);
    seg(y.dW2, y.s_dW2, n_dec, kDW * kDW, kDW * kDW);
    seg(y.dvec, y.s_dvec, n_dec, 4 * kDW, 4 * kDW);
    if (y.mlp) seg(y.dU, y.s_dU, y.n_chunk * y.dc, (size_t)y.I * kDW, y.I * kDW);
    if (y.has_g) seg(y.dguess, y.s_dguess, y.n_chunk * y.dc, y.I, y.I);
    if (y.has_l) seg(y.drec_item, y.s_ditem, y.n_chunk * y.ns, (size_t)y.I * y.D, y.I * y.D);
    if (y.cond) seg(y.trec, y.s_enc, y.gt, p.enc, p.enc);
    hipLaunchKernelGGL(dt_reduce_kernel, dim3((unsigned)blk), dim3(1024), 0, s, q);
    if (const int rc = launch_rc("vibo_dtrain_epilogue: reduce launch")) return rc;
    if (y.mlp) {
        DItem it;
        memset(&it, 0, sizeof(it));
        it.p = p; it.I = y.I; it.nwg = y.gi; it.P = params; it.item_feat = item_feat;
        it.h1 = scratch + y.ih1; it.h2 = scratch + y.ih2; it.hid = scratch + y.ihid; it.U = scratch + y.U;
        it.s_dU = scratch + y.s_dU; it.da = scratch + y.ida; it.db = scratch + y.idb; it.gx = scratch + y.gx;
        it.rec = scratch + y.irec; it.rec_stride = r.itotal; it.r_fi = r.fi; it.r_wci = r.wci;
        hipLaunchKernelGGL(dt_item_bwd_kernel, dim3((unsigned)y.gi), dim3(kDThreads), 0, s, it);
        if (const int rc = launch_rc("vibo_dtrain_epilogue: item backward launch")) return rc;
    }
    DEpilogue a;
    memset(&a, 0, sizeof(a));
    a.p = p; a.r = r; a.I = y.I; a.n_item_entries = y.I * y.D;
    a.n_dec_blocks = (p.total - (y.cond ? 0 : p.dec) + kEpiThreads - 1) / kEpiThreads;
    a.n_irec = y.mlp ? y.gi : 0; a.has_l = y.has_l ? 1 : 0; a.has_g = y.has_g ? 1 : 0;
    a.flat8 = scratch + y.flat8; a.s_p = scratch + y.s_p; a.s_dW2 = scratch + y.s_dW2; a.s_dvec = scratch + y.s_dvec;
    a.s_ditem = scratch + y.s_ditem; a.s_dguess = scratch + y.s_dguess; a.guess = scratch + y.guess;
    a.gx = y.mlp ? scratch + y.gx : nullptr; a.irec = scratch + y.irec;
    a.saved_h = scratch + y.saved_h; a.kl_parts = scratch + y.kl_parts; a.eps = eps_item; a.beta = beta; a.lr = lr;
    a.step_count = step_count; a.P = params; a.M = adam_m; a.V = adam_v; a.mu = item_mu; a.lv = item_logvar; a.im = item_m; a.iv = item_v;
    a.loss = loss_out;
    const int item_blocks = (a.n_item_entries + kEpiThreads - 1) / kEpiThreads;
    return hip_rc(launch_for_posterior(dt_epilogue_kernel, dt_epilogue_cond_kernel, 1 + a.n_dec_blocks + item_blocks, kEpiThreads, s, a,
                                       y.cond ? &cd : nullptr), "vibo_dtrain_epilogue launch");
}
extern "C" int vibo_dtrain_epilogue(const vibo_desc* d, int decoder, int hidden_dim, int person_chunk, float* scratch,
                                    const float* eps_item, const float* item_feat, const float* beta, const float* lr,
                                    int32_t* step_count, float* params, float* adam_m, float* adam_v, float* item_mu,
                                    float* item_logvar, float* item_m, float* item_v, float* loss_out, void* stream) {
    return dt_epilogue(kPostUncond, d, decoder, hidden_dim, person_chunk, scratch, eps_item, item_feat, beta, lr, step_count, params, adam_m,
                       adam_v, item_mu, item_logvar, item_m, item_v, loss_out, stream);
}
extern "C" int vibo_dtrain_epilogue_cond(const vibo_desc* d, int decoder, int hidden_dim, int person_chunk, float* scratch,
                                         const float* eps_item, const float* item_feat, const float* beta, const float* lr,
                                         int32_t* step_count, float* params, float* adam_m, float* adam_v, float* item_mu,
                                         float* item_logvar, float* item_m, float* item_v, float* loss_out, void* stream) {
    return dt_epilogue(kPostCond, d, decoder, hidden_dim, person_chunk, scratch, eps_item, item_feat, beta, lr, step_count, params, adam_m,
                       adam_v, item_mu, item_logvar, item_m, item_v, loss_out, stream);
}
