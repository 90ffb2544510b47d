// vibo_train_hook.hpp -- the O(I) head of a plain VIBO train step (item sample, item KL, the 2-row encoder MLP) as device
// routines shared by train_prologue_kernel (the first step of a run, and every step of the four-launch form) and by
// train_epilogue_fused_kernel, which leaves the NEXT step's head behind (vibo_trainer.hip).  Both execute the same statements
// in the same order, so the two forms of the step agree bit for bit
// (tests/test_gpu_trainer.py::test_folded_step_equals_the_unfolded_step).
// Below the MLP: what the plain, mean-merge and conditional / flow trainers (vibo_trainer.hip, vibo_mtrainer.hip,
// vibo_ctrainer.hip) and the MLP-decoder trainer (vibo_dtrainer.hip) have in common -- the item side of a prologue, the
// ability-noise block, Adam, the item update and the loss; at the end: the 2-row encoder backward + Adam of an epilogue's block 0
// (epi_mlp_block: vibo_trainer.hip's three epilogues and vibo_dtrainer.hip's).
//
// Reference statements (models.py:356-361, 575-582, 713-726, 506-510; utils.py:85-88):
//     item_feat = item_mu + exp(0.5 item_logvar) * eps_item
//     KL_item   = sum -0.5 (1 + logvar - mu^2 - exp(logvar))
//     table[c]  = W2 . elu(W1 . elu(W0 c + b0) + b1) + b2        c in {0, 1}
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vibo_hip.h"
#include "vibo_device.hpp"
#include "vibo_params.hpp"
#include "vibo_philox.hpp"

namespace vibo {

constexpr int kMaxHidden = 256;

// Parameter layout W0 [H] | b0 [H] | W1 [H][ld] | b1 [H] | W2 [O][ld] | b2 [O]: ld = H in the caller's flat buffer; the epilogue's
// LDS copy pads the matrix rows by one float (ld = H + 1) so that "thread j walks row j" is conflict-free.
struct MlpOffsets {
    int w0, b0, w1, b1, w2, b2, total, ld;
};
__host__ __device__ inline MlpOffsets mlp_offsets(int H, int O, int ld = 0) {
    MlpOffsets o;
    o.ld = ld > 0 ? ld : H;
    o.w0 = 0; o.b0 = H; o.w1 = 2 * H; o.b1 = o.w1 + H * o.ld; o.w2 = o.b1 + H; o.b2 = o.w2 + O * o.ld; o.total = o.b2 + O;
    return o;
}
// index of flat parameter k (ld = H layout) in the layout `t`
__device__ __forceinline__ int mlp_reindex(const int k, const int H, const int O, const MlpOffsets& t) {
    const MlpOffsets o = mlp_offsets(H, O);
    if (k < o.w1) return k;
    if (k < o.b1) return t.w1 + ((k - o.w1) / H) * t.ld + (k - o.w1) % H;
    if (k < o.w2) return t.b1 + (k - o.b1);
    if (k < o.b2) return t.w2 + ((k - o.w2) / H) * t.ld + (k - o.w2) % H;
    return t.b2 + (k - o.b2);
}

__device__ __forceinline__ float elu(float x) { return x > 0.f ? x : expm1f(x); }

// The 2-row MLP forward of ONE workgroup in three stages (a workgroup barrier between them).  h1, h2: [2][H] in LDS;
// P / o: the parameters and their layout (global memory, or the epilogue's padded LDS copy).
// Row j's dot product is one chain of fmaf's over k = 0 .. H-1 wherever it runs.
__device__ __forceinline__ void mlp2_layer0(const float* P, const MlpOffsets o, const int H, const int O, float* h1, const int tid,
                                            const int nthr) {
    for (int t = tid; t < 2 * H; t += nthr) {      // the input of row r is the response value r in {0, 1}
        const int r = t / H, j = t % H;
        h1[r * H + j] = elu(fmaf(P[o.w0 + j], (float)r, P[o.b0 + j]));
    }
}
__device__ __forceinline__ void mlp2_layer1(const float* P, const MlpOffsets o, const int H, const int O, const float* h1, float* h2,
                                            const int tid, const int nthr) {
    for (int t = tid; t < 2 * H; t += nthr) {
        const int r = t / H, j = t % H;
        float a = P[o.b1 + j];
#pragma unroll 16
        for (int k = 0; k < H; ++k) a = fmaf(P[o.w1 + j * o.ld + k], h1[r * H + k], a);
        h2[r * H + j] = elu(a);
    }
}
// layer 2 -> table [2][O]; the activations are kept for the backward: saved_h = h1 | h2
__device__ __forceinline__ void mlp2_layer2(const float* P, const MlpOffsets o, const int H, const int O, const float* h1, const float* h2,
                                            const int tid, const int nthr, float* table, float* saved_h) {
    for (int t = tid; t < 2 * O; t += nthr) {
        const int r = t / O, q = t % O;
        float a = P[o.b2 + q];
#pragma unroll 16
        for (int k = 0; k < H; ++k) a = fmaf(P[o.w2 + q * o.ld + k], h2[r * H + k], a);
        table[t] = a;
    }
    for (int t = tid; t < 2 * H; t += nthr) {
        saved_h[t] = h1[t];
        saved_h[2 * H + t] = h2[t];
    }
}

// entry idx of the [I][D] item sample (models.py:506-510) and its KL term (utils.py:85-88)
__device__ __forceinline__ float item_sample(const float m, const float l, const float e) { return fmaf(expf(0.5f * l), e, m); }
__device__ __forceinline__ float item_kl_term(const float m, const float l) { return -0.5f * (1.0f + l - m * m - expf(l)); }

// Item entries are walked dimension-major -- entry k = (dim k / I, item k % I), the order of the ELBO kernel's gradient records --
// in groups of 64 (one wave): kl_parts[g] = the wave total of the KL terms of entries [64 g, 64 g + 64).
__device__ __forceinline__ int item_entry_index(const int k, const int I, const int D) { return (k % I) * D + k / I; }
constexpr int kKlGroup = 64;
__host__ __device__ inline int kl_part_count(const int n_entries) { return (n_entries + kKlGroup - 1) / kKlGroup; }

// One item block (256 threads) of a prologue launch: entries 256 block + tid in that order, noise drawn (gen: Philox stream 0 at
// `counter`, kept in eps_w; its group of 4 is recomputed by 4 threads: O(I) work) or read from eps, item sample, KL term, and one
// KL part per wave into parts[4 block + wave] (the caller picks `parts`: the plain trainer double-buffers it by step parity).
__device__ __forceinline__ void item_prologue_block(const unsigned block, const int tid, const int I, const int D, const float* __restrict__ mu,
                                                    const float* __restrict__ lv, const float* __restrict__ eps, float* __restrict__ eps_w,
                                                    const int gen, const int32_t* counter, const uint32_t seed_lo, const uint32_t seed_hi,
                                                    float* __restrict__ item_feat, float* parts) {
    const int n_item_entries = I * D;
    const int k = block * 256 + tid;
    float kl = 0.f;
    if (k < n_item_entries) {
        const int idx = item_entry_index(k, I, D);
        const float m = mu[idx], l = lv[idx];
        float e;
        if (gen) {
            e = philox_normal1(idx, (uint32_t)*counter, 0u, seed_lo, seed_hi);
            eps_w[idx] = e;
        } else {
            e = eps[idx];
        }
        item_feat[idx] = item_sample(m, l, e);
        kl = item_kl_term(m, l);
    }
    kl = wave_total(kl);
    if ((tid & 63) == 0 && 256 * (int)block + (tid & ~63) < n_item_entries) parts[4 * block + (tid >> 6)] = kl;
}

// One ability-noise block (BS threads, 4 normals per thread) behind the item blocks: what vibo_fill_normal leaves in eps_ab [n_ab]
// for stream ab_stream at `counter`
__device__ __forceinline__ void ability_noise_block(const unsigned block, const int BS, const int tid, float* __restrict__ eps_ab,
                                                    const long long n_ab, const uint32_t counter, const uint32_t ab_stream,
                                                    const uint32_t seed_lo, const uint32_t seed_hi) {
    const long long g = (long long)block * BS + tid;
    if (4 * g < n_ab) store_normal4(eps_ab, n_ab, g, philox_normal4(g, counter, ab_stream, seed_lo, seed_hi));
}

// Adam's bias corrections at step t: 1 - 0.9^t and sqrt(1 - 0.999^t)
struct AdamBias {
    float bc1, bc2_sqrt;
};
__device__ __forceinline__ AdamBias adam_bias(const int step) {
    const float t = (float)step;
    return {1.0f - powf(0.9f, t), sqrtf(1.0f - powf(0.999f, t))};
}
// torch.optim.Adam's update (betas 0.9 / 0.999, eps 1e-8).  Every product-sum is pinned to one fma: the epilogue kernels of
// vibo_trainer.hip must agree bit for bit, and the contraction hipcc picks for a sum of two products depends on the
// surrounding code.
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, const float g, const float lr, const AdamBias bc) {
    m = fmaf(0.9f, m, 0.1f * g);                   // torch: exp_avg.lerp_(grad, 1 - beta1)
    v = fmaf(0.999f, v, (0.001f * g) * g);         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
    const float denom = sqrtf(v) / bc.bc2_sqrt + 1e-8f;
    p -= (lr / bc.bc1) * (m / denom);
}

// item entry idx: d loss / d item_feat = gf -> (item_mu, item_logvar) through the sample and the item KL, Adam in place
__device__ __forceinline__ void epi_item_update(const int idx, const int n_item_entries, const float gf, const float e, const float beta,
                                                const float lr, const AdamBias bc, float* mu, float* lv, float* im, float* iv, float& pm,
                                                float& pl) {
    const float m = mu[idx], l = lv[idx];
    const float g_mu = fmaf(beta, m, gf);
    const float half_sd = 0.5f * expf(0.5f * l);
    const float klg = (0.5f * beta) * (1.0f - expf(l));
    const float g_lv = fmaf(gf * half_sd, e, -klg);
    pm = m; pl = l;
    adam_update(pm, im[idx], iv[idx], g_mu, lr, bc);
    adam_update(pl, im[n_item_entries + idx], iv[n_item_entries + idx], g_lv, lr, bc);
    mu[idx] = pm;
    lv[idx] = pl;
}

// Wave 0 of an epilogue's block 0: item KL = the prologue's partial sums in a fixed order (lane-strided, then the wave sum), and
// loss = -LL + beta (REG + KL_item) from the ELBO scalars sc (VIBO_S_*)
__device__ __forceinline__ void item_kl_loss(const int tid, const float* __restrict__ kl_parts, const int n_kl_parts, const float* sc,
                                             const float beta, float* loss_out) {
    if (tid < 64) {
        float kl = 0.f;
        for (int k = tid; k < n_kl_parts; k += 64) kl += kl_parts[k];
        kl = wave_total(kl);
        if (tid == 0) *loss_out = fmaf(beta, sc[VIBO_S_REG] + kl, -sc[VIBO_S_LL]);
    }
}

constexpr int kEpiThreads = 1024;      // block 0's chain of small dependent stages is latency-bound: more lanes per stage, fewer passes
struct EpiLds {
    float h1[2][kMaxHidden], h2[2][kMaxHidden], gh2[2][kMaxHidden], gh1[2][kMaxHidden], gout[2][2 * VIBO_MAX_ABILITY_DIM_WIDE];
};

// Block 0 of the epilogue: loss, the 2-row MLP backward by hand, Adam on the MLP parameters.
//   sc: the 8 ELBO scalars (VIBO_S_*); gtab: d LL / d table [2][O] then d REG / d table [2][O]
//   W / ow: where the backward reads the weights and their layout -- the caller's flat buffer P (ld = H), or the fused
//   epilogue's padded LDS copy, which then also receives the updated values (Wout) for the next step's forward
//   pv / mv / vv: parameter, first and second moment of elements tid + 1024 u, loaded by the caller (as early as it can)
//   HC: the hidden width as a compile-time constant (64: the reference default), or 0 for a runtime width -- the Adam loop
//   decodes six flat indices per thread with / H and % H, ~40 instructions each when H is not a constant (5 us of the chain)
constexpr int kEpiU = 8;
template <int HC>
__device__ __forceinline__ void epi_mlp_block(EpiLds& L, const int H_, const int O, const int n_kl_parts, const float* sc, const float* gtab,
                                              const float* __restrict__ saved_h, const float* __restrict__ kl_parts, const float beta,
                                              const float lr, const AdamBias bc, const float* W, const MlpOffsets ow,
                                              float* Wout, float* P, float* M, float* V, float (&pv)[kEpiU], float (&mv)[kEpiU],
                                              float (&vv)[kEpiU], float* loss_out, const int tid) {
    constexpr int BS = kEpiThreads;
    const int H = HC > 0 ? HC : H_;
    const int n_table = 2 * O;
    const MlpOffsets o = mlp_offsets(H, O);
    for (int k = tid; k < 2 * H; k += BS) {
        L.h1[k / H][k % H] = saved_h[k];
        L.h2[k / H][k % H] = saved_h[2 * H + k];
    }
    // d loss / d table = -dLL + beta dREG
    for (int k = tid; k < n_table; k += BS) L.gout[k / O][k % O] = fmaf(beta, gtab[n_table + k], -gtab[k]);
    item_kl_loss(tid, kl_parts, n_kl_parts, sc, beta, loss_out);
    __syncthreads();
    // g_h2 = W2^T g_out * elu'(pre2),  elu'(x) = x > 0 ? 1 : elu(x) + 1
    for (int k = tid; k < 2 * H; k += BS) {
        const int r = k / H, j = k % H;
        float a = 0.f;
#pragma unroll 16
        for (int q = 0; q < O; ++q) a = fmaf(W[ow.w2 + q * ow.ld + j], L.gout[r][q], a);      // 16 loads in flight
        const float h = L.h2[r][j];
        L.gh2[r][j] = a * (h > 0.f ? 1.0f : h + 1.0f);
    }
    __syncthreads();
    // g_h1 = W1^T g_h2 * elu'(pre1): each of the 2 H dot products over H is cut into 8 pieces (8 neighbouring lanes)
    {
        const int len = (H + 7) / 8;
        for (int k0 = 0; k0 < 2 * H * 8; k0 += BS) {
            const int k = k0 + tid;
            const int out = k >> 3, part = k & 7;
            const int r = out / H, j = out % H;
            float a = 0.f;
            if (out < 2 * H) {
                const int q1 = min(H, (part + 1) * len);
                for (int q = part * len; q < q1; ++q) a = fmaf(W[ow.w1 + q * ow.ld + j], L.gh2[r][q], a);
            }
            a += __shfl_xor(a, 1);
            a += __shfl_xor(a, 2);
            a += __shfl_xor(a, 4);
            if (out < 2 * H && part == 0) {
                const float h = L.h1[r][j];
                L.gh1[r][j] = a * (h > 0.f ? 1.0f : h + 1.0f);
            }
        }
    }
    __syncthreads();      // all reads of the OLD weights are done: parameters may now be updated in place
    // Adam over the MLP parameters: 8 independent elements per thread and pass (the first pass's loads were issued by the caller)
    constexpr int U = kEpiU;
    for (int k0 = tid; k0 < o.total; k0 += BS * U) {
        if (k0 != tid) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + BS * u;
                const bool ok = k < o.total;
                pv[u] = ok ? P[k] : 0.f;
                mv[u] = ok ? M[k] : 0.f;
                vv[u] = ok ? V[k] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + BS * u;
            if (k >= o.total) continue;
            float g;
            if (k < o.b0) {                         // W0[j]: input of row r is r
                g = L.gh1[1][k - o.w0];
            } else if (k < o.w1) {
                const int j = k - o.b0;
                g = L.gh1[0][j] + L.gh1[1][j];
            } else if (k < o.b1) {
                const int j = (k - o.w1) / H, q = (k - o.w1) % H;
                g = fmaf(L.gh2[0][j], L.h1[0][q], L.gh2[1][j] * L.h1[1][q]);
            } else if (k < o.w2) {
                const int j = k - o.b1;
                g = L.gh2[0][j] + L.gh2[1][j];
            } else if (k < o.b2) {
                const int q = (k - o.w2) / H, j = (k - o.w2) % H;
                g = fmaf(L.gout[0][q], L.h2[0][j], L.gout[1][q] * L.h2[1][j]);
            } else {
                const int q = k - o.b2;
                g = L.gout[0][q] + L.gout[1][q];
            }
            adam_update(pv[u], mv[u], vv[u], g, lr, bc);
            P[k] = pv[u];
            M[k] = mv[u];
            V[k] = vv[u];
            if (Wout) Wout[mlp_reindex(k, H, O, ow)] = pv[u];      // (ow.ld = H + 1)
        }
    }
}
// the first pass's parameter / moment loads of epi_mlp_block
__device__ __forceinline__ void epi_mlp_prefetch(const int total, const float* P, const float* M, const float* V, float (&pv)[kEpiU],
                                                 float (&mv)[kEpiU], float (&vv)[kEpiU], const int tid) {
#pragma unroll
    for (int u = 0; u < kEpiU; ++u) {
        const int k = tid + kEpiThreads * u;
        const bool ok = k < total;
        pv[u] = ok ? P[k] : 0.f;
        mv[u] = ok ? M[k] : 0.f;
        vv[u] = ok ? V[k] : 0.f;
    }
}

}  // namespace vibo
