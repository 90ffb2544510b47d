// vibo_trainer.hip -- the O(I) part of a VIBO train step as two kernels (see include/vibo_hip.h):
// prologue (item sample, item KL, 2-row encoder MLP forward) and epilogue (loss, MLP backward, item
// backward, Adam).  One workgroup (block 0) owns the MLP; the other workgroups own 256 item entries each.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vibo_hip.h"
#include "../../include/vibo_hip_tile_rows.h"
#include "vibo_device.hpp"
#include "vibo_finalize.hpp"
#include "vibo_host.hpp"
#include "vibo_philox.hpp"
#include "vibo_train_hook.hpp"

namespace vibo {

__global__ __launch_bounds__(256) void train_prologue_kernel(int H, int O, int I, int D, const float* __restrict__ P,
                                                             const float* __restrict__ mu, const float* __restrict__ lv,
                                                             const float* __restrict__ eps, float* __restrict__ item_feat,
                                                             float* __restrict__ table, float* __restrict__ saved_h,
                                                             float* __restrict__ kl_parts, int32_t* step_count,
                                                             // tick: step_count[0] += 1 (the four-launch step); tick == 0 primes the
                                                             // folded step (whose ELBO launch ticks) and selects the half of the
                                                             // double-buffered kl_parts the coming step will read
                                                             int tick,
                                                             // noise (gen != 0): eps is written here instead of read, and the
                                                             // blocks past the item blocks fill eps_ab [n_ab]; both draws are
                                                             // the streams vibo_fill_normal gives for step_count[1]
                                                             int gen, uint32_t seed_lo, uint32_t seed_hi, float* __restrict__ eps_w,
                                                             float* __restrict__ eps_ab, long long n_ab, uint32_t ab_stream,
                                                             int n_item_blocks) {
    __shared__ float h1[2 * kMaxHidden], h2[2 * kMaxHidden];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        if (tick && tid == 0) *step_count += 1;
        const MlpOffsets o = mlp_offsets(H, O);
        mlp2_layer0(P, o, H, O, h1, tid, 256);
        __syncthreads();
        mlp2_layer1(P, o, H, O, h1, h2, tid, 256);
        __syncthreads();
        mlp2_layer2(P, o, H, O, h1, h2, tid, 256, table, saved_h);
        return;
    }
    if ((int)blockIdx.x > n_item_blocks) {          // ability noise (stream ab_stream)
        ability_noise_block(blockIdx.x - 1 - n_item_blocks, 256, tid, eps_ab, n_ab, (uint32_t)step_count[1], ab_stream, seed_lo, seed_hi);
        return;
    }
    // (tick == 0: the part buffer of the step that is about to run, step_count[0] + 1)
    float* parts = kl_parts + (tick ? 0 : (((*step_count + 1) & 1) ? kl_part_count(I * D) : 0));
    item_prologue_block(blockIdx.x - 1, tid, I, D, mu, lv, eps, eps_w, gen, step_count + 1, seed_lo, seed_hi, item_feat, parts);
}

__global__ __launch_bounds__(kEpiThreads) void train_epilogue_kernel(int H, int O, int n_item_entries, int n_kl_parts,
                                                             const float* __restrict__ flat, const float* __restrict__ saved_h,
                                                             const float* __restrict__ kl_parts, const float* __restrict__ eps,
                                                             const float* __restrict__ beta_p, const float* __restrict__ lr_p,
                                                             const int32_t* __restrict__ step_count, float* P, float* M, float* V,
                                                             float* mu, float* lv, float* im, float* iv, float* loss_out) {
    __shared__ EpiLds L;
    const int tid = threadIdx.x;
    const float beta = *beta_p, lr = *lr_p;
    const AdamBias bc = adam_bias(*step_count);
    const int n_table = 2 * O;
    constexpr int BS = kEpiThreads;
    if (blockIdx.x == 0) {
        if (tid == 0) const_cast<int32_t*>(step_count)[1] += 1;      // completed steps: the noise counter of the NEXT step
        // flat: [8 scalars | grad_table set 0 | set 1 | grad_item]
        float pv[kEpiU], mv[kEpiU], vv[kEpiU];
        const MlpOffsets o = mlp_offsets(H, O);
        epi_mlp_prefetch(o.total, P, M, V, pv, mv, vv, tid);
        if (H == 64) epi_mlp_block<64>(L, H, O, n_kl_parts, flat, flat + VIBO_NUM_SCALARS, saved_h, kl_parts, beta, lr, bc, P, o, nullptr,
                                       P, M, V, pv, mv, vv, loss_out, tid);
        else epi_mlp_block<0>(L, H, O, n_kl_parts, flat, flat + VIBO_NUM_SCALARS, saved_h, kl_parts, beta, lr, bc, P, o, nullptr, P, M, V,
                              pv, mv, vv, loss_out, tid);
        return;
    }
    const int idx = (blockIdx.x - 1) * BS + tid;
    if (idx < n_item_entries) {        // d loss / d item_feat = -dLL/ditem
        float pm, pl;
        epi_item_update(idx, n_item_entries, -flat[VIBO_NUM_SCALARS + 2 * n_table + idx], eps[idx], beta, lr, bc, mu, lv, im, iv, pm, pl);
    }
}

// The epilogue of the folded train step.  One launch does what finalize_kernel + train_epilogue_kernel do for THIS step and
// what vibo_train_prologue_noise does for the NEXT one (the step is software-pipelined across its own iterations: everything
// the ELBO kernel needs is already in memory when it starts):
//   * e.partial != null ("fused finalize", one GPU): the fixed-order fp64 sums over the ELBO kernel's per-workgroup partial
//     records happen here -- block 0 sums the 8 scalars and the table gradient, item block b the 64 item-gradient entries
//     it then applies -- in finalize_kernel<64>'s order (16 slices, record_slice_sum), so the step agrees bit for bit with
//     the four-launch form; the sums are also written to flat_out (what vibo_elbo_fwd_bwd would have returned).
//     e.partial == null (person-sharded: finalize_kernel ran before the all-reduce): the sums are read from flat_in.
//   * the next step's head: the thread that has just updated item entry idx redraws its noise (stream 0, counter
//     step_count[0] = what the next step's prologue would read from step_count[1]) and forms the next item sample and KL
//     term (kl_parts is double-buffered by step parity: this step's half is still being read by block 0); block 0, after
//     Adam, runs the 2-row MLP forward on the NEW parameters (table, saved_h); the blocks past the item blocks fill eps_ab.
//   * the table this step ran on stays behind the new one (e.table + 2 O): 16-64 floats, see block 0.
constexpr int kEpiOut = 64, kEpiSlices = kEpiThreads / kEpiOut;
constexpr int kEpiStageHidden = 64;
constexpr int kEpiStageFloats = 3 * kEpiStageHidden + (kEpiStageHidden + 2 * VIBO_MAX_ABILITY_DIM_WIDE) * (kEpiStageHidden + 1) + 2 * VIBO_MAX_ABILITY_DIM_WIDE;
static_assert(kEpiStageFloats * 8 >= 0 && kEpiThreads * kEpiU >= kEpiStageFloats, "one prefetch pass covers the staged parameters");
static_assert(kEpiOut == kKlGroup, "one KL part per item block");

template <int HC>
__global__ __launch_bounds__(kEpiThreads) void train_epilogue_fused_kernel(const EpiParams e) {
    __shared__ EpiLds L;
    __shared__ double part[kEpiSlices][kEpiOut], part2[kEpiSlices][kEpiOut];
    __shared__ float sc[VIBO_NUM_SCALARS];
    __shared__ float gt[8 * VIBO_MAX_ABILITY_DIM_WIDE];
    __shared__ float Pl[kEpiStageFloats];        // block 0: padded copy of the MLP parameters (encoders up to kEpiStageHidden wide)
    const int tid = threadIdx.x;
    const int lane = tid % kEpiOut, slice = tid / kEpiOut;
    const int n_table = 2 * e.O;                 // floats per table-gradient set
    const int step = e.step_count[0];            // Adam's t of this step (ticked by the ELBO launch; nothing in this launch writes it)
    if ((int)blockIdx.x > e.n_item_blocks) {     // the next step's ability noise
        ability_noise_block(blockIdx.x - 1 - e.n_item_blocks, kEpiThreads, tid, e.eps_ab, e.n_ab, (uint32_t)step, e.ab_stream, e.seed_lo, e.seed_hi);
        return;
    }
    const float beta = *e.beta, lr = *e.lr;
    const AdamBias bc = adam_bias(step);
    const int n_parts = kl_part_count(e.n_item_entries);
    const float* kl_now = e.kl_parts + ((step & 1) ? n_parts : 0);
    float* kl_next = e.kl_parts + ((step & 1) ? 0 : n_parts);
    if (blockIdx.x == 0) {
        if (tid == 0) e.step_count[1] += 1;      // completed steps (nothing in this launch reads it)
        // Block 0 is one chain of small dependent stages: every global load it needs is issued up front (parameters and
        // Adam moments into registers, a padded copy of the parameters into LDS for the stages in between), so that the
        // chain pays memory latency once instead of per stage (25 -> ~12 us at 1 000 items).
        const int H = HC > 0 ? HC : e.H;
        const MlpOffsets og = mlp_offsets(H, e.O);
        const bool staged = H <= kEpiStageHidden;                   // (wider encoders read the weights from global memory)
        const MlpOffsets ow = staged ? mlp_offsets(H, e.O, H + 1) : og;
        float pv[kEpiU], mv[kEpiU], vv[kEpiU];
        epi_mlp_prefetch(og.total, e.P, e.M, e.V, pv, mv, vv, tid);
        // the expert table THIS step ran on is kept behind the next one's (thread t writes the new table[t] below, after this read):
        // with it, the rows and the step's noise counter a caller can rebuild the step's ability sample, which the ELBO kernel
        // no longer stores where it draws its own noise
        if (tid < n_table) e.table[n_table + tid] = e.table[tid];
        const float* scp = e.flat_in;
        const float* gtp = e.flat_in + VIBO_NUM_SCALARS;
        if (e.partial) {
            // outputs [0, 8 + 2 n_table) of the logical vector: two sets of 64 outputs x 16 slices, their loads in flight together
            double* scd = &part2[0][0];          // (re-used below as 8 doubles, after the slice sums were consumed)
            double keep = 0.0;
            double ps[2];
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const int o = kEpiOut * pass + lane;
                const bool live = o < VIBO_NUM_SCALARS + 2 * n_table;
                ps[pass] = live ? record_slice_sum<kEpiSlices>(e.partial, (size_t)e.lay.stride, o, 0, e.nblk, slice) : 0.0;
            }
            part[slice][lane] = ps[0];
            part2[slice][lane] = ps[1];
            if (staged) {                        // (the parameter loads have landed by now)
#pragma unroll
                for (int u = 0; u < kEpiU; ++u) {
                    const int k = tid + kEpiThreads * u;
                    if (k < og.total) Pl[mlp_reindex(k, H, e.O, ow)] = pv[u];
                }
            }
            __syncthreads();
            if (slice < 2) {                     // (waves 0 and 1: one set each)
                const int o = kEpiOut * slice + lane;
                if (o < VIBO_NUM_SCALARS + 2 * n_table) {
                    double tsum = 0.0;
#pragma unroll
                    for (int s = 0; s < kEpiSlices; ++s) tsum += slice == 0 ? part[s][lane] : part2[s][lane];
                    if (o >= VIBO_NUM_SCALARS) {
                        gt[o - VIBO_NUM_SCALARS] = (float)tsum;
                        e.flat_out[o] = (float)tsum;
                    } else {
                        keep = tsum;
                    }
                }
            }
            __syncthreads();
            if (slice == 0 && lane < VIBO_NUM_SCALARS) scd[lane] = keep;
            __syncthreads();
            if (tid == 0) {
                // partial scalars: 0 ll, 1 kl, 2 logq0, 3 logp, 4 ladj, 5 nobs  (reg_mode KL: REG = KL)
                sc[VIBO_S_LL] = (float)scd[0]; sc[VIBO_S_REG] = (float)scd[1]; sc[VIBO_S_KL] = (float)scd[1];
                sc[VIBO_S_LOGQ0] = (float)scd[2]; sc[VIBO_S_LOGP] = (float)scd[3]; sc[VIBO_S_LADJ] = (float)scd[4];
                sc[VIBO_S_NOBS] = (float)scd[5]; sc[VIBO_S_RESERVED] = 0.f;
#pragma unroll
                for (int k = 0; k < VIBO_NUM_SCALARS; ++k) e.flat_out[k] = sc[k];
            }
            __syncthreads();
            scp = sc;
            gtp = gt;
        } else if (staged) {
#pragma unroll
            for (int u = 0; u < kEpiU; ++u) {
                const int k = tid + kEpiThreads * u;
                if (k < og.total) Pl[mlp_reindex(k, H, e.O, ow)] = pv[u];
            }
            __syncthreads();
        }
        const float* W = staged ? Pl : e.P;
        epi_mlp_block<HC>(L, H, e.O, n_parts, scp, gtp, e.saved_h, kl_now, beta, lr, bc, W, ow, staged ? Pl : nullptr, e.P, e.M, e.V,
                      pv, mv, vv, e.loss_out, tid);
        // the next step's expert table from the parameters just written (this workgroup's own stores: visible after the barrier)
        __syncthreads();
        float* h1 = &L.h1[0][0];
        float* h2 = &L.h2[0][0];
        mlp2_layer0(W, ow, H, e.O, h1, tid, kEpiThreads);
        __syncthreads();
        mlp2_layer1(W, ow, H, e.O, h1, h2, tid, kEpiThreads);
        __syncthreads();
        mlp2_layer2(W, ow, H, e.O, h1, h2, tid, kEpiThreads, e.table, e.saved_h);
        return;
    }
    // item block: entries k = 64 (block - 1) + lane in the records' order (dim-major: consecutive lanes = consecutive items)
    const int k = kEpiOut * ((int)blockIdx.x - 1) + lane;
    const bool live = k < e.n_item_entries;
    const int dd = live ? k / e.I : 0, i = live ? k % e.I : 0;
    const int idx = i * e.D + dd;
    float g = 0.f;
    if (e.partial) {
        part[slice][lane] = live ? record_slice_sum<kEpiSlices>(e.partial, (size_t)e.lay.stride, e.lay.off_item + dd * e.lay.i_pad + i, 0,
                                                                e.nblk, slice) : 0.0;
        __syncthreads();
        if (slice == 0 && live) {
            double tsum = 0.0;
#pragma unroll
            for (int s = 0; s < kEpiSlices; ++s) tsum += part[s][lane];
            g = (float)tsum;
            e.flat_out[VIBO_NUM_SCALARS + 2 * n_table + idx] = g;
        }
    } else if (slice == 0 && live) {
        g = e.flat_in[VIBO_NUM_SCALARS + 2 * n_table + idx];
    }
    if (slice == 0) {                            // (wave 0 of the block, all 64 lanes: the wave total below needs them)
        float kl = 0.f;
        if (live) {
            float pm, pl;
            epi_item_update(idx, e.n_item_entries, -g, e.eps_item[idx], beta, lr, bc, e.mu, e.lv, e.im, e.iv, pm, pl);
            const float en = philox_normal1(idx, (uint32_t)step, 0u, e.seed_lo, e.seed_hi);
            e.eps_item[idx] = en;
            e.item_feat[idx] = item_sample(pm, pl, en);
            kl = item_kl_term(pm, pl);
        }
        kl = wave_total(kl);
        if (lane == 0) kl_next[blockIdx.x - 1] = kl;
    }
}

__global__ __launch_bounds__(256) void fill_normal_kernel(float* __restrict__ out, long long n, uint32_t seed_lo, uint32_t seed_hi,
                                                          const int32_t* __restrict__ step_count, uint32_t stream_id) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;        // group of 4 outputs
    if (4 * g >= n) return;
    store_normal4(out, n, g, philox_normal4(g, (uint32_t)(*step_count), stream_id, seed_lo, seed_hi));
}

hipError_t launch_train_epilogue_fused(const EpiParams& e, hipStream_t s) {
    const long long ab_blocks = ((e.n_ab + 3) / 4 + kEpiThreads - 1) / kEpiThreads;
    if (e.H == 64) hipLaunchKernelGGL(train_epilogue_fused_kernel<64>, dim3((unsigned)(1 + e.n_item_blocks + ab_blocks)), dim3(kEpiThreads), 0, s, e);
    else hipLaunchKernelGGL(train_epilogue_fused_kernel<0>, dim3((unsigned)(1 + e.n_item_blocks + ab_blocks)), dim3(kEpiThreads), 0, s, e);
    return hipGetLastError();
}
int train_epilogue_item_blocks(int n_item_entries) { return (n_item_entries + kEpiOut - 1) / kEpiOut; }

}  // namespace vibo

using namespace vibo;

extern "C" int vibo_fill_normal(float* out, int64_t n, uint64_t seed, const int32_t* step_count, uint32_t stream_id, void* stream) {
    if (!out || !step_count || n < 0) return -5;
    if (n == 0) return 0;
    const long long groups = (n + 3) / 4;
    hipLaunchKernelGGL(fill_normal_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out,
                       (long long)n, (uint32_t)seed, (uint32_t)(seed >> 32), step_count, stream_id);
    return launch_rc("vibo_fill_normal launch");
}

// what the train-step entry points of this file take (they return -6 otherwise): the plain model, encoder width <= kMaxHidden
static bool plain_ok(const vibo_desc* d, int hidden_dim) {
    return d && hidden_dim >= 1 && hidden_dim <= kMaxHidden && d->posterior == VIBO_POSTERIOR_UNCONDITIONAL && d->n_flows == 0;
}
// (-8: VIBO_MASK_SIGN and VIBO_MASK_TILES are row formats of the ELBO call alone; these calls take the trainer's own descriptor)
static int plain_check(const vibo_desc* d, int hidden_dim) {
    if (d && VIBO_MASK_IS_ELBO_ONLY(d->mask_dtype)) return -8;
    return plain_ok(d, hidden_dim) ? 0 : -6;
}
// train_prologue_kernel: block 0, the item blocks and (gen) the ability-noise blocks behind them
static int launch_prologue(const vibo_desc* d, int hidden_dim, const float* mlp_params, const float* item_mu, const float* item_logvar,
                           const float* eps_item, float* item_feat, float* table, float* saved_h, float* kl_parts, int32_t* step_count,
                           int tick, int gen, uint64_t seed, float* eps_w, float* eps_ability, uint32_t ab_stream, void* stream) {
    const int D = item_feat_dim(d->irt_model, d->ability_dim);
    const int item_blocks = (d->num_item * D + 255) / 256;
    const long long n_ab = gen ? (long long)d->num_person * d->ability_dim : 0;
    const long long ab_blocks = ((n_ab + 3) / 4 + 255) / 256;
    hipLaunchKernelGGL(train_prologue_kernel, dim3((unsigned)(1 + item_blocks + ab_blocks)), dim3(256), 0, (hipStream_t)stream, hidden_dim,
                       2 * d->ability_dim, d->num_item, D, mlp_params, item_mu, item_logvar, eps_item, item_feat, table, saved_h, kl_parts,
                       step_count, tick, gen, (uint32_t)seed, (uint32_t)(seed >> 32), eps_w, eps_ability, n_ab, ab_stream, item_blocks);
    return launch_rc("train prologue launch");
}

extern "C" int vibo_train_prologue(const vibo_desc* d, int hidden_dim, const float* mlp_params, const float* item_mu,
                                   const float* item_logvar, const float* eps_item, float* item_feat, float* table,
                                   float* saved_h, float* kl_parts, int32_t* step_count, void* stream) {
    if (const int rc = plain_check(d, hidden_dim)) return rc;
    return launch_prologue(d, hidden_dim, mlp_params, item_mu, item_logvar, eps_item, item_feat, table, saved_h, kl_parts, step_count, 1, 0, 0,
                           nullptr, nullptr, 0u, stream);
}

extern "C" int vibo_train_prime(const vibo_desc* d, int hidden_dim, const float* mlp_params, const float* item_mu,
                                const float* item_logvar, const float* eps_item, float* item_feat, float* table,
                                float* saved_h, float* kl_parts, int32_t* step_count, void* stream) {
    if (const int rc = plain_check(d, hidden_dim)) return rc;
    if (!mlp_params || !item_mu || !item_logvar || !eps_item || !item_feat || !table || !saved_h || !kl_parts || !step_count) return -5;
    return launch_prologue(d, hidden_dim, mlp_params, item_mu, item_logvar, eps_item, item_feat, table, saved_h, kl_parts, step_count, 0, 0, 0,
                           nullptr, nullptr, 0u, stream);
}

extern "C" int vibo_train_prologue_noise(const vibo_desc* d, int hidden_dim, const float* mlp_params, const float* item_mu,
                                         const float* item_logvar, float* eps_item, float* item_feat, float* table,
                                         float* saved_h, float* kl_parts, int32_t* step_count, uint64_t seed, float* eps_ability,
                                         uint32_t ability_stream_id, void* stream) {
    if (const int rc = plain_check(d, hidden_dim)) return rc;
    if (!eps_item || !eps_ability || !step_count) return -5;
    return launch_prologue(d, hidden_dim, mlp_params, item_mu, item_logvar, eps_item, item_feat, table, saved_h, kl_parts, step_count, 1, 1, seed,
                           eps_item, eps_ability, ability_stream_id, stream);
}

extern "C" int vibo_train_epilogue(const vibo_desc* d, int hidden_dim, const float* flat, const float* saved_h,
                                   const float* kl_parts, const float* eps_item, const float* beta, const float* lr,
                                   const int32_t* step_count, float* mlp_params, float* mlp_m, float* mlp_v,
                                   float* item_mu, float* item_logvar, float* item_m, float* item_v, float* loss_out,
                                   void* stream) {
    if (const int rc = plain_check(d, hidden_dim)) return rc;
    const int n = d->num_item * item_feat_dim(d->irt_model, d->ability_dim);
    const int parts = kl_part_count(n);                      // the prologue's item-KL partial sums (one per 64 entries)
    hipLaunchKernelGGL(train_epilogue_kernel, dim3(1 + (n + kEpiThreads - 1) / kEpiThreads), dim3(kEpiThreads), 0, (hipStream_t)stream,
                       hidden_dim, 2 * d->ability_dim, n, parts, flat, saved_h, kl_parts, eps_item, beta, lr, step_count, mlp_params, mlp_m, mlp_v, item_mu,
                       item_logvar, item_m, item_v, loss_out);
    return launch_rc("vibo_train_epilogue launch");
}
