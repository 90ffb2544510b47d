// vibo_ptrainer.hip -- the native train step of the un-amortized methods (include/vibo_hip_person_tables.h): VI (vi.py: per-person
// mu / logvar tables) and maximum likelihood (mle.py: a per-person ability table), around vibo_elbo_fwd_bwd in
// VIBO_POSTERIOR_GIVEN mode.
//
// Reference (models.py:100-172 / 22-97, vi.py / mle.py's loops): the person rows are nn.Embedding lookups, the optimizer is
// torch.optim.Adam on the DENSE tables -- every row's moments decay and every row moves on momentum each step, in the minibatch or
// not.  Here:
//   pt_prologue_kernel   block 0 ticks Adam's t; item blocks: item sample / item KL / optional Philox noise (VI: vibo_train_hook.hpp);
//                        gather blocks: posterior[b] = the tables' rows of index[b] and the claim slot[index[b]] <- b; noise blocks
//   pt_epilogue_kernel   block 0: loss; item blocks: item backward + Adam; update blocks: the streaming Adam over the P A entries
//                        of each table (24 B per entry: p, m, v in and out), the minibatch's gradient rows found through `slot`
//   pt_reset_kernel      slot[index[b]] <- -1
// The inverse map: slot[p] is -1, or (b << 1) | 1 with b the FIRST position that names person p, bit 0 cleared when a second
// position names it too -- an unsigned atomicMin per position, and an atomicAnd by every position that found the word claimed: the
// final owner either found it claimed itself or is found by a later position, so its word always ends flagged.  Only a flagged
// owner scans the later positions (in order: a fixed sum), so permutation minibatches -- every loop of this project -- pay one
// load of the word and nothing else.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vibo_hip.h"
#include "../../include/vibo_hip_tile_rows.h"
#include "../../include/vibo_hip_person_tables.h"
#include "vibo_device.hpp"
#include "vibo_host.hpp"
#include "vibo_params.hpp"
#include "vibo_philox.hpp"
#include "vibo_train_hook.hpp"

namespace vibo {

constexpr unsigned kSlotEmpty = 0xFFFFFFFFu;      // (-1 as the int32 the caller fills the map with)
constexpr int kPtThreads = 256;

// position b names person idx (in range): first position owns, a second one flags
__device__ __forceinline__ void slot_claim(int32_t* slot, const long long idx, const int b) {
    unsigned* s = reinterpret_cast<unsigned*>(slot) + idx;
    const unsigned old = atomicMin(s, ((unsigned)b << 1) | 1u);
    if (old != kSlotEmpty) atomicAnd(s, ~1u);
}
__device__ __forceinline__ bool index_ok(const long long idx, const long long rows) { return (unsigned long long)idx < (unsigned long long)rows; }

struct PtPrologue {
    int mode, B, A, I, D, gen, n_item_blocks, n_gather_blocks;
    long long rows, n_ab;
    const float *ta, *tb, *item_mu, *item_lv;
    const int64_t* index;
    float *posterior, *eps_item, *eps_ab, *item_feat, *kl_parts;
    int32_t *slot, *bad, *step_count;
    uint32_t seed_lo, seed_hi, ab_stream;
};

__global__ __launch_bounds__(kPtThreads) void pt_prologue_kernel(const PtPrologue q) {
    const int tid = threadIdx.x;
    int blk = blockIdx.x;
    if (blk == 0) {
        if (tid == 0) q.step_count[0] += 1;
        return;
    }
    blk -= 1;
    if (blk < q.n_item_blocks) {                    // (VI only: n_item_blocks is 0 otherwise)
        item_prologue_block(blk, tid, q.I, q.D, q.item_mu, q.item_lv, q.eps_item, q.eps_item, q.gen, q.step_count + 1, q.seed_lo, q.seed_hi,
                            q.item_feat, q.kl_parts);
        return;
    }
    blk -= q.n_item_blocks;
    if (blk < q.n_gather_blocks) {                  // one thread per entry of the [B][2A] posterior table
        const int A2 = 2 * q.A;
        const int t = blk * kPtThreads + tid;
        if (t >= q.B * A2) return;
        const int b = t / A2, c = t % A2;
        const long long idx = q.index[b];
        const bool ok = index_ok(idx, q.rows);
        float val = 0.f;
        if (ok) {
            if (c < q.A) val = q.ta[idx * q.A + c];
            else if (q.mode == VIBO_PTRAIN_VI) val = q.tb[idx * q.A + (c - q.A)];
        }
        q.posterior[t] = val;
        if (c == 0) {
            if (ok) slot_claim(q.slot, idx, b);
            else atomicAdd(q.bad, 1);
        }
        return;
    }
    blk -= q.n_gather_blocks;                       // ability noise (stream ab_stream)
    ability_noise_block(blk, kPtThreads, tid, q.eps_ab, q.n_ab, (uint32_t)q.step_count[1], q.ab_stream, q.seed_lo, q.seed_hi);
}

// the claims alone (vibo_person_table_adam)
__global__ __launch_bounds__(kPtThreads) void pt_claim_kernel(const int64_t* __restrict__ index, int B, long long rows, int32_t* slot, int32_t* bad) {
    const int b = blockIdx.x * kPtThreads + threadIdx.x;
    if (b >= B) return;
    const long long idx = index[b];
    if (index_ok(idx, rows)) slot_claim(slot, idx, b);
    else atomicAdd(bad, 1);
}

__global__ __launch_bounds__(kPtThreads) void pt_reset_kernel(const int64_t* __restrict__ index, int B, long long rows, int32_t* slot) {
    const int b = blockIdx.x * kPtThreads + threadIdx.x;
    if (b >= B) return;
    const long long idx = index[b];
    if (index_ok(idx, rows)) slot[idx] = -1;
}

// ---- the person-table update ----
struct PtUpdate {
    int mode, B, n_tables;
    long long n;                     // entries per table: P A
    long long mstride;               // floats between the tables' moments
    const float *g0, *g1;            // grad_table sets [B][2A]: d LL, d REG
    const int64_t* index;
    const int32_t* slot;
    float *ta, *tb, *M, *V;
    float inv_cells;                 // MLE: 1 / (B num_item)
};

// d loss / d (table `tbl`, person, column a) of minibatch position b (autograd's per-position row, before embedding backward sums)
template <int A>
__device__ __forceinline__ float pt_row_grad(const PtUpdate& u, const float beta, const int b, const int tbl, const int a) {
    const int k = b * (2 * A) + tbl * A + a;
    if (u.mode == VIBO_PTRAIN_VI) return fmaf(beta, u.g1[k], -u.g0[k]);
    return -u.inv_cells * u.g0[k];
}
template <int A>
__device__ __forceinline__ float pt_entry_grad(const PtUpdate& u, const float beta, const int tbl, const long long person, const int a) {
    const unsigned s = (unsigned)u.slot[person];
    if (s == kSlotEmpty) return 0.f;               // not in the minibatch: exactly 0
    const int b = (int)(s >> 1);
    if (b >= u.B) return 0.f;                      // (a map the caller did not fill with -1: never an address outside the gradient rows)
    float g = pt_row_grad<A>(u, beta, b, tbl, a);
    if (!(s & 1u)) {                               // named more than once: the later positions, in order
        for (int b2 = b + 1; b2 < u.B; ++b2)
            if (u.index[b2] == person) g += pt_row_grad<A>(u, beta, b2, tbl, a);
    }
    return g;
}

// groups of 4 consecutive entries [4 gi, 4 gi + 4) of each table, gi = first, first + stride, ...: a group may straddle persons
// (A no multiple of 4); the last group of a table is partial when P A % 4 != 0 and goes entry by entry, like every group when a
// pointer is not 16-byte aligned (VEC false).  64-bit entry offsets.
template <int A, bool VEC>
__device__ __forceinline__ void pt_update(const PtUpdate& u, const float beta, const float lr, const AdamBias bc, const long long first,
                                          const long long stride) {
    const long long groups = (u.n + 3) / 4;
    for (int tbl = 0; tbl < u.n_tables; ++tbl) {
        float* __restrict__ P = tbl == 0 ? u.ta : u.tb;
        float* __restrict__ M = u.M + tbl * u.mstride;
        float* __restrict__ V = u.V + tbl * u.mstride;
        for (long long gi = first; gi < groups; gi += stride) {
            const long long e0 = 4 * gi;
            long long person = e0 / A;
            int a = (int)(e0 % A);
            if (VEC && e0 + 4 <= u.n) {
                float4 p4 = *reinterpret_cast<const float4*>(P + e0);
                float4 m4 = *reinterpret_cast<const float4*>(M + e0);
                float4 v4 = *reinterpret_cast<const float4*>(V + e0);
                float* p = &p4.x; float* m = &m4.x; float* v = &v4.x;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float g = pt_entry_grad<A>(u, beta, tbl, person, a);
                    adam_update(p[j], m[j], v[j], g, lr, bc);
                    if (++a == A) { a = 0; ++person; }
                }
                *reinterpret_cast<float4*>(P + e0) = p4;
                *reinterpret_cast<float4*>(M + e0) = m4;
                *reinterpret_cast<float4*>(V + e0) = v4;
            } else {
                const long long e1 = e0 + 4 < u.n ? e0 + 4 : u.n;
                for (long long e = e0; e < e1; ++e) {
                    float p = P[e], m = M[e], v = V[e];
                    const float g = pt_entry_grad<A>(u, beta, tbl, person, a);
                    adam_update(p, m, v, g, lr, bc);
                    P[e] = p; M[e] = m; V[e] = v;
                    if (++a == A) { a = 0; ++person; }
                }
            }
        }
    }
}

struct PtEpilogue {
    PtUpdate u;
    int head;                        // 1: block 0 and the item blocks in front of the update blocks (the train step); 0: the update alone
    int n_item_entries, n_item_blocks, n_kl_parts, n_table;
    const float *flat, *kl_parts, *eps_item, *beta, *lr;
    int32_t* step_count;
    float *item_mu, *item_lv, *im, *iv, *loss_out;
};

template <int A, bool VEC>
__global__ __launch_bounds__(kPtThreads) void pt_epilogue_kernel(const PtEpilogue e) {
    const int tid = threadIdx.x;
    const bool vi = e.u.mode == VIBO_PTRAIN_VI;
    const float beta = vi ? *e.beta : 0.f, lr = *e.lr;
    const AdamBias bc = adam_bias(e.step_count[0]);
    int blk = blockIdx.x;
    if (e.head) {
        if (blk == 0) {
            if (tid == 0) e.step_count[1] += 1;      // completed steps: the noise counter of the NEXT step (nothing in this launch reads it)
            if (vi) item_kl_loss(tid, e.kl_parts, e.n_kl_parts, e.flat, beta, e.loss_out);
            else if (tid == 0) *e.loss_out = -e.flat[VIBO_S_LL] * e.u.inv_cells;
            return;
        }
        blk -= 1;
        if (blk < e.n_item_blocks) {
            const int idx = blk * kPtThreads + tid;
            if (idx < e.n_item_entries) {
                const float gi = e.flat[VIBO_NUM_SCALARS + 2 * e.n_table + idx];      // d LL / d item
                if (vi) {
                    float pm, pl;
                    epi_item_update(idx, e.n_item_entries, -gi, e.eps_item[idx], beta, lr, bc, e.item_mu, e.item_lv, e.im, e.iv, pm, pl);
                } else {
                    float p = e.item_mu[idx];
                    adam_update(p, e.im[idx], e.iv[idx], -e.u.inv_cells * gi, lr, bc);
                    e.item_mu[idx] = p;
                }
            }
            return;
        }
        blk -= e.n_item_blocks;
    }
    const long long n_upd = (long long)(gridDim.x - (e.head ? 1 + e.n_item_blocks : 0)) * kPtThreads;
    pt_update<A, VEC>(e.u, beta, lr, bc, (long long)blk * kPtThreads + tid, n_upd);
}

static int pt_check(const vibo_desc* d, int mode, int64_t table_rows) {
    if (!d || d->abi_version != VIBO_ABI_VERSION) return -2;
    if (d->ability_dim < 1 || d->ability_dim > VIBO_MAX_ABILITY_DIM || d->num_item < 1 || d->num_person < 1) return -3;
    if (VIBO_MASK_IS_ELBO_ONLY(d->mask_dtype)) return -8;      // (VIBO_MASK_SIGN / _TILES: row formats of the ELBO call alone)
    if (d->posterior != VIBO_POSTERIOR_GIVEN || d->n_flows != 0 || d->reg_mode != VIBO_REG_KL) return -6;
    if (mode != VIBO_PTRAIN_VI && mode != VIBO_PTRAIN_MLE) return -6;
    if (table_rows < 1 || table_rows > ((int64_t)1 << 40)) return -3;
    return 0;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static int update_blocks(long long n) {
    const long long groups = (n + 3) / 4;
    const long long blocks = (groups + kPtThreads - 1) / kPtThreads;
    return (int)(blocks < VIBO_PTRAIN_MAX_BLOCKS ? blocks : VIBO_PTRAIN_MAX_BLOCKS);
}

template <int A>
static hipError_t launch_epilogue_a(const PtEpilogue& e, bool vec, unsigned blocks, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((pt_epilogue_kernel<A, true>), dim3(blocks), dim3(kPtThreads), 0, s, e);
    else hipLaunchKernelGGL((pt_epilogue_kernel<A, false>), dim3(blocks), dim3(kPtThreads), 0, s, e);
    return hipGetLastError();
}
static hipError_t launch_epilogue(const PtEpilogue& e, int A, hipStream_t s) {
    const PtUpdate& u = e.u;
    bool vec = aligned16(u.ta) && aligned16(u.M) && aligned16(u.V);
    if (u.n_tables > 1) vec = vec && aligned16(u.tb) && u.mstride % 4 == 0;
    const unsigned blocks = (unsigned)((e.head ? 1 + e.n_item_blocks : 0) + update_blocks(u.n));
    switch (A) {
        case 1: return launch_epilogue_a<1>(e, vec, blocks, s);
        case 2: return launch_epilogue_a<2>(e, vec, blocks, s);
        case 3: return launch_epilogue_a<3>(e, vec, blocks, s);
        case 4: return launch_epilogue_a<4>(e, vec, blocks, s);
        case 5: return launch_epilogue_a<5>(e, vec, blocks, s);
        case 6: return launch_epilogue_a<6>(e, vec, blocks, s);
        case 7: return launch_epilogue_a<7>(e, vec, blocks, s);
        default: return launch_epilogue_a<8>(e, vec, blocks, s);
    }
}

static PtUpdate make_update(const vibo_desc* d, int mode, int64_t table_rows, const int64_t* index, const float* grad_rows, float* table_a,
                            float* table_b, float* person_m, float* person_v, int64_t moment_stride, const int32_t* slot) {
    PtUpdate u;
    u.mode = mode; u.B = d->num_person; u.n_tables = mode == VIBO_PTRAIN_VI ? 2 : 1;
    u.n = (long long)table_rows * d->ability_dim;
    u.mstride = moment_stride;
    u.g0 = grad_rows; u.g1 = grad_rows + (size_t)d->num_person * 2 * d->ability_dim;
    u.index = index; u.slot = slot;
    u.ta = table_a; u.tb = table_b; u.M = person_m; u.V = person_v;
    u.inv_cells = 1.0f / (float)((double)d->num_person * (double)d->num_item);
    return u;
}

}  // namespace vibo

using namespace vibo;

extern "C" int vibo_ptrain_prologue(const vibo_desc* d, int mode, int64_t table_rows, const float* table_a, const float* table_b,
                                    const int64_t* index, float* posterior, int32_t* slot, int32_t* bad_count, const float* item_mu,
                                    const float* item_logvar, float* eps_item, uint64_t seed, int draw_noise, float* eps_ability,
                                    uint32_t ability_stream_id, float* item_feat, float* kl_parts, int32_t* step_count, void* stream) {
    if (const int rc = pt_check(d, mode, table_rows)) return rc;
    const bool vi = mode == VIBO_PTRAIN_VI;
    if (!table_a || !index || !posterior || !slot || !bad_count || !step_count) return -5;
    if (vi && (!table_b || !item_mu || !item_logvar || !eps_item || !item_feat || !kl_parts)) return -5;
    if (vi && draw_noise && !eps_ability) return -5;
    PtPrologue q;
    q.mode = mode; q.B = d->num_person; q.A = d->ability_dim; q.I = d->num_item; q.D = item_feat_dim(d->irt_model, d->ability_dim);
    q.gen = vi && draw_noise ? 1 : 0;
    q.n_item_blocks = vi ? (q.I * q.D + kPtThreads - 1) / kPtThreads : 0;
    q.n_gather_blocks = (q.B * 2 * q.A + kPtThreads - 1) / kPtThreads;
    q.rows = table_rows;
    q.n_ab = q.gen ? (long long)q.B * q.A : 0;
    q.ta = table_a; q.tb = table_b; q.item_mu = item_mu; q.item_lv = item_logvar;
    q.index = index;
    q.posterior = posterior; q.eps_item = eps_item; q.eps_ab = eps_ability; q.item_feat = item_feat; q.kl_parts = kl_parts;
    q.slot = slot; q.bad = bad_count; q.step_count = step_count;
    q.seed_lo = (uint32_t)seed; q.seed_hi = (uint32_t)(seed >> 32); q.ab_stream = ability_stream_id;
    const long long ab_blocks = ((q.n_ab + 3) / 4 + kPtThreads - 1) / kPtThreads;
    hipLaunchKernelGGL(pt_prologue_kernel, dim3((unsigned)(1 + q.n_item_blocks + q.n_gather_blocks + ab_blocks)), dim3(kPtThreads), 0,
                       (hipStream_t)stream, q);
    return launch_rc("vibo_ptrain_prologue launch");
}

extern "C" int vibo_ptrain_epilogue(const vibo_desc* d, int mode, int64_t table_rows, const float* flat, const int64_t* index,
                                    const float* kl_parts, const float* eps_item, const float* beta, const float* lr, int32_t* step_count,
                                    float* table_a, float* table_b, float* person_m, float* person_v, int64_t moment_stride,
                                    int32_t* slot, float* item_mu, float* item_logvar, float* item_m, float* item_v, float* loss_out,
                                    void* stream) {
    if (const int rc = pt_check(d, mode, table_rows)) return rc;
    const bool vi = mode == VIBO_PTRAIN_VI;
    if (!flat || !index || !lr || !step_count || !table_a || !person_m || !person_v || !slot || !item_mu || !item_m || !item_v || !loss_out)
        return -5;
    if (vi && (!kl_parts || !eps_item || !beta || !table_b || !item_logvar)) return -5;
    if (moment_stride < (long long)table_rows * d->ability_dim) return -3;
    hipStream_t s = (hipStream_t)stream;
    PtEpilogue e;
    e.n_table = d->num_person * 2 * d->ability_dim;
    e.u = make_update(d, mode, table_rows, index, flat + VIBO_NUM_SCALARS, table_a, table_b, person_m, person_v, moment_stride, slot);
    e.head = 1;
    e.n_item_entries = d->num_item * item_feat_dim(d->irt_model, d->ability_dim);
    e.n_item_blocks = (e.n_item_entries + kPtThreads - 1) / kPtThreads;
    e.n_kl_parts = kl_part_count(e.n_item_entries);
    e.flat = flat; e.kl_parts = kl_parts; e.eps_item = eps_item; e.beta = beta; e.lr = lr;
    e.step_count = step_count;
    e.item_mu = item_mu; e.item_lv = item_logvar; e.im = item_m; e.iv = item_v; e.loss_out = loss_out;
    if (const int rc = hip_rc(launch_epilogue(e, d->ability_dim, s), "vibo_ptrain_epilogue launch")) return rc;
    hipLaunchKernelGGL(pt_reset_kernel, dim3((d->num_person + kPtThreads - 1) / kPtThreads), dim3(kPtThreads), 0, s, index, d->num_person,
                       (long long)table_rows, slot);
    return launch_rc("vibo_ptrain_epilogue: slot reset launch");
}

extern "C" int vibo_person_table_adam(const vibo_desc* d, int mode, int64_t table_rows, const int64_t* index, const float* grad_rows,
                                      const float* beta, const float* lr, const int32_t* step_count, float* table_a, float* table_b,
                                      float* person_m, float* person_v, int64_t moment_stride, int32_t* slot, int32_t* bad_count,
                                      void* stream) {
    if (const int rc = pt_check(d, mode, table_rows)) return rc;
    const bool vi = mode == VIBO_PTRAIN_VI;
    if (!index || !grad_rows || !lr || !step_count || !table_a || !person_m || !person_v || !slot || !bad_count) return -5;
    if (vi && (!beta || !table_b)) return -5;
    if (moment_stride < (long long)table_rows * d->ability_dim) return -3;
    hipStream_t s = (hipStream_t)stream;
    const dim3 pos_blocks((d->num_person + kPtThreads - 1) / kPtThreads);
    hipLaunchKernelGGL(pt_claim_kernel, pos_blocks, dim3(kPtThreads), 0, s, index, d->num_person, (long long)table_rows, slot, bad_count);
    if (const int rc = launch_rc("vibo_person_table_adam: slot claim launch")) return rc;
    PtEpilogue e = {};
    e.u = make_update(d, mode, table_rows, index, grad_rows, table_a, table_b, person_m, person_v, moment_stride, slot);
    e.head = 0;
    e.beta = beta; e.lr = lr;
    e.step_count = const_cast<int32_t*>(step_count);      // (head == 0: only read)
    if (const int rc = hip_rc(launch_epilogue(e, d->ability_dim, s), "vibo_person_table_adam launch")) return rc;
    hipLaunchKernelGGL(pt_reset_kernel, pos_blocks, dim3(kPtThreads), 0, s, index, d->num_person, (long long)table_rows, slot);
    return launch_rc("vibo_person_table_adam: slot reset launch");
}
