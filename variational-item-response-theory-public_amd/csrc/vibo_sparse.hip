// vibo_sparse.hip -- the ELBO, the encode and the validation pass on sparse response rows (include/vibo_hip_sparse_rows.h: THE IMAGE,
// THE GRID RULE), with their extern "C" tails.  The plain model only: unconditional product-of-experts posterior, IRT decoder, no flows.
// What this unit shares with the row-driven item pass (vibo_sparse_row_driven.hip) is in vibo_sparse_device.hpp.
// The person, encode and item kernels are stated once and instantiated twice: for a contiguous range of persons (GATHER = false, the
// calls of that header) and for an index vector of persons (GATHER = true, include/vibo_hip_sparse_gather.h: THE INDEX AND THE MAP).
//
//   person pass   one wave per row of the call, lane l the row's cells l, l + 64, ...:
//                 counts (answered wrong / right) -> product of experts from the counts -> sample, heads -> decode over the row's cells
//                 (gather of the item's row, logit, log-likelihood, d LL / d theta) -> backward into per-wave sums of the 2-row table
//                 gradient.  theta goes to `ability`; every wave leaves one partial record.
//   item pass     one wave per chunk of a column's list: bisect the chunk to the call's persons, gather theta, the same logit
//                 statements again, d LL / d item summed over the chunk (no g[nnz] store, no read-back through a permutation).
//   gathered      the person pass takes a row's person from person_index; the item pass walks whole chunks and finds a person's row of
//                 the call in person_slot, a map built before the person pass (an integer atomicMin) and cleared after the item finish.
//   finish        fixed-order sums of the waves' records (heads, table gradient) and of the chunks' records (items of several chunks).
// The statements of the math are those of the unconditional branch of vibo_general.hip; the table gradient's row-invariant factors
// (tau; tau^2 exp(logvar)) are multiplied in once per wave instead of once per row.  No float atomics, no LDS, no index is trusted.
#include <hip/hip_runtime.h>
#include "vibo_sparse_device.hpp"

namespace vibo {

constexpr int kChunk = VIBO_SPARSE_CHUNK;
constexpr int kRec = VIBO_SPARSE_RECORD_FLOATS;
constexpr int kRecTable = 8;            // the record's table gradient starts here: [2][2][16]

// first k in [lo, hi) with (cell[k] >> 1) >= key, or hi
__device__ __forceinline__ long long lower_bound_cell(const uint32_t* cell, long long lo, long long hi, long long key) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if ((long long)(cell[mid] >> 1) < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The person q of the call's row r: row0 + r, or (GATHER) person_index[r].  -> whether the row is live: q inside the image and, where the
// call has a map (`mapped`: gradients), row r the one that owns q.  Wave-uniform.
template <bool GATHER>
__device__ __forceinline__ bool row_person(const SparseParams& p, const long long r, const bool mapped, long long& q) {
    if constexpr (!GATHER) {
        q = p.row0 + r;
        return true;
    } else {
        q = p.person_index[r];
        if (q < 0 || q >= p.P) return false;
        if (mapped && p.person_slot[q] != (int32_t)r) return false;
        unsigned qv = (unsigned)q;                  // (q < P < 2^31)
        asm volatile("" : "+v"(qv));                // (kept in a vector register: as scalars the person and its cell range spill scalar registers at MA = 3)
        q = qv;
        return true;
    }
}

// Person q: its cell range (pointer entries clamped to [0, nnz]) and its counts; cells whose item is >= I are counted in `bad`.
__device__ __forceinline__ void row_counts(const SparseParams& p, const long long q, const int lane, long long& k0, long long& k1,
                                           int& n0, int& n1, int& bad) {
    k0 = clamp_ll(p.row_ptr[q], 0, p.nnz);
    k1 = clamp_ll(p.row_ptr[q + 1], k0, p.nnz);
    int c0 = 0, c1 = 0;
    for (long long k = k0 + lane; k < k1; k += 64) {
        const uint32_t c = p.row_cell[k];
        if ((c >> 1) >= (uint32_t)p.I) { ++bad; continue; }
        if (c & 1u) ++c1; else ++c0;
    }
    n0 = wave_total_i(c0);
    n1 = wave_total_i(c1);
}

// Product of experts from the counts (vibo_general.hip pass 1 as a function of n0, n1 and I - n_observed): precision and mean of dim a.
__device__ __forceinline__ void poe_counts(const float n0, const float n1, const float nmiss_prior, const float tau0, const float tau1,
                                           const float m0, const float m1, float& ilam, float& amu) {
    float lam = n0 * tau0;
    lam = fmaf(n1, tau1, lam);
    lam = fmaf(nmiss_prior, 1.0f / (1.0f + kPoeEps), lam);
    float smu = n0 * (m0 * tau0);
    smu = fmaf(n1, m1 * tau1, smu);
    ilam = 1.0f / lam;
    amu = smu * ilam;
}

template <int MA, bool GATHER>
__global__ __launch_bounds__(256) void sparse_person_kernel(const SparseParams p) {
    const int lane = threadIdx.x & 63;
    constexpr int A = MA;      // (one instantiation per ability_dim: every `a < A` below is decided at compile time)
    const int D = p.D, irt = p.irt;
    const bool grad = p.want_grad != 0;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * 4;

    float tm[2][MA], tau[2][MA];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int a = 0; a < MA; ++a) {
            tm[c][a] = tau[c][a] = 0.f;
            if (a < A) {
                tm[c][a] = p.table[c * 2 * A + a];
                tau[c][a] = 1.0f / (expf(p.table[c * 2 * A + A + a]) + kPoeEps);
                asm volatile("" : "+v"(tm[c][a]));      // (kept in a vector register: as scalars the 2 x MA means spill at MA = 8)
            }
        }
    float acc_m[2][2][MA], acc_t[2][2][MA];      // [set][code][dim]: the row sums in front of the row-invariant factors
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int a = 0; a < MA; ++a) acc_m[s][c][a] = acc_t[s][c][a] = 0.f;
    float s_ll = 0.f, s_kl = 0.f, s_logq0 = 0.f, s_logp = 0.f;
    int s_nobs = 0;      // (an integer: the count of a large image is past fp32's 2^24)
    int bad = 0;

    for (long long r = w; r < p.B; r += n_waves) {
        long long q, k0, k1;
        if (!row_person<GATHER>(p, r, grad, q)) {      // an index outside the image, or a person an earlier row owns: zeros, one more in `bad`
            if (lane == 0) {
#pragma unroll
                for (int a = 0; a < MA; ++a)
                    if (a < A) p.ability_mu[r * A + a] = p.ability_logvar[r * A + a] = p.ability[r * A + a] = 0.f;
                ++bad;
            }
            continue;
        }
        int n0i, n1i;
        row_counts(p, q, lane, k0, k1, n0i, n1i, bad);
        const float n0 = (float)n0i, n1 = (float)n1i;
        const float nmiss = p.missing_mode == VIBO_MISSING_PRIOR ? (float)(p.I - n0i - n1i) : 0.f;
        s_nobs += n0i + n1i;

        float amu[MA], alv[MA], sig[MA], epsv[MA], th[MA], ilam[MA];
        float kl = 0.f, logq0 = 0.f, logp = 0.f;
#pragma unroll
        for (int a = 0; a < MA; ++a) {
            amu[a] = alv[a] = sig[a] = epsv[a] = th[a] = ilam[a] = 0.f;
            if (a < A) {
                poe_counts(n0, n1, nmiss, tau[0][a], tau[1][a], tm[0][a], tm[1][a], ilam[a], amu[a]);
                alv[a] = logf(ilam[a]);
                sig[a] = sqrtf(ilam[a]);
                epsv[a] = p.eps[r * A + a];
                asm volatile("" : "+v"(epsv[a]));
                th[a] = amu[a] + sig[a] * epsv[a];
                kl += -0.5f * (1.0f + alv[a] - amu[a] * amu[a] - ilam[a]);
                logq0 += -0.5f * kLog2Pi - 0.5f * alv[a] - 0.5f * epsv[a] * epsv[a];
                logp += -0.5f * kLog2Pi - 0.5f * th[a] * th[a];
            }
        }
        s_kl += kl; s_logq0 += logq0; s_logp += logp;
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < MA; ++a)
                if (a < A) {
                    p.ability_mu[r * A + a] = amu[a];
                    p.ability_logvar[r * A + a] = alv[a];
                    p.ability[r * A + a] = th[a];
                }
        }

        // decode over the row's cells
        float gth[MA];
#pragma unroll
        for (int a = 0; a < MA; ++a) gth[a] = 0.f;
        for (long long k = k0 + lane; k < k1; k += 64) {
            const uint32_t c = p.row_cell[k];
            const uint32_t i = c >> 1;
            if (i >= (uint32_t)p.I) continue;           // (counted by row_counts)
            const float* it = p.item + (size_t)i * D;
            float disc[MA], diff, glogit = 0.f;
#pragma unroll
            for (int a = 0; a < MA; ++a) disc[a] = 0.f;
            if (irt == 1) {
                diff = it[0];
            } else {
#pragma unroll
                for (int a = 0; a < MA; ++a)
                    if (a < A) disc[a] = it[a];
                diff = it[A];
                if (irt == 3) glogit = it[A + 1];
            }
            float ll, gl, gguess;
            cell_terms<MA>(irt, A, disc, diff, glogit, th, (c & 1u) ? 1.f : 0.f, ll, gl, gguess);
            s_ll += ll;
#pragma unroll
            for (int a = 0; a < MA; ++a)
                if (a < A) gth[a] = (irt == 1) ? gth[a] + gl : fmaf(gl, -disc[a], gth[a]);
        }
        if (!grad) continue;

        // backward through the sample and the product of experts (vibo_general.hip pass 3, unconditional)
#pragma unroll
        for (int a = 0; a < MA; ++a) {
            if (a < A) {
                float gz0 = wave_total(gth[a]);
                asm volatile("" : "+v"(gz0));           // (likewise: the wave totals are read by vector arithmetic only)
                const float gz1 = (p.reg_mode == VIBO_REG_SAMPLED) ? th[a] : 0.f;
                const float h = 0.5f * sig[a] * epsv[a];
                const float gmu0 = gz0, glv0 = gz0 * h;
                float gmu1 = gz1, glv1 = gz1 * h;
                if (p.reg_mode == VIBO_REG_KL) {
                    gmu1 += amu[a];
                    glv1 += -0.5f * (1.0f - ilam[a]);
                } else {
                    glv1 += -0.5f;
                }
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float nn = c ? n1 : n0;
                    acc_m[0][c][a] += gmu0 * ilam[a] * nn;
                    acc_t[0][c][a] += (gmu0 * (tm[c][a] - amu[a]) - glv0) * ilam[a] * nn;
                    acc_m[1][c][a] += gmu1 * ilam[a] * nn;
                    acc_t[1][c][a] += (gmu1 * (tm[c][a] - amu[a]) - glv1) * ilam[a] * nn;
                }
            }
        }
    }

    // the wave's record
    const float tll = wave_total(s_ll);
    const int tbad = wave_total_i(bad);
    if (lane == 0) {
        float* rec = p.records + (size_t)w * kRec;
        rec[0] = tll; rec[1] = s_kl; rec[2] = s_logq0; rec[3] = s_logp; rec[4] = __int_as_float(s_nobs); rec[5] = rec[6] = rec[7] = 0.f;
        // the table part [2][2][16]: entry j of a [2A] row -- the mean's gradient at j = a, the log-variance's at j = A + a; the rest stays zero
        for (int j = 0; j < 64; ++j) rec[kRecTable + j] = 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int a = 0; a < MA; ++a)
                    if (a < A) {
                        const float es = expf(p.table[c * 2 * A + A + a]);
                        rec[kRecTable + (s * 2 + c) * 16 + a] = acc_m[s][c][a] * tau[c][a];
                        rec[kRecTable + (s * 2 + c) * 16 + A + a] = -acc_t[s][c][a] * tau[c][a] * tau[c][a] * es;
                    }
        if (tbad > 0 && p.bad) atomicAdd(p.bad, (unsigned long long)tbad);
    }
}

// vibo_sparse_encode: the posterior of the call's rows from their counts
template <int MA, bool GATHER>
__global__ __launch_bounds__(256) void sparse_encode_kernel(const SparseParams p) {
    const int lane = threadIdx.x & 63;
    constexpr int A = MA;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * 4;
    int bad = 0;
    for (long long r = w; r < p.B; r += n_waves) {
        long long q, k0, k1;
        if (!row_person<GATHER>(p, r, false, q)) {      // (no map: every row is independent, repeats are ordinary rows)
            if (lane == 0) {
#pragma unroll
                for (int a = 0; a < MA; ++a)
                    if (a < A) p.ability_mu[r * A + a] = p.ability_logvar[r * A + a] = 0.f;
                ++bad;
            }
            continue;
        }
        int n0i, n1i;
        row_counts(p, q, lane, k0, k1, n0i, n1i, bad);
        const float nmiss = p.missing_mode == VIBO_MISSING_PRIOR ? (float)(p.I - n0i - n1i) : 0.f;
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < MA; ++a)
                if (a < A) {
                    const float tau0 = 1.0f / (expf(p.table[A + a]) + kPoeEps), tau1 = 1.0f / (expf(p.table[2 * A + A + a]) + kPoeEps);
                    float ilam, amu;
                    poe_counts((float)n0i, (float)n1i, nmiss, tau0, tau1, p.table[a], p.table[2 * A + a], ilam, amu);
                    p.ability_mu[r * A + a] = amu;
                    p.ability_logvar[r * A + a] = logf(ilam);
                }
        }
    }
    const int tbad = wave_total_i(bad);
    if (lane == 0 && tbad > 0 && p.bad) atomicAdd(p.bad, (unsigned long long)tbad);
}

template <int MA, bool GATHER>
__global__ __launch_bounds__(256) void sparse_item_kernel(const SparseParams p) {
    const int lane = threadIdx.x & 63;
    constexpr int A = MA;      // (one instantiation per ability_dim: every `a < A` below is decided at compile time)
    const int D = p.D, irt = p.irt;
    const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= p.num_chunk) return;                          // (wave-uniform)
    const int i = p.chunk_item[c];
    if (i < 0 || i >= p.I) return;                         // a chunk list that names no item: nothing is read or written
    const long long first = clamp_ll(p.chunk_first[c], 0, p.nnz);
    long long end = clamp_ll(p.col_ptr[i + 1], first, p.nnz);
    if (end > first + kChunk) end = first + kChunk;
    // the call's entries: a range of persons is one window of the sorted chunk; an index vector may name any of them (the whole chunk)
    long long lo = first, hi = end;
    if constexpr (!GATHER) {
        lo = lower_bound_cell(p.col_cell, first, end, p.row0);
        hi = lower_bound_cell(p.col_cell, lo, end, p.row0 + p.B);
    }

    const float* it = p.item + (size_t)i * D;
    float disc[MA], diff, glogit = 0.f;
#pragma unroll
    for (int a = 0; a < MA; ++a) disc[a] = 0.f;
    if (irt == 1) {
        diff = it[0];
    } else {
#pragma unroll
        for (int a = 0; a < MA; ++a)
            if (a < A) disc[a] = it[a];
        diff = it[A];
        if (irt == 3) glogit = it[A + 1];
    }

    float gd[MA], gb = 0.f, gg = 0.f;
#pragma unroll
    for (int a = 0; a < MA; ++a) gd[a] = 0.f;
    int bad = 0;
    for (long long k = lo + lane; k < hi; k += 64) {
        const uint32_t cell = p.col_cell[k];
        const long long q = cell >> 1;
        if (q >= p.P) { ++bad; continue; }
        long long r;
        if constexpr (GATHER) {
            r = p.person_slot[q];
            if (r == VIBO_SPARSE_NO_SLOT) continue;        // not a person of this call
        } else {
            r = q - p.row0;
        }
        if (r < 0 || r >= p.B) continue;                   // (a list out of order, a map entry that is no row: the person is not this call's)
        float th[MA];
#pragma unroll
        for (int a = 0; a < MA; ++a) th[a] = (a < A) ? p.ability[r * A + a] : 0.f;
        float ll, gl, gguess;
        cell_terms<MA>(irt, A, disc, diff, glogit, th, (cell & 1u) ? 1.f : 0.f, ll, gl, gguess);
        gb += gl;
        gg += gguess;
#pragma unroll
        for (int a = 0; a < MA; ++a)
            if (a < A) gd[a] = fmaf(-gl, th[a], gd[a]);
    }

    // column j of the item's row: 1PL [difficulty]; 2PL / 3PL [discrimination 0..A-1 | difficulty | guess logit]
    float out = 0.f;
    if (irt == 1) {
        out = wave_total(gb);
    } else {
#pragma unroll
        for (int a = 0; a < MA; ++a)
            if (a < A) {
                const float t = wave_total(gd[a]);
                if (lane == a) out = t;
            }
        const float tb = wave_total(gb);
        if (lane == A) out = tb;
        if (irt == 3) {
            const float tg = wave_total(gg);
            if (lane == A + 1) out = tg;
        }
    }
    const long long c0 = clamp_ll(p.col_chunk[i], 0, p.num_chunk), c1 = clamp_ll(p.col_chunk[i + 1], 0, p.num_chunk);
    float* dst = (c1 - c0 == 1) ? p.grad_item + (size_t)i * D : p.chunk_rec + (size_t)c * D;
    if (lane < D) dst[lane] = out;
    const int tbad = wave_total_i(bad);
    if (lane == 0 && tbad > 0 && p.bad) atomicAdd(p.bad, (unsigned long long)tbad);
}

// finish, heads and table gradient: workgroup 0 the four head sums and the cell count, workgroup 1 + e entry e of the records' [2][2][16] table part
__global__ __launch_bounds__(64) void sparse_finish_kernel(const float* records, const int n_rec, const int A, const int reg_mode,
                                                           float* out_scalars, float* grad_table) {
    const int lane = threadIdx.x;
    if (blockIdx.x == 0) {
        float t[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = 0.f;
            for (int r = lane; r < n_rec; r += 64) v += records[(size_t)r * kRec + e];
            t[e] = wave_total(v);
        }
        // the cells: the waves' int32 counts added exactly, rounded to fp32 once
        long long n = 0;
        for (int r = lane; r < n_rec; r += 64) n += __float_as_int(records[(size_t)r * kRec + 4]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m);
        if (lane == 0) {
            out_scalars[VIBO_S_LL] = t[0];
            out_scalars[VIBO_S_REG] = (reg_mode == VIBO_REG_KL) ? t[1] : (t[2] - 0.f - t[3]);
            out_scalars[VIBO_S_KL] = t[1];
            out_scalars[VIBO_S_LOGQ0] = t[2];
            out_scalars[VIBO_S_LOGP] = t[3];
            out_scalars[VIBO_S_LADJ] = 0.f;
            out_scalars[VIBO_S_NOBS] = (float)n;
            out_scalars[VIBO_S_RESERVED] = 0.f;
        }
        return;
    }
    const int e = blockIdx.x - 1, sc = e >> 4, j = e & 15;
    if (j >= 2 * A) return;
    float v = 0.f;
    for (int r = lane; r < n_rec; r += 64) v += records[(size_t)r * kRec + kRecTable + e];
    const float t = wave_total(v);
    if (lane == 0) grad_table[sc * 2 * A + j] = t;
}

// finish, items: an item of no chunk gets zeros, an item of several chunks the sum of its chunks' records in chunk order
__global__ __launch_bounds__(256) void sparse_item_finish_kernel(const int64_t* col_chunk, const long long num_chunk, const float* chunk_rec,
                                                                 const int I, const int D, float* grad_item) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)I * D) return;
    const int i = (int)(t / D), j = (int)(t - (long long)i * D);
    const long long c0 = clamp_ll(col_chunk[i], 0, num_chunk), c1 = clamp_ll(col_chunk[i + 1], 0, num_chunk);
    if (c1 - c0 == 1) return;
    float v = 0.f;
    for (long long c = c0; c < c1; ++c) v += chunk_rec[(size_t)c * D + j];
    grad_item[t] = v;
}

// ---- vibo_sparse_rows_check ----
// One side of the image: n_lists lists by `ptr` over `cell`, indices below `limit`.  other_ptr / other_cell: the row side, for the
// column side's membership checks (null on the row side).
__global__ __launch_bounds__(256) void sparse_check_side_kernel(const int64_t* ptr, const uint32_t* cell, const long long n_lists,
                                                                const long long limit, const long long nnz, const int64_t* other_ptr,
                                                                const uint32_t* other_cell, const long long other_lists,
                                                                unsigned long long* violations) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * 4;
    int v = 0;
    for (long long q = w; q < n_lists; q += n_waves) {
        const long long a = ptr[q], b = ptr[q + 1];
        if (lane == 0) {
            if (q == 0 && a != 0) ++v;
            if (q == n_lists - 1 && b != nnz) ++v;
        }
        if (a < 0 || a > nnz || b < 0 || b > nnz || a > b) {
            if (lane == 0) ++v;
            continue;
        }
        for (long long k = a + lane; k < b; k += 64) {
            const uint32_t c = cell[k];
            const long long idx = c >> 1;
            if (idx >= limit) ++v;
            if (k > a && (long long)(cell[k - 1] >> 1) >= idx) ++v;
            if (other_ptr != nullptr && idx < other_lists) {
                const long long ra = other_ptr[idx], rb = other_ptr[idx + 1];
                bool found = false;
                if (ra >= 0 && ra <= rb && rb <= nnz) {
                    const long long pos = lower_bound_cell(other_cell, ra, rb, q);
                    found = pos < rb && other_cell[pos] == (((uint32_t)q << 1) | (c & 1u));
                }
                if (!found) ++v;
            }
        }
    }
    const int tv = wave_total_i(v);
    if (lane == 0 && tv > 0) atomicAdd(violations, (unsigned long long)tv);
}

__global__ __launch_bounds__(256) void sparse_check_chunks_kernel(const int64_t* col_ptr, const int64_t* col_chunk, const int32_t* chunk_item,
                                                                  const int64_t* chunk_first, const long long I, const long long nnz,
                                                                  const long long num_chunk, unsigned long long* violations) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= I) return;
    int v = 0;
    const long long c0 = col_chunk[i], c1 = col_chunk[i + 1];
    if (i == 0 && c0 != 0) ++v;
    if (i == I - 1 && c1 != num_chunk) ++v;
    const long long a = col_ptr[i], b = col_ptr[i + 1];
    if (!(a < 0 || a > nnz || b < 0 || b > nnz || a > b)) {          // (a bad pair of pointers is the side pass's finding)
        const long long expect = (b - a + kChunk - 1) / kChunk;
        if (c0 < 0 || c1 > num_chunk || c1 - c0 != expect) {
            ++v;
        } else {
            for (long long t = 0; t < expect; ++t)
                if (chunk_item[c0 + t] != (int32_t)i || chunk_first[c0 + t] != a + t * kChunk) ++v;
        }
    }
    if (v > 0) atomicAdd(violations, (unsigned long long)v);
}

// ---- host ----
int sparse_desc_rc(const vibo_desc* d) {
    if (!d) return fail(-1, "sparse rows: null descriptor");
    if (d->abi_version != VIBO_ABI_VERSION) return fail(-2, "sparse rows: abi_version %d != %d", d->abi_version, VIBO_ABI_VERSION);
    if (d->num_person < 1) return fail(-3, "sparse rows: num_person must be >= 1");
    if (d->num_item < 1) return fail(-3, "sparse rows: num_item must be >= 1");
    if (d->ability_dim < 1 || d->ability_dim > VIBO_MAX_ABILITY_DIM_WIDE)
        return fail(-3, "sparse rows: ability_dim %d outside 1..%d", d->ability_dim, VIBO_MAX_ABILITY_DIM_WIDE);
    if (d->irt_model < 1 || d->irt_model > 3) return fail(-3, "sparse rows: irt_model must be 1, 2 or 3");
    if (d->posterior != VIBO_POSTERIOR_UNCONDITIONAL && d->posterior != VIBO_POSTERIOR_CONDITIONAL && d->posterior != VIBO_POSTERIOR_GIVEN)
        return fail(-3, "sparse rows: bad posterior");
    if (d->missing_mode != VIBO_MISSING_PRIOR && d->missing_mode != VIBO_MISSING_DROP) return fail(-3, "sparse rows: bad missing_mode");
    if (d->reg_mode != VIBO_REG_KL && d->reg_mode != VIBO_REG_SAMPLED) return fail(-3, "sparse rows: bad reg_mode");
    if (d->n_flows < 0 || d->n_flows > VIBO_MAX_FLOWS) return fail(-3, "sparse rows: n_flows outside 0..%d", VIBO_MAX_FLOWS);
    if (d->posterior == VIBO_POSTERIOR_CONDITIONAL) return fail(-8, "sparse rows: the conditional posterior is not covered (unconditional only)");
    if (d->posterior == VIBO_POSTERIOR_GIVEN) return fail(-8, "sparse rows: a caller-supplied posterior is not covered (unconditional only)");
    if (d->n_flows != 0) return fail(-8, "sparse rows: planar flows are not covered (n_flows must be 0)");
    if (d->ability_dim > VIBO_MAX_ABILITY_DIM) return fail(-8, "sparse rows: ability_dim %d is not covered (1..%d)", d->ability_dim, VIBO_MAX_ABILITY_DIM);
    return 0;
}

int sparse_item_dim(const vibo_desc* d) { return d->irt_model == 1 ? 1 : d->ability_dim + (d->irt_model == 3 ? 2 : 1); }
int sparse_person_blocks(int B) {
    const int g = (B + VIBO_SPARSE_ROWS_PER_BLOCK - 1) / VIBO_SPARSE_ROWS_PER_BLOCK;
    return g > VIBO_SPARSE_MAX_BLOCKS ? VIBO_SPARSE_MAX_BLOCKS : g;
}
size_t sparse_record_bytes(const vibo_desc* d) { return up256((size_t)sparse_person_blocks(d->num_person) * 4 * kRec * sizeof(float)); }

// the image against the descriptor and (ranged) the call's range: 0, or the code (error string set)
int sparse_image_rc(const vibo_desc* d, const vibo_sparse_image* im, int64_t row0, bool need_cols, bool ranged) {
    if (!im) return fail(-5, "sparse rows: null image");
    if (im->num_person < 1 || im->num_person >= (1ll << 31) || im->num_item < 1 || im->num_item >= (1ll << 31) || im->nnz < 0 || im->num_chunk < 0)
        return fail(-3, "sparse rows: image sizes out of range (1 <= P, I < 2^31; nnz, num_chunk >= 0)");
    if (d && im->num_item != d->num_item) return fail(-3, "sparse rows: the image has %lld items, the descriptor %d", (long long)im->num_item, d->num_item);
    if (d && ranged && (row0 < 0 || row0 + d->num_person > im->num_person))
        return fail(-3, "sparse rows: persons [%lld, %lld) are outside the image's %lld", (long long)row0, (long long)row0 + d->num_person, (long long)im->num_person);
    if (!im->row_ptr || (im->nnz > 0 && !im->row_cell)) return fail(-5, "sparse rows: null row side");
    if (need_cols) {
        if (!im->col_ptr) return fail(-8, "sparse rows: gradients need the image's column side");
        if (!im->col_chunk || (im->nnz > 0 && !im->col_cell) || (im->num_chunk > 0 && (!im->chunk_item || !im->chunk_first)))
            return fail(-5, "sparse rows: null column-side pointer");
    }
    return 0;
}

static SparseParams sparse_params(const vibo_desc* d, const vibo_sparse_image* im, int64_t row0) {
    SparseParams p = {};
    p.row_ptr = im->row_ptr; p.row_cell = im->row_cell; p.col_ptr = im->col_ptr; p.col_cell = im->col_cell;
    p.col_chunk = im->col_chunk; p.chunk_item = im->chunk_item; p.chunk_first = im->chunk_first;
    p.P = im->num_person; p.nnz = im->nnz; p.num_chunk = im->num_chunk; p.row0 = row0;
    p.I = d->num_item; p.B = d->num_person; p.A = d->ability_dim; p.D = sparse_item_dim(d);
    p.irt = d->irt_model; p.missing_mode = d->missing_mode; p.reg_mode = d->reg_mode; p.want_grad = d->want_grad ? 1 : 0;
    return p;
}

// one instantiation per ability_dim 1..VIBO_MAX_ABILITY_DIM, for a range (G = false) and for an index vector (G = true)
#define VIBO_SPARSE_LAUNCH(kernel, W, G, grid, stream, p) hipLaunchKernelGGL((kernel<W, G>), dim3((unsigned)(grid)), dim3(256), 0, stream, p)
#define VIBO_SPARSE_BY_WIDTH_G(kernel, A, G, grid, stream, p)                \
    switch (A) {                                                             \
        case 1: VIBO_SPARSE_LAUNCH(kernel, 1, G, grid, stream, p); break;    \
        case 2: VIBO_SPARSE_LAUNCH(kernel, 2, G, grid, stream, p); break;    \
        case 3: VIBO_SPARSE_LAUNCH(kernel, 3, G, grid, stream, p); break;    \
        case 4: VIBO_SPARSE_LAUNCH(kernel, 4, G, grid, stream, p); break;    \
        case 5: VIBO_SPARSE_LAUNCH(kernel, 5, G, grid, stream, p); break;    \
        case 6: VIBO_SPARSE_LAUNCH(kernel, 6, G, grid, stream, p); break;    \
        case 7: VIBO_SPARSE_LAUNCH(kernel, 7, G, grid, stream, p); break;    \
        default: VIBO_SPARSE_LAUNCH(kernel, 8, G, grid, stream, p); break;   \
    }
#define VIBO_SPARSE_BY_WIDTH(kernel, A, gather, grid, stream, p)             \
    if (gather) { VIBO_SPARSE_BY_WIDTH_G(kernel, A, true, grid, stream, p) } else { VIBO_SPARSE_BY_WIDTH_G(kernel, A, false, grid, stream, p) }

// The ELBO call on a range (gather == false: row0) or on an index vector (gather == true: person_index, person_slot), after the
// descriptor and the image have passed their checks: the rest of the checks and the launches.  max_row_cells > 0 (gathered, with
// gradients): the row-driven item pass of vibo_sparse_row_driven.hip in place of the column-driven one; the column side is not read.
int sparse_elbo_call(const vibo_desc* d, const vibo_sparse_image* im, bool gather, int64_t row0, const int64_t* person_index,
                     int32_t* person_slot, const float* table, const float* item, const float* eps, float* out_scalars,
                     float* ability_mu, float* ability_logvar, float* ability, float* grad_table, float* grad_item,
                     int64_t* bad_cells, void* workspace, size_t workspace_bytes, void* stream, long long max_row_cells) {
    int rc = 0;
    const bool grad = d->want_grad != 0;
    const bool row_driven = gather && grad && max_row_cells > 0;
    if (!table || !item || !eps || !out_scalars || !ability_mu || !ability_logvar || !ability || (grad && (!grad_table || !grad_item)))
        return fail(-5, "sparse rows: null required pointer");
    const size_t need = row_driven ? vibo_sparse_row_driven_workspace_bytes(d, im->num_item, im->num_person, max_row_cells)
                                   : vibo_sparse_workspace_bytes(d, grad ? im->num_chunk : 0);
    if (!workspace || workspace_bytes < need) return fail(-7, "sparse rows: workspace too small: %zu < %zu", workspace_bytes, need);
    if ((uintptr_t)workspace & 255) return fail(-7, "sparse rows: workspace must be 256-byte aligned");

    hipStream_t s = (hipStream_t)stream;
    SparseParams p = sparse_params(d, im, row0);
    p.person_index = person_index; p.person_slot = person_slot;
    p.table = table; p.item = item; p.eps = eps;
    p.ability_mu = ability_mu; p.ability_logvar = ability_logvar; p.ability = ability; p.grad_item = grad_item;
    p.records = static_cast<float*>(workspace);
    p.chunk_rec = reinterpret_cast<float*>(static_cast<char*>(workspace) + sparse_record_bytes(d));
    p.bad = reinterpret_cast<unsigned long long*>(bad_cells);
    const int G = sparse_person_blocks(p.B);
    const bool mapped = gather && grad;
    const unsigned map_grid = (unsigned)(((long long)p.B + 255) / 256);
    if (mapped) {
        hipLaunchKernelGGL(sparse_map_kernel<true>, dim3(map_grid), dim3(256), 0, s, person_index, (long long)p.B, p.P, person_slot);
        if ((rc = launch_rc("sparse rows map build launch")) != 0) return rc;
    }
    VIBO_SPARSE_BY_WIDTH(sparse_person_kernel, p.A, gather, G, s, p);
    if ((rc = launch_rc("sparse rows person pass launch")) != 0) return rc;
    hipLaunchKernelGGL(sparse_finish_kernel, dim3(grad ? 65u : 1u), dim3(64), 0, s, p.records, 4 * G, p.A, p.reg_mode, out_scalars, grad_table);
    if ((rc = launch_rc("sparse rows finish launch")) != 0) return rc;
    if (!grad) return 0;
    if (row_driven) {
        if ((rc = sparse_row_driven_item_pass(p, max_row_cells, static_cast<char*>(workspace) + sparse_record_bytes(d), s)) != 0) return rc;
    } else {
        if (p.num_chunk > 0) {
            const long long blocks = (p.num_chunk + 3) / 4;
            if (blocks > 0x7fffffffll) return fail(-8, "sparse rows: more chunks than one launch takes");
            VIBO_SPARSE_BY_WIDTH(sparse_item_kernel, p.A, gather, blocks, s, p);
            if ((rc = launch_rc("sparse rows item pass launch")) != 0) return rc;
        }
        hipLaunchKernelGGL(sparse_item_finish_kernel, dim3((unsigned)(((long long)p.I * p.D + 255) / 256)), dim3(256), 0, s, p.col_chunk, p.num_chunk,
                           p.chunk_rec, p.I, p.D, grad_item);
        if ((rc = launch_rc("sparse rows item finish launch")) != 0) return rc;
    }
    if (mapped) {
        hipLaunchKernelGGL(sparse_map_kernel<false>, dim3(map_grid), dim3(256), 0, s, person_index, (long long)p.B, p.P, person_slot);
        rc = launch_rc("sparse rows map clear launch");
    }
    return rc;
}

}  // namespace vibo

using namespace vibo;

extern "C" {

int vibo_sparse_rows_supported(const vibo_desc* d) { return sparse_desc_rc(d) == 0 ? 1 : 0; }

size_t vibo_sparse_workspace_bytes(const vibo_desc* d, int64_t num_chunk) {
    if (sparse_desc_rc(d) != 0 || num_chunk < 0) return 0;
    return sparse_record_bytes(d) + (d->want_grad ? up256((size_t)num_chunk * sparse_item_dim(d) * sizeof(float)) : 0);
}

int vibo_sparse_rows_check(const vibo_sparse_image* im, int64_t* violations, void* stream) {
    int rc = sparse_image_rc(nullptr, im, 0, im && im->col_ptr != nullptr);
    if (rc) return rc;
    if (!violations) return fail(-5, "sparse rows: null violations counter");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = hip_rc(hipMemsetAsync(violations, 0, sizeof(int64_t), s), "sparse rows check: counter reset")) != 0) return rc;
    unsigned long long* v = reinterpret_cast<unsigned long long*>(violations);
    auto side_grid = [](long long lists) { const long long g = (lists + 31) / 32; return (unsigned)(g > 4096 ? 4096 : g); };
    hipLaunchKernelGGL(sparse_check_side_kernel, dim3(side_grid(im->num_person)), dim3(256), 0, s, im->row_ptr, im->row_cell,
                       (long long)im->num_person, (long long)im->num_item, (long long)im->nnz, (const int64_t*)nullptr,
                       (const uint32_t*)nullptr, 0ll, v);
    if ((rc = launch_rc("sparse rows check (row side) launch")) != 0) return rc;
    if (!im->col_ptr) return 0;
    hipLaunchKernelGGL(sparse_check_side_kernel, dim3(side_grid(im->num_item)), dim3(256), 0, s, im->col_ptr, im->col_cell,
                       (long long)im->num_item, (long long)im->num_person, (long long)im->nnz, im->row_ptr, im->row_cell,
                       (long long)im->num_person, v);
    if ((rc = launch_rc("sparse rows check (column side) launch")) != 0) return rc;
    hipLaunchKernelGGL(sparse_check_chunks_kernel, dim3((unsigned)((im->num_item + 255) / 256)), dim3(256), 0, s, im->col_ptr, im->col_chunk,
                       im->chunk_item, im->chunk_first, (long long)im->num_item, (long long)im->nnz, (long long)im->num_chunk, v);
    return launch_rc("sparse rows check (chunk list) launch");
}

int vibo_sparse_elbo_fwd_bwd(const vibo_desc* d, const vibo_sparse_image* im, int64_t row0, const float* table, const float* item,
                             const float* eps, float* out_scalars, float* ability_mu, float* ability_logvar, float* ability,
                             float* grad_table, float* grad_item, int64_t* bad_cells, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = sparse_desc_rc(d);
    if (rc) return rc;
    if ((rc = sparse_image_rc(d, im, row0, d->want_grad != 0)) != 0) return rc;
    return sparse_elbo_call(d, im, false, row0, nullptr, nullptr, table, item, eps, out_scalars, ability_mu, ability_logvar, ability, grad_table,
                            grad_item, bad_cells, workspace, workspace_bytes, stream);
}

int vibo_sparse_encode(const vibo_desc* d, const vibo_sparse_image* im, int64_t row0, const float* table, float* ability_mu,
                       float* ability_logvar, int64_t* bad_cells, void* stream) {
    int rc = sparse_desc_rc(d);
    if (rc) return rc;
    if ((rc = sparse_image_rc(d, im, row0, false)) != 0) return rc;
    if (!table || !ability_mu || !ability_logvar) return fail(-5, "sparse rows: null required pointer");
    SparseParams p = sparse_params(d, im, row0);
    p.table = table; p.ability_mu = ability_mu; p.ability_logvar = ability_logvar;
    p.bad = reinterpret_cast<unsigned long long*>(bad_cells);
    VIBO_SPARSE_BY_WIDTH(sparse_encode_kernel, p.A, false, sparse_person_blocks(p.B), (hipStream_t)stream, p);
    return launch_rc("sparse rows encode launch");
}

int vibo_sparse_elbo_fwd_bwd_gather(const vibo_desc* d, const vibo_sparse_image* im, const int64_t* person_index, int32_t* person_slot,
                                    const float* table, const float* item, const float* eps, float* out_scalars, float* ability_mu,
                                    float* ability_logvar, float* ability, float* grad_table, float* grad_item, int64_t* bad_cells,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    int rc = sparse_desc_rc(d);
    if (rc) return rc;
    if ((rc = sparse_image_rc(d, im, 0, d->want_grad != 0, false)) != 0) return rc;
    if (!person_index) return fail(-5, "sparse rows: null person_index");
    if (d->want_grad && !person_slot) return fail(-5, "sparse rows: gradients of a gathered call need the person_slot map");
    return sparse_elbo_call(d, im, true, 0, person_index, person_slot, table, item, eps, out_scalars, ability_mu, ability_logvar, ability,
                            grad_table, grad_item, bad_cells, workspace, workspace_bytes, stream);
}

int vibo_sparse_encode_gather(const vibo_desc* d, const vibo_sparse_image* im, const int64_t* person_index, const float* table,
                              float* ability_mu, float* ability_logvar, int64_t* bad_cells, void* stream) {
    int rc = sparse_desc_rc(d);
    if (rc) return rc;
    if ((rc = sparse_image_rc(d, im, 0, false, false)) != 0) return rc;
    if (!person_index) return fail(-5, "sparse rows: null person_index");
    if (!table || !ability_mu || !ability_logvar) return fail(-5, "sparse rows: null required pointer");
    SparseParams p = sparse_params(d, im, 0);
    p.person_index = person_index;
    p.table = table; p.ability_mu = ability_mu; p.ability_logvar = ability_logvar;
    p.bad = reinterpret_cast<unsigned long long*>(bad_cells);
    VIBO_SPARSE_BY_WIDTH(sparse_encode_kernel, p.A, true, sparse_person_blocks(p.B), (hipStream_t)stream, p);
    return launch_rc("sparse rows encode launch");
}

}  // extern "C"
