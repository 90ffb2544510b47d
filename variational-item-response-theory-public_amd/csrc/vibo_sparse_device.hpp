// vibo_sparse_device.hpp -- what the two translation units of sparse response rows share, each stated once: vibo_sparse.hip (the range
// and the column-driven gathered calls) and vibo_sparse_row_driven.hip (the gathered call's row-driven item pass).  Device side: the
// kernels' parameter record, the cell's terms, the item's row, the gathered calls' map kernel.  Host side: the checks and the one call
// path of the ELBO entry points (defined in vibo_sparse.hip) and the row-driven item pass it hands over to (vibo_sparse_row_driven.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vibo_hip_sparse_row_driven.h"
#include "vibo_device.hpp"
#include "vibo_host.hpp"

namespace vibo {

struct SparseParams {
    const int64_t* row_ptr;
    const uint32_t* row_cell;
    const int64_t* col_ptr;
    const uint32_t* col_cell;
    const int64_t* col_chunk;
    const int32_t* chunk_item;
    const int64_t* chunk_first;
    long long P, nnz, num_chunk, row0;
    const int64_t* person_index;   // gathered calls: [B], the person of the call's row r
    int32_t* person_slot;          // gathered calls with gradients: [P], person -> the row of the call that owns it, or VIBO_SPARSE_NO_SLOT
    int I, B, A, D, irt, missing_mode, reg_mode, want_grad;
    const float* table;
    const float* item;
    const float* eps;
    float* ability_mu;
    float* ability_logvar;
    float* ability;
    float* grad_item;
    float* records;          // [4 G][kRec]
    float* chunk_rec;        // [num_chunk][D]
    unsigned long long* bad; // sticky counter (may be null)
};

__device__ __forceinline__ int wave_total_i(int v) { return lane63(wave_sum63(v)); }
__device__ __forceinline__ long long clamp_ll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One observed cell: logit, Bernoulli log-likelihood, d LL / d logit and d LL / d guess-logit (vibo_general.hip, pass 2).
// disc: the item's discriminations (2PL / 3PL), diff: its difficulty column, glogit: its guess logit (3PL).
template <int MA>
__device__ __forceinline__ void cell_terms(const int irt, const int A, const float (&disc)[MA], const float diff, const float glogit,
                                           const float (&th)[MA], const float x, float& ll, float& gl, float& gguess) {
    float l = diff;
    if (irt == 1) {
#pragma unroll
        for (int a = 0; a < MA; ++a)
            if (a < A) l += th[a];
    } else {
#pragma unroll
        for (int a = 0; a < MA; ++a)
            if (a < A) l = fmaf(-disc[a], th[a], l);
    }
    gguess = 0.f;
    if (irt != 3) {
        const float lc = fminf(fmaxf(l, -kLogitLo), kLogitLo);
        const bool live = (l >= -kLogitLo) && (l <= kLogitHi);
        const float e = expf(-fabsf(lc));
        ll = x * lc - fmaxf(lc, 0.f) - log1pf(e);
        const float r = 1.0f / (1.0f + e);
        const float sgm = (lc >= 0.f) ? r : e * r;
        gl = live ? (x - sgm) : 0.f;
    } else {
        const float guess = 1.0f / (1.0f + expf(-glogit));
        const float e = expf(-fabsf(l));
        const float r = 1.0f / (1.0f + e);
        const float sp = (l >= 0.f) ? r : e * r, sn = (l >= 0.f) ? e * r : r;
        const float pr = fmaf(1.0f - guess, sp, guess);
        const float qr = (1.0f - guess) * sn;
        const float pc = fminf(fmaxf(pr, kEps32), 1.0f - kEps32);
        const float qc = fminf(fmaxf(qr, kEps32), 1.0f - kEps32);
        ll = (x > 0.5f) ? logf(pc) : logf(qc);
        const float dll_dp = (pr == pc) ? ((x > 0.5f) ? 1.0f / pc : -1.0f / qc) : 0.f;
        const float common = dll_dp * (1.0f - guess) * sn;
        gl = common * sp;
        gguess = common * guess;
    }
}

// The item's row `it` [D] as cell_terms takes it (A = MA: one instantiation per ability_dim); glogit is the caller's 0 but for 3PL.
// The statements of the person and item kernels of vibo_sparse.hip, which keep them inline: called from there, the gathered item
// kernel's schedule moved by one instruction, and those kernels keep their code as it was.
// 1PL [difficulty]; 2PL / 3PL [discrimination 0..A-1 | difficulty | guess logit]
template <int MA>
__device__ __forceinline__ void item_row(const float* it, const int irt, float (&disc)[MA], float& diff, float& glogit) {
    constexpr int A = MA;
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
}

// The map of a gathered call with gradients, B threads.  BUILD: the smallest row r that names person q owns it (an integer minimum: the
// same whatever the arrival order); else the clear: the call's entries back to VIBO_SPARSE_NO_SLOT.  An index outside [0, P) writes nothing.
template <bool BUILD>
__global__ __launch_bounds__(256) void sparse_map_kernel(const int64_t* person_index, const long long B, const long long P, int32_t* person_slot) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= B) return;
    const long long q = person_index[r];
    if (q < 0 || q >= P) return;
    if (BUILD) atomicMin(&person_slot[q], (int32_t)r); else person_slot[q] = VIBO_SPARSE_NO_SLOT;
}

// ---- host (vibo_sparse.hip) ----
int sparse_desc_rc(const vibo_desc* d);            // the descriptor against the format: 0, or the code (error string set)
int sparse_image_rc(const vibo_desc* d, const vibo_sparse_image* im, int64_t row0, bool need_cols, bool ranged = true);
int sparse_item_dim(const vibo_desc* d);
int sparse_person_blocks(int B);                   // THE GRID RULE's G
size_t sparse_record_bytes(const vibo_desc* d);    // the person pass's records, 256-byte rounded: the head of every sparse workspace
// The ELBO call on a range or on an index vector after the descriptor and the image have passed their checks.  max_row_cells > 0
// (a gathered call with gradients): the item pass is the row-driven one below, on a workspace of vibo_sparse_row_driven_workspace_bytes.
int sparse_elbo_call(const vibo_desc* d, const vibo_sparse_image* im, bool gather, int64_t row0, const int64_t* person_index,
                     int32_t* person_slot, const float* table, const float* item, const float* eps, float* out_scalars,
                     float* ability_mu, float* ability_logvar, float* ability, float* grad_table, float* grad_item,
                     int64_t* bad_cells, void* workspace, size_t workspace_bytes, void* stream, long long max_row_cells = 0);

// ---- host (vibo_sparse_row_driven.hip) ----
// Launches 3..7 of include/vibo_hip_sparse_row_driven.h between the person pass's finish and the map clear: p as the person pass took
// it (map built, ability written in stream order), ws the workspace behind the records.
int sparse_row_driven_item_pass(const SparseParams& p, long long max_row_cells, char* ws, hipStream_t s);

}  // namespace vibo
