// vibo_helpers.hpp -- launch wrappers of the small kernels around the fused ELBO kernels (vibo_helpers.hip).  Each returns the
// launch's hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vibo_hip.h"
#include "vibo_params.hpp"

namespace vibo {

// item prep: [I][D] item sample -> [I][DP] rows the tiled / wave-per-row kernels read with scalar loads
hipError_t launch_item_prep(const float* item, float* prep, int I, int A, int AT, int D, int DP, int irt, hipStream_t s);

// packed counts (n_correct << 16 | n_observed) of every person row of aligned, chunkable rows; codes_out: also the rows' 1-byte cell codes
hipError_t launch_row_counts(const vibo_desc* d, int num_cu, const float* response, const void* mask, const int64_t* row_index, int* cnt,
                             uint8_t* codes_out, long long codes_stride, hipStream_t s);
// ... of rows the vector kernel cannot read (unaligned / not chunkable / int64 mask)
hipError_t launch_row_counts_scalar(const vibo_desc* d, const float* response, const void* mask, const int64_t* row_index, int* cnt,
                                    hipStream_t s);
// out[k] = all[row_index[k]]
hipError_t launch_gather_counts(const int32_t* all, const int64_t* row_index, int* out, int B, hipStream_t s);

// buf[0][e] += buf[1..panels-1][e] for e < n (fixed order)
hipError_t launch_panel_sum(float* buf, long long n, int panels, hipStream_t s);
// VIBO_POSTERIOR_GIVEN over more than one panel: the posterior as row statistics in, the coefficients as its gradient out
hipError_t launch_given_pre(const float* post, float* pre, long long B, int A, int I, hipStream_t s);
hipError_t launch_given_post(const float* post, const float* coef, int panels, float* grad, long long B, int A, hipStream_t s);

// fp32 rows + mask -> 1-byte cell codes; chunks: 4 cells per thread (aligned rows, codes_row_stride % 4 == 0).
// row_index (chunks only): the code rows are the minibatch's, in its order
// vibo_rows_sign_is_mask (chunks: aligned rows, 4 cells per thread)
hipError_t launch_sign_is_mask(const vibo_desc* d, const float* response, const void* mask, bool chunks, int32_t* differs, hipStream_t s);
// vibo_tile_rows_build (src: the source rows' descriptor; vec: its rows can be read in aligned 4-cell chunks)
hipError_t launch_tile_rows_build(const vibo_desc* src, const float* response, const void* mask, bool vec, void* image, hipStream_t s);
hipError_t launch_pack_codes(const vibo_desc* d, const float* response, const void* mask, uint8_t* codes, long long codes_row_stride,
                             bool chunks, hipStream_t s, const int64_t* row_index = nullptr);

// fixed-order sum of the partial records (+ f.tail in the same launch); sets f.n_fin
hipError_t launch_finalize(FinalizeParams& f, hipStream_t s);
hipError_t launch_multi_finalize(const float* partial, float* out_scalars, int nblk, int stride, int n_samples, int reg_mode, hipStream_t s);

struct EncodeParams {
    const float* response;
    const void* mask;
    const int64_t* row_index;
    const float* table;
    float* ability_mu;
    float* ability_logvar;
    long long resp_stride, mask_stride;
    int B, I, A, mask_dtype, missing_mode, conditional;
};
hipError_t launch_encode(const EncodeParams& p, hipStream_t s);
hipError_t launch_encode_finish(const int* cnt, const float* pre, int panels, const float* table, float* ability_mu, float* ability_logvar,
                                long long B, int I, int A, int missing_mode, hipStream_t s);

// the same finish for G item samples' stacked sums (launch_cond_stack_sums) -> post[G][B][2A] = mu | logvar
hipError_t launch_cond_stack_finish(const float* sums, int ldc, int cnt_col, float* post, long long B, int I, int A, int G, int missing_mode,
                                    hipStream_t s);

hipError_t launch_decode(const float* ability, const float* item, float* response_mu, long long B, int I, int A, int D, int irt,
                         hipStream_t s);
hipError_t launch_decode_mean(int num_samples, const float* ability, const float* item, float* response_mu_mean, long long B, int I, int A,
                              int D, int irt, hipStream_t s);

hipError_t launch_lane_swap_selftest(const float* in, float* out, hipStream_t s);

}  // namespace vibo
