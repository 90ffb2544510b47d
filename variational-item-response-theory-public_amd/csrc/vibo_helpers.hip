// vibo_helpers.hip -- the small kernels around the fused ELBO kernels (item prep, whole-row counts, cell-code packing, the
// caller-supplied posterior's hooks, partial finalize, forward-only encode, decode) and their launch wrappers (vibo_helpers.hpp).
#include "vibo_helpers.hpp"

#include "../../include/vibo_hip_tile_rows.h"
#include "vibo_cond_finalize.hpp"
#include "vibo_device.hpp"
#include "vibo_finalize.hpp"
#include "vibo_planner.hpp"
#include "vibo_variant.hpp"

namespace vibo {

// ---------------------------------------------------------------------------
// item prep: [I][D] item sample -> [I][DP] rows the fused kernel reads with scalar loads
// ---------------------------------------------------------------------------
__global__ void item_prep_kernel(const float* __restrict__ item, float* __restrict__ prep, int I, int A, int AT,
                                 int D, int DP, int irt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int I16 = (I + 15) & ~15;
    if (i >= I16) return;
    float* dst = prep + (size_t)i * DP;
    if (i >= I) {            // zero rows pad the item axis to a multiple of 16
        for (int a = 0; a < DP; ++a) dst[a] = 0.f;
        return;
    }
    const float* src = item + (size_t)i * D;
    // logits are carried in log2 units (x log2 e) so the kernel's exp2/log2 need no extra multiply
    for (int a = 0; a < DP; ++a) dst[a] = 0.f;
    if (irt == 1) {          // logit = sum_a theta_a + b   (models.py:731)
        for (int a = 0; a < A; ++a) dst[a] = kLog2e;
        dst[AT] = src[0] * kLog2e;
        return;
    }
    for (int a = 0; a < A; ++a) dst[a] = -src[a] * kLog2e;   // logit = -a.theta + b   (models.py:744,759)
    dst[AT] = src[A] * kLog2e;
    if (irt == 3) {
        const float g = 1.0f / (1.0f + expf(-src[A + 1]));   // guess = sigmoid(guess logit) (models.py:758)
        dst[AT + 1] = g;
        dst[AT + 2] = 1.0f - g;
    }
}

// ---------------------------------------------------------------------------
// panel mode: packed counts (n_correct << 16 | n_observed) of every person row, one wave per row
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void row_count_kernel(const float* __restrict__ response, const void* __restrict__ mask,
                                                        const int64_t* __restrict__ row_index, int* __restrict__ cnt,
                                                        long long resp_stride, long long mask_stride, int B, int I,
                                                        int mask_dtype, uint8_t* __restrict__ codes_out = nullptr,
                                                        long long codes_stride = 0) {
    const int lane = threadIdx.x & 63;
    const long long wave_id = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * 4;
    const int n4 = (I + 3) >> 2;
    const bool cell_codes = mask_dtype == VIBO_MASK_CODES;
    for (long long row = wave_id; row < B; row += n_waves) {
        const long long src = row_index ? row_index[row] : row;
        const float4* rp = reinterpret_cast<const float4*>(response + src * resp_stride);
        const uint32_t* mp = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(mask) + src * mask_stride);
        int packed = 0;
        for (int c0 = lane; c0 < n4; c0 += 256) {          // 4 chunks per lane in flight
            float4 x[4];
            uint32_t m[4], keep[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + 64 * u;
                x[u] = float4{0.f, 0.f, 0.f, 0.f};
                m[u] = 0u;
                keep[u] = 0u;
                if (c < n4) {
                    if (!cell_codes) x[u] = nt_load4(rp + c);       // (streamed once: see nt_load4)
                    m[u] = (mask_dtype == 0 || cell_codes) ? mp[c] : 0x01010101u;
                    keep[u] = ((I & 3) && c == (I >> 2)) ? (1u << (8 * (I & 3))) - 1u : 0xFFFFFFFFu;      // padded tail of the row
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (cell_codes) (void)pack_cell_codes4(m[u], keep[u], packed);
                else (void)pack_codes4(x[u], m[u] & keep[u], packed);
                // fp32 rows, more passes to come: leave the row behind as 1-byte cell codes (minibatch order)
                if (!cell_codes && codes_out && c0 + 64 * u < n4)
                    reinterpret_cast<uint32_t*>(codes_out + row * codes_stride)[c0 + 64 * u] = cell_codes4(x[u], m[u] & keep[u]);
            }
        }
        const int tot = lane63(wave_sum63(packed));
        if (lane == 0) cnt[row] = tot;
    }
}

// ---------------------------------------------------------------------------
// VIBO_POSTERIOR_GIVEN: the caller's per-person (mu | logvar) enters the row-split kernel through the hooks of the
// conditional pipeline: precision lam = exp(-logvar), s = mu lam, nobs = I (no prior experts are added); the kernel's
// per-person coefficients P1 = g_mu / lam, P2 = -(g_mu mu + g_lv) / lam come back as d / d (mu, logvar)
// ---------------------------------------------------------------------------
// conditional posterior, more than one 1024-item panel: the panels' row statistics summed once (fixed order) into panel 0's
// block, so the matrix kernel's per-person forward reads 3 values instead of 3 per panel inside its barrier phase
__global__ __launch_bounds__(256) void panel_sum_kernel(float* __restrict__ pre, long long n, int panels) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float t = pre[e];
    for (int pn = 1; pn < panels; ++pn) t += pre[(size_t)pn * n + e];
    pre[e] = t;
}

__global__ __launch_bounds__(256) void given_pre_kernel(const float* __restrict__ post, float* __restrict__ pre, long long B, int A,
                                                        int I) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * (A + 1)) return;
    const long long row = e / (A + 1);
    const int a = (int)(e % (A + 1));
    float* st = pre + row * (2 * A + 1);
    if (a == A) { st[2 * A] = (float)I; return; }
    const float mu = post[row * 2 * A + a], lam = expf(-post[row * 2 * A + A + a]);
    st[a] = lam;
    st[A + a] = mu * lam;
}
__global__ __launch_bounds__(256) void given_post_kernel(const float* __restrict__ post, const float* __restrict__ coef, int panels,
                                                         float* __restrict__ grad, long long B, int A) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * A) return;
    const long long row = e / A;
    const int a = (int)(e % A);
    const float mu = post[row * 2 * A + a], lam = expf(-post[row * 2 * A + A + a]);
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        float p1 = 0.f, p2 = 0.f;
        for (int pn = 0; pn < panels; ++pn) {
            const float* pc = coef + ((size_t)pn * B + row) * 4 * A;
            p1 += pc[(st * 2 + 0) * A + a];
            p2 += pc[(st * 2 + 1) * A + a];
        }
        const float gmu = p1 * lam;
        grad[((size_t)st * B + row) * 2 * A + a] = gmu;
        grad[((size_t)st * B + row) * 2 * A + A + a] = -p2 * lam - gmu * mu;
    }
}

// whole-row counts for rows the vector kernel cannot read (unaligned / not chunkable / int64 mask): wave per row
__global__ __launch_bounds__(256) void row_count_scalar_kernel(const float* __restrict__ response, const void* __restrict__ mask,
                                                               const int64_t* __restrict__ row_index, int* __restrict__ cnt,
                                                               long long resp_stride, long long mask_stride, int B, int I,
                                                               int mask_dtype) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const long long src = row_index ? row_index[row] : row;
    int packed = 0;
    for (int i = lane; i < I; i += 64) {
        bool k = true, one;
        if (mask_dtype == VIBO_MASK_CODES) {
            const uint8_t c = static_cast<const uint8_t*>(mask)[src * mask_stride + i];
            k = c != 2; one = c == 1;
        } else {
            if (mask_dtype == VIBO_MASK_U8) k = static_cast<const uint8_t*>(mask)[src * mask_stride + i] != 0;
            else if (mask_dtype == VIBO_MASK_I64) k = static_cast<const int64_t*>(mask)[src * mask_stride + i] != 0;
            one = response[src * resp_stride + i] == 1.0f;
        }
        if (k) packed += 1 + (one ? (1 << 16) : 0);
    }
    const int tot = lane63(wave_sum63(packed));
    if (lane == 0) cnt[row] = tot;
}

// ---------------------------------------------------------------------------
// Format P: response (fp32) + mask (u8 / int64 / none) -> 1-byte cell codes, rows padded with "missing" up to the
// code stride (datasets.py:928-940 stores responses as fp32 with -1 for missing and a separate mask)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_codes_kernel(const float* __restrict__ response, const void* __restrict__ mask,
                                                         uint8_t* __restrict__ codes, long long resp_stride, long long mask_stride,
                                                         long long code_stride, long long B, int I, int mask_dtype) {
    const long long n = B * code_stride;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long row = e / code_stride;
        const int i = (int)(e - row * code_stride);
        uint8_t c = 2;
        if (i < I) {
            bool k = true;
            if (mask_dtype == VIBO_MASK_U8) k = static_cast<const uint8_t*>(mask)[row * mask_stride + i] != 0;
            else if (mask_dtype == VIBO_MASK_I64) k = static_cast<const int64_t*>(mask)[row * mask_stride + i] != 0;
            if (k) c = response[row * resp_stride + i] == 1.0f ? 1 : 0;
        }
        codes[e] = c;
    }
}

// the same for 4-cell chunks of aligned rows (thread = one chunk: float4 + mask word in, one code word out); row_index: code row
// k is source row row_index[k] (a minibatch's rows, packed in its order)
__global__ __launch_bounds__(256) void pack_codes4_kernel(const float* __restrict__ response, const void* __restrict__ mask,
                                                          uint32_t* __restrict__ codes, long long resp_stride, long long mask_stride,
                                                          long long chunks_per_row, long long B, int I, int mask_dtype,
                                                          const int64_t* __restrict__ row_index) {
    const long long n = B * chunks_per_row;
    const int n4 = (I + 3) >> 2;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long row = e / chunks_per_row;
        const int c = (int)(e - row * chunks_per_row);
        uint32_t w = kAllMissing4;
        if (c < n4) {
            const long long src = row_index ? row_index[row] : row;
            const float4 x = reinterpret_cast<const float4*>(response + src * resp_stride)[c];
            uint32_t m = mask_dtype == VIBO_MASK_U8
                             ? reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(mask) + src * mask_stride)[c]
                             : 0x01010101u;
            m = ((m | (m >> 1) | (m >> 2) | (m >> 3) | (m >> 4) | (m >> 5) | (m >> 6) | (m >> 7)) & 0x01010101u);   // any bit -> 1
            if ((I & 3) && c == (I >> 2)) m &= (1u << (8 * (I & 3))) - 1u;
            const uint32_t one = (x.x == 1.0f ? 1u : 0u) | (x.y == 1.0f ? 1u << 8 : 0u) | (x.z == 1.0f ? 1u << 16 : 0u) |
                                 (x.w == 1.0f ? 1u << 24 : 0u);
            w = (one & m) | ((m ^ 0x01010101u) << 1);          // observed: 0 / 1; not observed (or padding): 2
        }
        codes[e] = w;
    }
}

// ---------------------------------------------------------------------------
// vibo_rows_sign_is_mask: is every mask byte 0 or 1, and (mask byte == 1) == (sign bit of the response clear), in every cell of
// the rows?  (A byte above 1 "differs": the matrix kernel's pack takes the mask bytes as 0 / 1, so only for those do the two
// formats form the same code words.)  One streaming pass; a thread that meets a cell where it does not hold stores 1 (every
// writer the same value: a plain store)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sign_is_mask4_kernel(const float* __restrict__ response, const uint8_t* __restrict__ mask,
                                                            long long resp_stride, long long mask_stride, long long B, int I,
                                                            int32_t* __restrict__ differs) {
    const int n4 = (I + 3) >> 2;
    const long long n = B * n4;
    bool bad = false;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long row = e / n4;
        const int c = (int)(e - row * n4);
        const float4 x = reinterpret_cast<const float4*>(response + row * resp_stride)[c];
        const uint32_t m = reinterpret_cast<const uint32_t*>(mask + row * mask_stride)[c];
        const uint32_t x0 = __builtin_bit_cast(uint32_t, x.x), x1 = __builtin_bit_cast(uint32_t, x.y);
        const uint32_t x2 = __builtin_bit_cast(uint32_t, x.z), x3 = __builtin_bit_cast(uint32_t, x.w);
        const uint32_t top = __builtin_amdgcn_perm(x1, x0, 0x0c0c0703u) | __builtin_amdgcn_perm(x3, x2, 0x07030c0cu);
        // bit 0 of a byte: mask bit against [sign clear]; bits 1..7: a mask byte above 1
        uint32_t diff = ((m ^ ~(top >> 7)) & 0x01010101u) | (m & 0xFEFEFEFEu);
        if ((I & 3) && c == (I >> 2)) diff &= (1u << (8 * (I & 3))) - 1u;      // (the row padding is not looked at)
        bad = bad || diff != 0u;
    }
    if (bad) *differs = 1;
}
// (rows that cannot be read in aligned 4-cell chunks: one cell per thread)
__global__ __launch_bounds__(256) void sign_is_mask_kernel(const float* __restrict__ response, const uint8_t* __restrict__ mask,
                                                           long long resp_stride, long long mask_stride, long long B, int I,
                                                           int32_t* __restrict__ differs) {
    const long long n = B * I;
    bool bad = false;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long row = e / I;
        const int i = (int)(e - row * I);
        const bool sign_clear = (__builtin_bit_cast(uint32_t, response[row * resp_stride + i]) >> 31) == 0u;
        const uint8_t mb = mask[row * mask_stride + i];
        bad = bad || mb > 1 || (mb == 1) != sign_clear;
    }
    if (bad) *differs = 1;
}

// ---------------------------------------------------------------------------
// vibo_tile_rows_build: the image of a matrix as the matrix row-split kernel's tile rows read it (include/vibo_hip_tile_rows.h: THE
// layout).  A wave forms one wave block -- 32 rows x 128 items -- as a wave of that kernel would: lane (g, i16) packs the cells of
// persons 16 h + 4 g + j at chunks 32 q + 16 u + i16 with the kernel's own pack of the source format and its keep words (cells past
// the row's end, rows past the matrix' end: dropped), the 16 lanes of a row group add their counts.  Rows of any alignment: `vec`
// says that 4-cell chunks can be read whole (rows_vec_ok), else cell by cell.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tile_rows_build_kernel(const float* __restrict__ response, const uint8_t* __restrict__ mask,
                                                              long long resp_stride, long long mask_stride, long long B, int I,
                                                              int mask_dtype, bool vec, uint32_t* __restrict__ image, long long n_wave_blocks,
                                                              int W) {
    __shared__ int row_cnt[4][32];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, i16 = lane & 15, g = lane >> 4;
    const int n4 = (I + 3) >> 2;
    const uint32_t tm_tail = (I & 3) ? ((1u << (8 * (I & 3))) - 1u) : 0xFFFFFFFFu;
    for (long long wb0 = (long long)blockIdx.x * 4; wb0 < n_wave_blocks; wb0 += (long long)gridDim.x * 4) {      // (block-uniform)
        const long long wb = wb0 + wv;
        const bool live = wb < n_wave_blocks;
        const long long bt = wb / W;
        const int q = (int)(wb - bt * W);
        uint32_t cw[2][8];
        int own = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long row = 32 * bt + 16 * h + 4 * g + j;
                int nobs = 0, n1 = 0;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int c = 32 * q + 16 * u + i16;
                    const uint32_t keep = (!live || row >= B || c >= n4) ? 0u : ((I & 3) && c == (I >> 2)) ? tm_tail : 0xFFFFFFFFu;
                    float4 x = float4{0.f, 0.f, 0.f, 0.f};
                    uint32_t w = 0u;
                    if (keep) {
                        if (vec) {
                            if (mask_dtype != VIBO_MASK_CODES) x = reinterpret_cast<const float4*>(response + row * resp_stride)[c];
                            if (mask) w = reinterpret_cast<const uint32_t*>(mask + row * mask_stride)[c];
                        } else {
                            float xs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                if (4 * c + k < I) {
                                    if (mask_dtype != VIBO_MASK_CODES) xs[k] = response[row * resp_stride + 4 * c + k];
                                    if (mask) w |= (uint32_t)mask[row * mask_stride + 4 * c + k] << (8 * k);
                                }
                            }
                            x = float4{xs[0], xs[1], xs[2], xs[3]};
                        }
                    }
                    cw[u][4 * h + j] = mask_dtype == VIBO_MASK_CODES  ? pack_cell_codes4_lut(w, keep, kPackLutCode, nobs, n1)
                                       : mask_dtype == VIBO_MASK_SIGN ? pack_codes4_sign_lut(x, keep & 0x01010101u, kPackLutFp32, nobs, n1)
                                       : mask_dtype == VIBO_MASK_U8   ? pack_codes4_lut(x, w & keep, kPackLutFp32, nobs, n1)
                                                                      : pack_codes4_lut(x, 0x01010101u & keep, kPackLutFp32, nobs, n1);
                }
                own += nobs;
                int t = nobs | (n1 << 16);                     // (<= 8 each per lane: 128 over the row group)
                t += __shfl_xor(t, 1, 16); t += __shfl_xor(t, 2, 16); t += __shfl_xor(t, 4, 16); t += __shfl_xor(t, 8, 16);
                if (i16 == 0) row_cnt[wv][16 * h + 4 * g + j] = t;
            }
        __syncthreads();
        if (live) {
            uint32_t* blk = image + wb * (kTileWaveBytes / 4);
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    reinterpret_cast<uint4*>(blk + 256 * (2 * h + u))[lane] = uint4{cw[u][4 * h], cw[u][4 * h + 1], cw[u][4 * h + 2], cw[u][4 * h + 3]};
            blk[kTileWordBytes / 4 + lane] = ((uint32_t)row_cnt[wv][lane & 31] & 0x00ffffffu) | ((uint32_t)own << 24);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// finalize: fixed-order sum of the per-block partial records (fp64 accumulate)
// ---------------------------------------------------------------------------
// 1024 threads = OUT outputs x (1024 / OUT) slices of the block list; OUT = 64 normally, 16 when there are many small
// records (one-wave workgroups of the row-split kernel: up to 8 per CU)
template <int OUT>
__global__ __launch_bounds__(1024) void finalize_kernel(const FinalizeParams f) {
    constexpr int SLICES = 1024 / OUT;
    __shared__ __attribute__((aligned(16))) double part[SLICES][OUT];
    if ((int)blockIdx.x >= f.n_fin) {      // the conditional posterior's table gradients (vibo_cond_finalize.hpp)
        cond_fin_tail_body(f.tail, (int)blockIdx.x - f.n_fin, &part[0][0]);
        return;
    }
    // element e of the logical output vector: [0,8) scalars | table grads | flow grads | item grads
    const int n_tab = 8 * f.A;
    const int n_flow = 2 * f.n_flows * (2 * f.A + 1);
    const int n_item = f.I * f.D;
    const int n_out = 8 + (f.want_grad ? n_tab + n_flow + n_item : 0);
    const int lane = threadIdx.x % OUT, slice = threadIdx.x / OUT;
    const int e = blockIdx.x * OUT + lane;
    double acc = 0.0;
    if (e < n_out) {
        int src, b0 = 0, b1 = f.nblk;
        if (e < 8 + n_tab + n_flow) {
            src = e;   // same offsets in the partial record (off_table = 8, off_flow = 8 + 8A)
        } else {
            const int k = e - (8 + n_tab + n_flow);
            const int dd = k / f.I, i = k % f.I;          // consecutive lanes = consecutive items: coalesced record reads
            const int panel = i / f.panel_items;          // panel mode: only this panel's blocks hold item i
            src = f.lay.off_item + dd * f.lay.i_pad + (i - panel * f.panel_items);
            b0 = panel * f.bpp;
            b1 = b0 + f.bpp;
        }
        // fixed order: slice s sums blocks s, s+SLICES, ... in fp64, then the slices are summed in order
        acc = record_slice_sum<SLICES>(f.partial, (size_t)f.lay.stride, src, b0, b1, slice);
    }
    part[slice][lane] = acc;
    __syncthreads();
    if (slice == 0 && e < n_out) {
        double t = 0.0;
#pragma unroll
        for (int s = 0; s < SLICES; ++s) t += part[s][lane];
        if (e < 8) {
            // partial scalars: 0 ll, 1 kl, 2 logq0, 3 logp, 4 ladj, 5 nobs
            part[0][lane] = t;
        } else if (e < 8 + n_tab) {
            if (f.grad_table) f.grad_table[e - 8] = (float)t;      // null: conditional posterior (cond_finalize_kernel)
        } else if (e < 8 + n_tab + n_flow) {
            f.grad_flow[e - 8 - n_tab] = (float)t;
        } else {
            const int k = e - 8 - n_tab - n_flow;
            f.grad_item[(size_t)(k % f.I) * f.D + k / f.I] = (float)t;
        }
    }
    if (blockIdx.x == 0) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const double ll = part[0][0], kl = part[0][1], logq0 = part[0][2], logp = part[0][3], ladj = part[0][4];
            f.out_scalars[VIBO_S_LL] = (float)ll;
            f.out_scalars[VIBO_S_REG] = (float)(f.reg_mode == VIBO_REG_KL ? kl : (logq0 - ladj - logp));
            f.out_scalars[VIBO_S_KL] = (float)kl;
            f.out_scalars[VIBO_S_LOGQ0] = (float)logq0;
            f.out_scalars[VIBO_S_LOGP] = (float)logp;
            f.out_scalars[VIBO_S_LADJ] = (float)ladj;
            f.out_scalars[VIBO_S_NOBS] = (float)part[0][5];
            f.out_scalars[VIBO_S_RESERVED] = 0.f;
        }
    }
}

// multi-sample forward: out_scalars[s][8] from the per-block records (8 scalars per sample at record[8 s ..])
__global__ __launch_bounds__(1024) void multi_finalize_kernel(const float* __restrict__ partial, float* __restrict__ out_scalars,
                                                              int nblk, int stride, int n_samples, int reg_mode) {
    __shared__ double part[32][32];
    const int e = threadIdx.x & 31, slice = threadIdx.x >> 5;      // e = 8 s + k
    double acc = 0.0;
    if (e < 8 * n_samples)
        for (int b = slice; b < nblk; b += 32) acc += (double)partial[(size_t)b * stride + e];
    part[slice][e] = acc;
    __syncthreads();
    if (slice == 0) {
        double t = 0.0;
        for (int s = 0; s < 32; ++s) t += part[s][e];
        part[0][e] = t;
    }
    __syncthreads();
    if (threadIdx.x < n_samples) {
        const int s = threadIdx.x;
        const double ll = part[0][8 * s + 0], kl = part[0][8 * s + 1], logq0 = part[0][8 * s + 2];
        const double logp = part[0][8 * s + 3], ladj = part[0][8 * s + 4];
        float* o = out_scalars + 8 * s;
        o[VIBO_S_LL] = (float)ll;
        o[VIBO_S_REG] = (float)(reg_mode == VIBO_REG_KL ? kl : (logq0 - ladj - logp));
        o[VIBO_S_KL] = (float)kl;
        o[VIBO_S_LOGQ0] = (float)logq0;
        o[VIBO_S_LOGP] = (float)logp;
        o[VIBO_S_LADJ] = (float)ladj;
        o[VIBO_S_NOBS] = (float)part[0][8 * s + 5];
        o[VIBO_S_RESERVED] = 0.f;
    }
}

// ---------------------------------------------------------------------------
// forward-only encode: one wave per person (models.py:356-371 under no_grad)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void encode_kernel(const EncodeParams p) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.B) return;
    const long long src = p.row_index ? p.row_index[row] : row;
    const float* rp = p.response + src * p.resp_stride;
    const int A = p.A, I = p.I;
    float lam[VIBO_MAX_ABILITY_DIM_WIDE], smu[VIBO_MAX_ABILITY_DIM_WIDE];
#pragma unroll
    for (int a = 0; a < VIBO_MAX_ABILITY_DIM_WIDE; ++a) lam[a] = smu[a] = 0.f;
    const float tau_prior = 1.0f / (1.0f + kPoeEps);
    for (int i = lane; i < I; i += 64) {
        bool k;
        if (p.mask_dtype == VIBO_MASK_U8) k = static_cast<const uint8_t*>(p.mask)[src * p.mask_stride + i] != 0;
        else if (p.mask_dtype == VIBO_MASK_I64) k = static_cast<const int64_t*>(p.mask)[src * p.mask_stride + i] != 0;
        else k = true;
        const int c = (rp[i] == 1.0f) ? 1 : 0;
        const float* te = p.conditional ? p.table + ((size_t)c * I + i) * 2 * A : p.table + (size_t)c * 2 * A;
#pragma unroll
        for (int a = 0; a < VIBO_MAX_ABILITY_DIM_WIDE; ++a) {
            if (a < A) {
                if (k) {
                    const float tau = 1.0f / (__expf(te[A + a]) + kPoeEps);
                    lam[a] += tau;
                    smu[a] = fmaf(te[a], tau, smu[a]);
                } else if (p.missing_mode == VIBO_MISSING_PRIOR) {
                    lam[a] += tau_prior;
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < VIBO_MAX_ABILITY_DIM_WIDE; ++a) {
        if (a < A) {
            const float L = wave_total(lam[a]);
            const float S = wave_total(smu[a]);
            if (lane == 0) {
                p.ability_mu[row * A + a] = S / L;
                p.ability_logvar[row * A + a] = logf(1.0f / L);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// decode: response_mu[B][I] (models.py:729-766)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void decode_kernel(const float* __restrict__ ability, const float* __restrict__ item,
                                                     float* __restrict__ out, int B, int I, int A, int D, int irt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const long long b = blockIdx.y;
    if (i >= I) return;
    const float* th = ability + b * A;
    const float* it = item + (size_t)i * D;
    float logit;
    if (irt == 1) {
        logit = it[0];
        for (int a = 0; a < A; ++a) logit += th[a];
    } else {
        logit = it[A];
        for (int a = 0; a < A; ++a) logit = fmaf(-it[a], th[a], logit);
    }
    float pr = 1.0f / (1.0f + expf(-logit));
    if (irt == 3) {
        const float g = 1.0f / (1.0f + expf(-it[A + 1]));
        pr = g + (1.0f - g) * pr;
    }
    out[b * I + i] = pr;
}

// forward-only posterior from whole-row statistics: thread = (person, ability dim).  stats = packed counts of
// row_count_kernel (unconditional: the experts are the two table rows) or the per-panel sums of cond_pre_kernel.
__global__ __launch_bounds__(256) void encode_finish_kernel(const int* __restrict__ cnt, const float* __restrict__ pre, int panels,
                                                            const float* __restrict__ table, float* __restrict__ ability_mu,
                                                            float* __restrict__ ability_logvar, long long B, int I, int A,
                                                            int missing_mode) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * A) return;
    const long long row = e / A;
    const int a = (int)(e % A);
    float lam, smu, nobs;
    if (cnt) {
        const int c = cnt[row];
        const float n1 = (float)(c >> 16);
        nobs = (float)(c & 0xffff);
        const float n0 = nobs - n1;
        const float tau0 = 1.0f / (expf(table[A + a]) + kPoeEps), tau1 = 1.0f / (expf(table[2 * A + A + a]) + kPoeEps);
        lam = n0 * tau0 + n1 * tau1;
        smu = n0 * table[a] * tau0 + n1 * table[2 * A + a] * tau1;
    } else {
        lam = smu = nobs = 0.f;
        for (int pn = 0; pn < panels; ++pn) {
            const float* st = pre + ((size_t)pn * B + row) * (2 * A + 1);
            lam += st[a]; smu += st[A + a]; nobs += st[2 * A];
        }
    }
    if (missing_mode == VIBO_MISSING_PRIOR) lam += ((float)I - nobs) * (1.0f / (1.0f + kPoeEps));
    ability_mu[e] = smu / lam;
    ability_logvar[e] = logf(1.0f / lam);
}

// the same finish for a group of G item samples of the conditional posterior (launch_cond_stack_sums: row p of `sums` holds
// lam | s of sample g at columns g 2A .., the row's observed count at column cnt_col): thread = (person, sample, dim), so a row's
// sums are read once; post[g][p] = mu | logvar, [G][B][2A].  The statements are encode_finish_kernel's: the same bits from the same sums
__global__ __launch_bounds__(256) void cond_stack_finish_kernel(const float* __restrict__ sums, int ldc, int cnt_col, float* __restrict__ post,
                                                                long long B, int I, int A, int G, int missing_mode) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * G * A) return;
    const long long row = e / (G * A);
    const int c = (int)(e - row * (G * A)), g = c / A, a = c - g * A;
    const float* st = sums + row * ldc;
    float lam = st[g * 2 * A + a];
    const float smu = st[g * 2 * A + A + a], nobs = st[cnt_col];
    if (missing_mode == VIBO_MISSING_PRIOR) lam += ((float)I - nobs) * (1.0f / (1.0f + kPoeEps));
    float* po = post + ((long long)g * B + row) * 2 * A;
    po[a] = smu / lam;
    po[A + a] = logf(1.0f / lam);
}

// posterior-predictive mean: thread = one item x 8 persons; per sample the item row is loaded once and reused for the
// 8 persons (ability rows are wave-uniform scalar loads)
__global__ __launch_bounds__(256) void decode_mean_kernel_strided(const float* __restrict__ ability, const float* __restrict__ item,
                                                                  float* __restrict__ out, int S, int B, int B_total, int I, int A,
                                                                  int D, int irt) {
    constexpr int RB = 8;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const long long b0 = (long long)blockIdx.y * RB;
    float acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = 0.f;
    const bool ok = i < I;
    for (int s = 0; s < S; ++s) {
        const float* it = item + ((size_t)s * I + (ok ? i : 0)) * D;
        float a[VIBO_MAX_ABILITY_DIM_WIDE];
#pragma unroll
        for (int k = 0; k < VIBO_MAX_ABILITY_DIM_WIDE; ++k) a[k] = (irt != 1 && k < A) ? it[k] : 0.f;
        const float bb = irt == 1 ? it[0] : it[A];
        float g = 0.f;
        if (irt == 3) g = 1.0f / (1.0f + expf(-it[A + 1]));
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const long long b = b0 + r;
            if (b >= B) break;
            const float* th = ability + ((size_t)s * B_total + b) * A;      // sample stride = all persons
            float logit = bb;
            if (irt == 1) {
                for (int k = 0; k < A; ++k) logit += th[k];
            } else {
#pragma unroll
                for (int k = 0; k < VIBO_MAX_ABILITY_DIM_WIDE; ++k)
                    if (k < A) logit = fmaf(-a[k], th[k], logit);
            }
            float pr = 1.0f / (1.0f + expf(-logit));
            if (irt == 3) pr = g + (1.0f - g) * pr;
            acc[r] += pr;
        }
    }
    if (ok) {
        const float inv = 1.0f / (float)S;
#pragma unroll
        for (int r = 0; r < RB; ++r)
            if (b0 + r < B) out[(b0 + r) * I + i] = acc[r] * inv;
    }
}

}  // namespace vibo

using namespace vibo;

// counts of the call's rows from the caller's per-source-row counts (vibo_elbo_fwd_bwd_counts with a row_index)
__global__ __launch_bounds__(256) void gather_counts_kernel(const int32_t* __restrict__ all, const int64_t* __restrict__ row_index,
                                                            int* __restrict__ out, int B) {
    const int k = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (k < B) out[k] = all[row_index[k]];
}

// xor16_add / xor32_add (v_permlane16_swap / v_permlane32_swap through inline asm, vibo_device.hpp) next to the __shfl_xor form
// they replace: out[0][lane] | out[1][lane] = the swap forms, out[2] | out[3] = the shuffle forms (tests/test_gpu_parity.py)
__global__ void lane_swap_selftest_kernel(const float* __restrict__ in, float* __restrict__ out) {
    const int lane = threadIdx.x;
    const float v = in[lane];
    out[lane] = xor16_add(v);
    out[64 + lane] = xor32_add(v);
    out[128 + lane] = v + __shfl_xor(v, 16);
    out[192 + lane] = v + __shfl_xor(v, 32);
    // chained, as the kernels use them (the second swap reads the first one's fresh result)
    out[256 + lane] = xor32_add(xor16_add(v));
    out[320 + lane] = [&] { const float t = v + __shfl_xor(v, 16); return t + __shfl_xor(t, 32); }();
}

// ---------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------
namespace vibo {

// one thread per element, 256 threads per workgroup
template <typename K, typename... Args>
static hipError_t launch_elementwise(K kernel, long long n, hipStream_t s, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, args...);
    return hipGetLastError();
}

hipError_t launch_item_prep(const float* item, float* prep, int I, int A, int AT, int D, int DP, int irt, hipStream_t s) {
    return launch_elementwise(item_prep_kernel, (long long)I + 15, s, item, prep, I, A, AT, D, DP, irt);
}

hipError_t launch_row_counts(const vibo_desc* d, int num_cu, const float* response, const void* mask, const int64_t* row_index, int* cnt,
                             uint8_t* codes_out, long long codes_stride, hipStream_t s) {
    hipLaunchKernelGGL(row_count_kernel, dim3(clamp_grid(num_cu, 8, d->num_person, 4)), dim3(256), 0, s, response, mask, row_index, cnt,
                       (long long)d->response_row_stride, (long long)d->mask_row_stride, d->num_person, d->num_item, d->mask_dtype,
                       codes_out, codes_stride);
    return hipGetLastError();
}
hipError_t launch_row_counts_scalar(const vibo_desc* d, const float* response, const void* mask, const int64_t* row_index, int* cnt,
                                    hipStream_t s) {
    hipLaunchKernelGGL(row_count_scalar_kernel, dim3((d->num_person + 3) / 4), dim3(256), 0, s, response, mask, row_index, cnt,
                       (long long)d->response_row_stride, (long long)d->mask_row_stride, d->num_person, d->num_item, d->mask_dtype);
    return hipGetLastError();
}
hipError_t launch_gather_counts(const int32_t* all, const int64_t* row_index, int* out, int B, hipStream_t s) {
    return launch_elementwise(gather_counts_kernel, B, s, all, row_index, out, B);
}

hipError_t launch_panel_sum(float* buf, long long n, int panels, hipStream_t s) {
    return launch_elementwise(panel_sum_kernel, n, s, buf, n, panels);
}
hipError_t launch_given_pre(const float* post, float* pre, long long B, int A, int I, hipStream_t s) {
    return launch_elementwise(given_pre_kernel, B * (A + 1), s, post, pre, B, A, I);
}
hipError_t launch_given_post(const float* post, const float* coef, int panels, float* grad, long long B, int A, hipStream_t s) {
    return launch_elementwise(given_post_kernel, B * A, s, post, coef, panels, grad, B, A);
}

hipError_t launch_pack_codes(const vibo_desc* d, const float* response, const void* mask, uint8_t* codes, long long codes_row_stride,
                             bool chunks, hipStream_t s, const int64_t* row_index) {
    if (chunks) {      // aligned rows, 4 cells per thread (16 B of responses + 4 B of mask -> one code word)
        const long long n = (long long)d->num_person * (codes_row_stride / 4);
        long long grid = (n + 255) / 256;
        if (grid > 262144) grid = 262144;
        hipLaunchKernelGGL(pack_codes4_kernel, dim3((unsigned)grid), dim3(256), 0, s, response, mask, reinterpret_cast<uint32_t*>(codes),
                           (long long)d->response_row_stride, (long long)d->mask_row_stride, (long long)(codes_row_stride / 4),
                           (long long)d->num_person, d->num_item, d->mask_dtype, row_index);
        return hipGetLastError();
    }
    const long long n = (long long)d->num_person * codes_row_stride;
    long long grid = (n + 255) / 256;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(pack_codes_kernel, dim3((unsigned)grid), dim3(256), 0, s, response, mask, codes, (long long)d->response_row_stride,
                       (long long)d->mask_row_stride, codes_row_stride, (long long)d->num_person, d->num_item, d->mask_dtype);
    return hipGetLastError();
}

hipError_t launch_sign_is_mask(const vibo_desc* d, const float* response, const void* mask, bool chunks, int32_t* differs, hipStream_t s) {
    hipError_t e = hipMemsetAsync(differs, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    const long long n = (long long)d->num_person * (chunks ? (d->num_item + 3) / 4 : d->num_item);
    long long grid = (n + 255) / 256;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(chunks ? sign_is_mask4_kernel : sign_is_mask_kernel, dim3((unsigned)grid), dim3(256), 0, s, response,
                       static_cast<const uint8_t*>(mask), (long long)d->response_row_stride, (long long)d->mask_row_stride,
                       (long long)d->num_person, d->num_item, differs);
    return hipGetLastError();
}

hipError_t launch_tile_rows_build(const vibo_desc* src, const float* response, const void* mask, bool vec, void* image, hipStream_t s) {
    const int W = (src->num_item + 127) / 128;
    const long long n_wave_blocks = ((long long)src->num_person + 31) / 32 * W;
    long long grid = (n_wave_blocks + 3) / 4;
    if (grid > (1 << 20)) grid = 1 << 20;
    hipLaunchKernelGGL(tile_rows_build_kernel, dim3((unsigned)grid), dim3(256), 0, s, response, static_cast<const uint8_t*>(mask),
                       (long long)src->response_row_stride, (long long)src->mask_row_stride, (long long)src->num_person, src->num_item,
                       src->mask_dtype, vec, static_cast<uint32_t*>(image), n_wave_blocks, W);
    return hipGetLastError();
}

hipError_t launch_finalize(FinalizeParams& f, hipStream_t s) {
    const int n_out = 8 + (f.want_grad ? 8 * f.A + 2 * f.n_flows * (2 * f.A + 1) + f.I * f.D : 0);
    // (the conditional posterior's table-gradient finalize rides in the same launch: workgroups past n_fin)
    const int n_tail = f.tail.kind ? f.tail.gx * f.tail.gy : 0;
    if (finalize_group(f.bpp, n_out) == 16) {    // (vibo_variant.hpp)
        f.n_fin = (n_out + 15) / 16;
        hipLaunchKernelGGL(finalize_kernel<16>, dim3(f.n_fin + n_tail), dim3(1024), 0, s, f);
    } else {
        f.n_fin = (n_out + 63) / 64;
        hipLaunchKernelGGL(finalize_kernel<64>, dim3(f.n_fin + n_tail), dim3(1024), 0, s, f);
    }
    return hipGetLastError();
}
hipError_t launch_multi_finalize(const float* partial, float* out_scalars, int nblk, int stride, int n_samples, int reg_mode, hipStream_t s) {
    hipLaunchKernelGGL(multi_finalize_kernel, dim3(1), dim3(1024), 0, s, partial, out_scalars, nblk, stride, n_samples, reg_mode);
    return hipGetLastError();
}

hipError_t launch_encode(const EncodeParams& p, hipStream_t s) {
    hipLaunchKernelGGL(encode_kernel, dim3((p.B + 3) / 4), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_encode_finish(const int* cnt, const float* pre, int panels, const float* table, float* ability_mu, float* ability_logvar,
                                long long B, int I, int A, int missing_mode, hipStream_t s) {
    return launch_elementwise(encode_finish_kernel, B * A, s, cnt, pre, panels, table, ability_mu, ability_logvar, B, I, A, missing_mode);
}

hipError_t launch_cond_stack_finish(const float* sums, int ldc, int cnt_col, float* post, long long B, int I, int A, int G, int missing_mode,
                                    hipStream_t s) {
    return launch_elementwise(cond_stack_finish_kernel, B * G * A, s, sums, ldc, cnt_col, post, B, I, A, G, missing_mode);
}

hipError_t launch_decode(const float* ability, const float* item, float* response_mu, long long B, int I, int A, int D, int irt,
                         hipStream_t s) {
    // grid.y is limited to 65535: loop in chunks
    for (long long b0 = 0; b0 < B; b0 += 65535) {
        const int nb = (int)((B - b0 < 65535) ? (B - b0) : 65535);
        hipLaunchKernelGGL(decode_kernel, dim3((I + 255) / 256, nb), dim3(256), 0, s, ability + b0 * A, item, response_mu + b0 * I, nb, I,
                           A, D, irt);
    }
    return hipGetLastError();
}
hipError_t launch_decode_mean(int num_samples, const float* ability, const float* item, float* response_mu_mean, long long B, int I, int A,
                              int D, int irt, hipStream_t s) {
    const long long by = (B + 7) / 8;
    // grid.y is limited to 65535: loop in chunks of 65535 * 8 persons
    for (long long y0 = 0; y0 < by; y0 += 65535) {
        const int ny = (int)((by - y0 < 65535) ? (by - y0) : 65535);
        const long long p0 = y0 * 8;
        const int nb = (int)((B - p0 < (long long)ny * 8) ? (B - p0) : (long long)ny * 8);
        // ability rows of sample s start at ability + s * B * A: pass the full B as the sample stride via a shifted base
        hipLaunchKernelGGL(decode_mean_kernel_strided, dim3((I + 255) / 256, ny), dim3(256), 0, s, ability + p0 * A, item,
                           response_mu_mean + p0 * I, num_samples, nb, (int)B, I, A, D, irt);
    }
    return hipGetLastError();
}

hipError_t launch_lane_swap_selftest(const float* in, float* out, hipStream_t s) {
    hipLaunchKernelGGL(lane_swap_selftest_kernel, dim3(1), dim3(64), 0, s, in, out);
    return hipGetLastError();
}

}  // namespace vibo
