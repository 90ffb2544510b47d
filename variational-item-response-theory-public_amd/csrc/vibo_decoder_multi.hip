// vibo_decoder_multi.hip -- the forward half of the per-term MLP decoder kernel (vibo_decoder.hip, decoder_kernel<false, HASL>)
// for S stacked samples in one launch: log_marginal's importance samples and posterior_predictive's draws of the
// --generative-model link | deep | residual models, which otherwise cost one launch (and its host-side preparation) per sample.
//
// Same formulation as the single kernel: a wave owns 16 items and walks its persons two at a time on the matrix pipe
// (v_mfma_f32_16x16x32_f16, hi + lo f16 operands).  What changes is around the person walk:
//   - grid (ceil(I / 64), person chunks, sample groups); a workgroup builds the forward weight images ONCE (Fh / Fl only: no
//     backward operands, no transposition image -- 16 KB of LDS instead of 51 KB) and then takes the samples of its group in
//     ascending order: per sample the lane's 16 U values and the guess probability, a zeroed log-likelihood sum, the chunk's
//     persons, one record  ll_part[s][wave_id]  (wave_id as in the single kernel);
//   - W2, b2, w3, b3, w1, resid are shared by the samples; response and mask rows are re-read per sample (L2);
//   - the pair's inputs are still loaded one iteration ahead, across the sample boundary too;
//   - prob_sum [B][I]: the mean-over-samples accumulator of posterior_predictive.  One sample group then, so one workgroup
//     owns a (person chunk, item block) cell for all samples and its g == 0 lane reads, adds and writes in sample order: no
//     atomics, a fixed order, the bits of the caller's own accumulate over S single launches.
// The per-term statements are those of decoder_kernel, repeated here (a shared function would have to leave the four existing
// instantiations' code unchanged under their scheduler options); every block below names the block of vibo_decoder.hip it
// mirrors, and tests/test_gpu_decoder_multi.py holds every record to the single kernel's bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/vibo_hip.h"
#include "../../include/vibo_hip_decoder_multi.h"
#include "vibo_decoder_device.hpp"
#include "vibo_planner.hpp"

namespace vibo {

struct DecMultiParams {
    const float* response; const uint8_t* mask;
    long long resp_stride, mask_stride;
    const float* U; const float* V; const float* L; const float* guess; const float* w1;
    const float* W2; const float* b2; const float* w3; const float* b3;
    float resid;
    int B, I, ppc;                 // persons per chunk (blockIdx.y)
    int S, spg;                    // samples, samples per group (blockIdx.z)
    long long n_wave;              // records per sample: 4 gridDim.x gridDim.y
    float* ll_part; float* prob_sum;
    int prob_accumulate;
};

struct alignas(16) DecMultiLds {
    _Float16 Fh[4][2][64][8], Fl[4][2][64][8];    // forward A operands: W2[16 nt + m][K(g) of step s], hi | lo
    float b2[kH], w3[kH], w1[kH];
};

// Two workgroups per CU (2 waves per SIMD, 256 registers each): the forward instantiations of the single kernel need 154 / 227,
// and a second resident wave hides the load latency at a sample boundary, where the U / guess loads are not prefetched.
template <bool HASL>
__global__ __launch_bounds__(256, 2) void decoder_multi_forward_kernel(const DecMultiParams p) {
    __shared__ DecMultiLds sm;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    // ---- forward weight images (once per workgroup, for all its samples): decoder_kernel's "weight images", Fh / Fl only ----
    for (int idx = tid; idx < 4 * 2 * 64; idx += 256) {
        const int nt = idx >> 7, s = (idx >> 6) & 1, l = idx & 63;
        const int m = l & 15, gg = l >> 4;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int kk = 16 * (2 * s + (e >> 2)) + 4 * gg + (e & 3);       // K(g) order of step s
            const float wf = p.W2[(16 * nt + m) * kH + kk];                    // forward: row n = 16 nt + m
            const _Float16 fh = (_Float16)dpk(wf, 0.f)[0];
            sm.Fh[nt][s][l][e] = fh; sm.Fl[nt][s][l][e] = dpk(wf - (float)fh, 0.f)[0];
        }
    }
    if (tid < kH) {
        sm.b2[tid] = p.b2[tid]; sm.w3[tid] = p.w3[tid];
        sm.w1[tid] = (HASL && p.w1) ? p.w1[tid] : 0.f;
    }
    __syncthreads();
    const float b3 = p.b3[0];
    const int item = 64 * (int)blockIdx.x + 16 * w + i16;
    const bool item_ok = item < p.I;
    const int it = item_ok ? item : 0;
    // per-lane constants: its 16 hidden units  k(kt, j) = 16 kt + 4 g + j  (index 4 kt + j below)
    float b2v[16], w3v[16], w1v[16];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            b2v[4 * kt + j] = sm.b2[16 * kt + 4 * g + j];
            w3v[4 * kt + j] = sm.w3[16 * kt + 4 * g + j];
            w1v[4 * kt + j] = sm.w1[16 * kt + 4 * g + j];
        }
    const bool has_guess = p.guess != nullptr;

    const long long p_begin = (long long)blockIdx.y * p.ppc;
    const long long p_end = p_begin + p.ppc < p.B ? p_begin + p.ppc : p.B;
    const int s_begin = (int)blockIdx.z * p.spg;
    const int s_end = s_begin + p.spg < p.S ? s_begin + p.spg : p.S;
    const long long wave_id = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 4 + w;      // as in the single kernel
    if (p_begin >= p_end) {      // a chunk past the last person (ppc is rounded up to pairs): its records are zeros, as the single kernel's
        if (lane == 0)
            for (int s = s_begin; s < s_end; ++s) p.ll_part[s * p.n_wave + wave_id] = 0.f;
        return;
    }
    // the pair's inputs are loaded one iteration ahead: decoder_kernel's load_pair, with the sample's offsets; persons past the
    // chunk's end are clamped to its last one, and the pair behind the group's last sample re-reads that sample's first one
    struct PersonIn { float4 v[4]; float x, l; unsigned m; };
    PersonIn cur[2], nxt[2];
    auto load_pair = [&](const int s, const long long pp, PersonIn (&d)[2]) {
        const float* Vs = p.V + (size_t)s * p.B * kH;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const long long pr = pp + r;
            const long long prc = pr < p_end ? pr : p_end - 1;
            d[r].x = p.response[prc * p.resp_stride + it];
            d[r].m = p.mask ? (unsigned)p.mask[prc * p.mask_stride + it] : 1u;
            d[r].l = 0.f;
            if constexpr (HASL) d[r].l = p.L[((long long)s * p.B + prc) * (long long)p.I + it];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) d[r].v[kt] = *reinterpret_cast<const float4*>(Vs + (size_t)prc * kH + 16 * kt + 4 * g);
        }
    };
    load_pair(s_begin, p_begin, cur);
#pragma unroll 1
    for (int s = s_begin; s < s_end; ++s) {
        // per-sample lane constants: decoder_kernel's u[] and guess loads
        float u[16];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const float4 t = p.U ? *reinterpret_cast<const float4*>(p.U + ((size_t)s * p.I + it) * kH + 16 * kt + 4 * g) : float4{0.f, 0.f, 0.f, 0.f};
            u[4 * kt] = t.x; u[4 * kt + 1] = t.y; u[4 * kt + 2] = t.z; u[4 * kt + 3] = t.w;
        }
        const float guess = (p.guess && item_ok) ? p.guess[(size_t)s * p.I + item] : 0.f;
        const bool first_write = s == 0 && !p.prob_accumulate;      // prob_sum: the call's first sample starts the sum
        float llsum = 0.f;
#pragma unroll 1
        for (long long pp = p_begin; pp < p_end; pp += 2) {
            if (pp + 2 < p_end) load_pair(s, pp + 2, nxt);
            else load_pair(s + 1 < s_end ? s + 1 : s, p_begin, nxt);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const long long pr = pp + r;
                const bool ok = pr < p_end && item_ok;
                const float x = cur[r].x;
                const bool obs = ok && cur[r].m != 0;
                const float l = cur[r].l;
                // ---- layer 1 (element-wise in the operand layout): decoder_kernel's "layer 1" ----
                float z1[16], h1f[16];
                dh8 h1h[2], h1l[2];
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    const float4 v = cur[r].v[kt];
                    z1[4 * kt] = u[4 * kt] + v.x; z1[4 * kt + 1] = u[4 * kt + 1] + v.y;
                    z1[4 * kt + 2] = u[4 * kt + 2] + v.z; z1[4 * kt + 3] = u[4 * kt + 3] + v.w;
                }
#pragma unroll
                for (int a = 0; a < 16; ++a) {
                    if constexpr (HASL) z1[a] = fmaf(w1v[a], l, z1[a]);
                    h1f[a] = elu(z1[a]);
                }
                split8(&h1f[0], h1h[0], h1l[0]);
                split8(&h1f[8], h1h[1], h1l[1]);
                // ---- layer 2: Z2^T = W2 . h1^T: decoder_kernel's "layer 2" ----
                float opart = 0.f;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    df4 acc = df4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int st = 0; st < 2; ++st) {
                        const dh8 ah = *reinterpret_cast<const dh8*>(&sm.Fh[nt][st][lane][0]);
                        const dh8 al = *reinterpret_cast<const dh8*>(&sm.Fl[nt][st][lane][0]);
                        acc = dmfma(ah, h1h[st], acc);
                        acc = dmfma(ah, h1l[st], acc);
                        acc = dmfma(al, h1h[st], acc);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float z2 = acc[j] + b2v[4 * nt + j];
                        const float h2 = elu(z2);
                        opart = fmaf(w3v[4 * nt + j], h2, opart);
                    }
                }
                opart = xor16_add(opart);
                opart = xor32_add(opart);
                float o = opart + b3;
                if constexpr (HASL) o = fmaf(p.resid, l, o);
                // ---- link + masked Bernoulli log-likelihood: decoder_kernel's block of that name (values only, no gradient) ----
                const float eo = expf(-fabsf(o));
                const float big = 1.0f / (1.0f + eo), small = eo * big;
                const float sg = o >= 0.f ? big : small, sq = o >= 0.f ? small : big;       // sigmoid(o), 1 - sigmoid(o)
                const float pr_ = has_guess ? guess + (1.0f - guess) * sg : sg;
                const float qr_ = has_guess ? (1.0f - guess) * sq : sq;
                const bool inside = pr_ >= kEps32 && pr_ <= 1.0f - kEps32;
                const float pc = inside ? pr_ : fminf(fmaxf(pr_, kEps32), 1.0f - kEps32);
                const float qc = inside ? qr_ : 1.0f - pc;
                float ll = 0.f;
                if (obs) {
                    const bool one = x > 0.5f;
                    ll = logf(fmaxf(one ? pc : qc, kEps32));
                }
                if (g == 0) llsum += ll;
                if (p.prob_sum && ok && g == 0) {
                    float* cell = p.prob_sum + pr * (long long)p.I + item;
                    *cell = first_write ? pr_ : *cell + pr_;
                }
            }
            cur[0] = nxt[0]; cur[1] = nxt[1];
        }
        const float t = wave_total(llsum);
        if (lane == 0) p.ll_part[s * p.n_wave + wave_id] = t;
    }
}

}  // namespace vibo

using namespace vibo;

extern "C" int vibo_decoder_multi_person_chunks(int num_person, int num_item, int num_samples) {
    if (num_person < 1 || num_item < 1 || num_samples < 1) return 0;
    const long long cells = (long long)((num_item + 63) / 64) * num_samples;      // workgroups the items and the samples supply already
    long long chunks = ((long long)device_cus() * 2 + cells - 1) / cells;         // about two workgroups per CU in flight
    const long long most = ((long long)num_person + 1) / 2;                        // at least one person pair per chunk
    if (chunks > most) chunks = most;
    if (chunks < 1) chunks = 1;
    return (int)chunks;
}

extern "C" int vibo_decoder_multi_forward(const vibo_decoder_desc* d, int num_samples, const float* response, const uint8_t* mask,
                                          const float* U, const float* V, const float* L, const float* guess, const float* w1,
                                          const float* W2, const float* b2, const float* w3, const float* b3,
                                          float* ll_part, float* prob_sum, int prob_accumulate, void* stream) {
    const char* const fn = "vibo_decoder_multi_forward";
    if (!d) return fail(-1, "%s: NULL descriptor", fn);
    if (d->num_person < 1 || d->num_item < 1 || num_samples < 1)
        return fail(-2, "%s: num_person = %d, num_item = %d, num_samples = %d (each at least 1)", fn, d->num_person, d->num_item, num_samples);
    if (d->hidden_dim != kH) return fail(-6, "%s: hidden_dim = %d (the kernel's width is %d; narrower networks go in zero-padded)", fn, d->hidden_dim, kH);
    if (d->person_chunks < 1 || d->person_chunks > d->num_person)
        return fail(-3, "%s: person_chunks = %d outside 1..num_person = %d", fn, d->person_chunks, d->num_person);
    if (!response || !V || !W2 || !b2 || !w3 || !b3 || !ll_part) return fail(-5, "%s: response, V, W2, b2, w3, b3 and ll_part are required", fn);
    const bool hasl = L != nullptr;
    if ((w1 || d->resid != 0.f) && !hasl) return fail(-5, "%s: w1 / resid without the logits L", fn);
    if (d->want_grad) return fail(-5, "%s: forward only (want_grad = 0); gradients come from vibo_decoder_fwd_bwd", fn);
    if ((((uintptr_t)V) | ((uintptr_t)U)) & 15) return fail(-4, "%s: U and V must be 16-byte aligned", fn);
    DecMultiParams p;
    memset(&p, 0, sizeof(p));
    p.response = response; p.mask = mask; p.resp_stride = d->response_row_stride; p.mask_stride = d->mask_row_stride;
    p.U = U; p.V = V; p.L = L; p.guess = guess; p.w1 = w1; p.W2 = W2; p.b2 = b2; p.w3 = w3; p.b3 = b3; p.resid = d->resid;
    p.B = d->num_person; p.I = d->num_item; p.S = num_samples;
    p.ppc = (int)((((long long)d->num_person + d->person_chunks - 1) / d->person_chunks + 1) & ~1ll);    // even: persons go in pairs
    const int n_ib = (d->num_item + 63) / 64;
    p.n_wave = 4ll * n_ib * d->person_chunks;
    // sample groups: about two workgroups per CU, at most one group per sample; one group when the cells of prob_sum are summed
    long long groups = 1;
    if (!prob_sum) {
        const long long cells = (long long)n_ib * d->person_chunks;
        groups = ((long long)device_cus() * 2 + cells - 1) / cells;
        if (groups > num_samples) groups = num_samples;
        if (groups < 1) groups = 1;
    }
    p.spg = (int)((num_samples + groups - 1) / groups);
    groups = (num_samples + p.spg - 1) / p.spg;
    if (groups > 65535) {      // the grid's z extent
        p.spg = (num_samples + 65534) / 65535;
        groups = (num_samples + p.spg - 1) / p.spg;
    }
    p.ll_part = ll_part; p.prob_sum = prob_sum; p.prob_accumulate = prob_accumulate;
    const dim3 grid((unsigned)n_ib, (unsigned)d->person_chunks, (unsigned)groups), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (hasl) hipLaunchKernelGGL((decoder_multi_forward_kernel<true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((decoder_multi_forward_kernel<false>), grid, block, 0, s, p);
    return launch_rc("vibo_decoder_multi_forward launch");
}
