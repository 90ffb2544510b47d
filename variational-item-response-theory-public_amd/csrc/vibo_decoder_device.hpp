// vibo_decoder_device.hpp -- what the per-term decoder kernels (vibo_decoder.hip, vibo_decoder_multi.hip) share on the device:
// the operand types of v_mfma_f32_16x16x32_f16, the hi + lo f16 split of an fp32 operand and the ELU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vibo_device.hpp"

namespace vibo {

typedef _Float16 dh8 __attribute__((ext_vector_type(8)));
typedef _Float16 dh4 __attribute__((ext_vector_type(4)));
typedef _Float16 dh2 __attribute__((ext_vector_type(2)));
typedef float df4 __attribute__((ext_vector_type(4)));
typedef short ds4 __attribute__((ext_vector_type(4)));

constexpr int kH = 64;             // hidden width of the per-term network (models.py:777, 824: hidden_dim = 64)

__device__ __forceinline__ df4 dmfma(const dh8 a, const dh8 b, const df4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ dh4 dtr16(const _Float16* p) {
    return __builtin_bit_cast(dh4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((ds4 __attribute__((address_space(3)))*)p));
}
__device__ __forceinline__ dh2 dpk(float a, float b) { return __builtin_bit_cast(dh2, __builtin_amdgcn_cvt_pkrtz(a, b)); }
// 8 floats -> f16 hi and lo pieces: x = hi + lo to 2^-22 |x| while lo is a normal f16, i.e. for |x| >= 2^-3; below that lo sits on
// the f16 subnormal grid and the pieces reassemble x to 2^-25 ABSOLUTE (3e-5 of an x near 1e-3); below 2^-14 hi is on that grid
// too.  No operand is rescaled: oracle/decoder_model.py carries this floor in its bounds, tests/test_gpu_decoder_cells.py holds the
// device's residual to it element by element (subnormal pieces are kept by the conversions and by the MFMA).
// (hi = round-toward-zero pair; lo = f16(x - hi) by two mixed-precision fmas that write the two halves of one register)
__device__ __forceinline__ void split8(const float* x, dh8& hi, dh8& lo) {
    uint32_t hw[4], lw[4];
    float xv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) xv[e] = x[e];
#pragma unroll
    for (int e = 0; e < 8; e += 2) hw[e >> 1] = __builtin_bit_cast(uint32_t, dpk(x[e], x[e + 1]));
    lo_pieces4(hw, xv, lw);      // (one asm block ending in the wait states an MFMA consumer needs: vibo_device.hpp)
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        const dh2 h = __builtin_bit_cast(dh2, hw[e >> 1]), l = __builtin_bit_cast(dh2, lw[e >> 1]);
        hi[e] = h[0]; hi[e + 1] = h[1];
        lo[e] = l[0]; lo[e + 1] = l[1];
    }
}
__device__ __forceinline__ float elu(float z) { return z > 0.f ? z : fast_exp2(z * kLog2e) - 1.0f; }

}  // namespace vibo
