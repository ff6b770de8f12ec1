// pbl_kv8_format.h -- the row format of the FP8 KV cache, on the device (the torch reference is runtime.kv8_quantize / kv8_dequantize).
//
// A cache row -- one token of one kv head, D = 64 or 128 values -- is D bytes of OCP e4m3fn and ONE power-of-two scale 2^e, kept as
// an fp32 in a side array [B, Hkv, max_len].  For a row x of fp16 values: amax = max |x|, e the smallest integer with
// amax <= 448 * 2^e, clamped to [-15, 7] (an all-zero row: -15); byte j = e4m3fn(x_j / 2^e), round to nearest even, the division
// exact.  With e in [-15, 7] every dequantised value byte * 2^e has a 4-bit significand between 2^-24 and 57344: it IS an fp16 value,
// and multiplying by 2^e commutes with every rounding the attention kernels do.
//
// Values outside the format: after the clamp at e = 7 a row with amax > 57344 (+-inf included) saturates at +-448.  A NaN element
// becomes a NaN byte (0x7f / 0xff) and does not enter amax (fmaxf drops it); a row of nothing but NaN takes e = -15.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int KV8_E_MIN = -15, KV8_E_MAX = 7;
constexpr float KV8_MAX = 448.f;               // the largest e4m3fn value

// 8 e4m3fn bytes -> their values (v_cvt_pk_f32_fp8: exact)
__device__ __forceinline__ void kv8_unpack8(const uint2 w, float* f) {
    typedef float v2f __attribute__((ext_vector_type(2)));
    const v2f a = __builtin_amdgcn_cvt_pk_f32_fp8(int(w.x), false), b = __builtin_amdgcn_cvt_pk_f32_fp8(int(w.x), true);
    const v2f c = __builtin_amdgcn_cvt_pk_f32_fp8(int(w.y), false), d = __builtin_amdgcn_cvt_pk_f32_fp8(int(w.y), true);
    f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1];
    f[4] = c[0]; f[5] = c[1]; f[6] = d[0]; f[7] = d[1];
}

// the row's exponent from its amax (>= 0, an fp16 value held in fp32, or +inf; NaN, from a row of nothing else, counts as 0):
// amax = 1.m x 2^x, and 448 = 1.75 x 2^8, so e = x - 8, one more where 1.m > 1.75.  Returns 2^e; *inv = 2^-e (x_j * 2^-e is the exact division).
__device__ __forceinline__ float kv8_scale(float amax, float* inv) {
    const uint32_t bits = __builtin_bit_cast(uint32_t, fmaxf(amax, 0.f));
    int e = int(bits >> 23) - 127 - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
    e = e < KV8_E_MIN ? KV8_E_MIN : (e > KV8_E_MAX ? KV8_E_MAX : e);
    *inv = __builtin_bit_cast(float, uint32_t(127 - e) << 23);
    return __builtin_bit_cast(float, uint32_t(127 + e) << 23);
}

// two values, already divided by the row's scale -> two bytes in the low half of the result (v_cvt_pk_fp8_f32: round to nearest
// even).  Values beyond +-448 saturate here, whatever the conversion's overflow mode; NaN passes the comparisons and stays NaN.
__device__ __forceinline__ uint32_t kv8_pack2(float a, float b) {
    a = a > KV8_MAX ? KV8_MAX : (a < -KV8_MAX ? -KV8_MAX : a);
    b = b > KV8_MAX ? KV8_MAX : (b < -KV8_MAX ? -KV8_MAX : b);
    return uint32_t(__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false)) & 0xffffu;
}

// max over the `width` lanes (a power of two <= 64, aligned) that share a row
__device__ __forceinline__ float kv8_group_max(float v, int width) {
    for (int off = width >> 1; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

}  // namespace
