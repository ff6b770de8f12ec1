// pbl_rope_math.h -- the argument block and the fp16 arithmetic of the rotary-embedding kernels (pbl_kernels.hip: pbl_rope_f16,
// pbl_rope_append_f16; pbl_kv8.hip: pbl_rope_append_kv8), stated once so that every one of them rounds alike.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

struct RopeArgs {
    const uint16_t* qkv;            // [M, ld] fp16: q heads at column q_off, k heads at k_off (token m = b * S + s)
    const uint16_t* cos;            // cos / sin [.., D] fp16: the row of token (b, s) at b * c_sb + s * c_ss (0: broadcast)
    const uint16_t* sin;
    uint16_t* q_out;                // element (b, h, s, d) at b * ob + h * oh + s * os + d
    uint16_t* k_out;
    int64_t c_sb, c_ss;
    int64_t q_ob, q_oh, q_os, k_ob, k_oh, k_os;
    uint32_t ld, q_off, k_off;
    int S, Hq, H, half, pairs;      // H = Hq + Hkv; pairs = M * H * half
};

// a value the compiler cannot trace back to an fp16 operand: the arithmetic on it stays fp32 (no fp16 / mixed-precision rewrite)
__device__ __forceinline__ float opaque(float v) {
    asm volatile("" : "+v"(v));
    return v;
}
// (a * b) rounded to fp16, as torch's `*` on half tensors: an fp32 product (exact for two fp16 values), one rounding.  The product
// is materialised before the rounding: fptrunc(fmul) would otherwise become v_fma_mixlo_f16 with a +0 addend, which turns a -0
// product into +0.
__device__ __forceinline__ float mul_f16(float a, float b) {
#pragma clang fp contract(off)
    return opaque(float(_Float16(opaque(opaque(a) * opaque(b)))));
}

}  // namespace
