// pbl_kernels.hip -- gfx950 (MI355X, CDNA4) kernels of libpbl.so.
//
// One kernel family: the partially-binarized GEMV
//     y[m, r] = sum_j v_rj * x[m, j] + bias_r            (m <= 4 tokens per pass)
// over the PBL1 packed format (include/pbl.h).  It replaces the reference's
//     w_sim = where(mask, W*outlier_scale, sign(W)*binary_scale); F.linear(x, w_sim, b)
// (quant/outlier_quantizer.py:83-106) and the stock nn.Linear forward over GPTQ-PB
// fake-quant weights (gptq_pb/gptq.py:180-184).
//
// Work decomposition: ONE WAVEFRONT (64 lanes) owns ONE RECORD = 16 output rows.
//   phase 0  the workgroup stages x (fp16) into LDS, zero padded
//   phase 1  sign plane: per 512-column panel one coalesced 1 KiB global_load_dwordx4
//            per wave; lane l holds x for ITS columns in 4 VGPRs (half2), unpacks a
//            pair of weights to a two-valued fp16 constant with ONE v_and(_or)_b32
//            ("bit classes") and accumulates with v_dot2_f32_f16
//   phase 2  salient list: lane-per-chunk (16 delta-coded columns + 16 uint8 codes,
//            coalesced 16 B/lane loads), x gathered from LDS
//   phase 3  transpose-reduce the 16 row accumulators across the wave, combine
//            with the per-chunk partials in fixed order (deterministic), store y.
// HBM-bound by design: every weight byte is read exactly once, x comes from L2/LDS.
// No inter-workgroup communication, so no XCD-placement dependence.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pbl.h"
#include "pbl_p2p_layout.h"
#include "pbl_rope_math.h"

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define PBL_WAVE 64

namespace {

__device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c) {
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, a), __builtin_bit_cast(h2, b), c, false);
}

// fl16(fl32(a*b)): the checkpoint's value of a salient weight is DOUBLE rounded (fp32 product,
// then `.to(fp16)`, gptq_pb/gptq.py:182).  hipcc would fuse mul + cvt into one single-rounding
// v_fma_mixlo_f16 (1 fp16 ulp off on ~1e-5 of the values); the empty asm keeps the fp32 product.
__device__ __forceinline__ _Float16 round_f16_twice(float prod) {
    asm volatile("" : "+v"(prod));
    return _Float16(prod);
}

// Bit classes 8..15 of an fp16 half-word: pair mask M and OR-constant C such that
// (w & M) | C is an fp16x2 holding {lo_c, lo_c + d_c} per element.  The signed
// sum over a lane's columns is  D = A_c * acc - B_c * Xl  (Xl = plain sum of x).
//   c=8 : {1,1.25}  c=9 : {1,1.5}  c=10..14 : {0, 2^-14, 2^-13, 2^-11, 2^-7, 2}  c=15 : {1,-1}
template <int CI> struct BitClass;
#define PBL_CLASS(ci, m, c) \
    template <> struct BitClass<ci> { static constexpr uint32_t M = m, C = c; };
PBL_CLASS(0, 0x01000100u, 0x3C003C00u)
PBL_CLASS(1, 0x02000200u, 0x3C003C00u)
PBL_CLASS(2, 0x04000400u, 0u)
PBL_CLASS(3, 0x08000800u, 0u)
PBL_CLASS(4, 0x10001000u, 0u)
PBL_CLASS(5, 0x20002000u, 0u)
PBL_CLASS(6, 0x40004000u, 0u)
PBL_CLASS(7, 0x80008000u, 0x3C003C00u)
#undef PBL_CLASS

__device__ __forceinline__ void class_consts(int ci, float& A, float& B) {
    const float a[8] = {8.f, 4.f, 32768.f, 16384.f, 4096.f, 256.f, 1.f, -1.f};
    const float b[8] = {9.f, 5.f, 1.f, 1.f, 1.f, 1.f, 1.f, 0.f};
    A = a[0]; B = b[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) { A = ci == k ? a[k] : A; B = ci == k ? b[k] : B; }
}

// (w & M) | C in one VALU op.  hipcc splits it into v_and + v_or because VOP3 takes no
// literal on gfx9; with M in an SGPR and C in a VGPR it is a single v_and_or_b32.
template <int CI>
__device__ __forceinline__ uint32_t unpack_pair(uint32_t w, uint32_t c_one, float order_after) {
    if constexpr (BitClass<CI>::C == 0u) {
        return w & BitClass<CI>::M;
    } else {
        // `order_after` (an accumulator the previous class step wrote) is an unused input: it pins this instruction behind that
        // step.  Without it hipcc schedules all 24 v_and_or of a tile first (to re-request the tile registers early), holds 24
        // temporaries and the kernel drops from 8 to 6 waves per SIMD.
        uint32_t t;
        asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(t) : "v"(w), "s"(BitClass<CI>::M), "v"(c_one), "v"(order_after));
        return t;
    }
}

template <int MB, int CI>
__device__ __forceinline__ void class_step(uint32_t w, uint32_t ws, uint32_t c_one, const uint32_t (&xr)[MB],
                                           float (&acc)[MB][16]) {
    const float dep = acc[0][(CI + 7) & 7];
    const uint32_t t0 = unpack_pair<CI>(w, c_one, dep);
    const uint32_t t1 = unpack_pair<CI>(ws, c_one, dep);
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        acc[m][CI] = dot2(t0, xr[m], acc[m][CI]);
        acc[m][8 + CI] = dot2(t1, xr[m], acc[m][8 + CI]);
    }
}

template <int MB>
__device__ __forceinline__ void word_step(uint32_t w, uint32_t c_one, const uint32_t (&xr)[MB],
                                          float (&acc)[MB][16], float (&xl)[MB]) {
    const uint32_t ws = w << 8;
#pragma unroll
    for (int m = 0; m < MB; ++m) xl[m] = dot2(c_one, xr[m], xl[m]);
    class_step<MB, 0>(w, ws, c_one, xr, acc);
    class_step<MB, 1>(w, ws, c_one, xr, acc);
    class_step<MB, 2>(w, ws, c_one, xr, acc);
    class_step<MB, 3>(w, ws, c_one, xr, acc);
    class_step<MB, 4>(w, ws, c_one, xr, acc);
    class_step<MB, 5>(w, ws, c_one, xr, acc);
    class_step<MB, 6>(w, ws, c_one, xr, acc);
    class_step<MB, 7>(w, ws, c_one, xr, acc);
}

// DPP / permlane helpers (wave64, gfx950).
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
constexpr int DPP_QUAD_XOR1 = 0xB1, DPP_QUAD_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_ROW_ROR8 = 0x128,
              DPP_ROW_MIRROR = 0x140;

// v_permlane{32,16}_swap exchange halves / odd-even rows of TWO registers in place.  The
// __builtin forms mis-pair their two results under hipcc 7.2 here (the second result is
// read from the first register), so the swap is issued from inline asm; "s_nop 1" covers
// the VALU-write -> permlane-read hazard, which the compiler does not pad inside asm.
// sum of a over the two 32-lane halves -> lanes 0..31 get a's total, lanes 32..63 b's
__device__ __forceinline__ float fold32(float a, float b) {
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return a + b;
}
// same across the odd/even 16-lane rows: even rows get a's total, odd rows get b's
__device__ __forceinline__ float fold16(float a, float b) {
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return a + b;
}

// 16 per-lane accumulators -> lane l holds the wave total of row
//   rho(l) = 8*bit5(l) + 4*bit4(l) + 2*bit3(l) + bit2(l)   (4 lanes per row).
__device__ __forceinline__ float transpose_reduce16(const float (&a)[16], int lane) {
    float v[8], u[4], t[2];
    const bool b3 = lane & 8, b2 = lane & 4;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = fold32(a[j], a[j + 8]);
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = fold16(v[j], v[j + 4]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float send = b3 ? u[j] : u[j + 2], keep = b3 ? u[j + 2] : u[j];
        t[j] = keep + dpp<DPP_ROW_ROR8>(send);
    }
    const float send = b2 ? t[0] : t[1], keep = b2 ? t[1] : t[0];
    float s = keep + dpp<DPP_HALF_MIRROR>(send);  // partner 7-i: opposite bit2, bijective on bits 0..1
    s += dpp<DPP_QUAD_XOR1>(s);
    s += dpp<DPP_QUAD_XOR2>(s);
    return s;
}

__device__ __forceinline__ float wave_sum(float v) {
    v += dpp<DPP_QUAD_XOR1>(v);
    v += dpp<DPP_QUAD_XOR2>(v);
    v += dpp<DPP_HALF_MIRROR>(v);
    v += dpp<DPP_ROW_MIRROR>(v);
    v = fold16(v, v);
    return fold32(v, v);
}

// sum over the 4 lanes that share a row (lane bits 0..1)
__device__ __forceinline__ float quad_sum(float v) {
    v += dpp<DPP_QUAD_XOR1>(v);
    return v + dpp<DPP_QUAD_XOR2>(v);
}

struct GemvArgs {
    pbl_layer layer;      // single-layer launch: by value
    const _Float16* x;    // [M, K]
    void* y;              // [M, N] fp16 or fp32
    // grouped launch: device arrays
    const pbl_layer* layers;
    const void* const* xs;
    void* const* ys;
    int M;                // tokens in this pass (== MB)
    int y_f32;
    int grouped;
    // fused launch (pbl_gemv_f16_fused): every layer reads the SAME x and writes its column range of ONE output
    // matrix y[M, ldy]; x_shared / y_shared override xs[] / ys[] when set
    const _Float16* x_shared;
    void* y_shared;
    const uint64_t* y_off;   // device: element offset of layer l's columns in a row of y
    uint32_t ldy;            // row stride of y in elements (0: the layer's own N)
    int Lc;                  // layers of a grouped launch (host side only)
    int tok0;                // column-group kernel in a grouped launch: first token of this pass (it takes 2 tokens per pass)
    // fused launch of at most PBL_FUSED_INLINE_MAX layers: the descriptors and output offsets travel IN the kernel arguments
    // (scalar loads from the argument segment) instead of a device table -- one dependent memory round trip less per workgroup
    int n_inl;
    pbl_layer inl[PBL_FUSED_INLINE_MAX];
    uint64_t inl_off[PBL_FUSED_INLINE_MAX];
    // fused peer push (pbl_linear_f16_push; K-split tensor parallelism): the row owners write their fp32 partials straight into
    // slot [set][rank] of EVERY rank's communication buffer (csrc/pbl_p2p_layout.h) instead of y, and every record counts itself
    // at the peers once its rows are visible system wide; pbl_p2p_reduce_f32_dev sums the slots.  push_world == 0: off.
    int push_world, push_rank;
    size_t push_cap;
    uint8_t* push_peer[PBL_P2P_MAX_WORLD];
    // bf16 activations IN the kernel (round 5; pbl_linear_bf16 / pbl_gemv_bf16_fused_host): x is bf16 -- the staging phase finds every
    // token's largest magnitude, scales the row by a power of two into fp16's range (exact) while it copies it into LDS, the epilogue
    // multiplies the result back and writes bf16 (fp32 when y_f32).  A token holding inf / NaN runs as its indicator row with scale
    // +inf.  Exactly the arithmetic of pbl_act_bf16_prepare + the fp16 kernel + pbl_act_finish (csrc/pbl_act.hip), in ONE launch.
    int x_bf16;
    // x prologues (XP; pbl_gemv_f16_fused_norm_host / pbl_linear_f16_swiglu): the staging phase builds the multiplied row from the
    // decoder layer's raw tensors.  RMSNorm: x is the hidden state, norm_w [K] fp16 the norm's weight.  SwiGLU: x is a [M, ldx]
    // matrix whose row holds gate at column 0 and up at column up_off.  (At the END of the struct: no kernarg offset moves.)
    const _Float16* norm_w;
    float norm_eps;
    uint32_t ldx;
    uint32_t up_off;
    // residual epilogue (XE_RESIDUAL; pbl_linear_f16_residual / pbl_linear_f16_swiglu_residual): y[m, n] = fp16(fp16(linear) +
    // residual[m * ldr + n]) -- HF's `residual + hidden_states` after the linear's own fp16 result.  (At the END of the struct.)
    const _Float16* residual;
    uint32_t ldr;
};
// XP: the x prologue in bits 0..1, the residual epilogue as bit 2 (a flag, so that XP_NONE -- the headline kernel -- keeps its name)
enum { XP_NONE = 0, XP_RMSNORM = 1, XP_SWIGLU = 2, XE_RESIDUAL = 4 };

// Gather 8 fp16 values from LDS byte addresses a[0..7] into 4 packed half2 registers
// (entry 2p in the low half, 2p+1 in the high half).  All loads are in flight and waited
// for once inside the statement (guide 5.7 form (i)); hipcc's own schedule waits per load.
// d16/d16_hi loads cannot build the pair: with SRAM-ECC (always on here) they ZERO the
// other half of the destination instead of preserving it, so the halves are merged with
// one v_lshl_or_b32 per pair.
__device__ __forceinline__ void gather8(const uint32_t (&a)[8], uint32_t (&x)[4]) {
    uint32_t t[8];
    asm volatile(
        "ds_read_u16 %0, %8\n\tds_read_u16 %1, %9\n\tds_read_u16 %2, %10\n\tds_read_u16 %3, %11\n\t"
        "ds_read_u16 %4, %12\n\tds_read_u16 %5, %13\n\tds_read_u16 %6, %14\n\tds_read_u16 %7, %15\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "=&v"(t[4]), "=&v"(t[5]), "=&v"(t[6]), "=&v"(t[7])
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7])
        : "memory");
#pragma unroll
    for (int p = 0; p < 4; ++p) x[p] = (t[2 * p + 1] << 16) | t[2 * p];
}

// One salient chunk (lane-private): 16 delta-coded columns + 16 uint8 codes, processed as
// two halves of 4 pairs (keeps the live register set small -> more waves per SIMD).
// Codes become fp16 (1024+q) with ONE v_perm_b32 per pair (0x64 exponent byte), so
//   Qb += dot2((1024+q0, 1024+q1), (x0, x1))   and   S += dot2((1,1), (x0,x1));
// the true code sum is Qb - 1024*S.  Deltas are stored pre-doubled (byte steps into the
// fp16 x tile), so one SDWA add per entry yields the LDS address.
//
// SF (PBL_FLAG_SAL_F16 layers, fp16 checkpoints): the salient weight is fl16(ss*(q-sz)); it
// is rebuilt per entry (v_cvt_f32_ubyte, v_sub, v_mul) and the pair rounded with ONE
// v_cvt_pk_f16_f32, so Q accumulates the exact checkpoint value times x.
template <int MB, bool PRED, bool SF>
__device__ __forceinline__ void chunk_accumulate(uint32_t xbase, uint32_t tok_stride_bytes, uint32_t col0,
                                                 const u32x4& d4, const u32x4& q4, int cnt, uint32_t zaddr,
                                                 uint32_t c_one, float ss, float sz, float (&Q)[MB], float (&S)[MB]) {
    uint32_t run = xbase + 2u * col0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        uint32_t a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = 8 * h + k;
            run += (d4[e >> 2] >> (8 * (e & 3))) & 0xFFu;
            a[k] = PRED ? (e < cnt ? run : zaddr) : run;
        }
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            uint32_t x[4];
            gather8(a, x);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                uint32_t qp;
                if constexpr (SF) {
                    const uint32_t qw = q4[2 * h + (p >> 1)] >> ((p & 1) * 16);
                    h2 w;
                    w.x = round_f16_twice(ss * (float(qw & 0xFFu) - sz));
                    w.y = round_f16_twice(ss * (float((qw >> 8) & 0xFFu) - sz));
                    qp = __builtin_bit_cast(uint32_t, w);
                } else {
                    qp = __builtin_amdgcn_perm(q4[2 * h + (p >> 1)], 0x64646464u, (p & 1) ? 0x00070006u : 0x00050004u);
                }
                Q[m] = dot2(qp, x[p], Q[m]);
                S[m] = dot2(c_one, x[p], S[m]);
            }
            if (m + 1 < MB) {
#pragma unroll
                for (int k = 0; k < 8; ++k) a[k] += tok_stride_bytes;
            }
        }
    }
}

// fp32 -> bf16 bits, round to nearest even; NaN stays NaN (csrc/pbl_act.hip)
__device__ __forceinline__ uint32_t bf16_bits_rne(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x0040u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
// one bf16 (low 16 bits of b) -> the fp16 bits the kernel multiplies with: scaled by `down` (a power of two: exact) when the token is
// finite; else the indicator finite -> 0, +-inf -> +-1, NaN -> NaN (csrc/pbl_act.hip: act_bf16_prepare_kernel, the same arithmetic)
__device__ __forceinline__ uint32_t bf16_to_scaled_f16(uint32_t b, bool finite, float down) {
    const float f = __builtin_bit_cast(float, b << 16);
    float r;
    if (finite) r = f * down;
    else {
        const uint32_t a = (b << 16) & 0x7FFFFFFFu;
        r = a > 0x7F800000u ? f : (a == 0x7F800000u ? ((b & 0x8000u) ? -1.f : 1.f) : 0.f);
    }
    return uint32_t(__builtin_bit_cast(uint16_t, _Float16(r)));
}

// HF's SwiGLU on half tensors, one element: F.silu (fp32 opmath, g / (1 + exp(-g)), one rounding to fp16), then `*` (the product of
// two fp16 values is exact in fp32: one rounding).  +-inf / NaN propagate as torch's do.
__device__ __forceinline__ uint32_t swiglu_f16(uint32_t gb, uint32_t ub) {
    const float g = float(__builtin_bit_cast(_Float16, uint16_t(gb)));
    const _Float16 s = _Float16(g / (1.0f + expf(-g)));
    const _Float16 r = _Float16(float(s) * float(__builtin_bit_cast(_Float16, uint16_t(ub))));
    return uint32_t(__builtin_bit_cast(uint16_t, r));
}
// HF's LlamaRMSNorm, one element of an fp16 row with normaliser r: fp16(g * fp16(x * r)) -- normalise in fp32, round to the input
// dtype, multiply by the fp16 weight (exact in fp32), round once.
__device__ __forceinline__ uint32_t rmsnorm_f16(uint32_t xb, uint32_t gb, float r) {
    const _Float16 h = _Float16(float(__builtin_bit_cast(_Float16, uint16_t(xb))) * r);
    const _Float16 o = _Float16(float(__builtin_bit_cast(_Float16, uint16_t(gb))) * float(h));
    return uint32_t(__builtin_bit_cast(uint16_t, o));
}

// Phase 0's copy of one token: dst[i] = f(a[i], b[i]) for i < K, then zeroes in [K, xstride).  f maps fp16 / bf16 bit patterns to
// fp16 bits; b is the transform's second operand (the norm's weight, SwiGLU's up; a itself where there is none).  vec (the caller's
// test: K % 8 == 0 and every source 16-byte aligned): 8 halves per lane and step; else one.
template <int NTHR, typename F>
__device__ __forceinline__ void stage_row(_Float16* dst, const uint16_t* a, const uint16_t* b, int K, int xstride, bool vec, int tid, F f) {
    if (vec) {
        const u32x4* asrc = reinterpret_cast<const u32x4*>(a);
        const u32x4* bsrc = reinterpret_cast<const u32x4*>(b);
        for (int i = tid; i < (K >> 3); i += NTHR) {
            const u32x4 v = asrc[i], w = bsrc[i];
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = f(v[j] & 0xFFFFu, w[j] & 0xFFFFu) | (f(v[j] >> 16, w[j] >> 16) << 16);
            reinterpret_cast<u32x4*>(dst)[i] = o;
        }
    } else {
        for (int i = tid; i < K; i += NTHR) reinterpret_cast<uint16_t*>(dst)[i] = uint16_t(f(a[i], b[i]));
    }
    for (int i = K + tid; i < xstride; i += NTHR) dst[i] = _Float16(0);
}

// s_waitcnt vmcnt(N) alone (gfx9 encoding: vmcnt in bits 3:0 and 15:14; expcnt, bits 6:4, and lgkmcnt, bits 11:8, left at their
// maxima): returns once at most N of this wave's vector-memory requests are outstanding; loads retire in issue order.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 16, "one field");
    __builtin_amdgcn_s_waitcnt(0x0F70 | N);
}

// Tile register sets of pbl_gemv_kernel's sign phase: 3 = a static ring, a tile is requested two panels before its use; 2 = two
// registers rotated, one panel.  The ring costs the kernel 12 VGPRs (56 -> 68: off the 64 step), so only the instantiation it
// was measured on takes it: the one-token code-mode kernel of the grouped decode launch, fp16 activations, no prologue or
// epilogue.  Not the split kernels either: a wave strides WSTEP panels, the ring's first loop needs more than 4 WSTEP of them,
// and no layer has 17 (SPLIT = 4) or 33 (SPLIT = 8) panels.  Every other instantiation keeps the rotation and with it the
// machine code it had (profiles/r16_gemv_lookahead.md).
template <int MB, bool SF, int SPLIT, bool XB, int XP>
constexpr int gemv_tile_sets() {
    return MB == 1 && !SF && SPLIT == 1 && !XB && XP == 0 ? 3 : 2;
}

// SPLIT == 1: each of the WPB waves of a workgroup owns its own record (throughput mode, the
// L-layer stream).  SPLIT > 1 (== WPB): the waves of a workgroup COOPERATE on one record --
// wave w takes panels w, w+S, ... and salient rounds w, w+S, ... and the partial sums are
// merged through LDS -- so one small layer (256 records at N = 4096) still puts thousands of
// waves on the chip (latency mode, sequential decode).
// XB: bf16 activations converted in the staging phase, bf16 result (GemvArgs.x_bf16).  A template parameter, not a run-time branch:
// the fp16 instantiations -- the headline kernel among them -- are the code they were.  XP (x prologue, fp16 only): XP_RMSNORM stages
// LlamaRMSNorm(x) (pass 1: every token's sum of squares, one barrier, pass 2: the normalised row), XP_SWIGLU stages silu(gate) * up.
// XE_RESIDUAL (or-ed in) adds the residual in the store: fp16 result, then the fp16 add.
template <int MB, int WPB, bool SF, int SPLIT, bool XB = false, int XP = XP_NONE>
__global__ __launch_bounds__(WPB * PBL_WAVE, 1) void pbl_gemv_kernel(GemvArgs args) {
    static_assert(SPLIT == 1 || SPLIT == WPB, "split mode uses every wave of the workgroup on one record");
    static_assert(!(XB && XP != XP_NONE), "the x prologues and the residual epilogue take fp16 activations");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ uint32_t s_amax[XB ? MB * WPB : 1];           // XB: per (token, wave) the largest |x| bit pattern
    __shared__ float s_tscale[XB ? MB : 1];                  //     per token the power of two (or +inf) the result is multiplied with
    __shared__ float s_ssq[(XP & 3) == XP_RMSNORM ? MB * WPB : 1]; // XP_RMSNORM: per (token, wave) the partial sum of squares
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    pbl_layer L;
    const _Float16* xg;
    void* yg;
    if (args.grouped && args.n_inl) {
        L = args.inl[blockIdx.y];
        xg = args.x_shared;
        yg = static_cast<char*>(args.y_shared) + args.inl_off[blockIdx.y] * (args.y_f32 ? 4 : 2);
    } else if (args.grouped) {
        L = args.layers[blockIdx.y];
        xg = args.x_shared ? args.x_shared : static_cast<const _Float16*>(args.xs[blockIdx.y]);
        yg = args.y_shared ? static_cast<char*>(args.y_shared) + args.y_off[blockIdx.y] * (args.y_f32 ? 4 : 2) : args.ys[blockIdx.y];
    } else {
        L = args.layer; xg = args.x; yg = args.y;
    }
    const size_t ldy = args.ldy ? size_t(args.ldy) : size_t(L.N);
    // XCD-aware record mapping (speed only, never correctness): the dispatcher places
    // workgroup b on XCD b % 8, so give each XCD a CONTIGUOUS range of a layer's records and
    // the 128-byte lines shared by neighbouring records stay within one L2.  Measured neutral
    // (FETCH_SIZE 1416.8 -> 1414.0 MB per 224-layer launch): there is no inter-record reuse.
    const uint32_t nwg = SPLIT > 1 ? L.NRB : (L.NRB + WPB - 1) / WPB;
    if (blockIdx.x >= nwg) return;  // whole workgroup exits together (grouped launches over-provision)
    const uint32_t xq = nwg >> 3, xr_ = nwg & 7, xcd = blockIdx.x & 7, xi = blockIdx.x >> 3;
    const uint32_t wg = (xcd < xr_ ? xcd * (xq + 1) : xr_ * (xq + 1) + (xcd - xr_) * xq) + xi;
    const uint32_t rb0 = SPLIT > 1 ? wg : wg * WPB;
    // fused push: the call number lives in this rank's buffer (last finished call + 1; the reduce kernel of the previous call has
    // published it: same stream); its parity picks the slot set
    int push_set = 0;
    if (args.push_world) {
        uint32_t q = __hip_atomic_load(pblp2p::ctl_ptr(args.push_peer[args.push_rank]) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
        q = q ? q : 1u;
        push_set = int(__builtin_amdgcn_readfirstlane(q) & 1u);
    }
    const int wslot = SPLIT > 1 ? wave : 0;      // this wave's first panel / salient round
    constexpr int WSTEP = SPLIT;                 // ... and its stride

    const int K = int(L.K), P = int(L.P);
    const int Kp = P * PBL_PANEL_COLS;
    const int xstride = Kp + 8;            // halves per token in LDS; [K, Kp+8) is zero
    _Float16* xs = reinterpret_cast<_Float16*>(smem);
    float2* part_all = reinterpret_cast<float2*>(smem + ((size_t(MB) * xstride * 2 + 15) & ~size_t(15)));

    // ---- record lookup + first loads, issued BEFORE x is staged so that HBM latency of
    //      the weight stream overlaps the L2->LDS copy of x and the barrier ----------------
    const uint32_t rb = SPLIT > 1 ? rb0 : rb0 + wave;
    const bool active = rb < L.NRB;
    const uint8_t* blob = static_cast<const uint8_t*>(L.blob);
    const uint4 info = reinterpret_cast<const uint4*>(blob + sizeof(pbl_blob_header))[active ? rb : rb0];
    const uint8_t* rec = blob + size_t(__builtin_amdgcn_readfirstlane(info.x)) * 16;
    const int nfull = __builtin_amdgcn_readfirstlane(info.y);
    const int ntail = __builtin_amdgcn_readfirstlane(info.z);
    const int nexc = __builtin_amdgcn_readfirstlane(info.w);
    const int nch = nfull + ntail;
    const uint32_t tiles_off = PBL_TILES_OFF(L.G);
    const uint32_t off_sal = tiles_off + uint32_t(P) * 1024u;
    const uint32_t nchu = uint32_t(nch);

    constexpr int D = gemv_tile_sets<MB, SF, SPLIT, XB, XP>();
    const u32x4* tiles = reinterpret_cast<const u32x4*>(rec + tiles_off) + lane;
    const uint8_t* sal = rec + off_sal;
    const uint16_t* col0p = reinterpret_cast<const uint16_t*>(sal);
    const u32x4* deltap = reinterpret_cast<const u32x4*>(sal + PBL_SAL_DELTA_OFF(nchu));
    const u32x4* codep = reinterpret_cast<const u32x4*>(sal + PBL_SAL_CODE_OFF(nchu));
    const uint8_t* tailcnt = sal + PBL_SAL_TAILCNT_OFF(nchu);

    // The tile registers of phase 1, of which the first two are requested here, and this wave's first salient round.  The weight
    // stream is read once: every load of it is non-temporal.  D = 2: two registers, rotated (t0 <- t1 <- the panel two steps on).
    // D = 3: a ring of three sets, panel number n of this wave computes from set n % 3; a tile load takes a wave-uniform base (the
    // panel's 1 KiB, an SGPR pair) and ONE 32-bit lane offset, as the salient loads do.  (Two declarations, of which an
    // instantiation uses one -- t0 / t1 at D = 2, t[] at D = 3 -- and the other is dead and allocates nothing: as elements of t[]
    // hipcc splits the rotated registers into words and waits for the second tile here, in front of phase 0.)
    u32x4 t0 = {0, 0, 0, 0}, t1 = {0, 0, 0, 0};
    u32x4 t[3];
    t[0] = u32x4{0, 0, 0, 0}; t[1] = u32x4{0, 0, 0, 0};
    uint32_t lane16 = uint32_t(lane) * 16u;
    const uint8_t* tile0 = rec + tiles_off;     // (a local of its own: with rec + tiles_off inside the lambda every load goes flat)
    auto tile_fetch = [&](int p) {
        // both offsets opaque per request: else hipcc hoists the lane's address out of the loop as a 64-bit VGPR base, or folds the
        // panel's offset into an immediate that overflows at the fourth KiB and falls back to a 64-bit VGPR address
        size_t off = size_t(uint32_t(p)) * 1024u;
        asm volatile("" : "+s"(off), "+v"(lane16));
        return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(tile0 + off + size_t(lane16)));
    };
    // One salient round's loads: chunk min(c, nch - 1) of the three streams.  The bases are wave-uniform and the chunk index is
    // unsigned, so each load takes an SGPR base and ONE 32-bit lane offset (no 64-bit address arithmetic per round).
    auto sal_fetch = [&](int c, uint32_t& c0, u32x4& d4, u32x4& q4) {
        const uint32_t cn = uint32_t(c < nch ? c : nch - 1);
        c0 = *reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(col0p) + size_t(cn * 2u));
        d4 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(reinterpret_cast<const uint8_t*>(deltap) + size_t(cn * 16u)));
        q4 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(reinterpret_cast<const uint8_t*>(codep) + size_t(cn * 16u)));
    };
    uint32_t s_c0 = 0;
    u32x4 s_d4 = {0, 0, 0, 0}, s_q4 = {0, 0, 0, 0};
    if (active) {
        if constexpr (D == 2) {
            if (wslot < P) t0 = __builtin_nontemporal_load(tiles + wslot * 64);
            if (wslot + WSTEP < P) t1 = __builtin_nontemporal_load(tiles + (wslot + WSTEP) * 64);
        } else {
            if (wslot < P) t[0] = tile_fetch(wslot);
            if (wslot + WSTEP < P) t[1] = tile_fetch(wslot + WSTEP);
        }
        if (nch > wslot * PBL_WAVE) sal_fetch(wslot * PBL_WAVE + lane, s_c0, s_d4, s_q4);
    }

    // ---- phase 0: stage x ---------------------------------------------------------
    if constexpr (XB) {
        // bf16 x: pass 1 finds every token's largest magnitude (bf16 << 16 is the fp32 pattern; |x| patterns order like unsigned
        // integers, inf / NaN on top), one barrier, pass 2 re-reads the row (L1 / L2) and writes the scaled fp16 copy
        const int nthr = WPB * PBL_WAVE;
        const uint16_t* xb = reinterpret_cast<const uint16_t*>(xg);
        const bool vec = (K & 7) == 0 && (reinterpret_cast<uintptr_t>(xb) & 15) == 0;
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            uint32_t mx = 0;
            if (vec) {
                const u32x4* src = reinterpret_cast<const u32x4*>(xb + size_t(m) * K);
                for (int i = tid; i < (K >> 3); i += nthr) {
                    const u32x4 v = src[i];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t lo = (v[j] << 16) & 0x7FFFFFFFu, hi = v[j] & 0x7FFF0000u;
                        mx = lo > mx ? lo : mx;
                        mx = hi > mx ? hi : mx;
                    }
                }
            } else {
                for (int i = tid; i < K; i += nthr) {
                    const uint32_t a_ = (uint32_t(xb[size_t(m) * K + i]) << 16) & 0x7FFFFFFFu;
                    mx = a_ > mx ? a_ : mx;
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const uint32_t o = uint32_t(__shfl_xor(int(mx), off, PBL_WAVE));
                mx = o > mx ? o : mx;
            }
            if (lane == 0) s_amax[m * WPB + wave] = mx;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            uint32_t mx = 0;
#pragma unroll
            for (int w = 0; w < WPB; ++w) mx = s_amax[m * WPB + w] > mx ? s_amax[m * WPB + w] : mx;
            const bool finite = mx < 0x7F800000u;
            const int eb = int(mx >> 23) - 127 - 14;                     // 2^-e, e = max(0, exponent(amax) - 14): amax / 2^e < 2^15
            const int e = eb > 0 ? eb : 0;
            const float down = __builtin_bit_cast(float, uint32_t(127 - e) << 23);
            if (tid == 0) s_tscale[m] = finite ? __builtin_bit_cast(float, uint32_t(127 + e) << 23) : __builtin_inff();
            stage_row<nthr>(xs + m * xstride, xb + size_t(m) * K, xb + size_t(m) * K, K, xstride, vec, tid,
                            [&](uint32_t v, uint32_t) { return bf16_to_scaled_f16(v, finite, down); });
        }
    } else if constexpr ((XP & 3) == XP_RMSNORM) {
        // LlamaRMSNorm.forward on an fp16 row: pass 1 sums x^2 in fp32 (x^2 of an fp16 value is exact), one partial per (token, wave),
        // one barrier; pass 2 re-reads the row and the weight (L1 / L2) and writes fp16(g * fp16(x * r)), r = 1 / sqrt(mean + eps)
        // with an IEEE sqrt and divide.  mean = sum * (1 / K) as torch's mean kernel scales.  inf / NaN in a row: r = 0 or NaN, as HF.
        const int nthr = WPB * PBL_WAVE;
        const uint16_t* xb = reinterpret_cast<const uint16_t*>(xg);
        const uint16_t* gw = reinterpret_cast<const uint16_t*>(args.norm_w);
        const bool vec = (K & 7) == 0 && ((reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(gw)) & 15) == 0;
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            float ss = 0.f;
            if (vec) {
                const u32x4* src = reinterpret_cast<const u32x4*>(xb + size_t(m) * K);
                for (int i = tid; i < (K >> 3); i += nthr) {
                    const u32x4 v = src[i];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float lo = float(__builtin_bit_cast(_Float16, uint16_t(v[j] & 0xFFFFu)));
                        const float hi = float(__builtin_bit_cast(_Float16, uint16_t(v[j] >> 16)));
                        ss = fmaf(lo, lo, ss);
                        ss = fmaf(hi, hi, ss);
                    }
                }
            } else {
                for (int i = tid; i < K; i += nthr) {
                    const float f = float(xg[size_t(m) * K + i]);
                    ss = fmaf(f, f, ss);
                }
            }
            ss = wave_sum(ss);
            if (lane == 0) s_ssq[m * WPB + wave] = ss;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            float ss = 0.f;
#pragma unroll
            for (int w = 0; w < WPB; ++w) ss += s_ssq[m * WPB + w];
            const float r = 1.0f / sqrtf(ss * (1.0f / float(K)) + args.norm_eps);
            stage_row<nthr>(xs + m * xstride, xb + size_t(m) * K, gw, K, xstride, vec, tid,
                            [&](uint32_t v, uint32_t g) { return rmsnorm_f16(v, g, r); });
        }
    } else if constexpr ((XP & 3) == XP_SWIGLU) {
        // silu(gate) * up from the fused gate/up launch's output: row m holds gate at [0, K) and up at [up_off, up_off + K)
        const int nthr = WPB * PBL_WAVE;
        const uint16_t* xb = reinterpret_cast<const uint16_t*>(xg);
        const size_t ldx = args.ldx;
        const uint32_t uo = args.up_off;
        const bool vec = (K & 7) == 0 && (reinterpret_cast<uintptr_t>(xb) & 15) == 0 && (ldx & 7) == 0 && (uo & 7) == 0;
        for (int m = 0; m < MB; ++m)
            stage_row<nthr>(xs + m * xstride, xb + size_t(m) * ldx, xb + size_t(m) * ldx + uo, K, xstride, vec, tid, swiglu_f16);
    } else {
        const int nthr = WPB * PBL_WAVE;
        const uint16_t* xb = reinterpret_cast<const uint16_t*>(xg);
        const bool vec = (K & 7) == 0 && (reinterpret_cast<uintptr_t>(xb) & 15) == 0;
        for (int m = 0; m < MB; ++m)
            stage_row<nthr>(xs + m * xstride, xb + size_t(m) * K, xb + size_t(m) * K, K, xstride, vec, tid,
                            [](uint32_t v, uint32_t) { return v; });
    }
    __syncthreads();
    if (!active) return;  // no barriers below this point

    // ---- phase 1: sign plane ----------------------------------------------------------
    float acc[MB][16];
    float xl[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        xl[m] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    }
    // fp16x2 (1.0, 1.0) kept in a VGPR the compiler cannot constant-fold into a literal
    uint32_t c_one = 0x3C003C00u;
    asm volatile("" : "+v"(c_one));
    auto panel = [&](const u32x4& t, int p) {
        const uint32_t* xw = reinterpret_cast<const uint32_t*>(xs + p * PBL_PANEL_COLS) + lane;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t xr[MB];
#pragma unroll
            for (int m = 0; m < MB; ++m) xr[m] = xw[(m * xstride) / 2 + i * 64];
            word_step<MB>(t[i], c_one, xr, acc, xl);
        }
    };
    if constexpr (D == 2) {
        // The load for panel p + 2 is requested before panel p's arithmetic; the rotation below copies into the register of that
        // load, hipcc waits vmcnt(0) in front of the copy, and so the prefetch is one panel deep (1 KiB per wave in flight).
        for (int p = wslot; p < P; p += WSTEP) {
            u32x4 tn = t1;
            if (p + 2 * WSTEP < P) tn = __builtin_nontemporal_load(tiles + (p + 2 * WSTEP) * 64);
            panel(t0, p);
            t0 = t1;
            t1 = tn;
        }
    } else {
        // Three panels per trip over the ring's three sets (the inner loop is unrolled, so h is a constant and no tile register is
        // ever copied): the panel waits for its own set, requests the panel two steps on into the set its predecessor has just
        // released, and computes.  The wait is a counted one: the request for the next panel stays outstanding behind it, so a
        // tile has two panels of arithmetic to arrive in.  The ring holds the three sets the rotation above allocates anyway (its
        // t0, t1 and tn); the ring of profiles/r03_gemv_ring.md had no pin in unpack_pair, cost 74 VGPRs and two waves per SIMD.
        //
        // The counted wait needs requests that are NOT conditional: where a request sits under a test, hipcc's own wait insertion
        // has to assume that it may not have been issued, takes the set in use for the newest request and adds vmcnt(0) at its
        // first use, behind the new request.  So whole trips in which every request exists run first, with nothing under a test;
        // the last one to four panels run in the second loop, which drains the counter before each request and so looks one panel
        // ahead, as the rotation does.  (The loads requested before phase 0 have landed -- the staging loops waited for x,
        // requested behind them -- but they sit under tests; the drain in front of the loop takes them out of hipcc's books.  The
        // scheduling barrier keeps hipcc from sinking the request below the panel's arithmetic.)
        //
        // INVARIANT behind vmcnt(1): panel() issues no vector-memory operation (x comes from LDS), so the only requests of this
        // wave between two waits are the tile loads, one per panel.  A global load or store added to panel() would be the newest
        // request at the next wait, which then means "all tiles landed": still correct (hipcc adds its own waits for what it
        // loads), but the lookahead would silently be one panel again.
        wait_vmcnt<0>();
        int p0 = wslot;
        for (; p0 + 4 * WSTEP < P; p0 += 3 * WSTEP) {
#pragma unroll
            for (int h = 0; h < 3; ++h) {
                wait_vmcnt<1>();
                t[(h + 2) % 3] = tile_fetch(p0 + (h + 2) * WSTEP);
                __builtin_amdgcn_sched_barrier(0);
                panel(t[h], p0 + h * WSTEP);
            }
        }
        for (; p0 < P; p0 += 3 * WSTEP) {
#pragma unroll
            for (int h = 0; h < 3; ++h) {
                const int p = p0 + h * WSTEP;
                if (h && p >= P) break;
                wait_vmcnt<0>();
                if (p + 2 * WSTEP < P) t[(h + 2) % 3] = tile_fetch(p + 2 * WSTEP);
                __builtin_amdgcn_sched_barrier(0);
                panel(t[h], p);
            }
        }
    }

    // row-owner lanes: lane l owns row rho(l) (4 lanes per row).  Their row parameters are requested here, in front of the
    // reduction: phase 3 must not wait on HBM, and the first salient round -- which waits for its own loads in issue order --
    // finds these already landed instead of exposing their latency.
    const int rho = ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
    const int sub = lane & 3;
    const pbl_rowparams pr = reinterpret_cast<const pbl_rowparams*>(rec + PBL_REC_PARAMS_OFF)[rho];
    const pbl_rowinfo ri = reinterpret_cast<const pbl_rowinfo*>(rec + PBL_REC_ROWINFO_OFF)[rho];

    // reduce the 16 row accumulators now: from here on one register per token carries the
    // binary result (lane l holds row rho(l), see transpose_reduce16)
    float accsum[MB], X[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        X[m] = wave_sum(xl[m]);
        accsum[m] = transpose_reduce16(acc[m], lane);
    }

    // SF layers in a mixed grouped launch are told apart at run time (wave-uniform)
    const bool sf = SF && (L.flags & PBL_FLAG_SAL_F16);
    const uint8_t* crow = sal + PBL_SAL_CROW_OFF(nchu, uint32_t(ntail));
    const bool has_crow = L.flags & (PBL_FLAG_HAS_GROUPS | PBL_FLAG_SAL_F16);

    // ---- phase 2: salient chunks (next round's loads issued before this round's math) ---
    float2* part = part_all + (SPLIT > 1 ? size_t(0) : size_t(wave) * L.max_nch * MB);
    {
        const uint32_t xbase = uint32_t(reinterpret_cast<uintptr_t>(xs));      // LDS byte offset of x
        const uint32_t tok_stride = uint32_t(xstride) * 2u;
        const uint32_t zaddr = xbase + 2u * uint32_t(Kp);                      // a zero slot
        constexpr int RSTEP = WSTEP * PBL_WAVE;
        // Two rounds per trip over two register sets (the inner loop is unrolled, so h is a constant): round h computes from set
        // h while the next round's loads land in the other set -- set 0 is (s_c0, s_d4, s_q4), loaded before phase 0 and by
        // every odd round; set 1 lives inside one trip.  No register is copied between rounds.  (The round is written out in place: inside a lambda hipcc no longer proves
        // the blob's pointers global, and every load of the kernel becomes a flat load.)
        for (int base0 = wslot * PBL_WAVE; base0 < nch; base0 += 2 * RSTEP) {
            uint32_t rc0[2];
            u32x4 rd4[2], rq4[2];
            rc0[0] = s_c0; rd4[0] = s_d4; rq4[0] = s_q4;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int base = base0 + h * RSTEP;
                if (h && base >= nch) break;
                // every round first waits for its own set, explicitly, and only then requests the next one.  Left to hipcc, the wait
                // lands at the set's first use BEHIND the new requests -- vmcnt counts in issue order, so it would wait for those
                // too and the prefetch would hide nothing (measured: a 4-token launch, one wave per SIMD, 12 % slower).
                __builtin_amdgcn_s_waitcnt(0x0F70);                     // s_waitcnt vmcnt(0) alone
                if (base + RSTEP < nch) {
                    if (h) sal_fetch(base + RSTEP + lane, s_c0, s_d4, s_q4);
                    else sal_fetch(base + RSTEP + lane, rc0[1], rd4[1], rq4[1]);
                }
                const int c = base + lane;
                const bool full = base + PBL_WAVE <= nfull;             // wave-uniform: 64 full chunks, every lane valid
                const bool valid = full || c < nch;
                const int cc = valid ? c : nch - 1;
                float Q[MB], S[MB];
#pragma unroll
                for (int m = 0; m < MB; ++m) { Q[m] = 0.f; S[m] = 0.f; }
                int cnt = 16;
                if (!full) {
                    if (cc >= nfull) cnt = tailcnt[cc - nfull];
                    if (!valid) cnt = 0;
                }
                if (SF && sf) {
                    // this chunk's row -> its (scale, zero) from the row-owner lane (no memory round trip)
                    const int crw = crow[cc];
                    const int owner = ((crw & 8) << 2) | ((crw & 4) << 2) | ((crw & 2) << 2) | ((crw & 1) << 2);
                    const float ss = __shfl(pr.sscale, owner, PBL_WAVE), sz = __shfl(pr.szero, owner, PBL_WAVE);
                    if (full)
                        chunk_accumulate<MB, false, true>(xbase, tok_stride, rc0[h], rd4[h], rq4[h], 16, zaddr, c_one, ss, sz, Q, S);
                    else
                        chunk_accumulate<MB, true, true>(xbase, tok_stride, rc0[h], rd4[h], rq4[h], cnt, zaddr, c_one, ss, sz, Q, S);
                } else if (full) {
                    chunk_accumulate<MB, false, false>(xbase, tok_stride, rc0[h], rd4[h], rq4[h], 16, zaddr, c_one, 0.f, 0.f, Q, S);
                } else {
                    chunk_accumulate<MB, true, false>(xbase, tok_stride, rc0[h], rd4[h], rq4[h], cnt, zaddr, c_one, 0.f, 0.f, Q, S);
                }
                if (valid) {
#pragma unroll
                    for (int m = 0; m < MB; ++m)   // code mode: undo the 1024 code bias here, once per chunk
                        part[size_t(m) * L.max_nch + c] = make_float2((SF && sf) ? Q[m] : fmaf(-1024.f, S[m], Q[m]), S[m]);
                }
            }
        }
    }
    if constexpr (SPLIT > 1) {
        // merge the S waves' binary partials (lane l of every wave holds row rho(l)); the chunk
        // partials already sit in the shared `part` array
        float2* red = part_all + size_t(L.max_nch) * MB;
#pragma unroll
        for (int m = 0; m < MB; ++m) red[(m * SPLIT + wave) * PBL_WAVE + lane] = make_float2(accsum[m], X[m]);
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            float a_ = 0.f, x_ = 0.f;
#pragma unroll
            for (int w = 0; w < SPLIT; ++w) {
                const float2 v = red[(m * SPLIT + w) * PBL_WAVE + lane];
                a_ += v.x; x_ += v.y;
            }
            accsum[m] = a_; X[m] = x_;
        }
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }

    // ---- phase 3: reduce, combine, store -------------------------------------------
    float A, B;
    class_consts(rho & 7, A, B);
    const float alpha = 0.5f * (pr.hi - pr.lo), mu = 0.5f * (pr.hi + pr.lo);
    const uint32_t row = rb * 16 + rho;
    // exceptions are read as ONE aligned 64-bit word each: a scalar load of the fp32
    // field off a 2-byte-aligned base silently drops the low address bits on gfx950
    const uint2* exc = reinterpret_cast<const uint2*>(sal + PBL_SAL_EXC_OFF(nchu, uint32_t(ntail), has_crow));

#pragma unroll
    for (int m = 0; m < MB; ++m) {
        float Q = 0.f, S = 0.f;
        const float2* pm = part + size_t(m) * L.max_nch;
        for (int k = sub; k < int(ri.nfull); k += 4) {
            const float2 v = pm[ri.start + k];
            Q += v.x; S += v.y;
        }
        for (int k = sub; k < int(ri.ntail); k += 4) {
            const float2 v = pm[nfull + ri.tailidx + k];
            Q += v.x; S += v.y;
        }
        Q = quad_sum(Q); S = quad_sum(S);
        float e = 0.f;
        for (int k = 0; k < nexc; ++k) {
            const uint2 ex = exc[k];  // {col | row << 16, value}
            if (int(ex.x >> 16) == rho)
                e += (__builtin_bit_cast(float, ex.y) - pr.hi) * float(xs[m * xstride + (ex.x & 0xFFFFu)]);
        }
        // explicit fma chain: every template instantiation rounds identically (M=4 == 4 x M=1)
        const float D = fmaf(A, accsum[m], -(B * X[m]));
        const float sal = (SF && sf) ? fmaf(-pr.hi, S, Q) : fmaf(pr.sscale, fmaf(-pr.szero, S, Q), -(pr.hi * S));
        float yv = fmaf(alpha, D, fmaf(mu, X[m], sal)) + e;
        if constexpr (XB) {                                      // back to the token's own scale, then the bias: pbl_act_finish's fma
            const float bv = (L.bias && row < L.N) ? L.bias[row] : 0.f;
            yv = fmaf(yv, s_tscale[m], bv);
        } else if (L.bias && row < L.N) yv += L.bias[row];
        if (sub == 0 && row < L.N) {
            if (args.push_world) {
                for (int p = 0; p < args.push_world; ++p)       // 7 xGMI stores + 1 local, 4 bytes each from 16 lanes (64-byte runs)
                    pblp2p::slot_ptr(args.push_peer[p], push_set, args.push_rank, args.push_world, args.push_cap)[size_t(m) * ldy + row] = yv;
            } else if (args.y_f32) static_cast<float*>(yg)[size_t(m) * ldy + row] = yv;
            else if constexpr (XB) static_cast<uint16_t*>(yg)[size_t(m) * ldy + row] = uint16_t(bf16_bits_rne(yv));
            else if constexpr ((XP & XE_RESIDUAL) != 0) {
                // two roundings, as HF: the linear's fp16 output, then the fp16 add (fp32 opmath); +-inf / NaN propagate
                const _Float16 lin = _Float16(yv);
                static_cast<_Float16*>(yg)[size_t(m) * ldy + row] = _Float16(float(lin) + float(args.residual[size_t(m) * args.ldr + row]));
            } else static_cast<_Float16*>(yg)[size_t(m) * ldy + row] = _Float16(yv);
        }
    }
    if (args.push_world) {
        // this record's rows are visible system wide, THEN it counts itself at every rank (program order of one wave: the
        // fence drains the stores above before the atomics below are issued)
        __threadfence_system();
        if (lane == 0)
            for (int p = 0; p < args.push_world; ++p)
                __hip_atomic_fetch_add(pblp2p::count_ptr(args.push_peer[p], push_set, args.push_rank), 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

size_t lds_bytes(uint32_t P, uint32_t max_nch, int mb, int wpb, int split = 1) {
    const size_t xstride = size_t(P) * PBL_PANEL_COLS + 8;
    size_t s = (size_t(mb) * xstride * 2 + 15) & ~size_t(15);
    if (split > 1) s += (size_t(max_nch) + size_t(split) * PBL_WAVE) * mb * sizeof(float2);
    else s += size_t(wpb) * max_nch * mb * sizeof(float2);
    return s + 16;
}

template <int MB, int WPB, bool SF, int SPLIT = 1, int XP = XP_NONE>
int launch(const GemvArgs& a, dim3 grid, size_t lds, hipStream_t st) {
    void (*k)(GemvArgs);
    if constexpr (XP != XP_NONE) k = pbl_gemv_kernel<MB, WPB, SF, SPLIT, false, XP>;     // (prologues / epilogue: fp16 only)
    else k = a.x_bf16 ? pbl_gemv_kernel<MB, WPB, SF, SPLIT, true> : pbl_gemv_kernel<MB, WPB, SF, SPLIT, false>;
    // the bf16 instantiation holds s_amax / s_tscale in STATIC LDS on top of the dynamic size (4 MB (WPB + 1) bytes, rounded up):
    // both limits are on the sum (a layer just under a limit failed the launch instead of answering UNSUPPORTED, which
    // pbl_linear_bf16's callers turn into the three-launch form); the RMSNorm prologue holds s_ssq (4 MB WPB bytes) the same way
    const size_t stat = a.x_bf16 ? ((size_t(4) * MB * (WPB + 1) + 15) & ~size_t(15)) + 16
                      : (XP & 3) == XP_RMSNORM ? ((size_t(4) * MB * WPB + 15) & ~size_t(15)) + 16 : 16;
    const bool declines = a.x_bf16 || XP != XP_NONE;             // callers that have an unfused form to fall back to
    if (lds + stat > 64 * 1024) {
        if (lds + stat > 160 * 1024) return PBL_ERR_UNSUPPORTED;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                int(lds)) != hipSuccess)
            return declines ? PBL_ERR_UNSUPPORTED : PBL_ERR_LAUNCH;
    }
    GemvArgs args = a;
    void* argv[] = {&args};
    return hipLaunchKernel(reinterpret_cast<const void*>(k), grid, dim3(WPB * PBL_WAVE), argv, lds, st) == hipSuccess
               ? PBL_OK : PBL_ERR_LAUNCH;
}


// ---------------------------------------------------------------------------------------
// Column-group variant (G > 1: per-(row, group) hi/lo, gptq_pb --groupsize 128).  Same
// record format and bit classes; the 16 accumulators are flushed into per-row totals at
// every group boundary with per-(row,group) coefficients  ca = alpha*A_c,  cb = mu - alpha*B_c
// kept in LDS, and the salient correction looks hi up per entry.  A correctness-first
// kernel for the non-default configuration; the G == 1 kernel above is the tuned one.
template <int MB, int WPB>
__global__ __launch_bounds__(WPB * PBL_WAVE) void pbl_gemv_groups_kernel(GemvArgs args, int gshift) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    pbl_layer L;
    const _Float16* xg;
    void* yg;
    if (args.grouped && args.n_inl) {
        L = args.inl[blockIdx.y];
        xg = args.x_shared;
        yg = static_cast<char*>(args.y_shared) + args.inl_off[blockIdx.y] * (args.y_f32 ? 4 : 2);
    } else if (args.grouped) {
        L = args.layers[blockIdx.y];
        xg = args.x_shared ? args.x_shared : static_cast<const _Float16*>(args.xs[blockIdx.y]);
        yg = args.y_shared ? static_cast<char*>(args.y_shared) + args.y_off[blockIdx.y] * (args.y_f32 ? 4 : 2) : args.ys[blockIdx.y];
    } else {
        L = args.layer; xg = args.x; yg = args.y;
    }
    const size_t ldy = args.ldy ? size_t(args.ldy) : size_t(L.N);
    xg += size_t(args.tok0) * L.K;
    yg = static_cast<char*>(yg) + size_t(args.tok0) * ldy * (args.y_f32 ? 4 : 2);
    const uint32_t rb0 = blockIdx.x * WPB;
    if (rb0 >= L.NRB) return;
    const int K = int(L.K), P = int(L.P), G = int(L.G);
    const int Kp = P * PBL_PANEL_COLS, xstride = Kp + 8;
    const int gw = (K / G) / 128;  // dwords of a lane per column group
    if (gshift < 0) gshift = G > 1 ? 31 - __builtin_clz(uint32_t(K / G)) : 31;   // grouped launch: every layer has its own group size (G == 1: one group)
    _Float16* xs = reinterpret_cast<_Float16*>(smem);
    char* after_x = smem + ((size_t(MB) * xstride * 2 + 15) & ~size_t(15));
    float2* cacb = reinterpret_cast<float2*>(after_x) + size_t(wave) * G * 16;          // [g][rho]
    float* hitab = reinterpret_cast<float*>(after_x + size_t(WPB) * G * 16 * 8) + size_t(wave) * G * 16;
    char* after_tab = after_x + size_t(WPB) * G * 16 * 12;
    float2* part = reinterpret_cast<float2*>(after_tab) + size_t(wave) * L.max_nch * MB;
    float* partH = reinterpret_cast<float*>(after_tab + size_t(WPB) * L.max_nch * MB * 8) + size_t(wave) * L.max_nch * MB;

    const uint32_t rb = rb0 + wave;
    const bool active = rb < L.NRB;
    const uint8_t* blob = static_cast<const uint8_t*>(L.blob);
    const uint4 info = reinterpret_cast<const uint4*>(blob + sizeof(pbl_blob_header))[active ? rb : rb0];
    const uint8_t* rec = blob + size_t(__builtin_amdgcn_readfirstlane(info.x)) * 16;
    const int nfull = __builtin_amdgcn_readfirstlane(info.y);
    const int ntail = __builtin_amdgcn_readfirstlane(info.z);
    const int nexc = __builtin_amdgcn_readfirstlane(info.w);
    const int nch = nfull + ntail;
    const uint32_t tiles_off = PBL_TILES_OFF(uint32_t(G));
    const uint32_t off_sal = tiles_off + uint32_t(P) * 1024u;

    {   // stage x, build this wave's coefficient tables
        const int nthr = WPB * PBL_WAVE;
        for (int m = 0; m < MB; ++m) {
            for (int i = tid; i < K; i += nthr) xs[m * xstride + i] = xg[size_t(m) * K + i];
            for (int i = K + tid; i < xstride; i += nthr) xs[m * xstride + i] = _Float16(0);
        }
        if (active) {
            const float2* ghl = reinterpret_cast<const float2*>(rec + PBL_REC_GHL_OFF);
            const pbl_rowparams* rp = reinterpret_cast<const pbl_rowparams*>(rec + PBL_REC_PARAMS_OFF);
            for (int idx = lane; idx < 16 * G; idx += PBL_WAVE) {
                const int rho = idx & 15, g = idx >> 4;
                // a group-free layer riding along in a grouped launch has no ghl table: its one "group" is the row's own levels
                const float2 hl = G > 1 ? ghl[rho * G + g] : make_float2(rp[rho].hi, rp[rho].lo);
                float A, B;
                class_consts(rho & 7, A, B);
                const float al = 0.5f * (hl.x - hl.y), mu = 0.5f * (hl.x + hl.y);
                cacb[idx] = make_float2(al * A, fmaf(-al, B, mu));
                hitab[idx] = hl.x;
            }
        }
    }
    __syncthreads();
    if (!active) return;

    float acc[MB][16], tot[MB][16], xl[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        xl[m] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[m][r] = 0.f; tot[m][r] = 0.f; }
    }
    uint32_t c_one = 0x3C003C00u;
    asm volatile("" : "+v"(c_one));
    const u32x4* tiles = reinterpret_cast<const u32x4*>(rec + tiles_off) + lane;
    int wi = 0, g = 0;
    for (int p = 0; p < P; ++p) {
        const u32x4 t = __builtin_nontemporal_load(tiles + p * 64);
        const uint32_t* xw = reinterpret_cast<const uint32_t*>(xs + p * PBL_PANEL_COLS) + lane;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t xr[MB];
#pragma unroll
            for (int m = 0; m < MB; ++m) xr[m] = xw[(m * xstride) / 2 + i * 64];
            word_step<MB>(t[i], c_one, xr, acc, xl);
            if (++wi == gw) {
                if (g < G) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float2 c = cacb[g * 16 + r];
#pragma unroll
                        for (int m = 0; m < MB; ++m)
                            tot[m][r] = fmaf(c.y, xl[m], fmaf(c.x, acc[m][r], tot[m][r]));
                    }
                }
#pragma unroll
                for (int m = 0; m < MB; ++m) {
                    xl[m] = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
                }
                wi = 0;
                ++g;
            }
        }
    }
    float T[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) T[m] = transpose_reduce16(tot[m], lane);

    // salient chunks: per entry  q*x, x and hi[row][group(col)]*x
    const uint8_t* sal = rec + off_sal;
    const uint32_t nchu = uint32_t(nch);
    const uint16_t* col0p = reinterpret_cast<const uint16_t*>(sal);
    const u32x4* deltap = reinterpret_cast<const u32x4*>(sal + PBL_SAL_DELTA_OFF(nchu));
    const u32x4* codep = reinterpret_cast<const u32x4*>(sal + PBL_SAL_CODE_OFF(nchu));
    const uint8_t* tailcnt = sal + PBL_SAL_TAILCNT_OFF(nchu);
    const uint8_t* crow = sal + PBL_SAL_CROW_OFF(nchu, uint32_t(ntail));
    const bool has_crow = (L.flags & (PBL_FLAG_HAS_GROUPS | PBL_FLAG_SAL_F16)) != 0;
    const pbl_rowinfo* rinfo = reinterpret_cast<const pbl_rowinfo*>(rec + PBL_REC_ROWINFO_OFF);
    for (int base = 0; base < nch; base += PBL_WAVE) {
        const int c = base + lane;
        if (c < nch) {
            const u32x4 d4 = deltap[c], q4 = codep[c];
            const int cnt = c >= nfull ? int(tailcnt[c - nfull]) : 16;
            int row = 0;
            if (has_crow) row = crow[c];
            else {            // (group-free member without per-chunk row ids: the row whose chunk range holds c)
                for (int r = 0; r < 16; ++r) {
                    const pbl_rowinfo q = rinfo[r];
                    const bool in = c < nfull ? (c >= int(q.start) && c < int(q.start) + int(q.nfull))
                                              : (c - nfull >= int(q.tailidx) && c - nfull < int(q.tailidx) + int(q.ntail));
                    row = in ? r : row;
                }
            }
            const pbl_rowparams cp = reinterpret_cast<const pbl_rowparams*>(rec + PBL_REC_PARAMS_OFF)[row];
            const bool sf16 = L.flags & PBL_FLAG_SAL_F16;
            uint32_t col2 = 2u * col0p[c];
            float Q[MB], S[MB], H[MB];
#pragma unroll
            for (int m = 0; m < MB; ++m) { Q[m] = 0.f; S[m] = 0.f; H[m] = 0.f; }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                col2 += (d4[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                if (k < cnt) {
                    const uint32_t col = col2 >> 1;
                    float qf = cp.sscale * (float((q4[k >> 2] >> (8 * (k & 3))) & 0xFFu) - cp.szero);  // the weight itself
                    if (sf16) qf = float(round_f16_twice(qf));
                    const float hv = hitab[(col >> gshift) * 16 + row];
#pragma unroll
                    for (int m = 0; m < MB; ++m) {
                        const float xv = float(xs[m * xstride + col]);
                        Q[m] = fmaf(qf, xv, Q[m]);
                        S[m] += xv;
                        H[m] = fmaf(hv, xv, H[m]);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                part[size_t(m) * L.max_nch + c] = make_float2(Q[m], S[m]);
                partH[size_t(m) * L.max_nch + c] = H[m];
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    const int rho = ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
    const int sub = lane & 3;
    const pbl_rowinfo ri = reinterpret_cast<const pbl_rowinfo*>(rec + PBL_REC_ROWINFO_OFF)[rho];
    const uint32_t row = rb * 16 + rho;
    const uint2* exc = reinterpret_cast<const uint2*>(sal + (has_crow ? PBL_SAL_EXC_OFF(nchu, uint32_t(ntail), true)
                                                                       : PBL_SAL_EXC_OFF(nchu, uint32_t(ntail), false)));
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        float Q = 0.f, S = 0.f, H = 0.f;
        const float2* pm = part + size_t(m) * L.max_nch;
        const float* ph = partH + size_t(m) * L.max_nch;
        for (int k = sub; k < int(ri.nfull); k += 4) {
            const float2 v = pm[ri.start + k];
            Q += v.x; S += v.y; H += ph[ri.start + k];
        }
        for (int k = sub; k < int(ri.ntail); k += 4) {
            const float2 v = pm[nfull + ri.tailidx + k];
            Q += v.x; S += v.y; H += ph[nfull + ri.tailidx + k];
        }
        Q = quad_sum(Q); S = quad_sum(S); H = quad_sum(H);
        float e = 0.f;
        for (int k = 0; k < nexc; ++k) {
            const uint2 ex = exc[k];
            if (int(ex.x >> 16) == rho) {
                const uint32_t col = ex.x & 0xFFFFu;
                e += (__builtin_bit_cast(float, ex.y) - hitab[(col >> gshift) * 16 + rho]) * float(xs[m * xstride + col]);
            }
        }
        float yv = T[m] + (Q - H) + e;
        if (L.bias && row < L.N) yv += L.bias[row];
        if (sub == 0 && row < L.N) {
            if (args.y_f32) static_cast<float*>(yg)[size_t(m) * ldy + row] = yv;
            else static_cast<_Float16*>(yg)[size_t(m) * ldy + row] = _Float16(yv);
        }
    }
}


// ---------------------------------------------------------------------------------------
// Device-side unpack: PBL1 -> dense row-major [N,K] (fp16 or fp32); the GEMM-regime path
// (the dense matrix lives only in a transient workspace).
template <typename OutT>
__global__ __launch_bounds__(4 * PBL_WAVE) void pbl_unpack_kernel(pbl_layer L, OutT* __restrict__ Wout, int seg_panels) {
    // A workgroup owns 4 rows of a record (grid = 4 * NRB), one per wave; a wave builds its output row in LDS, in
    // column segments of seg_panels * 512 columns -- sign plane expanded, then the row's salient chunks
    // (column-sorted) and exceptions written over it -- and streams the finished segment out with contiguous
    // 16-byte stores.  No global scatter: every HBM line is written whole, once.
    extern __shared__ __attribute__((aligned(16))) char smem_u[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t rb = blockIdx.x >> 2;
    const int row0 = int(blockIdx.x & 3) * 4;
    const int K = int(L.K), P = int(L.P), G = int(L.G);
    const uint8_t* blob = static_cast<const uint8_t*>(L.blob);
    const uint4 info = reinterpret_cast<const uint4*>(blob + sizeof(pbl_blob_header))[rb];
    const uint8_t* rec = blob + size_t(__builtin_amdgcn_readfirstlane(info.x)) * 16;
    const int nfull = __builtin_amdgcn_readfirstlane(info.y), ntail = __builtin_amdgcn_readfirstlane(info.z);
    const int nexc = __builtin_amdgcn_readfirstlane(info.w), nch = nfull + ntail;
    const bool groups = L.flags & PBL_FLAG_HAS_GROUPS, sf16 = L.flags & PBL_FLAG_SAL_F16;
    const uint32_t tiles_off = PBL_TILES_OFF(uint32_t(G));
    const pbl_rowparams* params = reinterpret_cast<const pbl_rowparams*>(rec + PBL_REC_PARAMS_OFF);
    const pbl_rowinfo* rinfo = reinterpret_cast<const pbl_rowinfo*>(rec + PBL_REC_ROWINFO_OFF);
    const float2* ghl = reinterpret_cast<const float2*>(rec + PBL_REC_GHL_OFF);
    const int gwords = groups ? (K / G) / 128 : (1 << 30);   // dwords of a lane per column group
    const int nrows = (L.N - rb * 16) < 16u ? int(L.N - rb * 16) : 16;
    const u32x4* tiles = reinterpret_cast<const u32x4*>(rec + tiles_off) + lane;
    const uint8_t* sal = rec + tiles_off + uint32_t(P) * 1024u;
    const uint32_t nchu = uint32_t(nch);
    const uint16_t* col0p = reinterpret_cast<const uint16_t*>(sal);
    const u32x4* deltap = reinterpret_cast<const u32x4*>(sal + PBL_SAL_DELTA_OFF(nchu));
    const u32x4* codep = reinterpret_cast<const u32x4*>(sal + PBL_SAL_CODE_OFF(nchu));
    const uint8_t* tailcnt = sal + PBL_SAL_TAILCNT_OFF(nchu);
    const bool has_crow = L.flags & (PBL_FLAG_HAS_GROUPS | PBL_FLAG_SAL_F16);
    const uint2* exc = reinterpret_cast<const uint2*>(sal + PBL_SAL_EXC_OFF(nchu, uint32_t(ntail), has_crow));
    const int seg_cols = seg_panels * PBL_PANEL_COLS;
    OutT* rowbuf = reinterpret_cast<OutT*>(smem_u) + size_t(wave) * seg_cols;   // this wave's row segment under construction
    const bool vec_ok = (size_t(K) * sizeof(OutT)) % 16 == 0;                    // every row starts 16-byte aligned

    const int rho = row0 + wave;
    if (rho < nrows) {
        const int pos = rho < 8 ? rho + 8 : rho - 8;
        const pbl_rowparams pr = params[rho];
        const pbl_rowinfo ri = rinfo[rho];
        const int n_full = int(ri.nfull), n_all = n_full + int(ri.ntail);
        for (int p0 = 0; p0 < P; p0 += seg_panels) {
            const int p1 = p0 + seg_panels < P ? p0 + seg_panels : P;
            const uint32_t c_lo = uint32_t(p0) * PBL_PANEL_COLS, c_n = uint32_t(p1 - p0) * PBL_PANEL_COLS;
            // 1. sign plane of the row: lane l owns columns 512p + 128i + 2l + {0,1}
            for (int p = p0; p < p1; ++p) {
                const u32x4 t = tiles[p * 64];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float hi = pr.hi, lo = pr.lo;
                    if (groups) { const int g = (p * 4 + i) / gwords; const float2 hl = ghl[rho * G + (g < G ? g : G - 1)]; hi = hl.x; lo = hl.y; }
                    OutT* d = rowbuf + (p - p0) * PBL_PANEL_COLS + i * 128 + 2 * lane;
                    d[0] = OutT(((t[i] >> pos) & 1u) ? hi : lo);
                    d[1] = OutT(((t[i] >> (16 + pos)) & 1u) ? hi : lo);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // 2. the row's salient chunks (full chunks [start, start + nfull), then its tail chunks); entries outside
            //    the segment are skipped
            for (int j = lane; j < n_all; j += PBL_WAVE) {
                const int c = j < n_full ? int(ri.start) + j : nfull + int(ri.tailidx) + (j - n_full);
                const int cnt = c >= nfull ? int(tailcnt[c - nfull]) : 16;
                const u32x4 d4 = deltap[c], q4 = codep[c];
                uint32_t col = uint32_t(col0p[c]) - c_lo;                 // wraps for columns left of the segment
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    col += ((d4[e >> 2] >> (8 * (e & 3))) & 0xFFu) >> 1;
                    float w = pr.sscale * (float((q4[e >> 2] >> (8 * (e & 3))) & 0xFFu) - pr.szero);
                    if (sf16) w = float(round_f16_twice(w));
                    if (e < cnt && col < c_n) rowbuf[col] = OutT(w);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // 3. exceptions of the row (explicit values, written last)
            for (int k = lane; k < nexc; k += PBL_WAVE) {
                const uint2 ex = exc[k];
                const uint32_t col = (ex.x & 0xFFFFu) - c_lo;
                if (int(ex.x >> 16) == rho && col < c_n) rowbuf[col] = OutT(__builtin_bit_cast(float, ex.y));
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // 4. stream the segment out
            OutT* dst = Wout + size_t(rb * 16 + rho) * K + c_lo;
            const int ncol = int(c_lo + c_n) <= K ? int(c_n) : K - int(c_lo);
            if (vec_ok) {
                constexpr int V = 16 / sizeof(OutT);
                for (int j = lane * V; j < ncol; j += PBL_WAVE * V) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(rowbuf + j);
                    *reinterpret_cast<u32x4*>(dst + j) = v;
                }
            } else {
                for (int j = lane; j < ncol; j += PBL_WAVE) dst[j] = rowbuf[j];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

size_t lds_bytes_groups(uint32_t P, uint32_t G, uint32_t max_nch, int mb, int wpb) {
    const size_t xstride = size_t(P) * PBL_PANEL_COLS + 8;
    size_t s = (size_t(mb) * xstride * 2 + 15) & ~size_t(15);
    s += size_t(wpb) * G * 16 * 12;
    s += size_t(wpb) * max_nch * mb * 12;
    return s + 16;
}

template <int MB>
int launch_groups(const GemvArgs& a, int gshift, dim3 grid, size_t lds, hipStream_t st) {
    auto k = pbl_gemv_groups_kernel<MB, 1>;
    if (lds > 160 * 1024) return PBL_ERR_UNSUPPORTED;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)) != hipSuccess)
        return PBL_ERR_LAUNCH;
    GemvArgs args = a;
    void* argv[] = {&args, &gshift};
    return hipLaunchKernel(reinterpret_cast<const void*>(k), grid, dim3(PBL_WAVE), argv, lds, st) == hipSuccess
               ? PBL_OK : PBL_ERR_LAUNCH;
}

int linear_groups(const pbl_layer* layer, const void* x, void* y, int M, int y_f32, hipStream_t st) {
    const uint32_t gs = layer->K / layer->G;
    if (layer->K % layer->G || gs % 128 || (gs & (gs - 1))) return PBL_ERR_UNSUPPORTED;  // power-of-two groups
    int gshift = 0;
    while ((1u << gshift) < gs) ++gshift;
    const size_t esz = y_f32 ? 4 : 2;
    int mb_max = 2;   // two tokens per weight pass keeps the 2x16 accumulators in registers
    while (mb_max > 1 && lds_bytes_groups(layer->P, layer->G, layer->max_nch, mb_max, 1) > 96 * 1024) --mb_max;
    for (int m0 = 0; m0 < M; m0 += mb_max) {
        const int mb = M - m0 < mb_max ? M - m0 : mb_max;
        GemvArgs a{};
        a.layer = *layer;
        a.x = static_cast<const _Float16*>(x) + size_t(m0) * layer->K;
        a.y = static_cast<char*>(y) + size_t(m0) * layer->N * esz;
        a.M = mb; a.y_f32 = y_f32; a.grouped = 0;
        const dim3 grid(layer->NRB, 1, 1);
        const size_t lds = lds_bytes_groups(layer->P, layer->G, layer->max_nch, mb, 1);
        const int rc = mb == 1 ? launch_groups<1>(a, gshift, grid, lds, st) : launch_groups<2>(a, gshift, grid, lds, st);
        if (rc != PBL_OK) return rc;
    }
    return PBL_OK;
}

// Grouped / fused launch of layers that carry column groups (groupsize 128 / 256 / ...: gptq_pb/run_all.sh): the column-group
// kernel, one wave per record, grid (records, layers); every layer's group size must be a power of two (each layer decodes
// its own from K / G) and every K a multiple of 128.  Group-free layers may ride along (they are one group).
int grouped_groups(const GemvArgs& a, int M, uint32_t max_NRB, uint32_t max_K, uint32_t max_nch, hipStream_t st) {
    if (max_K & 127) return PBL_ERR_UNSUPPORTED;
    const uint32_t P = (max_K + PBL_PANEL_COLS - 1) / PBL_PANEL_COLS, Gmax = max_K / 128;
    const dim3 grid(max_NRB, a.Lc, 1);
    for (int m0 = 0; m0 < M; m0 += 2) {                       // two tokens per weight pass (the 2 x 16 accumulators stay in registers)
        const int mb = M - m0 < 2 ? M - m0 : 2;
        GemvArgs b = a;
        b.M = mb; b.tok0 = m0;
        const size_t lds = lds_bytes_groups(P, Gmax, max_nch, mb, 1);
        const int rc = mb == 1 ? launch_groups<1>(b, -1, grid, lds, st) : launch_groups<2>(b, -1, grid, lds, st);
        if (rc != PBL_OK) return rc;
    }
    return PBL_OK;
}

constexpr uint32_t PBL_SPLIT_TARGET_WAVES = 8192u;   // a full chip of waves (256 CUs x 32)
constexpr int PBL_THROUGHPUT_WPB = 4;                // waves per workgroup when every wave owns a record
// waves per record so that a launch of `records` records fields about a full chip of waves;
// more waves per record shorten every wave's serial load -> compute chain.
// The third condition holds at s = 1 for every P, so a launch of fewer than PBL_SPLIT_TARGET_WAVES records always splits: the
// answer 1 means records >= PBL_SPLIT_TARGET_WAVES, which fill the chip at PBL_THROUGHPUT_WPB waves per workgroup.  One wave per
// workgroup with SPLIT = 1 therefore never ran and is not instantiated.
int pick_split(uint32_t records, uint32_t P) {
    int s = 1;
    while (s < 8 && records * uint32_t(s) < PBL_SPLIT_TARGET_WAVES && uint32_t(2 * s) <= (P > 1 ? P : 1u) * 2u) s *= 2;
    return s;
}

// THE launch configuration of a group-free GEMV pass (pbl_gemv_route answers from here, so it cannot drift from what is launched).
// members == 0: one layer of NRB records (route_of: throughput mode, a wave per record and 4 per workgroup, when the records fill
// the chip; otherwise latency mode, S waves share a record).  members == L >= 1: a fused / grouped launch of L members whose
// largest has NRB records (few records in total -- fused q/k/v, gate+up at decode time -- run latency mode).
struct GemvRoute {
    int split, wpb;   // waves per record, waves per workgroup
};
GemvRoute gemv_route(uint32_t NRB, uint32_t P, int members) {
    GemvRoute g;
    const uint64_t records = uint64_t(NRB) * uint64_t(members > 0 ? members : 1);
    g.split = records >= PBL_SPLIT_TARGET_WAVES ? 1 : pick_split(uint32_t(records), P);
    g.wpb = g.split > 1 ? g.split : PBL_THROUGHPUT_WPB;
    return g;
}

// THE launcher of pbl_gemv_kernel: one pass of M tokens on route g over `layers` layers (grid.y) of at most `records` records
// (grid.x) each, P panels and max_nch salient chunks per record at most; sf: PBL_FLAG_SAL_F16 layers may be among them.
template <int XP = XP_NONE>
int launch_gemv(GemvRoute g, uint32_t records, int layers, uint32_t P, uint32_t max_nch, int M, bool sf, const GemvArgs& a,
                hipStream_t st) {
    if (M < 1 || M > PBL_MAX_TOKENS_PER_LAUNCH) return PBL_ERR_INVALID_ARG;
    const dim3 grid(g.split > 1 ? records : (records + g.wpb - 1) / g.wpb, layers, 1);
    const size_t lds = lds_bytes(P, max_nch, M, g.wpb, g.split);
    using Fn = int (*)(const GemvArgs&, dim3, size_t, hipStream_t);
#define PBL_MB(MB, W, S) {launch<MB, W, false, S, XP>, launch<MB, W, true, S, XP>}
#define PBL_CFG(W, S) {PBL_MB(1, W, S), PBL_MB(2, W, S), PBL_MB(3, W, S), PBL_MB(4, W, S)}
    static constexpr Fn table[4][PBL_MAX_TOKENS_PER_LAUNCH][2] = {PBL_CFG(PBL_THROUGHPUT_WPB, 1), PBL_CFG(2, 2), PBL_CFG(4, 4), PBL_CFG(8, 8)};
#undef PBL_CFG
#undef PBL_MB
    return table[g.split == 8 ? 3 : g.split == 4 ? 2 : g.split == 2 ? 1 : 0][M - 1][sf](a, grid, lds, st);
}

// one pass of a.M tokens over the single layer a.layer
template <int XP = XP_NONE>
int one_pass(GemvRoute g, const GemvArgs& a, void* stream) {
    const pbl_layer& l = a.layer;
    return launch_gemv<XP>(g, l.NRB, 1, l.P, l.max_nch, a.M, l.flags & PBL_FLAG_SAL_F16, a, static_cast<hipStream_t>(stream));
}

// [a, a + na) and [b, b + nb) share a byte
bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return na && nb && x < y + nb && y < x + na;
}

// ---- rotary position embedding of a decode step (pbl_rope_f16) -----------------------------------------------------------------
// (RopeArgs and the fp16 products mul_f16: pbl_rope_math.h)
// HF's apply_rotary_pos_emb on half tensors, one (d, d + D/2) pair per thread: q * cos and rotate_half(q) * sin each rounded to
// fp16, then their sum rounded to fp16 -- the three torch kernels' roundings, never contracted into an fma.  inf / NaN propagate.
__global__ __launch_bounds__(256) void pbl_rope_kernel(RopeArgs a) {
#pragma clang fp contract(off)
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.pairs) return;
    const int i = idx % a.half, t = idx / a.half;
    const int h = t % a.H, m = t / a.H;
    const int b = m / a.S, s = m - b * a.S;
    const bool isq = h < a.Hq;
    const int hh = isq ? h : h - a.Hq;
    const int D = 2 * a.half;
    const uint16_t* x = a.qkv + size_t(m) * a.ld + (isq ? a.q_off : a.k_off) + size_t(hh) * D;
    const int64_t crow = b * a.c_sb + s * a.c_ss;
    const float x1 = float(__builtin_bit_cast(_Float16, x[i])), x2 = float(__builtin_bit_cast(_Float16, x[i + a.half]));
    const float c1 = float(__builtin_bit_cast(_Float16, a.cos[crow + i])), c2 = float(__builtin_bit_cast(_Float16, a.cos[crow + i + a.half]));
    const float s1 = float(__builtin_bit_cast(_Float16, a.sin[crow + i])), s2 = float(__builtin_bit_cast(_Float16, a.sin[crow + i + a.half]));
    const _Float16 o1 = _Float16(mul_f16(x1, c1) + mul_f16(-x2, s1));      // rotate_half: (-x2, x1); fp32 sum, one rounding
    const _Float16 o2 = _Float16(mul_f16(x2, c2) + mul_f16(x1, s2));
    uint16_t* out = isq ? a.q_out + (b * a.q_ob + hh * a.q_oh + s * a.q_os) : a.k_out + (b * a.k_ob + hh * a.k_oh + s * a.k_os);
    out[i] = __builtin_bit_cast(uint16_t, o1);
    out[i + a.half] = __builtin_bit_cast(uint16_t, o2);
}

// ---- RoPE + static KV-cache append of a decode step (pbl_rope_append_f16) ------------------------------------------------------
struct RopeAppendArgs {
    RopeArgs r;                     // q / k as in pbl_rope_kernel (r.k_out unused); r.H = Hq + 2 Hkv: the v heads follow the k heads
    uint16_t* k_cache;              // [B, Hkv, max_len, D] fp16
    uint16_t* v_cache;
    const int64_t* pos;             // the layer's position: token (b, s) goes to cache row pos + s
    uint32_t v_off;
    int Hkv, max_len;
};

// pbl_rope_kernel's arithmetic for the q and k heads (the same roundings, bit for bit); k goes to cache row pos + s instead of a
// fresh tensor, and the v heads are copied there unchanged.  The position is read on the device: one captured graph serves every
// position.  Rows at or beyond max_len are not written.
__global__ __launch_bounds__(256) void pbl_rope_append_kernel(RopeAppendArgs a) {
#pragma clang fp contract(off)
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.r.pairs) return;
    const int i = idx % a.r.half, t = idx / a.r.half;
    const int h = t % a.r.H, m = t / a.r.H;
    const int b = m / a.r.S, s = m - b * a.r.S;
    const int D = 2 * a.r.half;
    const int64_t row = *a.pos + s;
    if (h >= a.r.Hq + a.Hkv) {                                              // a v head: copied as it is
        const int hh = h - a.r.Hq - a.Hkv;
        if (row < 0 || row >= a.max_len) return;
        const uint16_t* x = a.r.qkv + size_t(m) * a.r.ld + a.v_off + size_t(hh) * D;
        uint16_t* out = a.v_cache + ((size_t(b) * a.Hkv + hh) * a.max_len + row) * D;
        out[i] = x[i];
        out[i + a.r.half] = x[i + a.r.half];
        return;
    }
    const bool isq = h < a.r.Hq;
    const int hh = isq ? h : h - a.r.Hq;
    if (!isq && (row < 0 || row >= a.max_len)) return;
    const uint16_t* x = a.r.qkv + size_t(m) * a.r.ld + (isq ? a.r.q_off : a.r.k_off) + size_t(hh) * D;
    const int64_t crow = b * a.r.c_sb + s * a.r.c_ss;
    const float x1 = float(__builtin_bit_cast(_Float16, x[i])), x2 = float(__builtin_bit_cast(_Float16, x[i + a.r.half]));
    const float c1 = float(__builtin_bit_cast(_Float16, a.r.cos[crow + i])), c2 = float(__builtin_bit_cast(_Float16, a.r.cos[crow + i + a.r.half]));
    const float s1 = float(__builtin_bit_cast(_Float16, a.r.sin[crow + i])), s2 = float(__builtin_bit_cast(_Float16, a.r.sin[crow + i + a.r.half]));
    const _Float16 o1 = _Float16(mul_f16(x1, c1) + mul_f16(-x2, s1));      // rotate_half: (-x2, x1); fp32 sum, one rounding
    const _Float16 o2 = _Float16(mul_f16(x2, c2) + mul_f16(x1, s2));
    uint16_t* out = isq ? a.r.q_out + (b * a.r.q_ob + hh * a.r.q_oh + s * a.r.q_os)
                        : a.k_cache + ((size_t(b) * a.Hkv + hh) * a.max_len + row) * D;
    out[i] = __builtin_bit_cast(uint16_t, o1);
    out[i + a.r.half] = __builtin_bit_cast(uint16_t, o2);
}

}  // namespace

extern "C" {

size_t pbl_gemv_lds_bytes(const pbl_layer* layer, int m) {
    if (!layer || m < 1 || m > PBL_MAX_TOKENS_PER_LAUNCH) return 0;
    return lds_bytes(layer->P, layer->max_nch, m, 4);
}

// Host only: which pbl_gemv_kernel configuration a group-free launch gets (gemv_route, the helper every launcher asks).
int pbl_gemv_route(uint32_t NRB, uint32_t P, int members, int* split, int* wpb) {
    if (!split || !wpb || members < 0 || !NRB || !P) return PBL_ERR_INVALID_ARG;
    const GemvRoute g = gemv_route(NRB, P, members);
    *split = g.split; *wpb = g.wpb;
    return PBL_OK;
}

int pbl_linear_f16(const pbl_layer* layer, const void* x, void* y, int M, int y_f32, void* stream) {
    return pbl_linear_f16_ws(layer, x, y, M, y_f32, nullptr, 0, stream);
}

// Routing of one layer's forward between the GEMV (weights streamed once per `mb` tokens) and the matrix-core kernel (once per
// 32 tokens, but with a per-record expansion cost that only pays off from a handful of tokens on).  Measured on MI355X
// (tools/bench_route.py): the GEMV wins while all tokens fit ONE pass whose LDS footprint (x tile + chunk partials) leaves at
// least two workgroups per CU; a pass squeezed into a single workgroup per CU (K = 11008 with 3 tokens, 13824x5120 at 20 %
// salients with 4) is 3-10x slower than the matrix-core kernel, and so is the matrix-core kernel without its K split.
struct Route {
    GemvRoute g;              // GEMV: waves per record, waves per workgroup
    int mb_max;               //       tokens per pass
    bool mfma;                // more tokens than one GEMV pass takes and the matrix-core kernel applies
};
constexpr size_t PBL_GEMV_LDS_BUDGET = 80 * 1024;   // two workgroups per CU
static Route route_of(const pbl_layer* layer, int M, bool x_aligned) {
    Route r;
    if (layer->G != 1) {
        r.g = {1, 1}; r.mb_max = 2;               // the column-group GEMV: a wave per workgroup, 2 x 16 accumulators in registers
        while (r.mb_max > 1 && lds_bytes_groups(layer->P, layer->G, layer->max_nch, r.mb_max, 1) > 96 * 1024) --r.mb_max;
    } else {
        // throughput mode (a wave per record, 4 per workgroup) when there are enough records to fill the
        // chip; otherwise latency mode: S waves share a record
        r.g = gemv_route(layer->NRB, layer->P, 0);
        r.mb_max = PBL_MAX_TOKENS_PER_LAUNCH;
        while (r.mb_max > 1 && lds_bytes(layer->P, layer->max_nch, r.mb_max, r.g.wpb, r.g.split) > PBL_GEMV_LDS_BUDGET) --r.mb_max;
    }
    // (tiny layers at M <= 8 stay on the GEMV: both are launch-latency bound and the GEMV starts faster)
    r.mfma = M > r.mb_max && (M > 8 || layer->NRB >= 128) && !(layer->K & 7) && x_aligned &&
             (layer->flags & PBL_FLAG_TAIL_REPEAT) && (layer->flags & PBL_FLAG_SLABS);
    if (r.mfma && M <= 8 && layer->G == 1) {
        // a few tokens more than one pass holds: several GEMV passes can still beat the matrix-core kernel.  Estimates in us,
        // fitted to tools/bench_route.py on MI355X (4096^2, 11008x4096, 4096x11008, 13824x5120 at 5-20 % salients; within 20 %):
        //   GEMV pass of mb tokens   3.5 + packed bytes / 6.5 TB/s + (N K / 1e6) * (0.04 + 0.33 * salient density) * mb
        //   matrix-core kernel       8.5 + (N K / 1e6) * (0.27 + 0.7 * salient density)      (flat in M up to 16 tokens)
        const double wm = double(layer->N) * layer->K * 1e-6;
        const double nnz = double(layer->max_nch) * layer->NRB * 16.0;             // upper bound: every record as full as the fullest
        const double bytes = double(layer->N) * layer->K / 8 + nnz * 2.125;
        const double pass0 = 3.5 + bytes / 6.5e6, per_tok = wm * (0.04 + 0.33 * nnz / (wm * 1e6));
        double gemv = 0;
        for (int m0 = 0; m0 < M; m0 += r.mb_max) gemv += pass0 + per_tok * (M - m0 < r.mb_max ? M - m0 : r.mb_max);
        r.mfma = 8.5 + wm * (0.27 + 0.7 * nnz / (wm * 1e6)) < gemv;
    }
    if (r.mfma && layer->G != 1) {
        const uint32_t gs = layer->K / layer->G;
        r.mfma = gs * layer->G == layer->K && !(gs & (gs - 1)) && gs >= 128;
    }
    return r;
}

// what every entry that runs ONE GEMV pass of a group-free layer checks first: PBL_OK and the route, else the entry's
// return code (a misaligned blob; column groups or more rows than one pass takes: PBL_ERR_UNSUPPORTED)
static int one_pass_route(const pbl_layer* layer, int M, Route& r) {
    if (reinterpret_cast<uintptr_t>(layer->blob) & 15) return PBL_ERR_MISALIGNED;
    if (layer->G != 1) return PBL_ERR_UNSUPPORTED;
    r = route_of(layer, M, true);
    return M > r.mb_max ? PBL_ERR_UNSUPPORTED : PBL_OK;
}

size_t pbl_linear_workspace_bytes(const pbl_layer* layer, int M) {
    if (!layer || M < 1) return 0;
    return route_of(layer, M, true).mfma ? pbl_mfma_workspace_bytes(layer, M < 32 ? M : 32) : 0;
}

static int mfma_passes(const pbl_layer* layer, const void* x, void* y, int M, int y_f32, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t esz = y_f32 ? 4 : 2;
    int rc = PBL_OK;
    for (int m0 = 0; m0 < M && rc == PBL_OK; m0 += 32) {
        const int mb = M - m0 < 32 ? M - m0 : 32;
        rc = pbl_gemm_mfma_f16_ws(layer, static_cast<const _Float16*>(x) + size_t(m0) * layer->K,
                                  static_cast<char*>(y) + size_t(m0) * layer->N * esz, mb, y_f32, workspace, workspace_bytes, stream);
    }
    return rc;
}

int pbl_linear_f16_ws(const pbl_layer* layer, const void* x, void* y, int M, int y_f32, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (!layer || !layer->blob || !x || !y || M < 1) return PBL_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(layer->blob) & 15) return PBL_ERR_MISALIGNED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t esz = y_f32 ? 4 : 2;
    const Route r = route_of(layer, M, !(reinterpret_cast<uintptr_t>(x) & 15));
    if (r.mfma) {
        // Without the K-split workspace the matrix-core kernel leaves most of the chip idle on all but the largest layers:
        // a few tokens are then better served by GEMV passes.
        const size_t need = pbl_mfma_workspace_bytes(layer, M < 32 ? M : 32);
        const bool ws_ok = !need || (workspace && workspace_bytes >= need);
        if (ws_ok || M > 8) {
            const int rc = mfma_passes(layer, x, y, M, y_f32, workspace, workspace_bytes, stream);
            if (rc != PBL_ERR_UNSUPPORTED) return rc;   // unsupported (LDS budget): every pass failed the same way, fall through
        }
    }
    if (layer->G != 1) return linear_groups(layer, x, y, M, y_f32, st);
    for (int m0 = 0; m0 < M; m0 += r.mb_max) {
        const int mb = M - m0 < r.mb_max ? M - m0 : r.mb_max;
        GemvArgs a{};
        a.layer = *layer;
        a.x = static_cast<const _Float16*>(x) + size_t(m0) * layer->K;
        a.y = static_cast<char*>(y) + size_t(m0) * layer->N * esz;
        a.M = mb; a.y_f32 = y_f32; a.grouped = 0;
        if (const int rc = one_pass(r.g, a, stream)) return rc;
    }
    return PBL_OK;
}

// bf16 activations in ONE launch (round 5): x [M, K] bf16, y [M, N] bf16 (fp32 with y_f32) = F.linear(x, W, bias) as the reference's
// bf16 runs compute it (qat/run_qat.py:120; quant/outlier_quantizer.py:101-106 under bf16) -- the GEMV's staging phase scales every
// token's row by a power of two into fp16's range while it copies it into LDS (exact; a token holding inf / NaN runs as its indicator
// row), the epilogue scales back, adds the bias and rounds to bf16: the arithmetic of pbl_act_bf16_prepare + pbl_linear_f16 +
// pbl_act_finish, bit for bit, without the two extra launches.  One GEMV pass of a group-free layer only (M <= the route's limit,
// at most 4): PBL_ERR_UNSUPPORTED otherwise -- the caller then runs the three-launch form, which serves every kernel family.
int pbl_linear_bf16(const pbl_layer* layer, const void* x_bf16, void* y, int M, int y_f32, void* stream) {
    if (!layer || !layer->blob || !x_bf16 || !y || M < 1) return PBL_ERR_INVALID_ARG;
    Route r;
    if (const int rc = one_pass_route(layer, M, r)) return rc;
    GemvArgs a{};
    a.layer = *layer;
    a.x = static_cast<const _Float16*>(x_bf16);                  // (bf16 bits: the XB instantiation reads them as such)
    a.y = y;
    a.M = M; a.y_f32 = y_f32; a.grouped = 0; a.x_bf16 = 1;
    return one_pass(r.g, a, stream);
}

// LLaMA's MLP tail in ONE launch: y [M, N] = down_proj(silu(gate) * up), the GEMV's staging phase building its x row from the fused
// gate/up launch's output (gate_up [M, ldx] fp16: gate at column 0, up at column up_off) with torch's roundings (swiglu_f16).  One
// GEMV pass of a group-free layer, like pbl_linear_bf16: PBL_ERR_UNSUPPORTED otherwise (column groups, more rows than one pass
// takes, every row count route_of sends to the matrix-core kernel) -- the caller then runs silu and * in torch and the layer.
int pbl_linear_f16_swiglu(const pbl_layer* layer, const void* gate_up, uint32_t ldx, uint32_t up_off, void* y, int M, int y_f32,
                          void* stream) {
    if (!layer || !layer->blob || !gate_up || !y || M < 1 || up_off < layer->K || uint64_t(ldx) < uint64_t(up_off) + layer->K)
        return PBL_ERR_INVALID_ARG;
    Route r;
    if (const int rc = one_pass_route(layer, M, r)) return rc;
    GemvArgs a{};
    a.layer = *layer;
    a.x = static_cast<const _Float16*>(gate_up);
    a.y = y;
    a.M = M; a.y_f32 = y_f32; a.grouped = 0;
    a.ldx = ldx; a.up_off = up_off;
    return one_pass<XP_SWIGLU>(r.g, a, stream);
}

// A decoder layer's residual adds in the GEMV's store (XE_RESIDUAL): y [M, N] fp16 = fp16(fp16(layer(x)) + residual), residual
// [M, ldr] fp16 -- HF's `residual + o_proj(attn)` in ONE launch.  One GEMV pass of a group-free layer (as pbl_linear_f16_swiglu):
// PBL_ERR_UNSUPPORTED otherwise -- the caller runs the layer and the add.  y must not overlap x or the residual.
int pbl_linear_f16_residual(const pbl_layer* layer, const void* x, const void* residual, uint32_t ldr, void* y, int M, void* stream) {
    if (!layer || !layer->blob || !x || !residual || !y || M < 1 || M > (1 << 20) || ldr < layer->N) return PBL_ERR_INVALID_ARG;
    const size_t ybytes = size_t(M) * layer->N * 2;
    if (overlaps(y, ybytes, x, size_t(M) * layer->K * 2) || overlaps(y, ybytes, residual, (size_t(M - 1) * ldr + layer->N) * 2))
        return PBL_ERR_INVALID_ARG;
    Route r;
    if (const int rc = one_pass_route(layer, M, r)) return rc;
    GemvArgs a{};
    a.layer = *layer;
    a.x = static_cast<const _Float16*>(x);
    a.y = y;
    a.M = M; a.y_f32 = 0; a.grouped = 0;
    a.residual = static_cast<const _Float16*>(residual); a.ldr = ldr;
    return one_pass<XP_NONE | XE_RESIDUAL>(r.g, a, stream);
}

// LLaMA's whole MLP tail in ONE launch: y [M, N] fp16 = fp16(fp16(layer(silu(gate) * up)) + residual) -- pbl_linear_f16_swiglu's
// prologue and pbl_linear_f16_residual's epilogue.  Same declines; y must not overlap gate_up or the residual.
int pbl_linear_f16_swiglu_residual(const pbl_layer* layer, const void* gate_up, uint32_t ldx, uint32_t up_off, const void* residual,
                                   uint32_t ldr, void* y, int M, void* stream) {
    if (!layer || !layer->blob || !gate_up || !residual || !y || M < 1 || M > (1 << 20) || up_off < layer->K ||
        uint64_t(ldx) < uint64_t(up_off) + layer->K || ldr < layer->N)
        return PBL_ERR_INVALID_ARG;
    const size_t ybytes = size_t(M) * layer->N * 2;
    if (overlaps(y, ybytes, gate_up, (size_t(M - 1) * ldx + up_off + layer->K) * 2) ||
        overlaps(y, ybytes, residual, (size_t(M - 1) * ldr + layer->N) * 2))
        return PBL_ERR_INVALID_ARG;
    Route r;
    if (const int rc = one_pass_route(layer, M, r)) return rc;
    GemvArgs a{};
    a.layer = *layer;
    a.x = static_cast<const _Float16*>(gate_up);
    a.y = y;
    a.M = M; a.y_f32 = 0; a.grouped = 0;
    a.ldx = ldx; a.up_off = up_off;
    a.residual = static_cast<const _Float16*>(residual); a.ldr = ldr;
    return one_pass<XP_SWIGLU | XE_RESIDUAL>(r.g, a, stream);
}

// HF's apply_rotary_pos_emb for the q and k heads of a fused q/k/v output, in ONE launch (pbl_rope_kernel).  Token m = b * S + s
// of qkv [B S, ld] fp16 holds Hq q heads from column q_off and Hkv k heads from column k_off, head_dim D each.  cos / sin: the row
// of token (b, s) starts at b * cos_sb + s * cos_ss elements (a stride of 0 broadcasts), cos_dim its length.  q_out / k_out
// [B, H, S, D] fp16 with element strides {b, h, s} in q_ostride / k_ostride (host arrays) and unit d stride: the layout torch's
// elementwise kernels give the result.  PBL_ERR_INVALID_ARG (before any device work): NULL pointers, sizes < 1, negative strides,
// heads outside a row of qkv, an output overlapping an input or the other output.  PBL_ERR_UNSUPPORTED: odd D, D > 256,
// cos_dim != D.  No allocation, no synchronisation: capturable in a hipGraph.
int pbl_rope_f16(const void* qkv, uint32_t ld, uint32_t q_off, uint32_t k_off, int B, int S, int Hq, int Hkv, int D,
                 const void* cos, const void* sin, int cos_dim, int64_t cos_sb, int64_t cos_ss,
                 void* q_out, const int64_t* q_ostride, void* k_out, const int64_t* k_ostride, void* stream) {
    if (!qkv || !cos || !sin || !q_out || !k_out || !q_ostride || !k_ostride || B < 1 || S < 1 || Hq < 1 || Hkv < 1 || D < 1 ||
        cos_dim < 1 || cos_sb < 0 || cos_ss < 0)
        return PBL_ERR_INVALID_ARG;
    for (int j = 0; j < 3; ++j)
        if (q_ostride[j] < 0 || k_ostride[j] < 0) return PBL_ERR_INVALID_ARG;
    const int64_t M = int64_t(B) * S;
    const int64_t qend = int64_t(q_off) + int64_t(Hq) * D, kend = int64_t(k_off) + int64_t(Hkv) * D;
    if (qend > ld || kend > ld || M * (Hq + Hkv) * D > (int64_t(1) << 30)) return PBL_ERR_INVALID_ARG;
    auto out_bytes = [&](const int64_t* o, int H) {
        return size_t(((B - 1) * o[0] + int64_t(H - 1) * o[1] + (S - 1) * o[2] + D) * 2);
    };
    const size_t qb = out_bytes(q_ostride, Hq), kb = out_bytes(k_ostride, Hkv);
    const size_t xb = size_t(((M - 1) * ld + (qend > kend ? qend : kend)) * 2);
    const size_t cb = size_t(((B - 1) * cos_sb + (S - 1) * cos_ss + cos_dim) * 2);
    if (overlaps(q_out, qb, k_out, kb) || overlaps(q_out, qb, qkv, xb) || overlaps(k_out, kb, qkv, xb) ||
        overlaps(q_out, qb, cos, cb) || overlaps(k_out, kb, cos, cb) || overlaps(q_out, qb, sin, cb) || overlaps(k_out, kb, sin, cb))
        return PBL_ERR_INVALID_ARG;
    if ((D & 1) || D > 256 || cos_dim != D) return PBL_ERR_UNSUPPORTED;
    RopeArgs a{};
    a.qkv = static_cast<const uint16_t*>(qkv);
    a.cos = static_cast<const uint16_t*>(cos); a.sin = static_cast<const uint16_t*>(sin);
    a.q_out = static_cast<uint16_t*>(q_out); a.k_out = static_cast<uint16_t*>(k_out);
    a.c_sb = cos_sb; a.c_ss = cos_ss;
    a.q_ob = q_ostride[0]; a.q_oh = q_ostride[1]; a.q_os = q_ostride[2];
    a.k_ob = k_ostride[0]; a.k_oh = k_ostride[1]; a.k_os = k_ostride[2];
    a.ld = ld; a.q_off = q_off; a.k_off = k_off;
    a.S = S; a.Hq = Hq; a.H = Hq + Hkv; a.half = D / 2;
    a.pairs = int(M * (Hq + Hkv) * (D / 2));
    void* argv[] = {&a};
    return hipLaunchKernel(reinterpret_cast<const void*>(pbl_rope_kernel), dim3((a.pairs + 255) / 256), dim3(256), argv, 0,
                           static_cast<hipStream_t>(stream)) == hipSuccess ? PBL_OK : PBL_ERR_LAUNCH;
}

// pbl_rope_f16 for q, and k / v appended to a layer's static KV cache in the same launch (pbl_rope_append_kernel).  Scope of the
// decode-attention path (pbl_decode_attn_f16): PBL_ERR_UNSUPPORTED unless D is 64 or 128, S <= 4, B <= 4 and Hkv divides Hq.
int pbl_rope_append_f16(const void* qkv, uint32_t ld, uint32_t q_off, uint32_t k_off, uint32_t v_off, int B, int S, int Hq, int Hkv,
                        int D, const void* cos, const void* sin, int cos_dim, int64_t cos_sb, int64_t cos_ss,
                        void* q_out, const int64_t* q_ostride, void* k_cache, void* v_cache, int max_len, const int64_t* pos,
                        void* stream) {
    if (!qkv || !cos || !sin || !q_out || !q_ostride || !k_cache || !v_cache || !pos || B < 1 || S < 1 || Hq < 1 || Hkv < 1 ||
        D < 1 || cos_dim < 1 || cos_sb < 0 || cos_ss < 0 || max_len < 1)
        return PBL_ERR_INVALID_ARG;
    for (int j = 0; j < 3; ++j)
        if (q_ostride[j] < 0) return PBL_ERR_INVALID_ARG;
    const int64_t M = int64_t(B) * S;
    const int64_t qend = int64_t(q_off) + int64_t(Hq) * D, kend = int64_t(k_off) + int64_t(Hkv) * D;
    const int64_t vend = int64_t(v_off) + int64_t(Hkv) * D;
    const int64_t xend = qend > kend ? (qend > vend ? qend : vend) : (kend > vend ? kend : vend);
    if (xend > ld || M * (Hq + 2 * Hkv) * D > (int64_t(1) << 30) || int64_t(B) * Hkv * max_len * D > (int64_t(1) << 40))
        return PBL_ERR_INVALID_ARG;
    const size_t qb = size_t(((B - 1) * q_ostride[0] + int64_t(Hq - 1) * q_ostride[1] + (S - 1) * q_ostride[2] + D) * 2);
    const size_t cacheb = size_t(int64_t(B) * Hkv * max_len * D * 2);
    const size_t xb = size_t(((M - 1) * ld + xend) * 2);
    const size_t cb = size_t(((B - 1) * cos_sb + (S - 1) * cos_ss + cos_dim) * 2);
    const void* outs[3] = {q_out, k_cache, v_cache};
    const size_t outb[3] = {qb, cacheb, cacheb};
    for (int j = 0; j < 3; ++j) {
        if (overlaps(outs[j], outb[j], qkv, xb) || overlaps(outs[j], outb[j], cos, cb) || overlaps(outs[j], outb[j], sin, cb) ||
            overlaps(outs[j], outb[j], pos, 8))
            return PBL_ERR_INVALID_ARG;
        for (int o = j + 1; o < 3; ++o)
            if (overlaps(outs[j], outb[j], outs[o], outb[o])) return PBL_ERR_INVALID_ARG;
    }
    if ((D != 64 && D != 128) || S > 4 || B > 4 || Hq % Hkv || cos_dim != D) return PBL_ERR_UNSUPPORTED;
    RopeAppendArgs a{};
    a.r.qkv = static_cast<const uint16_t*>(qkv);
    a.r.cos = static_cast<const uint16_t*>(cos); a.r.sin = static_cast<const uint16_t*>(sin);
    a.r.q_out = static_cast<uint16_t*>(q_out);
    a.r.c_sb = cos_sb; a.r.c_ss = cos_ss;
    a.r.q_ob = q_ostride[0]; a.r.q_oh = q_ostride[1]; a.r.q_os = q_ostride[2];
    a.r.ld = ld; a.r.q_off = q_off; a.r.k_off = k_off;
    a.r.S = S; a.r.Hq = Hq; a.r.H = Hq + 2 * Hkv; a.r.half = D / 2;
    a.r.pairs = int(M * (Hq + 2 * Hkv) * (D / 2));
    a.k_cache = static_cast<uint16_t*>(k_cache); a.v_cache = static_cast<uint16_t*>(v_cache);
    a.pos = pos; a.v_off = v_off; a.Hkv = Hkv; a.max_len = max_len;
    void* argv[] = {&a};
    return hipLaunchKernel(reinterpret_cast<const void*>(pbl_rope_append_kernel), dim3((a.r.pairs + 255) / 256), dim3(256), argv, 0,
                           static_cast<hipStream_t>(stream)) == hipSuccess ? PBL_OK : PBL_ERR_LAUNCH;
}

// K-split tensor parallelism, fused: the GEMV of this rank's column shard with its epilogue pushing the fp32 partial y[M, N]
// straight into slot [set][rank] of every rank's peer-mapped communication buffer (pbl_comm_alloc / pbl_ipc_open; layout in
// csrc/pbl_p2p_layout.h) -- 7 xGMI stores + 1 local per row owner -- and counting every finished record at the peers.
// pbl_p2p_reduce_f32_dev(.., expect_records = layer->NRB, ..) then sums the slots: the partial never makes the round trip
// through local HBM and the push has no launch of its own.  One GEMV pass only (M <= 4 with the x tile in LDS, group-free
// layers): PBL_ERR_UNSUPPORTED otherwise -- the caller then runs pbl_linear_f16 + pbl_p2p_allreduce_f32_dev.
int pbl_linear_f16_push(const pbl_layer* layer, const void* x, int M, void* const* peer_bufs, int rank, int world, size_t max_elems,
                        void* stream) {
    if (!layer || !layer->blob || !x || !peer_bufs || M < 1 || world < 1 || world > PBL_P2P_MAX_WORLD || rank < 0 || rank >= world)
        return PBL_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(layer->blob) & 15) return PBL_ERR_MISALIGNED;
    const size_t cap = (max_elems + 3) & ~size_t(3);
    if (size_t(M) * layer->N > cap) return PBL_ERR_CAPACITY;
    if (layer->G != 1) return PBL_ERR_UNSUPPORTED;
    const Route r = route_of(layer, M, !(reinterpret_cast<uintptr_t>(x) & 15));
    if (M > r.mb_max) return PBL_ERR_UNSUPPORTED;
    GemvArgs a{};
    a.layer = *layer;
    a.layer.bias = rank == 0 ? layer->bias : nullptr;         // (the bias is added once: by rank 0's partial)
    a.x = static_cast<const _Float16*>(x);
    a.y = nullptr;
    a.M = M; a.y_f32 = 1; a.grouped = 0;
    a.push_world = world; a.push_rank = rank; a.push_cap = cap;
    for (int p = 0; p < world; ++p) {
        if (!peer_bufs[p]) return PBL_ERR_INVALID_ARG;
        a.push_peer[p] = static_cast<uint8_t*>(peer_bufs[p]);
    }
    return one_pass(r.g, a, stream);
}

// The largest M pbl_linear_f16_push takes for this shard: route_of's one-pass limit, which follows the shard's fullest record
// (LDS: x tile + chunk partials).  The ranks of a K-split layer agree on the minimum (pb_llm_amd/parallel.py).
int pbl_linear_push_max_tokens(const pbl_layer* layer) {
    if (!layer || layer->G != 1) return 0;
    return route_of(layer, PBL_MAX_TOKENS_PER_LAUNCH, true).mb_max;
}

int pbl_unpack_dev(const pbl_layer* layer, void* W_out, int out_f32, void* stream) {
    if (!layer || !layer->blob || !W_out) return PBL_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(layer->blob) & 15) return PBL_ERR_MISALIGNED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    pbl_layer L = *layer;
    // one LDS row-segment buffer per wave: at most 16 KiB each, so that several workgroups share a CU
    const size_t esz = out_f32 ? 4 : 2;
    int seg_panels = int((16 * 1024) / (PBL_PANEL_COLS * esz));           // 16 (fp16) or 8 (fp32) panels
    if (seg_panels > int(layer->P)) seg_panels = int(layer->P);
    const size_t lds = size_t(seg_panels) * PBL_PANEL_COLS * esz * 4;
    void* argv[] = {&L, &W_out, &seg_panels};
    const void* k = out_f32 ? reinterpret_cast<const void*>(pbl_unpack_kernel<float>)
                            : reinterpret_cast<const void*>(pbl_unpack_kernel<_Float16>);
    return hipLaunchKernel(k, dim3(4 * layer->NRB), dim3(4 * PBL_WAVE), argv, lds, st) == hipSuccess ? PBL_OK : PBL_ERR_LAUNCH;
}

int pbl_gemv_f16_grouped(const pbl_layer* layers_dev, const void* const* x_dev, void* const* y_dev, int Lc,
                         int M, uint32_t max_NRB, uint32_t max_K, uint32_t max_nch, uint32_t max_nexc,
                         int any_groups, int y_f32, void* stream) {
    (void)max_nexc;
    if (!layers_dev || !x_dev || !y_dev || Lc < 1 || M < 1 || M > PBL_MAX_TOKENS_PER_LAUNCH)
        return PBL_ERR_INVALID_ARG;
    if (Lc > 65535) return PBL_ERR_UNSUPPORTED;
    GemvArgs a{};
    a.layers = layers_dev; a.xs = x_dev; a.ys = y_dev; a.M = M; a.y_f32 = y_f32; a.grouped = 1; a.Lc = Lc;
    if (any_groups & 1) return grouped_groups(a, M, max_NRB, max_K, max_nch, static_cast<hipStream_t>(stream));
    const uint32_t P = (max_K + PBL_PANEL_COLS - 1) / PBL_PANEL_COLS;
    // bit 1 of any_groups: the group may contain PBL_FLAG_SAL_F16 layers
    return launch_gemv(gemv_route(max_NRB, P, Lc), max_NRB, Lc, P, max_nch, M, (any_groups & 2) != 0, a, static_cast<hipStream_t>(stream));
}

// A fused launch of Lc members reading K columns each (column groups: the column-group kernel).  With a.norm_w set (group-free
// members only: the caller has checked) the RMSNorm prologue stages x, and what one pass under route_of's LDS budget cannot take
// is declined.
static int fused_launch(GemvArgs& a, int Lc, int M, uint32_t max_NRB, uint32_t K, uint32_t max_nch, int group_flags, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (group_flags & 1) { a.Lc = Lc; return grouped_groups(a, M, max_NRB, K, max_nch, st); }
    const uint32_t P = (K + PBL_PANEL_COLS - 1) / PBL_PANEL_COLS;
    const bool sf = (group_flags & 2) != 0;
    const GemvRoute g = gemv_route(max_NRB, P, Lc);
    if (!a.norm_w) return launch_gemv(g, max_NRB, Lc, P, max_nch, M, sf, a, st);
    if (lds_bytes(P, max_nch, M, g.wpb, g.split) > PBL_GEMV_LDS_BUDGET) return PBL_ERR_UNSUPPORTED;
    return launch_gemv<XP_RMSNORM>(g, max_NRB, Lc, P, max_nch, M, sf, a, st);
}

int pbl_gemv_f16_fused(const pbl_layer* layers_dev, const uint64_t* y_off_dev, const void* x, void* y, int Lc, int M,
                       uint32_t ldy, uint32_t max_NRB, uint32_t K, uint32_t max_nch, int group_flags, int y_f32, void* stream) {
    if (!layers_dev || !y_off_dev || !x || !y || Lc < 1 || M < 1 || M > PBL_MAX_TOKENS_PER_LAUNCH || !ldy)
        return PBL_ERR_INVALID_ARG;
    if (Lc > 65535) return PBL_ERR_UNSUPPORTED;
    GemvArgs a{};
    a.layers = layers_dev; a.M = M; a.y_f32 = y_f32; a.grouped = 1;
    a.x_shared = static_cast<const _Float16*>(x); a.y_shared = y; a.y_off = y_off_dev; a.ldy = ldy;
    return fused_launch(a, Lc, M, max_NRB, K, max_nch, group_flags, stream);
}

static int fused_host(const pbl_layer* layers_host, const uint64_t* y_off_host, const void* x, void* y, int Lc, int M,
                      uint32_t ldy, uint32_t max_NRB, uint32_t K, uint32_t max_nch, int group_flags, int y_f32, int x_bf16, void* stream,
                      const void* norm_w = nullptr, float norm_eps = 0.f);

int pbl_gemv_f16_fused_host(const pbl_layer* layers_host, const uint64_t* y_off_host, const void* x, void* y, int Lc, int M,
                            uint32_t ldy, uint32_t max_NRB, uint32_t K, uint32_t max_nch, int group_flags, int y_f32, void* stream) {
    return fused_host(layers_host, y_off_host, x, y, Lc, M, ldy, max_NRB, K, max_nch, group_flags, y_f32, 0, stream);
}

// the same launch with LlamaRMSNorm folded into its staging phase: x is the RAW hidden state [M, K] fp16, norm_w [K] fp16 the norm's
// weight (XP_RMSNORM).  Every member reads K columns.  PBL_ERR_UNSUPPORTED for column groups and for more rows than one pass takes
// under the GEMV's LDS budget (route_of's) -- the caller then applies the norm in torch and runs pbl_gemv_f16_fused_host.
int pbl_gemv_f16_fused_norm_host(const pbl_layer* layers_host, const uint64_t* y_off_host, const void* x, void* y, int Lc, int M,
                                 uint32_t ldy, uint32_t max_NRB, uint32_t K, uint32_t max_nch, int group_flags, int y_f32,
                                 const void* norm_w, float norm_eps, void* stream) {
    if (!layers_host || !y_off_host || !x || !y || !norm_w || Lc < 1 || Lc > PBL_FUSED_INLINE_MAX || M < 1 || !ldy || K < 1)
        return PBL_ERR_INVALID_ARG;
    for (int l = 0; l < Lc; ++l)
        if (layers_host[l].K != K) return PBL_ERR_INVALID_ARG;           // (the weight is read for K columns)
    if ((group_flags & 1) || M > PBL_MAX_TOKENS_PER_LAUNCH) return PBL_ERR_UNSUPPORTED;
    return fused_host(layers_host, y_off_host, x, y, Lc, M, ldy, max_NRB, K, max_nch, group_flags, y_f32, 0, stream, norm_w, norm_eps);
}

// the same launch with bf16 activations converted in the kernel and a bf16 (or fp32) result: see pbl_linear_bf16.  Group-free members
// only (PBL_ERR_UNSUPPORTED when bit 0 of group_flags is set: the column-group kernel has no bf16 instantiation).
int pbl_gemv_bf16_fused_host(const pbl_layer* layers_host, const uint64_t* y_off_host, const void* x_bf16, void* y, int Lc, int M,
                             uint32_t ldy, uint32_t max_NRB, uint32_t K, uint32_t max_nch, int group_flags, int y_f32, void* stream) {
    if (group_flags & 1) return PBL_ERR_UNSUPPORTED;
    return fused_host(layers_host, y_off_host, x_bf16, y, Lc, M, ldy, max_NRB, K, max_nch, group_flags, y_f32, 1, stream);
}

static int fused_host(const pbl_layer* layers_host, const uint64_t* y_off_host, const void* x, void* y, int Lc, int M,
                      uint32_t ldy, uint32_t max_NRB, uint32_t K, uint32_t max_nch, int group_flags, int y_f32, int x_bf16, void* stream,
                      const void* norm_w, float norm_eps) {
    if (!layers_host || !y_off_host || !x || !y || Lc < 1 || Lc > PBL_FUSED_INLINE_MAX || M < 1 || M > PBL_MAX_TOKENS_PER_LAUNCH || !ldy)
        return PBL_ERR_INVALID_ARG;
    GemvArgs a{};
    a.M = M; a.y_f32 = y_f32; a.grouped = 1; a.n_inl = Lc; a.x_bf16 = x_bf16;
    for (int l = 0; l < Lc; ++l) {
        if (!layers_host[l].blob || (reinterpret_cast<uintptr_t>(layers_host[l].blob) & 15)) return PBL_ERR_MISALIGNED;
        a.inl[l] = layers_host[l]; a.inl_off[l] = y_off_host[l];
    }
    a.x_shared = static_cast<const _Float16*>(x); a.y_shared = y; a.ldy = ldy;
    if (norm_w) {
        a.norm_w = static_cast<const _Float16*>(norm_w); a.norm_eps = norm_eps;
    }
    return fused_launch(a, Lc, M, max_NRB, K, max_nch, group_flags, stream);
}

}  // extern "C"
