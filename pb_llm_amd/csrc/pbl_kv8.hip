// pbl_kv8.hip -- the FP8 KV cache: pbl_rope_append_kv8, pbl_decode_attn_kv8 and pbl_prefill_attn_kv8, the counterparts of
// pbl_rope_append_f16, pbl_decode_attn_f16 and pbl_prefill_attn_f16 over a cache whose rows are D bytes of OCP e4m3fn and one
// power-of-two scale each (the format and what it does with inf / NaN: pbl_kv8_format.h).
//
// The two append kernels quantise: the lanes that hold a row find its amax with lane shuffles (a row never straddles a wave), every
// lane converts its share and one of them writes the scale.  The two attention entries run the fp16 entries' kernels with another
// row loader (pbl_attn_kernels.h, pbl_prefill_kernels.h): same key-to-lane mapping, same reduction orders, same combine and advance
// kernels.  A dequantised value is an fp16 value and its scale a power of two, so each entry returns bit for bit what its fp16
// counterpart returns over a cache that holds the dequantised rows.
#include "pbl_attn_kernels.h"
#include "pbl_prefill_kernels.h"
#include "pbl_rope_math.h"

namespace {

// ---- RoPE + quantising append of a decode step (pbl_rope_append_kv8) -------------------------------------------------------------
struct RopeAppendKv8Args {
    RopeArgs r;                     // q / k as in pbl_rope_kernel (r.k_out unused); r.H = Hq + 2 Hkv: the v heads follow the k heads
    uint8_t* k_cache;               // [B, Hkv, max_len, D] e4m3fn
    uint8_t* v_cache;
    float* k_scale;                 // [B, Hkv, max_len]
    float* v_scale;
    const int64_t* pos;             // the layer's position: token (b, s) goes to cache row pos + s
    uint32_t v_off;
    int Hkv, max_len;
};

// pbl_rope_append_kernel with a quantising store: one (d, d + D/2) pair per thread, so the D/2 threads of a head are consecutive
// lanes of one wave (256-thread workgroups, D/2 = 32 or 64).  No thread leaves before the shuffles; the stores are guarded.
__global__ __launch_bounds__(256) void pbl_rope_append_kv8_kernel(RopeAppendKv8Args a) {
#pragma clang fp contract(off)
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const bool on = idx < a.r.pairs;
    const int pi = on ? idx : 0;
    const int i = pi % a.r.half, t = pi / a.r.half;
    const int h = t % a.r.H, m = t / a.r.H;
    const int b = m / a.r.S, s = m - b * a.r.S;
    const int D = 2 * a.r.half;
    const int64_t row = *a.pos + s;
    const bool isq = h < a.r.Hq, isv = h >= a.r.Hq + a.Hkv;
    const int hh = isq ? h : (isv ? h - a.r.Hq - a.Hkv : h - a.r.Hq);
    const uint16_t* x = a.r.qkv + size_t(m) * a.r.ld + (isq ? a.r.q_off : (isv ? a.v_off : a.r.k_off)) + size_t(hh) * D;
    const float x1 = float(__builtin_bit_cast(_Float16, x[i])), x2 = float(__builtin_bit_cast(_Float16, x[i + a.r.half]));
    float o1 = x1, o2 = x2;                                                  // a v head: as it is
    if (!isv) {
        const int64_t crow = b * a.r.c_sb + s * a.r.c_ss;
        const float c1 = float(__builtin_bit_cast(_Float16, a.r.cos[crow + i])), c2 = float(__builtin_bit_cast(_Float16, a.r.cos[crow + i + a.r.half]));
        const float s1 = float(__builtin_bit_cast(_Float16, a.r.sin[crow + i])), s2 = float(__builtin_bit_cast(_Float16, a.r.sin[crow + i + a.r.half]));
        o1 = float(_Float16(mul_f16(x1, c1) + mul_f16(-x2, s1)));           // rotate_half: (-x2, x1); fp32 sum, one rounding
        o2 = float(_Float16(mul_f16(x2, c2) + mul_f16(x1, s2)));
    }
    const float amax = kv8_group_max(fmaxf(fabsf(o1), fabsf(o2)), a.r.half);
    if (!on) return;
    if (isq) {
        uint16_t* out = a.r.q_out + (b * a.r.q_ob + hh * a.r.q_oh + s * a.r.q_os);
        out[i] = __builtin_bit_cast(uint16_t, _Float16(o1));
        out[i + a.r.half] = __builtin_bit_cast(uint16_t, _Float16(o2));
        return;
    }
    if (row < 0 || row >= a.max_len) return;
    float inv;
    const float scale = kv8_scale(amax, &inv);
    const uint32_t w = kv8_pack2(o1 * inv, o2 * inv);
    const size_t crow = (size_t(b) * a.Hkv + hh) * a.max_len + size_t(row);
    uint8_t* out = (isv ? a.v_cache : a.k_cache) + crow * D;
    out[i] = uint8_t(w & 0xffu);
    out[i + a.r.half] = uint8_t(w >> 8);
    if (i == 0) (isv ? a.v_scale : a.k_scale)[crow] = scale;
}

// ---- quantising append of a prefill (pbl_prefill_attn_kv8) --------------------------------------------------------------------------
struct AppendKv8Args {
    AppendArgs f;                   // k / v, their strides and vector flags, pos, S, Hkv, D, max_len (f.kc / f.vc unused)
    uint8_t* kc;                    // [B, Hkv, max_len, D] e4m3fn
    uint8_t* vc;
    float* ksc;                     // [B, Hkv, max_len]
    float* vsc;
};

// cache rows [p, p + S) <- quantised k_new / v_new: the D / 8 consecutive lanes of a (row, head) slice hold 8 values each (load8, with
// its scalar fallback for rows that are not 16-B aligned), find the row's amax together and store 8 bytes each
__global__ __launch_bounds__(PF_THREADS) void pbl_prefill_append_kv8_kernel(AppendKv8Args a) {
    const int cpr = a.f.D / 8;
    const int64_t e = int64_t(blockIdx.x) * PF_THREADS + threadIdx.x;
    const bool on = e < int64_t(a.f.S) * cpr;
    const int s = on ? int(e / cpr) : 0, ch = int(e % cpr), h = blockIdx.y, b = blockIdx.z;
    const int64_t row = clamped_pos(a.f.pos, a.f.max_len) + s;
    const uint4 kw = load8(a.f.k + b * a.f.k_sb + h * a.f.k_sh + s * a.f.k_ss + ch * 8, a.f.k_vec);
    const uint4 vw = load8(a.f.v + b * a.f.v_sb + h * a.f.v_sh + s * a.f.v_ss + ch * 8, a.f.v_vec);
    float kf[8], vf[8], ka = 0.f, va = 0.f;
    unpack8(kw, kf);
    unpack8(vw, vf);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        ka = fmaxf(ka, fabsf(kf[j]));
        va = fmaxf(va, fabsf(vf[j]));
    }
    ka = kv8_group_max(ka, cpr);
    va = kv8_group_max(va, cpr);
    if (!on || row >= a.f.max_len) return;
    float kinv, vinv;
    const float kscale = kv8_scale(ka, &kinv), vscale = kv8_scale(va, &vinv);
    uint32_t kb[4], vb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        kb[j] = kv8_pack2(kf[2 * j] * kinv, kf[2 * j + 1] * kinv);
        vb[j] = kv8_pack2(vf[2 * j] * vinv, vf[2 * j + 1] * vinv);
    }
    const size_t crow = (size_t(b) * a.f.Hkv + h) * a.f.max_len + size_t(row);
    *reinterpret_cast<uint2*>(a.kc + crow * a.f.D + size_t(ch) * 8) = make_uint2(kb[0] | (kb[1] << 16), kb[2] | (kb[3] << 16));
    *reinterpret_cast<uint2*>(a.vc + crow * a.f.D + size_t(ch) * 8) = make_uint2(vb[0] | (vb[1] << 16), vb[2] | (vb[3] << 16));
    if (ch == 0) {
        a.ksc[crow] = kscale;
        a.vsc[crow] = vscale;
    }
}

}  // namespace

extern "C" {

// pbl_rope_append_f16 with the FP8 cache as the destination of k and v: the same q_out (values, layout, bits); the rotated k heads
// and the raw v heads are quantised row by row (pbl_kv8_format.h) into rows [pos, pos + S) of k_cache / v_cache and their scales
// into the same rows of k_scale / v_scale.  Rows at or beyond max_len are not written; *pos is read on the device and not changed.
int pbl_rope_append_kv8(const void* qkv, uint32_t ld, uint32_t q_off, uint32_t k_off, uint32_t v_off, int B, int S, int Hq, int Hkv,
                        int D, const void* cos, const void* sin, int cos_dim, int64_t cos_sb, int64_t cos_ss, void* q_out,
                        const int64_t* q_ostride, void* k_cache, void* v_cache, void* k_scale, void* v_scale, int max_len,
                        const int64_t* pos, void* stream) {
    if (!qkv || !cos || !sin || !q_out || !q_ostride || !k_cache || !v_cache || !k_scale || !v_scale || !pos || B < 1 || S < 1 ||
        Hq < 1 || Hkv < 1 || D < 1 || cos_dim < 1 || cos_sb < 0 || cos_ss < 0 || max_len < 1)
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
    const size_t cacheb = size_t(int64_t(B) * Hkv * max_len * D), scaleb = size_t(int64_t(B) * Hkv * max_len * 4);
    const size_t xb = size_t(((M - 1) * ld + xend) * 2);
    const size_t cb = size_t(((B - 1) * cos_sb + (S - 1) * cos_ss + cos_dim) * 2);
    const void* outs[5] = {q_out, k_cache, v_cache, k_scale, v_scale};
    const size_t outb[5] = {qb, cacheb, cacheb, scaleb, scaleb};
    for (int j = 0; j < 5; ++j) {
        if (attn_overlaps(outs[j], outb[j], qkv, xb) || attn_overlaps(outs[j], outb[j], cos, cb) ||
            attn_overlaps(outs[j], outb[j], sin, cb) || attn_overlaps(outs[j], outb[j], pos, 8))
            return PBL_ERR_INVALID_ARG;
        for (int o = j + 1; o < 5; ++o)
            if (attn_overlaps(outs[j], outb[j], outs[o], outb[o])) return PBL_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale)) % 4) return PBL_ERR_MISALIGNED;
    if ((D != 64 && D != 128) || S > ATTN_MAX_S || B > ATTN_MAX_B || Hq % Hkv || cos_dim != D) return PBL_ERR_UNSUPPORTED;
    RopeAppendKv8Args a{};
    a.r.qkv = static_cast<const uint16_t*>(qkv);
    a.r.cos = static_cast<const uint16_t*>(cos); a.r.sin = static_cast<const uint16_t*>(sin);
    a.r.q_out = static_cast<uint16_t*>(q_out);
    a.r.c_sb = cos_sb; a.r.c_ss = cos_ss;
    a.r.q_ob = q_ostride[0]; a.r.q_oh = q_ostride[1]; a.r.q_os = q_ostride[2];
    a.r.ld = ld; a.r.q_off = q_off; a.r.k_off = k_off;
    a.r.S = S; a.r.Hq = Hq; a.r.H = Hq + 2 * Hkv; a.r.half = D / 2;
    a.r.pairs = int(M * (Hq + 2 * Hkv) * (D / 2));
    a.k_cache = static_cast<uint8_t*>(k_cache); a.v_cache = static_cast<uint8_t*>(v_cache);
    a.k_scale = static_cast<float*>(k_scale); a.v_scale = static_cast<float*>(v_scale);
    a.pos = pos; a.v_off = v_off; a.Hkv = Hkv; a.max_len = max_len;
    void* argv[] = {&a};
    return hipLaunchKernel(reinterpret_cast<const void*>(pbl_rope_append_kv8_kernel), dim3((a.r.pairs + 255) / 256), dim3(256), argv, 0,
                           static_cast<hipStream_t>(stream)) == hipSuccess ? PBL_OK : PBL_ERR_LAUNCH;
}

// pbl_decode_attn_f16 over the FP8 cache: the same kernels, split rule, reduction orders, workspace
// (pbl_decode_attn_workspace_bytes) and combine; a lane loads 8 bytes of a row and the row's scale.
int pbl_decode_attn_kv8(const void* q, const int64_t* q_stride, const void* k_cache, const void* v_cache, const void* k_scale,
                        const void* v_scale, int B, int S, int Hq, int Hkv, int D, int max_len, float scaling, int64_t* pos, void* out,
                        uint32_t ldo, void* ws, size_t ws_bytes, void* stream) {
    AttnArgsKv8 a{};
    a.ksc = static_cast<const float*>(k_scale);
    a.vsc = static_cast<const float*>(v_scale);
    const void* scales[2] = {k_scale, v_scale};
    const size_t scaleb = B < 1 || Hkv < 1 || max_len < 1 ? 0 : size_t(B) * Hkv * max_len * sizeof(float);
    const size_t scale_bytes[2] = {scaleb, scaleb};
    return attn_run(a, q, q_stride, k_cache, v_cache, size_t(D), scales, scale_bytes, 2, B, S, Hq, Hkv, D, max_len, scaling, pos, out, ldo,
                    ws, ws_bytes, stream);
}

// pbl_prefill_attn_f16 over the FP8 cache: k_new / v_new are quantised into cache rows [p, p + S), then pbl_prefill_attn_kernel
// attends with every key and value read back -- dequantised -- from the cache, and *pos advances by S.
int pbl_prefill_attn_kv8(const void* q, const int64_t* q_stride, const void* k_new, const int64_t* k_stride, const void* v_new,
                         const int64_t* v_stride, void* k_cache, void* v_cache, void* k_scale, void* v_scale, int B, int S, int Hq,
                         int Hkv, int D, int max_len, float scaling, int64_t* pos, void* out, uint32_t ldo, void* stream) {
    const void* scales[2] = {k_scale, v_scale};
    const int rc = prefill_check(q, q_stride, k_new, k_stride, v_new, v_stride, k_cache, v_cache, size_t(D), scales, 2, B, S, Hq, Hkv, D,
                                 max_len, pos, out, ldo);
    if (rc != PBL_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);

    AppendKv8Args ap{};
    ap.f.k = static_cast<const uint16_t*>(k_new); ap.f.v = static_cast<const uint16_t*>(v_new);
    ap.f.pos = pos;
    ap.f.k_sb = k_stride[0]; ap.f.k_sh = k_stride[1]; ap.f.k_ss = k_stride[2];
    ap.f.v_sb = v_stride[0]; ap.f.v_sh = v_stride[1]; ap.f.v_ss = v_stride[2];
    ap.f.S = S; ap.f.Hkv = Hkv; ap.f.D = D; ap.f.max_len = max_len;
    ap.f.k_vec = pf_vec(k_new, k_stride); ap.f.v_vec = pf_vec(v_new, v_stride);
    ap.kc = static_cast<uint8_t*>(k_cache); ap.vc = static_cast<uint8_t*>(v_cache);
    ap.ksc = static_cast<float*>(k_scale); ap.vsc = static_cast<float*>(v_scale);
    void* apv[] = {&ap};
    const unsigned ablocks = unsigned((int64_t(S) * (D / 8) + PF_THREADS - 1) / PF_THREADS);
    if (hipLaunchKernel(reinterpret_cast<const void*>(pbl_prefill_append_kv8_kernel), dim3(ablocks, Hkv, B), dim3(PF_THREADS), apv, 0, st) != hipSuccess)
        return PBL_ERR_LAUNCH;

    PrefillArgsKv8 a{};
    a.ksc = ap.ksc; a.vsc = ap.vsc;
    return prefill_attend(a, q, q_stride, k_cache, v_cache, B, S, Hq, Hkv, D, max_len, scaling, pos, out, ldo, st);
}

}  // extern "C"
