// pbl_prefill.hip -- causal prefill attention over a static KV cache (pbl_prefill_attn_f16).
//
// S new rows per sequence at the layer's device position p = *pos: pbl_prefill_append_kernel copies the rotated k rows and the raw v
// rows bit for bit into cache rows [p, p + S) (rows at or beyond max_len are dropped), pbl_prefill_attn_kernel attends, reading every
// key and value back from the cache -- a second chunk at p > 0 goes the way the first went --, and a one-thread launch advances *pos
// by S after everything that reads it has run.  Three launches in stream order, no workspace, no allocation, no host read of the
// position: one captured graph serves every position.
//
// Tiling.  One workgroup of four waves per (128 query rows, query head, batch entry); wave w owns query rows [32 w, 32 w + 32) of the
// tile.  Keys go in tiles of PF_TK = 64 rows laid from ABSOLUTE key row 0, the same for every launch; tiles wholly above the
// workgroup's (and, inside it, the wave's) diagonal are not visited, and the key range is not split.  A K tile lies in LDS as rows
// (padded by 16 B), a V tile TRANSPOSED ([d][key], 8-byte key groups XOR-swizzled so that the transposing writes and the operand
// reads spread over the banks); the next tile's global loads are in flight while the current one is multiplied.  Rows at or beyond
// min(p + S, max_len) enter LDS as zeros whatever the cache holds: a masked probability is 0, but 0 x NaN = NaN inside an MFMA.
//
// Products (v_mfma_f32_32x32x16_f16).  The first is K q^T -- K is the A operand, q^T the B operand --, so a lane holds the scores of
// ONE query (column lane & 31) against 16 keys of each 32-key block in its registers: row max and row sum are register loops plus
// one exchange with lane ^ 32, and the accumulator, rounded to fp16, IS the B operand of the second product O^T = V^T P^T with no
// trip through LDS.  Registers 8 s .. 8 s + 7 of a block form k-step s, whose element j of lane half h is key 16 s + 8 (j >> 2) +
// 4 h + (j & 3): the V^T operand is read from LDS in that k order (two 8-byte key groups per step).
//
// Numerics.  Scores are fp32 sums of fp16 products on the matrix cores.  The online softmax runs in fp32 over the key tiles (base 2:
// score x scaling x log2 e).  P is rounded to fp16 for the P V product and the denominator is summed from the ROUNDED P.  The
// accumulator is fp32; acc / l is rounded to fp16 once.  A fully masked tile is an exact no-op (p = 0, rescale factor 1), so a query
// row's result depends only on its own q, its keys and the 64-key tiling from row 0 -- not on which rows share its query tile, on S,
// or on how a prompt was chunked.  No atomics, fixed order: bit-stable from run to run, eager or replayed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pbl.h"

namespace {

typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int PF_THREADS = 256;
constexpr int PF_TQ = 128;                     // query rows per workgroup, 32 per wave
constexpr int PF_TK = 64;                      // keys per tile, laid from absolute key row 0
constexpr float PF_LOG2E = 1.4426950408889634f;

struct PrefillArgs {
    const uint16_t* q;              // element (b, h, s, d) at b * q_sb + h * q_sh + s * q_ss + d
    const uint16_t* kc;             // [B, Hkv, max_len, D]
    const uint16_t* vc;
    const int64_t* pos;
    uint16_t* out;                  // [B S, ldo]: row b S + s, head h at column h D
    int64_t q_sb, q_sh, q_ss;
    float scale_log2;               // scaling * log2(e)
    uint32_t ldo;
    int S, Hq, group, Hkv, max_len;
    int q_vec, o_vec;               // q rows 16-B aligned / out rows 8-B aligned: vector accesses
};

struct AppendArgs {
    const uint16_t* k;              // element (b, h, s, d) at b * sb + h * sh + s * ss + d
    const uint16_t* v;
    uint16_t* kc;
    uint16_t* vc;
    const int64_t* pos;
    int64_t k_sb, k_sh, k_ss, v_sb, v_sh, v_ss;
    int S, Hkv, D, max_len, k_vec, v_vec;
};

__device__ __forceinline__ int64_t clamped_pos(const int64_t* pos, int max_len) {
    const int64_t p = *pos;
    return p < 0 ? 0 : (p > max_len ? int64_t(max_len) : p);
}

__device__ __forceinline__ uint4 load8(const uint16_t* src, int vec) {
    if (vec) return *reinterpret_cast<const uint4*>(src);
    uint32_t u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = uint32_t(src[2 * j]) | (uint32_t(src[2 * j + 1]) << 16);
    return make_uint4(u[0], u[1], u[2], u[3]);
}

// cache rows [p, p + S) <- k_new / v_new, 16 bytes of each per thread
__global__ __launch_bounds__(PF_THREADS) void pbl_prefill_append_kernel(AppendArgs a) {
    const int cpr = a.D / 8;
    const int64_t e = int64_t(blockIdx.x) * PF_THREADS + threadIdx.x;
    if (e >= int64_t(a.S) * cpr) return;
    const int s = int(e / cpr), ch = int(e % cpr), h = blockIdx.y, b = blockIdx.z;
    const int64_t row = clamped_pos(a.pos, a.max_len) + s;
    if (row >= a.max_len) return;
    const size_t dst = ((size_t(b) * a.Hkv + h) * a.max_len + size_t(row)) * a.D + size_t(ch) * 8;
    *reinterpret_cast<uint4*>(a.kc + dst) = load8(a.k + b * a.k_sb + h * a.k_sh + s * a.k_ss + ch * 8, a.k_vec);
    *reinterpret_cast<uint4*>(a.vc + dst) = load8(a.v + b * a.v_sb + h * a.v_sh + s * a.v_ss + ch * 8, a.v_vec);
}

__global__ void pbl_prefill_advance_kernel(int64_t* pos, int S) {
    if (blockIdx.x == 0 && threadIdx.x == 0) pos[0] = pos[0] + S;
}

// the 8-byte key group `g` (0 .. 15) of row `row` of the transposed V tile sits at group g ^ vt_swizzle(row) of the row: the 16
// rows 8 c + j that one transposing write instruction touches, and the 32 consecutive rows that one operand read touches, land on
// different banks
__device__ __forceinline__ int vt_swizzle(int row) { return ((row >> 1) & 15) ^ ((row >> 5) & 3); }

template <int D>
__global__ __launch_bounds__(PF_THREADS) void pbl_prefill_attn_kernel(PrefillArgs a) {
    constexpr int KS = D / 16;                             // k-steps of the first product
    constexpr int DB = D / 32;                             // 32-row blocks of O^T
    constexpr int CPR = D / 8;                             // 16-byte chunks per cache row
    constexpr int KROW = D + 8;                            // halves per K row in LDS
    constexpr int KCH = PF_TK * CPR / PF_THREADS;          // K chunks per thread and tile
    constexpr int VITEMS = (PF_TK / 4) * CPR;              // (4 keys) x (8 columns) items of a V tile, one per thread
    static_assert(PF_TK * CPR % PF_THREADS == 0 && VITEMS <= PF_THREADS, "tile / thread mapping");
    __shared__ __attribute__((aligned(16))) uint16_t k_lds[PF_TK * KROW];
    __shared__ __attribute__((aligned(16))) uint16_t vt_lds[D * PF_TK];

    const int qt = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int hk = head / a.group;
    const int64_t p = clamped_pos(a.pos, a.max_len);
    const int64_t kend64 = p + a.S > a.max_len ? int64_t(a.max_len) : p + a.S;
    const int kend = int(kend64);                          // rows [0, kend) of the cache are valid
    const int q0 = qt * PF_TQ;
    const int last_q = q0 + PF_TQ - 1 < a.S - 1 ? q0 + PF_TQ - 1 : a.S - 1;
    const int64_t wg_lim = p + last_q < a.max_len - 1 ? p + last_q : int64_t(a.max_len - 1);
    const int nt = int(wg_lim / PF_TK) + 1;                // key tiles this workgroup visits
    const int wq0 = q0 + 32 * wave;
    const int wlast = wq0 + 31 < a.S - 1 ? wq0 + 31 : a.S - 1;
    const int64_t w_lim = p + wlast < a.max_len - 1 ? p + wlast : int64_t(a.max_len - 1);
    const int wnt = wq0 < a.S ? int(w_lim / PF_TK) + 1 : 0;        // ... and this wave multiplies
    const int sq = wq0 + r;                                 // this lane's query row
    const bool q_ok = sq < a.S;
    const int64_t lim64 = p + sq < a.max_len - 1 ? p + sq : int64_t(a.max_len - 1);
    const int lim = int(lim64);                             // its last key
    const size_t kvbase = (size_t(b) * a.Hkv + hk) * a.max_len;

    v8h qf[KS];
    {
        const uint16_t* qrow = a.q + b * a.q_sb + head * a.q_sh + int64_t(q_ok ? sq : 0) * a.q_ss;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const uint4 w = q_ok ? load8(qrow + ks * 16 + 8 * hh, a.q_vec) : make_uint4(0, 0, 0, 0);
            qf[ks] = __builtin_bit_cast(v8h, w);
        }
    }

    const int va = tid / CPR, vcc = tid % CPR;             // V item: keys 4 va .. 4 va + 3, columns 8 vcc .. 8 vcc + 7
    const bool v_on = tid < VITEMS;
    uint4 kreg[KCH], vreg[4];
    auto load_tile = [&](int t) {
        const int k0 = t * PF_TK;
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            const int ci = tid + PF_THREADS * i, key = k0 + ci / CPR, ch = ci % CPR;
            kreg[i] = key < kend ? *reinterpret_cast<const uint4*>(a.kc + (kvbase + key) * D + ch * 8) : make_uint4(0, 0, 0, 0);
        }
        if (v_on) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int key = k0 + 4 * va + i;
                vreg[i] = key < kend ? *reinterpret_cast<const uint4*>(a.vc + (kvbase + key) * D + vcc * 8) : make_uint4(0, 0, 0, 0);
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            const int ci = tid + PF_THREADS * i, key = ci / CPR, ch = ci % CPR;
            *reinterpret_cast<uint4*>(&k_lds[key * KROW + ch * 8]) = kreg[i];
        }
        if (v_on) {
            uint32_t u[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { u[i][0] = vreg[i].x; u[i][1] = vreg[i].y; u[i][2] = vreg[i].z; u[i][3] = vreg[i].w; }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int row = vcc * 8 + j, sh = 16 * (j & 1);
                uint2 w;
                w.x = ((u[0][j >> 1] >> sh) & 0xffffu) | (((u[1][j >> 1] >> sh) & 0xffffu) << 16);
                w.y = ((u[2][j >> 1] >> sh) & 0xffffu) | (((u[3][j >> 1] >> sh) & 0xffffu) << 16);
                *reinterpret_cast<uint2*>(&vt_lds[row * PF_TK + 4 * (va ^ vt_swizzle(row))]) = w;
            }
        }
    };

    v16f o[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int g = 0; g < 16; ++g) o[db][g] = 0.f;
    float m = -INFINITY, l = 0.f;                           // running max (base-2 scores) and this lane half's share of the sum

    load_tile(0);
    for (int t = 0; t < nt; ++t) {
        __syncthreads();                                    // the previous tile's reads are done
        store_tile();
        __syncthreads();
        if (t + 1 < nt) load_tile(t + 1);                   // in flight under this tile's products
        if (t >= wnt) continue;                             // wholly above this wave's diagonal (wave-uniform)
        const int k0 = t * PF_TK;
        v16f x[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int g = 0; g < 16; ++g) x[kb][g] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const v8h kf = *reinterpret_cast<const v8h*>(&k_lds[(kb * 32 + r) * KROW + ks * 16 + 8 * hh]);
                x[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], x[kb], 0, 0, 0);
            }
        }
        // x[kb][g]: key k0 + 32 kb + (g & 3) + 8 (g >> 2) + 4 hh against query sq
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int key = k0 + 32 * kb + (g & 3) + 8 * (g >> 2) + 4 * hh;
                const float sc = key <= lim ? x[kb][g] * a.scale_log2 : -INFINITY;
                x[kb][g] = sc;
                mx = fmaxf(mx, sc);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m, mx);                   // finite from tile 0 on: key 0 is valid for every row
        const float alpha = __builtin_amdgcn_exp2f(m - m_new);
        m = m_new;
        v8h pf[2][2];
        float lsum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const _Float16 ph = _Float16(__builtin_amdgcn_exp2f(x[kb][g] - m_new));
                pf[kb][g >> 3][g & 7] = ph;
                lsum += float(ph);                          // the denominator sees what the product sees
            }
        l = l * alpha + lsum;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
#pragma unroll
            for (int g = 0; g < 16; ++g) o[db][g] *= alpha;
            const int row = db * 32 + r, sw = vt_swizzle(row);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int g1 = kb * 8 + 4 * s + hh;     // keys 4 g1 .. 4 g1 + 3 (elements 0 - 3) and 4 (g1 + 2) .. (elements 4 - 7)
                    const uint2 lo = *reinterpret_cast<const uint2*>(&vt_lds[row * PF_TK + 4 * (g1 ^ sw)]);
                    const uint2 hi = *reinterpret_cast<const uint2*>(&vt_lds[row * PF_TK + 4 * ((g1 + 2) ^ sw)]);
                    const v8h vf = __builtin_bit_cast(v8h, make_uint4(lo.x, lo.y, hi.x, hi.y));
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[kb][s], o[db], 0, 0, 0);
                }
        }
    }

    // o[db][g]: column 32 db + (g & 3) + 8 (g >> 2) + 4 hh of query sq
    l += __shfl_xor(l, 32);
    if (!q_ok) return;
    uint16_t* orow = a.out + (size_t(b) * a.S + sq) * a.ldo + size_t(head) * D;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            uint16_t w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = __builtin_bit_cast(uint16_t, _Float16(o[db][4 * gq + j] / l));
            uint16_t* dst = orow + 32 * db + 8 * gq + 4 * hh;
            if (a.o_vec) {
                *reinterpret_cast<uint2*>(dst) = make_uint2(uint32_t(w[0]) | (uint32_t(w[1]) << 16), uint32_t(w[2]) | (uint32_t(w[3]) << 16));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) dst[j] = w[j];
            }
        }
}

bool pf_overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

size_t pf_extent(const int64_t* st, int B, int H, int S, int D) {      // bytes a strided [B, H, S, D] fp16 tensor spans
    return size_t((B - 1) * st[0] + int64_t(H - 1) * st[1] + int64_t(S - 1) * st[2] + D) * 2;
}

bool pf_vec(const void* p, const int64_t* st) {                         // every row starts on a 16-byte boundary
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && st[0] % 8 == 0 && st[1] % 8 == 0 && st[2] % 8 == 0;
}

}  // namespace

extern "C" {

int pbl_prefill_attn_f16(const void* q, const int64_t* q_stride, const void* k_new, const int64_t* k_stride, const void* v_new,
                         const int64_t* v_stride, void* k_cache, void* v_cache, int B, int S, int Hq, int Hkv, int D, int max_len,
                         float scaling, int64_t* pos, void* out, uint32_t ldo, void* stream) {
    if (!q || !q_stride || !k_new || !k_stride || !v_new || !v_stride || !k_cache || !v_cache || !pos || !out || B < 1 || S < 1 ||
        Hq < 1 || Hkv < 1 || D < 1 || max_len < 1 || int64_t(ldo) < int64_t(Hq) * D || S > max_len)
        return PBL_ERR_INVALID_ARG;
    for (int j = 0; j < 3; ++j)
        if (q_stride[j] < 0 || k_stride[j] < 0 || v_stride[j] < 0) return PBL_ERR_INVALID_ARG;
    if (double(B) * Hkv * double(max_len) * D > double(int64_t(1) << 40)) return PBL_ERR_INVALID_ARG;
    const size_t cacheb = size_t(B) * Hkv * max_len * D * 2;
    const size_t ob = size_t((int64_t(B) * S - 1) * ldo + int64_t(Hq) * D) * 2;
    const void* ins[3] = {q, k_new, v_new};
    const size_t inb[3] = {pf_extent(q_stride, B, Hq, S, D), pf_extent(k_stride, B, Hkv, S, D), pf_extent(v_stride, B, Hkv, S, D)};
    const void* outs[4] = {k_cache, v_cache, out, pos};
    const size_t outb[4] = {cacheb, cacheb, ob, 8};
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 3; ++j)
            if (pf_overlaps(outs[i], outb[i], ins[j], inb[j])) return PBL_ERR_INVALID_ARG;
        for (int j = i + 1; j < 4; ++j)
            if (pf_overlaps(outs[i], outb[i], outs[j], outb[j])) return PBL_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache)) % 16) return PBL_ERR_MISALIGNED;
    if ((D != 64 && D != 128) || Hq % Hkv || Hq > 65535 || B > 65535) return PBL_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);

    AppendArgs ap{};
    ap.k = static_cast<const uint16_t*>(k_new); ap.v = static_cast<const uint16_t*>(v_new);
    ap.kc = static_cast<uint16_t*>(k_cache); ap.vc = static_cast<uint16_t*>(v_cache);
    ap.pos = pos;
    ap.k_sb = k_stride[0]; ap.k_sh = k_stride[1]; ap.k_ss = k_stride[2];
    ap.v_sb = v_stride[0]; ap.v_sh = v_stride[1]; ap.v_ss = v_stride[2];
    ap.S = S; ap.Hkv = Hkv; ap.D = D; ap.max_len = max_len;
    ap.k_vec = pf_vec(k_new, k_stride); ap.v_vec = pf_vec(v_new, v_stride);
    void* apv[] = {&ap};
    const unsigned ablocks = unsigned((int64_t(S) * (D / 8) + PF_THREADS - 1) / PF_THREADS);
    if (hipLaunchKernel(reinterpret_cast<const void*>(pbl_prefill_append_kernel), dim3(ablocks, Hkv, B), dim3(PF_THREADS), apv, 0, st) != hipSuccess)
        return PBL_ERR_LAUNCH;

    PrefillArgs a{};
    a.q = static_cast<const uint16_t*>(q);
    a.kc = ap.kc; a.vc = ap.vc;
    a.pos = pos;
    a.out = static_cast<uint16_t*>(out);
    a.q_sb = q_stride[0]; a.q_sh = q_stride[1]; a.q_ss = q_stride[2];
    a.scale_log2 = scaling * PF_LOG2E;
    a.ldo = ldo;
    a.S = S; a.Hq = Hq; a.group = Hq / Hkv; a.Hkv = Hkv; a.max_len = max_len;
    a.q_vec = pf_vec(q, q_stride);
    a.o_vec = reinterpret_cast<uintptr_t>(out) % 8 == 0 && ldo % 4 == 0;
    void* argv[] = {&a};
    const void* kern = D == 64 ? reinterpret_cast<const void*>(pbl_prefill_attn_kernel<64>)
                               : reinterpret_cast<const void*>(pbl_prefill_attn_kernel<128>);
    if (hipLaunchKernel(kern, dim3((S + PF_TQ - 1) / PF_TQ, Hq, B), dim3(PF_THREADS), argv, 0, st) != hipSuccess) return PBL_ERR_LAUNCH;
    int S_arg = S;
    void* adv[] = {&pos, &S_arg};
    return hipLaunchKernel(reinterpret_cast<const void*>(pbl_prefill_advance_kernel), dim3(1), dim3(1), adv, 0, st) == hipSuccess
               ? PBL_OK : PBL_ERR_LAUNCH;
}

}  // extern "C"
