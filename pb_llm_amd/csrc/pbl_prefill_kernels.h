// pbl_prefill_kernels.h -- the kernels and launch helpers of the causal prefill attention, shared by its two cache formats: fp16 rows
// (pbl_prefill.hip, pbl_prefill_attn_f16; the design is described there) and FP8 rows with one power-of-two scale each (pbl_kv8.hip,
// pbl_prefill_attn_kv8).  pbl_prefill_attn_kernel is ONE template: the cache format changes how a tile's rows come out of global
// memory (PrefillChunk) and nothing else -- the LDS layouts, the products, the softmax and the store exist once.  Which keys at or
// below a row's diagonal it sees is a mask policy: CausalMask (all of them: the two prefill entries) or BranchMask (pbl_branch.hip,
// pbl_branch_attn_f16: the rows of several continuations packed behind one shared context).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pbl.h"
#include "pbl_kv8_format.h"

namespace {

typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int PF_THREADS = 256;
constexpr int PF_TQ = 128;                     // query rows per workgroup, 32 per wave
constexpr int PF_TK = 64;                      // keys per tile, laid from absolute key row 0
constexpr float PF_LOG2E = 1.4426950408889634f;
constexpr float PF_P_OFFSET = 14.f;            // P = exp2(x - fl(m - 14)): the row's maximum at 2^14 (pbl_prefill.hip, Numerics)

struct PrefillArgs {
    const uint16_t* q;              // element (b, h, s, d) at b * q_sb + h * q_sh + s * q_ss + d
    const void* kc;                 // [B, Hkv, max_len, D] fp16, or e4m3fn bytes (PrefillArgsKv8)
    const void* vc;
    const int64_t* pos;
    uint16_t* out;                  // [B S, ldo]: row b S + s, head h at column h D
    int64_t q_sb, q_sh, q_ss;
    float scale_log2;               // scaling * log2(e)
    uint32_t ldo;
    int S, Hq, group, Hkv, max_len;
    int q_vec, o_vec;               // q rows 16-B aligned / out rows 8-B aligned: vector accesses
};

struct PrefillArgsKv8 : PrefillArgs {
    const float* ksc;               // [B, Hkv, max_len]: the power-of-two scale of each K / V row
    const float* vsc;
};

struct PrefillArgsBranch : PrefillArgs {
    const int32_t* trunk;           // [B]: keys below p + trunk[b] are seen by every row of batch entry b
    const int32_t* lo;              // [B, S]: row s also sees keys from p + lo[b, s] on (its own branch), up to its diagonal
};

template <typename Args> struct prefill_is_kv8 { static constexpr bool value = false; };
template <> struct prefill_is_kv8<PrefillArgsKv8> { static constexpr bool value = true; };

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

// 8 e4m3fn bytes of a row and the row's scale -> the 8 fp16 values they stand for (exact: pbl_kv8_format.h)
__device__ __forceinline__ uint4 kv8_to_halves(const uint2 w, const float scale) {
    float f[8];
    kv8_unpack8(w, f);
    uint32_t u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        u[j] = uint32_t(__builtin_bit_cast(uint16_t, _Float16(f[2 * j] * scale))) |
               (uint32_t(__builtin_bit_cast(uint16_t, _Float16(f[2 * j + 1] * scale))) << 16);
    return make_uint4(u[0], u[1], u[2], u[3]);
}

// what a thread keeps of a cache row between the tile's global load and its LDS store: 16 bytes of fp16, or 8 bytes of e4m3fn and
// the row's scale, turned into the same 8 halves when the tile is stored (so that the conversion does not wait for the load)
template <bool KV8> struct PrefillChunk;
template <> struct PrefillChunk<false> {
    uint4 w;
    __device__ __forceinline__ void load(const void* cache, const float*, size_t row, int D, int ch, bool on) {
        w = on ? *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(cache) + row * D + ch * 8) : make_uint4(0, 0, 0, 0);
    }
    __device__ __forceinline__ uint4 halves() const { return w; }
};
template <> struct PrefillChunk<true> {
    uint2 w;
    float scale;
    __device__ __forceinline__ void load(const void* cache, const float* scales, size_t row, int D, int ch, bool on) {
        w = on ? *reinterpret_cast<const uint2*>(static_cast<const uint8_t*>(cache) + row * D + ch * 8) : make_uint2(0, 0);
        scale = on ? scales[row] : 0.f;
    }
    __device__ __forceinline__ uint4 halves() const { return kv8_to_halves(w, scale); }
};

// The mask policy: which keys at or below its diagonal a query row sees.  CausalMask: all of them -- nothing is computed, the kernel is
// what it was before the policy existed.
struct CausalMask {
    static constexpr bool finite_v = false;
    template <typename Args> __device__ __forceinline__ void init(const Args&, int, int, bool, int64_t) {}
    __device__ __forceinline__ bool sees(int) const { return true; }
};

// BranchMask: key k iff k < p + trunk[b] (the shared context) or k >= p + lo[b, s] (the row's own branch).  The tables are made safe
// here: lo is clamped to [0, s] (a row always sees itself, and no index leaves [p, p + S)), p + trunk to [1, max_len] -- key 0 is
// seen by every row whatever the tables hold, which the online softmax relies on (the running maximum is finite from tile 0).
// Kept as tr = p + trunk and gap = the number of keys from tr on that the row does NOT see (0 where its branch starts at or below
// tr): key k is seen iff unsigned(k - tr) >= gap -- one subtraction and one comparison per score.
struct BranchMask {
    static constexpr bool finite_v = true;
    int tr;
    unsigned gap;
    __device__ __forceinline__ void init(const PrefillArgsBranch& a, int b, int sq, bool q_ok, int64_t p) {
        int64_t t = p + int64_t(a.trunk[b]);
        tr = int(t < 1 ? 1 : (t > a.max_len ? int64_t(a.max_len) : t));
        int l = q_ok ? a.lo[size_t(b) * a.S + sq] : 0;
        l = l < 0 ? 0 : (l > sq ? sq : l);
        const int64_t la = p + l;
        gap = la > tr ? unsigned(la - tr) : 0u;
    }
    __device__ __forceinline__ bool sees(int key) const { return unsigned(key - tr) >= gap; }
};

// 8 halves with every Inf / NaN among them replaced by +0 (BranchMask's V tiles: a masked probability is 0, but 0 x NaN = NaN inside
// an MFMA, and a V tile is shared by rows that see a key and rows that do not)
__device__ __forceinline__ uint4 finite_halves(uint4 w) {
    auto flags = [](uint32_t x) { return ((x & 0x7c007c00u) + 0x04000400u) & 0x80008000u; };   // bit 15 of a half: exponent all ones
    if ((flags(w.x) | flags(w.y) | flags(w.z) | flags(w.w)) == 0) return w;
    auto clear = [&](uint32_t x) { const uint32_t f = flags(x); return x & ~((f - (f >> 15)) | f); };
    return make_uint4(clear(w.x), clear(w.y), clear(w.z), clear(w.w));
}

// Args: PrefillArgs (fp16 cache), PrefillArgsKv8 (FP8 cache: only the tile loader differs) or PrefillArgsBranch (with BranchMask)
template <int D, typename Args, typename Mask = CausalMask>
__global__ __launch_bounds__(PF_THREADS) void pbl_prefill_attn_kernel(Args a) {
    constexpr bool KV8 = prefill_is_kv8<Args>::value;
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
    Mask mask;
    mask.init(a, b, sq, q_ok, p);

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
    const float* ksc = nullptr;
    const float* vsc = nullptr;
    if constexpr (KV8) {
        ksc = a.ksc;
        vsc = a.vsc;
    }
    PrefillChunk<KV8> kreg[KCH], vreg[4];
    auto load_tile = [&](int t) {
        const int k0 = t * PF_TK;
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            const int ci = tid + PF_THREADS * i, key = k0 + ci / CPR, ch = ci % CPR;
            kreg[i].load(a.kc, ksc, kvbase + key, D, ch, key < kend);
        }
        if (v_on) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int key = k0 + 4 * va + i;
                vreg[i].load(a.vc, vsc, kvbase + key, D, vcc, key < kend);
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            const int ci = tid + PF_THREADS * i, key = ci / CPR, ch = ci % CPR;
            *reinterpret_cast<uint4*>(&k_lds[key * KROW + ch * 8]) = kreg[i].halves();
        }
        if (v_on) {
            uint32_t u[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint4 w = vreg[i].halves();
                if constexpr (Mask::finite_v) w = finite_halves(w);
                u[i][0] = w.x; u[i][1] = w.y; u[i][2] = w.z; u[i][3] = w.w;
            }
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
    float m_p = -INFINITY;                                  // what P, l and o are relative to: m - 14, rounded (below)

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
                const float sc = key <= lim && mask.sees(key) ? x[kb][g] * a.scale_log2 : -INFINITY;
                x[kb][g] = sc;
                mx = fmaxf(mx, sc);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m, mx);                   // finite from tile 0 on: key 0 is valid for every row
        m = m_new;
        // P, l and o are kept relative to m_p = fl(m - 14), not to m: fp16's normal range then reaches down to 2^-28 of the row's
        // maximum.  The subtraction is rounded to fp32; where that rounding would put the maximum above 2^15 (|m - 14| >= 2^25: fp32's
        // spacing is 4 or more) the offset is dropped, so P <= 2^15 < 65504 whatever the scores.  alpha comes from the same m_p, so
        // every tile's contribution is scaled by 2^-m_p exactly, however the rounding falls from tile to tile.
        float m_p_new = m_new - PF_P_OFFSET;
        if (m_new - m_p_new > PF_P_OFFSET + 1.f) m_p_new = m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_p - m_p_new);
        m_p = m_p_new;
        v8h pf[2][2];
        float lsum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const _Float16 ph = _Float16(__builtin_amdgcn_exp2f(x[kb][g] - m_p));
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

// The checks every prefill entry makes before any device work.  cache_row_bytes: what a cache row of D values takes; scales: the
// n_scales further outputs of scale_bytes each (the FP8 cache's scale arrays), which must not overlap anything either.
int prefill_check(const void* q, const int64_t* q_stride, const void* k_new, const int64_t* k_stride, const void* v_new,
                  const int64_t* v_stride, const void* k_cache, const void* v_cache, size_t cache_row_bytes, const void* const* scales,
                  int n_scales, int B, int S, int Hq, int Hkv, int D, int max_len, const int64_t* pos, const void* out, uint32_t ldo) {
    if (!q || !q_stride || !k_new || !k_stride || !v_new || !v_stride || !k_cache || !v_cache || !pos || !out || B < 1 || S < 1 ||
        Hq < 1 || Hkv < 1 || D < 1 || max_len < 1 || int64_t(ldo) < int64_t(Hq) * D || S > max_len)
        return PBL_ERR_INVALID_ARG;
    for (int j = 0; j < n_scales; ++j)
        if (!scales[j]) return PBL_ERR_INVALID_ARG;
    for (int j = 0; j < 3; ++j)
        if (q_stride[j] < 0 || k_stride[j] < 0 || v_stride[j] < 0) return PBL_ERR_INVALID_ARG;
    if (double(B) * Hkv * double(max_len) * D > double(int64_t(1) << 40)) return PBL_ERR_INVALID_ARG;
    const size_t cacheb = size_t(B) * Hkv * max_len * cache_row_bytes;
    const size_t ob = size_t((int64_t(B) * S - 1) * ldo + int64_t(Hq) * D) * 2;
    const void* ins[3] = {q, k_new, v_new};
    const size_t inb[3] = {pf_extent(q_stride, B, Hq, S, D), pf_extent(k_stride, B, Hkv, S, D), pf_extent(v_stride, B, Hkv, S, D)};
    const void* outs[6] = {k_cache, v_cache, out, pos};
    size_t outb[6] = {cacheb, cacheb, ob, 8};
    const int n_out = 4 + (n_scales < 2 ? n_scales : 2);
    for (int j = 4; j < n_out; ++j) {
        outs[j] = scales[j - 4];
        outb[j] = size_t(B) * Hkv * max_len * sizeof(float);
    }
    for (int i = 0; i < n_out; ++i) {
        for (int j = 0; j < 3; ++j)
            if (pf_overlaps(outs[i], outb[i], ins[j], inb[j])) return PBL_ERR_INVALID_ARG;
        for (int j = i + 1; j < n_out; ++j)
            if (pf_overlaps(outs[i], outb[i], outs[j], outb[j])) return PBL_ERR_INVALID_ARG;
    }
    if ((reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache)) % 16) return PBL_ERR_MISALIGNED;
    for (int j = 0; j < n_scales; ++j)
        if (reinterpret_cast<uintptr_t>(scales[j]) % 4) return PBL_ERR_MISALIGNED;
    if ((D != 64 && D != 128) || Hq % Hkv || Hq > 65535 || B > 65535) return PBL_ERR_UNSUPPORTED;
    return PBL_OK;
}

// the fp16 cache's append launch: k_new / v_new bit for bit into cache rows [p, p + S)
int prefill_append(const void* k_new, const int64_t* k_stride, const void* v_new, const int64_t* v_stride, void* k_cache, void* v_cache,
                   int B, int S, int Hkv, int D, int max_len, const int64_t* pos, hipStream_t st) {
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
    return hipLaunchKernel(reinterpret_cast<const void*>(pbl_prefill_append_kernel), dim3(ablocks, Hkv, B), dim3(PF_THREADS), apv, 0, st) == hipSuccess
               ? PBL_OK : PBL_ERR_LAUNCH;
}

// the attention launch over the cache rows that the entry's append launch has written, and the advance of *pos; the caller has put
// into `a` what its cache format adds to PrefillArgs
template <typename Mask = CausalMask, typename Args>
int prefill_attend(Args& a, const void* q, const int64_t* q_stride, const void* k_cache, const void* v_cache, int B, int S, int Hq,
                   int Hkv, int D, int max_len, float scaling, int64_t* pos, void* out, uint32_t ldo, hipStream_t st) {
    a.q = static_cast<const uint16_t*>(q);
    a.kc = k_cache; a.vc = v_cache;
    a.pos = pos;
    a.out = static_cast<uint16_t*>(out);
    a.q_sb = q_stride[0]; a.q_sh = q_stride[1]; a.q_ss = q_stride[2];
    a.scale_log2 = scaling * PF_LOG2E;
    a.ldo = ldo;
    a.S = S; a.Hq = Hq; a.group = Hq / Hkv; a.Hkv = Hkv; a.max_len = max_len;
    a.q_vec = pf_vec(q, q_stride);
    a.o_vec = reinterpret_cast<uintptr_t>(out) % 8 == 0 && ldo % 4 == 0;
    void* argv[] = {&a};
    const void* kern = D == 64 ? reinterpret_cast<const void*>(pbl_prefill_attn_kernel<64, Args, Mask>)
                               : reinterpret_cast<const void*>(pbl_prefill_attn_kernel<128, Args, Mask>);
    if (hipLaunchKernel(kern, dim3((S + PF_TQ - 1) / PF_TQ, Hq, B), dim3(PF_THREADS), argv, 0, st) != hipSuccess) return PBL_ERR_LAUNCH;
    int S_arg = S;
    void* adv[] = {&pos, &S_arg};
    return hipLaunchKernel(reinterpret_cast<const void*>(pbl_prefill_advance_kernel), dim3(1), dim3(1), adv, 0, st) == hipSuccess
               ? PBL_OK : PBL_ERR_LAUNCH;
}

}  // namespace
