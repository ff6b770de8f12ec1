// pbl_attn_kernels.h -- the kernels and launch plan of the decode attention, shared by its two cache formats: fp16 rows
// (pbl_attn.hip, pbl_decode_attn_f16) and FP8 rows with one power-of-two scale each (pbl_kv8.hip, pbl_decode_attn_kv8).  The
// partial kernel is ONE template: the cache format changes what a lane loads (16 bytes of fp16, or 8 bytes of e4m3fn and the row's
// scale) and nothing else -- which lane sums which keys, every reduction order, the workspace layout and the combine kernel are the
// same, so the FP8 kernel gives bit for bit the fp16 kernel's result over a cache that holds the dequantised rows.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pbl.h"
#include "pbl_kv8_format.h"

namespace {

constexpr int ATTN_THREADS = 256;
constexpr int ATTN_MAX_S = 4;
constexpr int ATTN_MAX_B = 4;
constexpr int ATTN_KEYS_PER_SPLIT = 32;        // the chunk grows in steps of this so that nsplit <= ATTN_MAX_SPLITS
constexpr int ATTN_MAX_SPLITS = 128;
constexpr int ATTN_MAX_CHUNK = 512;            // max_len <= 512 * 128
constexpr int ATTN_ROWS_IN_FLIGHT = 4;         // fp16 K / V rows a lane loads before it uses the first
constexpr int ATTN_ROWS_IN_FLIGHT_KV8 = 8;     // FP8 rows: twice as many, the same bytes in flight

struct AttnArgs {
    const uint16_t* q;              // element (b, h, s, d) at b * q_sb + h * q_sh + s * q_ss + d
    const void* kc;                 // [B, Hkv, max_len, D] fp16, or e4m3fn bytes (AttnArgsKv8)
    const void* vc;
    const int64_t* pos;
    float* part_ml;                 // [B, Hq, S, nsplit] x {m, l}
    float* part_acc;                // [B, Hq, S, nsplit, D]
    int64_t q_sb, q_sh, q_ss;
    float scaling;
    int S, Hq, group, Hkv, max_len, chunk, nsplit;
};

struct AttnArgsKv8 : AttnArgs {
    const float* ksc;               // [B, Hkv, max_len]: the power-of-two scale of each K / V row
    const float* vsc;
};

template <typename Args> struct attn_is_kv8 { static constexpr bool value = false; };
template <> struct attn_is_kv8<AttnArgsKv8> { static constexpr bool value = true; };

__device__ __forceinline__ void unpack8(const uint4 w, float* f) {
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = float(__builtin_bit_cast(_Float16, uint16_t(u[j] & 0xffffu)));
        f[2 * j + 1] = float(__builtin_bit_cast(_Float16, uint16_t(u[j] >> 16)));
    }
}

// one lane's slice of a cache row: 8 values as the row format stores them
template <bool KV8> struct AttnRow;
template <> struct AttnRow<false> {
    uint4 w;
    __device__ __forceinline__ void load(const void* cache, const float*, size_t row, int D, int li, bool on) {
        w = on ? *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(cache) + row * D + li * 8) : make_uint4(0, 0, 0, 0);
    }
    __device__ __forceinline__ void values(float* f) const { unpack8(w, f); }
};
template <> struct AttnRow<true> {
    uint2 w;
    float scale;                    // read once per key row and lane, not per element
    __device__ __forceinline__ void load(const void* cache, const float* scales, size_t row, int D, int li, bool on) {
        w = on ? *reinterpret_cast<const uint2*>(static_cast<const uint8_t*>(cache) + row * D + li * 8) : make_uint2(0, 0);
        scale = on ? scales[row] : 0.f;
    }
    __device__ __forceinline__ void values(float* f) const { kv8_unpack8(w, f); }      // the bytes' values, unscaled
};

template <int D, typename Args>
__global__ __launch_bounds__(ATTN_THREADS) void pbl_attn_partial_kernel(Args a) {
    constexpr bool KV8 = attn_is_kv8<Args>::value;
    constexpr int RIF = KV8 ? ATTN_ROWS_IN_FLIGHT_KV8 : ATTN_ROWS_IN_FLIGHT;
    constexpr int LPK = D / 8;                     // lanes per key row, 8 values each
    constexpr int KP = ATTN_THREADS / LPK;         // keys per pass of the workgroup
    __shared__ float sc[ATTN_MAX_S][ATTN_MAX_CHUNK];
    __shared__ float red[ATTN_THREADS / 64][ATTN_MAX_S * D];
    __shared__ float ml[ATTN_MAX_S][2];
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = tid % LPK, kg = tid / LPK;
    const int hk = h / a.group;
    int64_t pos = *a.pos;
    if (pos < 0) pos = 0;
    const int64_t k0 = int64_t(split) * a.chunk;
    int64_t kend = pos + a.S;
    if (kend > a.max_len) kend = a.max_len;
    const int64_t left = kend - k0;
    const int n = left <= 0 ? 0 : (left > a.chunk ? a.chunk : int(left));
    const size_t row0 = (size_t(b) * a.Hq + h) * a.S * a.nsplit + split;      // partial (b, h, s, split) at row0 + s * nsplit
    if (n == 0) {                                                               // no key of this split is valid for any row
        if (tid < a.S) {
            a.part_ml[(row0 + size_t(tid) * a.nsplit) * 2] = -INFINITY;
            a.part_ml[(row0 + size_t(tid) * a.nsplit) * 2 + 1] = 0.f;
        }
        for (int e = tid; e < a.S * D; e += ATTN_THREADS)                      // (the combine weighs it by 0: no branch there)
            a.part_acc[(row0 + size_t(e / D) * a.nsplit) * D + e % D] = 0.f;
        return;
    }
    float qv[ATTN_MAX_S][8];
#pragma unroll
    for (int s = 0; s < ATTN_MAX_S; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            qv[s][j] = s < a.S ? float(__builtin_bit_cast(_Float16, a.q[b * a.q_sb + h * a.q_sh + s * a.q_ss + li * 8 + j])) : 0.f;
    const size_t kvbase = (size_t(b) * a.Hkv + hk) * a.max_len + k0;
    const float* ksc = nullptr;
    const float* vsc = nullptr;
    if constexpr (KV8) {
        ksc = a.ksc;
        vsc = a.vsc;
    }

    // scores: key kk of the split is read by lanes [kg * LPK, kg * LPK + LPK) -- an 8-value slice each, reduced across those lanes.
    // RIF rows per lane are loaded before the first is used.
    for (int kk0 = 0; kk0 < n; kk0 += RIF * KP) {
        AttnRow<KV8> kw[RIF];
#pragma unroll
        for (int u = 0; u < RIF; ++u) {
            const int kk = kk0 + u * KP + kg;
            kw[u].load(a.kc, ksc, kvbase + kk, D, li, kk < n);
        }
#pragma unroll
        for (int u = 0; u < RIF; ++u) {
            const int kk = kk0 + u * KP + kg;
            float kf[8], d[ATTN_MAX_S] = {0.f, 0.f, 0.f, 0.f};
            kw[u].values(kf);
#pragma unroll
            for (int s = 0; s < ATTN_MAX_S; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) d[s] += qv[s][j] * kf[j];
#pragma unroll
            for (int off = LPK / 2; off >= 1; off >>= 1)
#pragma unroll
                for (int s = 0; s < ATTN_MAX_S; ++s) d[s] += __shfl_xor(d[s], off);
            if (li == 0 && kk < n)
                for (int s = 0; s < a.S; ++s) {
                    float ds = d[s];
                    if constexpr (KV8) ds *= kw[u].scale;      // exact: a power of two, and every sum above scales with it
                    sc[s][kk] = k0 + kk <= pos + s ? ds * a.scaling : -INFINITY;   // causal inside the S rows
                }
        }
    }
    __syncthreads();

    // softmax of the split, one wave per query row: m = max, p = exp(score - m) kept in place, l = sum p
    if (wave < a.S) {
        const int s = wave;
        float m = -INFINITY;
        for (int kk = lane; kk < n; kk += 64) m = fmaxf(m, sc[s][kk]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        float l = 0.f;
        for (int kk = lane; kk < n; kk += 64) {
            const float p = m == -INFINITY ? 0.f : expf(sc[s][kk] - m);
            sc[s][kk] = p;
            l += p;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) l += __shfl_xor(l, off);
        if (lane == 0) {
            ml[s][0] = m;
            ml[s][1] = l;
        }
    }
    __syncthreads();

    // acc = sum_k p_k V_k: each lane an 8-value slice of its keys' V rows, then the key groups of a wave (shuffles), then the waves (LDS)
    float acc[ATTN_MAX_S][8];
#pragma unroll
    for (int s = 0; s < ATTN_MAX_S; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[s][j] = 0.f;
    for (int kk0 = 0; kk0 < n; kk0 += RIF * KP) {
        AttnRow<KV8> vw[RIF];
#pragma unroll
        for (int u = 0; u < RIF; ++u) {
            const int kk = kk0 + u * KP + kg;
            vw[u].load(a.vc, vsc, kvbase + kk, D, li, kk < n);
        }
#pragma unroll
        for (int u = 0; u < RIF; ++u) {
            const int kk = kk0 + u * KP + kg;
            if (kk < n) {
                float vf[8];
                vw[u].values(vf);
                if constexpr (KV8) {
                    // the scale goes on the V element, where it is exact for every p: on p, a p below 2^-111 would lose bits
#pragma unroll
                    for (int j = 0; j < 8; ++j) vf[j] *= vw[u].scale;
                }
#pragma unroll
                for (int s = 0; s < ATTN_MAX_S; ++s) {
                    const float p = s < a.S ? sc[s][kk] : 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[s][j] += p * vf[j];
                }
            }
        }
    }
#pragma unroll
    for (int off = LPK; off < 64; off <<= 1)
#pragma unroll
        for (int s = 0; s < ATTN_MAX_S; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[s][j] += __shfl_xor(acc[s][j], off);
    if (lane < LPK)
        for (int s = 0; s < a.S; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) red[wave][s * D + li * 8 + j] = acc[s][j];
    __syncthreads();
    for (int e = tid; e < a.S * D; e += ATTN_THREADS) {
        const float v = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
        const int s = e / D, dd = e - s * D;
        a.part_acc[(row0 + size_t(s) * a.nsplit) * D + dd] = v;
    }
    if (tid < a.S) {
        a.part_ml[(row0 + size_t(tid) * a.nsplit) * 2] = ml[tid][0];
        a.part_ml[(row0 + size_t(tid) * a.nsplit) * 2 + 1] = ml[tid][1];
    }
}

struct CombineArgs {
    const float* part_ml;
    const float* part_acc;
    uint16_t* out;                  // [B S, ldo]: row b S + s, head h at column h D
    int64_t* pos;
    uint32_t ldo;
    int S, Hq, D, nsplit;
};

// one workgroup per (s, h, b) query row, one lane per output column; splits merged in split order.  The weights exp(m_i - M) are
// found once per workgroup (one lane per split), so the merge of acc is a branch-free stream of independent loads.  The partial
// launch has finished reading the position, and nothing here reads it: workgroup (0, 0, 0) advances it by S.
__global__ __launch_bounds__(ATTN_MAX_SPLITS) void pbl_attn_combine_kernel(CombineArgs a) {
    __shared__ float w[ATTN_MAX_SPLITS], lw[ATTN_MAX_SPLITS], wmax[ATTN_MAX_SPLITS / 64];
    const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    const size_t row0 = ((size_t(b) * a.Hq + h) * a.S + s) * a.nsplit;
    float m = -INFINITY, l = 0.f;
    if (t < a.nsplit) {
        l = a.part_ml[(row0 + t) * 2 + 1];
        if (l > 0.f) m = a.part_ml[(row0 + t) * 2];
    }
    float M = m;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) M = fmaxf(M, __shfl_xor(M, off));
    if ((t & 63) == 0) wmax[t >> 6] = M;
    __syncthreads();
    M = wmax[0];
#pragma unroll
    for (int i = 1; i < ATTN_MAX_SPLITS / 64; ++i) M = fmaxf(M, wmax[i]);
    const float wi = l > 0.f ? expf(m - M) : 0.f;
    w[t] = wi;
    lw[t] = l * wi;
    __syncthreads();
    if (t < a.D) {
        float L = 0.f, acc = 0.f;
#pragma unroll 8
        for (int i = 0; i < a.nsplit; ++i) {
            L += lw[i];
            acc += a.part_acc[(row0 + i) * a.D + t] * w[i];
        }
        a.out[(size_t(b) * a.S + s) * a.ldo + size_t(h) * a.D + t] = __builtin_bit_cast(uint16_t, _Float16(acc / L));
    }
    if (s == 0 && h == 0 && b == 0 && t == 0) a.pos[0] = a.pos[0] + a.S;
}

int attn_chunk(int max_len) {
    const int per = ATTN_KEYS_PER_SPLIT * ATTN_MAX_SPLITS;
    return ATTN_KEYS_PER_SPLIT * ((max_len + per - 1) / per);
}

bool attn_overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

size_t attn_workspace_bytes(int B, int S, int Hq, int D, int max_len) {
    if (B < 1 || S < 1 || Hq < 1 || D < 1 || max_len < 1) return 0;
    const int chunk = attn_chunk(max_len);
    const size_t nsplit = size_t((max_len + chunk - 1) / chunk);
    return size_t(B) * Hq * S * nsplit * (2 + size_t(D)) * sizeof(float);
}

// The checks and the two launches of a decode attention call; the cache format enters through cache_row_bytes (what a row of D
// values takes), through `extra` (n_extra further input buffers that the outputs must not overlap: the scale arrays) and through
// what the caller has already put into `a` beyond AttnArgs.
template <typename Args>
int attn_run(Args& a, const void* q, const int64_t* q_stride, const void* k_cache, const void* v_cache, size_t cache_row_bytes,
             const void* const* extra, const size_t* extra_bytes, int n_extra, int B, int S, int Hq, int Hkv, int D, int max_len,
             float scaling, int64_t* pos, void* out, uint32_t ldo, void* ws, size_t ws_bytes, void* stream) {
    if (!q || !q_stride || !k_cache || !v_cache || !pos || !out || !ws || B < 1 || S < 1 || Hq < 1 || Hkv < 1 || D < 1 ||
        max_len < 1 || int64_t(ldo) < int64_t(Hq) * D)
        return PBL_ERR_INVALID_ARG;
    for (int j = 0; j < n_extra; ++j)
        if (!extra[j]) return PBL_ERR_INVALID_ARG;
    for (int j = 0; j < 3; ++j)
        if (q_stride[j] < 0) return PBL_ERR_INVALID_ARG;
    const size_t need = attn_workspace_bytes(B, S, Hq, D, max_len);
    if (ws_bytes < need) return PBL_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache) | reinterpret_cast<uintptr_t>(ws)) % 16)
        return PBL_ERR_MISALIGNED;
    for (int j = 0; j < n_extra; ++j)
        if (reinterpret_cast<uintptr_t>(extra[j]) % 4) return PBL_ERR_MISALIGNED;
    const size_t cacheb = size_t(B) * Hkv * max_len * cache_row_bytes;
    const size_t qb = size_t(((B - 1) * q_stride[0] + int64_t(Hq - 1) * q_stride[1] + (S - 1) * q_stride[2] + D) * 2);
    const size_t ob = size_t((int64_t(B) * S - 1) * ldo + int64_t(Hq) * D) * 2;
    const void* ins[7] = {q, k_cache, v_cache, pos, ws};
    size_t inb[7] = {qb, cacheb, cacheb, 8, ws_bytes};
    for (int j = 0; j < n_extra && j < 2; ++j) {
        ins[5 + j] = extra[j];
        inb[5 + j] = extra_bytes[j];
    }
    for (int j = 0; j < 5 + n_extra; ++j)
        if (attn_overlaps(out, ob, ins[j], inb[j])) return PBL_ERR_INVALID_ARG;
    for (int j = 0; j < 5 + n_extra; ++j)
        if (j != 4 && attn_overlaps(ws, ws_bytes, ins[j], inb[j])) return PBL_ERR_INVALID_ARG;
    if ((D != 64 && D != 128) || S > ATTN_MAX_S || B > ATTN_MAX_B || Hq % Hkv || max_len > ATTN_MAX_CHUNK * ATTN_MAX_SPLITS)
        return PBL_ERR_UNSUPPORTED;
    const int chunk = attn_chunk(max_len);
    const int nsplit = (max_len + chunk - 1) / chunk;
    a.q = static_cast<const uint16_t*>(q);
    a.kc = k_cache;
    a.vc = v_cache;
    a.pos = pos;
    a.part_ml = static_cast<float*>(ws);
    a.part_acc = a.part_ml + size_t(B) * Hq * S * nsplit * 2;
    a.q_sb = q_stride[0]; a.q_sh = q_stride[1]; a.q_ss = q_stride[2];
    a.scaling = scaling;
    a.S = S; a.Hq = Hq; a.group = Hq / Hkv; a.Hkv = Hkv; a.max_len = max_len; a.chunk = chunk; a.nsplit = nsplit;
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* argv[] = {&a};
    const void* kern = D == 64 ? reinterpret_cast<const void*>(pbl_attn_partial_kernel<64, Args>)
                               : reinterpret_cast<const void*>(pbl_attn_partial_kernel<128, Args>);
    if (hipLaunchKernel(kern, dim3(nsplit, Hq, B), dim3(ATTN_THREADS), argv, 0, st) != hipSuccess) return PBL_ERR_LAUNCH;
    CombineArgs c{};
    c.part_ml = a.part_ml; c.part_acc = a.part_acc;
    c.out = static_cast<uint16_t*>(out);
    c.pos = pos; c.ldo = ldo;
    c.S = S; c.Hq = Hq; c.D = D; c.nsplit = nsplit;
    void* cargv[] = {&c};
    return hipLaunchKernel(reinterpret_cast<const void*>(pbl_attn_combine_kernel), dim3(S, Hq, B), dim3(ATTN_MAX_SPLITS), cargv, 0, st) == hipSuccess
               ? PBL_OK : PBL_ERR_LAUNCH;
}

}  // namespace
