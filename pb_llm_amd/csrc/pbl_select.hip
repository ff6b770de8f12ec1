// pbl_select.hip -- token selection of a decode step (pbl_select_token_f16, pbl_select_token_minp_f16): temperature, top-k, top-p,
// min-p, the draw, and the eos / pad bookkeeping of a generation loop, on the device.
//
// One workgroup of 1024 threads per row of logits [B, V] fp16.  Everything is defined on VALUES, not on a sort order: an fp16 row
// has at most 65536 distinct values, so a threshold is found by an MSB-first radix select over an order-preserving 16-bit key (12
// bits, then 4) with histograms in LDS.  The histograms hold integers only -- counts for top-k; for top-p the weights
// w_i = exp(s_i - max s) as 2^44-scaled integers (exact for w_i >= 2^-21, truncated by less than 2^-44 below; at most 2^19 of them
// fit a uint64) -- so every sum is exact and independent of the order in which the atomics land: the same logits, uniforms and
// parameters give the same token on every run, eager or replayed.  The draw walks the row in vocabulary order (wave segments, then
// a wave-wide scan inside the segment that holds the target) over the same integers.
//
// The row is read from global memory (L2: the lm_head GEMM wrote it just before) once per pass: maximum / argmax, two passes per
// active filter, two for the draw.  No allocation, no synchronisation, nothing read on the host; the step counter lives on the
// device and is advanced by the launch, so one captured graph serves every step.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pbl.h"

namespace {

constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int SEL_BINS = 4096;                 // the high 12 bits of a key; its low 4 bits are the second level
constexpr int SEL_LOW = 16;
constexpr int SEL_MAX_V = 1 << 19;             // 2^19 weights of at most 2^44 each: their sum fits a uint64
constexpr uint32_t SEL_NONE = 0xffffffffu;     // an element beyond the row
constexpr uint32_t SEL_KEY_NAN = 0xffffu, SEL_KEY_PINF = 0xfc00u, SEL_KEY_NINF = 0x03ffu;

typedef unsigned long long u64;

struct SelArgs {
    const uint16_t* logits;         // row b at logits + b * ld
    int64_t ld;
    const float* u;                 // [n_steps, B] or NULL (greedy)
    int64_t n_steps;
    int64_t* step;
    const int64_t* eos;
    int64_t pad;
    uint8_t* unfinished;            // [B]
    int64_t* tokens;                // [B, total]
    int64_t total, col0;
    int64_t* next_ids;              // [B]
    int32_t* n_unfinished;
    int32_t* status;
    uint8_t* kept;                  // [B, V] or NULL
    float temperature, top_p, min_p;
    int top_k, n_eos, B, V, vec, finish;
};

// fp16 bits -> a 16-bit key that orders as the values do: -0 is +0, every NaN is the maximum (as in torch.argmax)
__device__ __forceinline__ uint32_t sel_key(uint32_t h) {
    if ((h & 0x7fffu) > 0x7c00u) return SEL_KEY_NAN;
    if (h == 0x8000u) h = 0;
    return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}

__device__ __forceinline__ float sel_value(uint32_t key) {
    const uint16_t h = uint16_t((key & 0x8000u) ? (key & 0x7fffu) : ~key);
    return float(__builtin_bit_cast(_Float16, h));
}

// the weight of a key as an integer: floor(2^44 exp(s - m)), s = value / temperature in fp32 (the key of the maximum gives 2^44)
__device__ __forceinline__ u64 sel_weight(uint32_t key, float temperature, float m) {
    return u64(expf(sel_value(key) / temperature - m) * 0x1p44f);
}

// The weight of a key in the draw, 0 for a key that does not stay.  A key stays iff it passes the top-k / top-p cut and, with min_p > 0,
// exp(s - max s) >= min_p -- its probability relative to the top one, which no normaliser enters: a rule on the value alone, on the
// one exponential that is also the weight (the maximum gives exp(0) = 1 and always stays).  min_p = 0: sel_weight of the keys >= kcut.
__device__ __forceinline__ u64 sel_kept_weight(uint32_t key, uint32_t kcut, float temperature, float m, float min_p, bool* keep) {
    *keep = false;
    if (key < kcut) return 0;                              // (no exponential for what top-k / top-p removed)
    const float e = expf(sel_value(key) / temperature - m);
    *keep = e >= min_p;                                    // (e >= 0 always: rows with a NaN are not sampled)
    return *keep ? u64(e * 0x1p44f) : 0;
}

struct SelRow {
    const uint16_t* p;
    int V, vec, seg;                // wave w owns elements [w * seg, w * seg + seg) of the row, seg a multiple of 8
};

// the fp16 bits of elements [i0, i0 + 8) of the row (zeros at and beyond `end`, which is at most V)
__device__ __forceinline__ uint4 sel_load8(const SelRow& r, int i0, int end) {
    if (i0 >= end) return make_uint4(0, 0, 0, 0);
    if (r.vec && i0 + 8 <= r.V) return *reinterpret_cast<const uint4*>(r.p + i0);
    auto h = [&](int j) -> uint32_t { return i0 + j < end ? uint32_t(r.p[i0 + j]) : 0u; };
    return make_uint4(h(0) | (h(1) << 16), h(2) | (h(3) << 16), h(4) | (h(5) << 16), h(6) | (h(7) << 16));
}

// their keys; SEL_NONE at and beyond `end`
__device__ __forceinline__ void sel_keys8(const uint4 w, int i0, int end, uint32_t (&k)[8]) {
    auto key = [&](uint32_t h, int j) -> uint32_t { return i0 + j < end ? sel_key(h) : SEL_NONE; };
    k[0] = key(w.x & 0xffffu, 0); k[1] = key(w.x >> 16, 1); k[2] = key(w.y & 0xffffu, 2); k[3] = key(w.y >> 16, 3);
    k[4] = key(w.z & 0xffffu, 4); k[5] = key(w.z >> 16, 5); k[6] = key(w.w & 0xffffu, 6); k[7] = key(w.w >> 16, 7);
}

// f(i0, keys[8]) over the row: wave w walks its segment 512 elements at a time (lane l: 8 consecutive ones), four 16-byte
// loads in flight per lane; the trip count is the same for every lane of a wave
template <class F>
__device__ __forceinline__ void sel_for_each8(const SelRow& r, F f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int begin = wave * r.seg, end = min(r.V, begin + r.seg);
    for (int base = begin; base < end; base += 2048) {
        const int i0 = base + lane * 8;                    // (named registers: an indexed array of them ends up in scratch)
        const uint4 r0 = sel_load8(r, i0, end), r1 = sel_load8(r, i0 + 512, end), r2 = sel_load8(r, i0 + 1024, end),
                    r3 = sel_load8(r, i0 + 1536, end);
        uint32_t k[8];
        sel_keys8(r0, i0, end, k);
        f(i0, k);
        if (base + 512 < end) {
            sel_keys8(r1, i0 + 512, end, k);
            f(i0 + 512, k);
        }
        if (base + 1024 < end) {
            sel_keys8(r2, i0 + 1024, end, k);
            f(i0 + 1024, k);
        }
        if (base + 1536 < end) {
            sel_keys8(r3, i0 + 1536, end, k);
            f(i0 + 1536, k);
        }
    }
}

__device__ __forceinline__ u64 sel_wave_max(u64 v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const u64 o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ u64 sel_wave_sum(u64 v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ u64 sel_wave_scan(u64 v) {          // inclusive, over the lanes of a wave
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}

struct SelShared {
    u64 hist[SEL_BINS];
    u64 wave[SEL_WAVES];
    u64 total, below;
    uint32_t bin;
    int64_t token;
};

// The smallest key x, among the elements with key >= kmin, whose ascending cumulative weight sum{w_i : kmin <= key_i <= x}
// exceeds the threshold.  MASS: w_i = sel_weight and the threshold is floor(frac * total) (at most total - 1, so the largest key
// always passes); otherwise w_i = 1 and the threshold is `count`.  *total_out = the weight of all elements with key >= kmin.
template <bool MASS>
__device__ __forceinline__ uint32_t sel_threshold(const SelRow& r, SelShared& sh, uint32_t kmin, u64 count, double frac, float temperature, float m,
                                  u64* total_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SEL_BINS / SEL_THREADS; ++j) sh.hist[tid + j * SEL_THREADS] = 0;
    __syncthreads();
    sel_for_each8(r, [&](int, const uint32_t (&k)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k[j] != SEL_NONE && k[j] >= kmin) {
                const u64 w = MASS ? sel_weight(k[j], temperature, m) : 1;
                if (w) atomicAdd(&sh.hist[k[j] >> 4], w);
            }
    });
    __syncthreads();
    constexpr int PER = SEL_BINS / SEL_THREADS;            // thread t owns bins [PER t, PER t + PER): ascending keys
    u64 c[PER], mine = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        c[j] = sh.hist[tid * PER + j];
        mine += c[j];
    }
    u64 incl = sel_wave_scan(mine);
    if (lane == 63) sh.wave[wave] = incl;
    __syncthreads();
    u64 before = 0, total = 0;
    for (int w = 0; w < SEL_WAVES; ++w) {
        if (w < wave) before += sh.wave[w];
        total += sh.wave[w];
    }
    incl += before;
    u64 thr = count;
    if (MASS) {
        thr = u64(frac * double(total));
        if (thr >= total) thr = total - 1;
    }
    if (incl - mine <= thr && thr < incl) {                // one thread: the first-level bin that crosses the threshold
        u64 run = incl - mine;
        for (int j = 0; j < PER; ++j) {
            if (run + c[j] > thr) {
                sh.bin = uint32_t(tid * PER + j);
                sh.below = run;
                break;
            }
            run += c[j];
        }
    }
    __syncthreads();
    const uint32_t bin = sh.bin;
    const u64 below = sh.below;
    __syncthreads();
    if (tid < SEL_LOW) sh.hist[tid] = 0;
    __syncthreads();
    sel_for_each8(r, [&](int, const uint32_t (&k)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k[j] != SEL_NONE && k[j] >= kmin && (k[j] >> 4) == bin) {
                const u64 w = MASS ? sel_weight(k[j], temperature, m) : 1;
                if (w) atomicAdd(&sh.hist[k[j] & (SEL_LOW - 1)], w);
            }
    });
    __syncthreads();
    u64 run = below;
    uint32_t key = (bin << 4) | (SEL_LOW - 1);
    for (int j = 0; j < SEL_LOW; ++j) {
        run += sh.hist[j];
        if (run > thr) {
            key = (bin << 4) | uint32_t(j);
            break;
        }
    }
    *total_out = total;
    return key;
}

__global__ __launch_bounds__(SEL_THREADS) void pbl_select_token_kernel(SelArgs a) {
    __shared__ SelShared sh;
    __shared__ int64_t sh_step;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    SelRow r;
    r.p = a.logits + int64_t(b) * a.ld;
    r.V = a.V;
    r.vec = a.vec;
    r.seg = ((a.V + SEL_WAVES - 1) / SEL_WAVES + 7) & ~7;
    if (tid == 0) sh_step = *a.step;

    // the maximum and its lowest index: (key, ~index) packed, so one integer maximum finds both
    u64 best = 0;
    sel_for_each8(r, [&](int i0, const uint32_t (&k)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k[j] != SEL_NONE) {
                const u64 v = (u64(k[j]) << 32) | (0xffffffffu - uint32_t(i0 + j));
                best = v > best ? v : best;
            }
    });
    best = sel_wave_max(best);
    if (lane == 0) sh.wave[wave] = best;
    __syncthreads();
    best = sh.wave[0];
    for (int w = 1; w < SEL_WAVES; ++w) best = sh.wave[w] > best ? sh.wave[w] : best;
    const uint32_t kmax = uint32_t(best >> 32);
    const int64_t argmax = int64_t(0xffffffffu - uint32_t(best));
    const int64_t step = sh_step;
    const bool in_range = step >= 0 && a.col0 + step < a.total && (!a.u || step < a.n_steps);
    const bool bad = kmax >= SEL_KEY_PINF || kmax == SEL_KEY_NINF;      // NaN or +inf in the row, or nothing finite
    const bool sample = a.u && !bad;
    uint32_t kcut = kmax;                                                 // greedy: the kept set is the token alone

    if (sample) {
        const float m = sel_value(kmax) / a.temperature;
        u64 total = 0;
        kcut = 0;
        if (a.top_k > 0 && a.top_k < a.V)          // the k-th largest: the smallest x with fewer than k elements above it
            kcut = sel_threshold<false>(r, sh, 0, u64(a.V - a.top_k), 0.0, a.temperature, m, &total);
        if (a.top_p < 1.f)                         // remove x iff M(x) <= (1 - top_p) total, i.e. keep from the first x that exceeds it
            kcut = sel_threshold<true>(r, sh, kcut, 0, 1.0 - double(a.top_p), a.temperature, m, &total);
        if (kcut > kmax) kcut = kmax;

        // the draw, in vocabulary order: the weight of every wave's segment, then a scan inside the segment that holds the target
        u64 mine = 0;
        sel_for_each8(r, [&](int i0, const uint32_t (&k)[8]) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (k[j] != SEL_NONE) {
                    bool keep;
                    mine += sel_kept_weight(k[j], kcut, a.temperature, m, a.min_p, &keep);
                    if (a.kept) a.kept[int64_t(b) * a.V + i0 + j] = keep;
                }
        });
        mine = sel_wave_sum(mine);
        __syncthreads();
        if (lane == 0) sh.wave[wave] = mine;
        if (tid == 0) sh.token = argmax;
        __syncthreads();
        u64 W = 0;
        for (int w = 0; w < SEL_WAVES; ++w) W += sh.wave[w];
        float u = in_range ? a.u[step * a.B + b] : 0.f;
        if (!(u >= 0.f)) u = 0.f;
        u64 target = u64(double(u) * double(W));
        if (target >= W) target = W - 1;                                  // (W >= 2^44: the maximum is always kept)
        u64 before = 0;
        int owner = 0;
        for (int w = 0; w < SEL_WAVES; ++w) {
            if (before + sh.wave[w] > target) {
                owner = w;
                break;
            }
            before += sh.wave[w];
        }
        if (wave == owner) {
            const int begin = wave * r.seg, end = min(r.V, begin + r.seg);
            u64 run = before;
            for (int base = begin; base < end; base += 512) {
                const int i0 = base + lane * 8;
                uint32_t k[8];
                u64 q[8], sum = 0;
                sel_keys8(sel_load8(r, i0, end), i0, end, k);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    bool keep;
                    q[j] = k[j] != SEL_NONE ? sel_kept_weight(k[j], kcut, a.temperature, m, a.min_p, &keep) : 0;
                    sum += q[j];
                }
                const u64 incl = sel_wave_scan(sum);
                const u64 all = __shfl(incl, 63);
                if (run + all > target) {                                 // (the same decision in every lane)
                    u64 lo = run + incl - sum;
                    if (lo <= target && target < lo + sum) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            if (lo <= target && target < lo + q[j]) sh.token = i0 + j;
                            lo += q[j];
                        }
                    }
                    break;
                }
                run += all;
            }
        }
        __syncthreads();
    } else {
        if (a.kept)
            for (int i = tid; i < a.V; i += SEL_THREADS) a.kept[int64_t(b) * a.V + i] = i == argmax;
    }

    if (tid == 0) {
        int64_t tok = sample ? sh.token : argmax;
        int flags = (a.u && bad ? 1 : 0) | (in_range ? 0 : 2);
        if (flags) atomicOr(a.status, flags);
        uint8_t unf = a.unfinished[b];
        if (!unf) tok = a.pad;
        else
            for (int j = 0; j < a.n_eos; ++j)
                if (tok == a.eos[j]) unf = 0;
        a.unfinished[b] = unf;
        if (in_range) a.tokens[int64_t(b) * a.total + a.col0 + step] = tok;
        a.next_ids[b] = tok;
        if (a.finish) {                                                   // one row: nothing to wait for
            *a.n_unfinished = unf;
            *a.step = step + 1;
        }
    }
}

// several rows: counts the rows still unfinished and advances the step once every row's workgroup has read it
__global__ __launch_bounds__(64) void pbl_select_token_kernel_finish(const uint8_t* unfinished, int B, int32_t* n_unfinished, int64_t* step) {
    int n = 0;
    for (int i = threadIdx.x; i < B; i += 64) n += unfinished[i] != 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off);
    if (threadIdx.x == 0) {
        *n_unfinished = n;
        *step = *step + 1;
    }
}

bool sel_overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
}

}  // namespace

extern "C" {

int pbl_select_token_minp_f16(const void* logits, int64_t ld, int B, int V, float temperature, int top_k, float top_p, float min_p,
                              const float* u, int64_t n_steps, int64_t* step, const int64_t* eos, int n_eos, int64_t pad,
                              uint8_t* unfinished, int64_t* tokens, int64_t total, int64_t col0, int64_t* next_ids,
                              int32_t* n_unfinished, int32_t* status, uint8_t* kept, void* stream) {
    if (!logits || !step || !unfinished || !tokens || !next_ids || !n_unfinished || !status || B < 1 || V < 1 || ld < V || total < 1 ||
        col0 < 0 || col0 >= total || n_eos < 0 || (n_eos > 0 && !eos) || (u && n_steps < 1))
        return PBL_ERR_INVALID_ARG;
    if (!(temperature > 0.f) || !(top_p > 0.f && top_p <= 1.f) || top_k < 0 || !(min_p >= 0.f && min_p <= 1.f)) return PBL_ERR_INVALID_ARG;
    const void* ins[3] = {logits, u, eos};
    const size_t inb[3] = {size_t((int64_t(B) - 1) * ld + V) * 2, u ? size_t(n_steps) * B * 4 : 0, size_t(n_eos) * 8};
    const void* outs[7] = {step, unfinished, tokens, next_ids, n_unfinished, status, kept};
    const size_t outb[7] = {8, size_t(B), size_t(B) * size_t(total) * 8, size_t(B) * 8, 4, 4, kept ? size_t(B) * V : 0};
    for (int i = 0; i < 7; ++i) {
        for (int j = 0; j < 3; ++j)
            if (sel_overlaps(outs[i], outb[i], ins[j], inb[j])) return PBL_ERR_INVALID_ARG;
        for (int j = i + 1; j < 7; ++j)
            if (sel_overlaps(outs[i], outb[i], outs[j], outb[j])) return PBL_ERR_INVALID_ARG;
    }
    if (V > SEL_MAX_V) return PBL_ERR_UNSUPPORTED;
    SelArgs a{};
    a.logits = static_cast<const uint16_t*>(logits);
    a.ld = ld;
    a.u = u; a.n_steps = n_steps; a.step = step;
    a.eos = eos; a.pad = pad;
    a.unfinished = unfinished; a.tokens = tokens; a.total = total; a.col0 = col0; a.next_ids = next_ids;
    a.n_unfinished = n_unfinished; a.status = status; a.kept = kept;
    a.temperature = temperature; a.top_p = top_p; a.min_p = min_p; a.top_k = top_k; a.n_eos = n_eos; a.B = B; a.V = V;
    a.vec = reinterpret_cast<uintptr_t>(logits) % 16 == 0 && (B == 1 || ld % 8 == 0);
    a.finish = B == 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* argv[] = {&a};
    if (hipLaunchKernel(reinterpret_cast<const void*>(pbl_select_token_kernel), dim3(B), dim3(SEL_THREADS), argv, 0, st) != hipSuccess)
        return PBL_ERR_LAUNCH;
    if (B == 1) return PBL_OK;
    void* fargv[] = {&unfinished, &B, &n_unfinished, &step};
    return hipLaunchKernel(reinterpret_cast<const void*>(pbl_select_token_kernel_finish), dim3(1), dim3(64), fargv, 0, st) == hipSuccess
               ? PBL_OK : PBL_ERR_LAUNCH;
}

int pbl_select_token_f16(const void* logits, int64_t ld, int B, int V, float temperature, int top_k, float top_p, const float* u,
                         int64_t n_steps, int64_t* step, const int64_t* eos, int n_eos, int64_t pad, uint8_t* unfinished,
                         int64_t* tokens, int64_t total, int64_t col0, int64_t* next_ids, int32_t* n_unfinished, int32_t* status,
                         uint8_t* kept, void* stream) {
    return pbl_select_token_minp_f16(logits, ld, B, V, temperature, top_k, top_p, 0.f, u, n_steps, step, eos, n_eos, pad, unfinished, tokens,
                                     total, col0, next_ids, n_unfinished, status, kept, stream);
}

}  // extern "C"
