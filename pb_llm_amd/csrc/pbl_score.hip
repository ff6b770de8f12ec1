// pbl_score.hip -- token scoring of an evaluation pass (pbl_score_tokens_f16): per row of fp16 logits the log-probability of a
// target token and whether that token is the arg-max, and per request the sum / AND over a span of rows.
//
// One workgroup of 256 threads per row; the row is streamed from memory ONCE, 16 bytes per lane and load, four loads in flight.
// The chunks of 8 elements are laid over the row from the 16-byte boundary at or below its first element, so every chunk that lies
// inside the row is one aligned vector load whatever the row's offset (out.logits[0, :-1, :50257] included); the two edge chunks
// take element loads and read nothing outside the row.  Lane `tid` owns chunks tid, tid + 256, ... in ascending order and keeps
//   (m, l)      the running maximum and sum{exp(x - m)} of online softmax, rescaled once per chunk that raises the maximum;
//   (bi0, bw)   the chunk that first reached m, kept in registers: the arg-max index is resolved once per lane at the end;
//   nan_idx     the lowest index of a NaN (a NaN counts as the maximum, as in torch.argmax);
//   tw          the chunk that holds the target element.
// The empty-partial rule: a partial whose maximum is -inf (no element, or only -inf / NaN) is never rescaled -- a rescale happens only
// when a chunk's maximum is strictly above m, and two partials whose maxima are both -inf merge by adding their sums (0, or NaN once
// a NaN was seen) -- so exp(-inf - -inf) is never evaluated.  Lanes merge by a xor butterfly, waves in ascending order: a fixed
// order, so the result is bit-stable from run to run, eager or replayed.  Whether the row scores NaN is decided on the arg-max KEY
// (an integer), not on the floats.
//
// The span sums are a second launch on the same stream: one wave per span, lane j adds rows begin + j, begin + j + 64, ... in fp64,
// then a xor butterfly.  No atomics on floating-point values anywhere; *status is OR-ed with an integer atomic.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pbl.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_MAX_V = 1 << 20;
constexpr int SC_STRIDE = SC_THREADS * 8;      // elements one pass of the workgroup covers
constexpr uint32_t SC_KEY_NAN = 0xffffu, SC_KEY_PINF = 0xfc00u, SC_KEY_NINF = 0x03ffu;
constexpr uint32_t SC_PAD = 0xfc00u;           // what an element outside the row reads as: -inf

typedef unsigned long long u64;

struct ScArgs {
    const uint16_t* logits;         // row t at logits + t * ld
    int64_t ld;
    const int64_t* targets;         // [T]
    int64_t ignore_index;
    float* logprob;                 // [T]
    uint8_t* greedy;                // [T] or NULL
    int32_t* status;
    int V;
};

// fp16 bits -> a 16-bit key that orders as the values do: -0 is +0, every NaN is the maximum (pbl_select.hip's sel_key)
__device__ __forceinline__ uint32_t sc_key(uint32_t h) {
    if ((h & 0x7fffu) > 0x7c00u) return SC_KEY_NAN;
    if (h == 0x8000u) h = 0;
    return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}

__device__ __forceinline__ float sc_float(uint32_t h) { return float(__builtin_bit_cast(_Float16, uint16_t(h))); }

__device__ __forceinline__ uint32_t sc_half(const uint4& w, int j) {
    const uint32_t d = j < 2 ? w.x : j < 4 ? w.y : j < 6 ? w.z : w.w;
    return (j & 1) ? d >> 16 : d & 0xffffu;
}

// the fp16 bits of virtual elements [i0, i0 + 8) of a row whose elements are the virtual indices [lo, hi) from the aligned pointer
// pv; SC_PAD outside the row, which is never read
__device__ __forceinline__ uint4 sc_load8(const uint16_t* pv, int lo, int hi, int i0) {
    if (i0 >= lo && i0 + 8 <= hi) return *reinterpret_cast<const uint4*>(pv + i0);
    if (i0 + 8 <= lo || i0 >= hi) return make_uint4(SC_PAD | (SC_PAD << 16), SC_PAD | (SC_PAD << 16), SC_PAD | (SC_PAD << 16), SC_PAD | (SC_PAD << 16));
    auto h = [&](int j) -> uint32_t { return i0 + j >= lo && i0 + j < hi ? uint32_t(pv[i0 + j]) : SC_PAD; };
    return make_uint4(h(0) | (h(1) << 16), h(2) | (h(3) << 16), h(4) | (h(5) << 16), h(6) | (h(7) << 16));
}

struct ScLane {
    float m, l;
    int bi0, nan_idx;
    uint4 bw, tw;
};

__device__ __forceinline__ void sc_step(ScLane& s, const uint4 w, int i0, int tbase) {
    const float f0 = sc_float(w.x & 0xffffu), f1 = sc_float(w.x >> 16), f2 = sc_float(w.y & 0xffffu), f3 = sc_float(w.y >> 16),
                f4 = sc_float(w.z & 0xffffu), f5 = sc_float(w.z >> 16), f6 = sc_float(w.w & 0xffffu), f7 = sc_float(w.w >> 16);
    const float cm = fmaxf(fmaxf(fmaxf(f0, f1), fmaxf(f2, f3)), fmaxf(fmaxf(f4, f5), fmaxf(f6, f7)));     // (fmaxf drops NaNs)
    if (cm > s.m) {                                     // strictly above: m = cm = -inf never gets here
        s.l *= __expf(s.m - cm);                        // m = -inf: l is 0 (or NaN) and stays so
        s.m = cm;
        s.bi0 = i0;
        s.bw = w;
    }
    const float ms = s.m == -INFINITY ? 0.f : s.m;      // still -inf: the chunk holds only -inf and NaN, which give 0 and NaN
    const float sum = ((__expf(f0 - ms) + __expf(f1 - ms)) + (__expf(f2 - ms) + __expf(f3 - ms))) +
                      ((__expf(f4 - ms) + __expf(f5 - ms)) + (__expf(f6 - ms) + __expf(f7 - ms)));
    s.l += sum;
    if (sum != sum) {                                   // a NaN or a +inf in the chunk
#pragma unroll
        for (int j = 7; j >= 0; --j)
            if (sc_key(sc_half(w, j)) == SC_KEY_NAN && i0 + j < s.nan_idx) s.nan_idx = i0 + j;
    }
    if (i0 == tbase) s.tw = w;
}

__device__ __forceinline__ void sc_merge(float& m, float& l, float m2, float l2) {
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) l = l + l2;                     // two empty partials: no rescale
    else l = l * __expf(m - M) + l2 * __expf(m2 - M);   // (exp(-inf - M) = 0 for one empty partial)
    m = M;
}

struct ScShared {
    float m[SC_WAVES], l[SC_WAVES];
    u64 cand[SC_WAVES];
    uint32_t xt;
};

__global__ __launch_bounds__(SC_THREADS) void pbl_score_tokens_kernel(ScArgs a) {
    __shared__ ScShared sh;
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t target = a.targets[t];
    if (target == a.ignore_index || target < 0 || target >= a.V) {          // (the same decision in every thread)
        if (tid == 0) {
            const bool ignored = target == a.ignore_index;
            a.logprob[t] = ignored ? 0.f : NAN;
            if (a.greedy) a.greedy[t] = 0;
            if (!ignored) atomicOr(a.status, 1);
        }
        return;
    }
    const uint16_t* p = a.logits + t * a.ld;
    const int off = int((reinterpret_cast<uintptr_t>(p) >> 1) & 7);         // elements between the 16-byte boundary below p and p
    const uint16_t* pv = p - off;
    const int lo = off, hi = off + a.V;
    const int tv = int(target) + off, tbase = tv & ~7;

    ScLane s;
    s.m = -INFINITY;
    s.l = 0.f;
    s.bi0 = 0;
    s.nan_idx = INT_MAX;
    s.bw = s.tw = make_uint4(0, 0, 0, 0);
    const int nit = (hi + SC_STRIDE - 1) / SC_STRIDE;
    for (int c = 0; c < nit; c += 4) {
        const int i0 = c * SC_STRIDE + tid * 8;            // (named registers: an indexed array of them ends up in scratch)
        const uint4 r0 = sc_load8(pv, lo, hi, i0), r1 = sc_load8(pv, lo, hi, i0 + SC_STRIDE), r2 = sc_load8(pv, lo, hi, i0 + 2 * SC_STRIDE),
                    r3 = sc_load8(pv, lo, hi, i0 + 3 * SC_STRIDE);
        sc_step(s, r0, i0, tbase);
        if (c + 1 < nit) sc_step(s, r1, i0 + SC_STRIDE, tbase);
        if (c + 2 < nit) sc_step(s, r2, i0 + 2 * SC_STRIDE, tbase);
        if (c + 3 < nit) sc_step(s, r3, i0 + 3 * SC_STRIDE, tbase);
    }

    // the lane's arg-max candidate: (key, ~index) packed, so one integer maximum finds the largest key at its lowest index
    u64 cand = 0;                                                            // below every real key: a lane without an element
    if (s.nan_idx != INT_MAX) {
        cand = (u64(SC_KEY_NAN) << 32) | (0xffffffffu - uint32_t(s.nan_idx - off));
    } else if (s.m > -INFINITY) {
        int j = 7;                                                           // (m came from this chunk: one element equals it)
#pragma unroll
        for (int q = 6; q >= 0; --q)
            if (sc_float(sc_half(s.bw, q)) == s.m) j = q;
        cand = (u64(sc_key(sc_half(s.bw, j))) << 32) | (0xffffffffu - uint32_t(s.bi0 + j - off));
    } else if (tid * 8 + 8 > lo && tid * 8 < hi) {                           // only -inf: the lane's first element
        cand = (u64(SC_KEY_NINF) << 32) | (0xffffffffu - uint32_t(max(tid * 8, lo) - off));
    }
    float m = s.m, l = s.l;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        sc_merge(m, l, __shfl_xor(m, o), __shfl_xor(l, o));
        const u64 oc = __shfl_xor(cand, o);
        cand = oc > cand ? oc : cand;
    }
    if (lane == 0) {
        sh.m[wave] = m;
        sh.l[wave] = l;
        sh.cand[wave] = cand;
    }
    if (tid == ((tbase >> 3) & (SC_THREADS - 1))) sh.xt = sc_half(s.tw, tv & 7);
    __syncthreads();
    if (tid == 0) {
        m = sh.m[0];
        l = sh.l[0];
        cand = sh.cand[0];
        for (int w = 1; w < SC_WAVES; ++w) {
            sc_merge(m, l, sh.m[w], sh.l[w]);
            cand = sh.cand[w] > cand ? sh.cand[w] : cand;
        }
        const uint32_t kmax = uint32_t(cand >> 32);
        const int64_t argmax = int64_t(0xffffffffu - uint32_t(cand));
        const bool bad = kmax >= SC_KEY_PINF || kmax == SC_KEY_NINF;        // NaN or +inf in the row, or nothing finite
        a.logprob[t] = bad ? NAN : sc_float(sh.xt) - (m + logf(l));
        if (a.greedy) a.greedy[t] = argmax == target;
    }
}

// one wave per span: lane j adds the counted rows begin + j, begin + j + 64, ... in fp64, then a xor butterfly
__global__ __launch_bounds__(64) void pbl_score_spans_kernel(const float* logprob, const uint8_t* greedy, const int64_t* targets,
                                                             int64_t ignore_index, int64_t T, const int64_t* spans, double* span_sum,
                                                             uint8_t* span_greedy, int32_t* span_count, int32_t* status) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int64_t begin = spans[2 * r], end = spans[2 * r + 1];
    if (begin < 0 || end > T || begin > end) {
        if (lane == 0) {
            span_sum[r] = double(NAN);
            span_greedy[r] = 0;
            span_count[r] = 0;
            atomicOr(status, 2);
        }
        return;
    }
    double acc = 0.0;
    int n = 0, g = 1;
    for (int64_t i = begin + lane; i < end; i += 64)
        if (targets[i] != ignore_index) {
            acc += double(logprob[i]);
            n += 1;
            g &= greedy[i] != 0;
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        acc += __shfl_xor(acc, o);
        n += __shfl_xor(n, o);
        g &= __shfl_xor(g, o);
    }
    if (lane == 0) {
        span_sum[r] = acc;
        span_greedy[r] = uint8_t(g);
        span_count[r] = n;
    }
}

bool sc_overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}

}  // namespace

extern "C" {

int pbl_score_tokens_f16(const void* logits, int64_t ld, int64_t T, int V, const int64_t* targets, int64_t ignore_index,
                         float* logprob, uint8_t* greedy, const int64_t* spans, int R, double* span_sum, uint8_t* span_greedy,
                         int32_t* span_count, int32_t* status, void* stream) {
    if (!logits || !targets || !logprob || !status || T < 1 || V < 1 || ld < V || R < 0) return PBL_ERR_INVALID_ARG;
    if (R > 0 && (!spans || !span_sum || !span_greedy || !span_count || !greedy)) return PBL_ERR_INVALID_ARG;
    if (V > SC_MAX_V || T > INT_MAX) return PBL_ERR_UNSUPPORTED;
    const size_t nT = size_t(T), nR = size_t(R);
    const void* ins[3] = {logits, targets, spans};
    const size_t inb[3] = {(size_t(T - 1) * size_t(ld) + size_t(V)) * 2, nT * 8, nR * 16};
    const void* outs[6] = {logprob, greedy, status, span_sum, span_greedy, span_count};
    const size_t outb[6] = {nT * 4, greedy ? nT : 0, 4, nR * 8, nR, nR * 4};
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 3; ++j)
            if (sc_overlaps(outs[i], outb[i], ins[j], inb[j])) return PBL_ERR_INVALID_ARG;
        for (int j = i + 1; j < 6; ++j)
            if (sc_overlaps(outs[i], outb[i], outs[j], outb[j])) return PBL_ERR_INVALID_ARG;
    }
    ScArgs a{};
    a.logits = static_cast<const uint16_t*>(logits);
    a.ld = ld;
    a.targets = targets;
    a.ignore_index = ignore_index;
    a.logprob = logprob;
    a.greedy = greedy;
    a.status = status;
    a.V = V;
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* argv[] = {&a};
    if (hipLaunchKernel(reinterpret_cast<const void*>(pbl_score_tokens_kernel), dim3(unsigned(T)), dim3(SC_THREADS), argv, 0, st) != hipSuccess)
        return PBL_ERR_LAUNCH;
    if (R == 0) return PBL_OK;
    const float* lp = logprob;
    const uint8_t* gr = greedy;
    void* sargv[] = {&lp, &gr, &targets, &ignore_index, &T, &spans, &span_sum, &span_greedy, &span_count, &status};
    return hipLaunchKernel(reinterpret_cast<const void*>(pbl_score_spans_kernel), dim3(unsigned(R)), dim3(64), sargv, 0, st) == hipSuccess
               ? PBL_OK : PBL_ERR_LAUNCH;
}

}  // extern "C"
