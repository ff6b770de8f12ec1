// pbl_spec.hip -- the control plane of prompt-lookup speculative decoding (pbl_spec_verify_f16, pbl_ngram_draft), on the device.
//
// A speculative step feeds S = 1 + K tokens per row -- the last emitted token and K drafts -- through the decode kernels, which are
// built for up to four rows per launch anyway.  Two launches then close the step:
//   1. pbl_spec_argmax_kernel, one workgroup of 1024 threads per row (b, s) of the fp16 logits: the arg-max with the rule of
//      pbl_select_token_f16's greedy mode ((key, ~index) packed into one integer maximum), written to the stats block;
//   2. pbl_spec_finish_kernel, ONE workgroup: thread 0 compares the drafts with the arg-maxes of the rows before them, emits the
//      accepted prefix plus one bonus token per row with the eos / pad bookkeeping of the one-token loop and advances the cursor;
//      the threads take the rejected rows back from every layer's cache position; then the whole workgroup drafts the next K tokens
//      of every row by an n-gram lookup in the row's own history (one pass over the history finds the latest match of every
//      length 1 .. 4; "latest" is an integer maximum, so the draft is the same on every run).
// The drafting is also an entry of its own (the first drafts follow the prefill).  No allocation, no synchronisation, nothing read
// on the host, plain loads and vector stores only: the pair is capturable in a hipGraph, and one captured graph serves every step.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pbl.h"

namespace {

constexpr int SPEC_THREADS = 1024;
constexpr int SPEC_WAVES = SPEC_THREADS / 64;
constexpr int SPEC_MAX_ROWS = 4;               // B * S: what one decode launch takes
constexpr int SPEC_MAX_NGRAM = 4;
constexpr int SPEC_MAX_V = 1 << 19;            // pbl_select_token_f16's limit: the two entries serve the same logits
constexpr int SPEC_STAT_ARGMAX = 4;            // stats[4 + r]: the arg-max of row r = b * S + s of the last call

typedef unsigned long long u64;

// fp16 bits -> a 16-bit key that orders as the values do: -0 is +0, every NaN is the maximum (pbl_select.hip's sel_key)
__device__ __forceinline__ uint32_t spec_key(uint32_t h) {
    if ((h & 0x7fffu) > 0x7c00u) return 0xffffu;
    if (h == 0x8000u) h = 0;
    return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}

__device__ __forceinline__ u64 spec_pack(uint32_t h, int i) { return (u64(spec_key(h)) << 32) | (0xffffffffu - uint32_t(i)); }

__device__ __forceinline__ u64 spec_max(u64 a, u64 b) { return a > b ? a : b; }

// One workgroup per row: elements up to the first 16-byte boundary and after the last one take element loads, the chunks between
// them 16-byte loads -- a row may start at any element of a wider buffer (out.logits[:, -S:, :V]).
__global__ __launch_bounds__(SPEC_THREADS) void pbl_spec_argmax_kernel(const uint16_t* logits, int64_t ld_b, int64_t ld_s, int S, int V,
                                                                       int64_t* stats) {
    __shared__ u64 sh[SPEC_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x;
    const uint16_t* p = logits + int64_t(r / S) * ld_b + int64_t(r % S) * ld_s;
    const int head = min(V, int(((16u - uint32_t(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / 2u));
    const int nvec = (V - head) / 8;
    u64 best = 0;
    if (tid < head) best = spec_pack(p[tid], tid);
    const uint4* pv = reinterpret_cast<const uint4*>(p + head);
#pragma unroll 4
    for (int c = tid; c < nvec; c += SPEC_THREADS) {
        const uint4 w = pv[c];
        const int i0 = head + c * 8;
        best = spec_max(best, spec_max(spec_pack(w.x & 0xffffu, i0), spec_pack(w.x >> 16, i0 + 1)));
        best = spec_max(best, spec_max(spec_pack(w.y & 0xffffu, i0 + 2), spec_pack(w.y >> 16, i0 + 3)));
        best = spec_max(best, spec_max(spec_pack(w.z & 0xffffu, i0 + 4), spec_pack(w.z >> 16, i0 + 5)));
        best = spec_max(best, spec_max(spec_pack(w.w & 0xffffu, i0 + 6), spec_pack(w.w >> 16, i0 + 7)));
    }
    const int tail = head + nvec * 8 + tid;                // fewer than 8 elements are left
    if (tail < V) best = spec_max(best, spec_pack(p[tail], tail));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = spec_max(best, __shfl_xor(best, off));
    if ((tid & 63) == 0) sh[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SPEC_WAVES; ++w) best = spec_max(best, sh[w]);
        stats[SPEC_STAT_ARGMAX + r] = int64_t(0xffffffffu - uint32_t(best));
    }
}

struct SpecArgs {
    int64_t* ids;                   // [B, S]
    int64_t* tokens;                // [B, total]
    int64_t total;
    int64_t* cursor;
    uint8_t* unfinished;            // [B]
    const int64_t* eos;
    int64_t pad;
    int32_t* n_unfinished;
    int32_t* status;
    int64_t* const* positions;      // [L] pointers to the layers' positions
    int64_t* stats;
    int B, S, n_eos, L, max_ngram, verify;
};

// ids[b][1 .. S-1] of every row from the history tokens[b, :len] (the whole workgroup; see pbl_ngram_draft in include/pbl.h)
__device__ void spec_draft(const SpecArgs& a, int64_t len) {
    __shared__ int sh_best[SPEC_WAVES][SPEC_MAX_NGRAM];
    const int tid = threadIdx.x, K = a.S - 1;
    const int n_len = int(len);
    for (int b = 0; b < a.B; ++b) {
        const int64_t* h = a.tokens + int64_t(b) * a.total;
        int best[SPEC_MAX_NGRAM] = {0, 0, 0, 0};           // best[N - 1]: the latest end e of an earlier occurrence of the last N tokens
        const bool search = a.unfinished[b] && n_len >= 2;
        if (search) {
            int64_t t[SPEC_MAX_NGRAM];
#pragma unroll
            for (int k = 0; k < SPEC_MAX_NGRAM; ++k) t[k] = k < n_len ? h[n_len - 1 - k] : 0;
            const int nmax = min(a.max_ngram, n_len - 1);
            for (int e = 1 + tid; e < n_len; e += SPEC_THREADS) {          // the occurrence is h[e - N, e), e < len
                if (h[e - 1] != t[0]) continue;
                int m = 1;
                while (m < nmax && m < e && h[e - 1 - m] == t[m]) ++m;
#pragma unroll
                for (int k = 0; k < SPEC_MAX_NGRAM; ++k)
                    if (k < m) best[k] = max(best[k], e);
            }
        }
#pragma unroll
        for (int k = 0; k < SPEC_MAX_NGRAM; ++k) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) best[k] = max(best[k], __shfl_xor(best[k], off));
        }
        __syncthreads();                                                   // (the previous row's sh_best has been read)
        if ((tid & 63) == 0)
            for (int k = 0; k < SPEC_MAX_NGRAM; ++k) sh_best[tid >> 6][k] = best[k];
        __syncthreads();
        if (tid == 0) {
            int e = 0;
            for (int k = min(a.max_ngram, SPEC_MAX_NGRAM) - 1; k >= 0 && !e; --k)
                for (int w = 0; w < SPEC_WAVES; ++w) e = max(e, sh_best[w][k]);
            int64_t* d = a.ids + int64_t(b) * a.S;
            for (int j = 0; j < K; ++j) {                                  // a self-overlapping copy: ext = h followed by the drafts
                const int src = e + j;
                d[1 + j] = !e ? d[0] : (src < n_len ? h[src] : d[1 + src - n_len]);
            }
        }
    }
}

__global__ __launch_bounds__(SPEC_THREADS) void pbl_spec_finish_kernel(SpecArgs a) {
    __shared__ int64_t sh_len;
    __shared__ int sh_back, sh_draft;
    const int tid = threadIdx.x;
    if (tid == 0) {
        const int64_t c = *a.cursor;
        int back = 0, draft = 1;
        if (a.verify) {
            const int64_t* am = a.stats + SPEC_STAT_ARGMAX;
            int live = 0, n = a.S - 1;
            for (int b = 0; b < a.B; ++b) {
                if (!a.unfinished[b]) continue;
                ++live;
                int nb = 0;
                while (nb < a.S - 1 && a.ids[b * a.S + nb + 1] == am[b * a.S + nb]) ++nb;
                n = min(n, nb);
            }
            if (c < 1 || c > a.total) atomicOr(a.status, 2);
            if (c < 1 || c >= a.total || !live) {          // finished: nothing is emitted, the step's S positions are taken back
                back = a.S;
                draft = 0;
                *a.n_unfinished = live;
            } else {
                const int w = int(min(int64_t(n + 1), a.total - c));
                live = 0;
                for (int b = 0; b < a.B; ++b) {
                    uint8_t unf = a.unfinished[b];
                    int64_t tok = a.pad;
                    for (int j = 0; j < w; ++j) {
                        tok = unf ? am[b * a.S + j] : a.pad;
                        for (int q = 0; unf && q < a.n_eos; ++q)
                            if (tok == a.eos[q]) unf = 0;
                        a.tokens[int64_t(b) * a.total + c + j] = tok;
                    }
                    a.unfinished[b] = unf;
                    a.ids[b * a.S] = tok;
                    live += unf;
                }
                *a.cursor = c + w;
                *a.n_unfinished = live;
                a.stats[0] += 1;
                a.stats[1] += w - 1;
                a.stats[2] += w;
                back = a.S - 1 - n;
                sh_len = c + w;
            }
        } else {
            sh_len = c < 0 ? 0 : (c > a.total ? a.total : c);
        }
        sh_back = back;
        sh_draft = draft;
    }
    __syncthreads();
    const int back = sh_back;
    if (back)
        for (int l = tid; l < a.L; l += SPEC_THREADS) *a.positions[l] -= back;
    if (sh_draft && a.S > 1 && a.max_ngram > 0) spec_draft(a, sh_len);
}

bool spec_overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}

// every output apart from every other one and from the inputs
bool spec_aliased(const void* const* outs, const size_t* outb, int n_out, const void* const* ins, const size_t* inb, int n_in) {
    for (int i = 0; i < n_out; ++i) {
        for (int j = 0; j < n_in; ++j)
            if (spec_overlaps(outs[i], outb[i], ins[j], inb[j])) return true;
        for (int j = i + 1; j < n_out; ++j)
            if (spec_overlaps(outs[i], outb[i], outs[j], outb[j])) return true;
    }
    return false;
}

int spec_launch_finish(const SpecArgs& a, void* stream) {
    void* argv[] = {const_cast<SpecArgs*>(&a)};
    return hipLaunchKernel(reinterpret_cast<const void*>(pbl_spec_finish_kernel), dim3(1), dim3(SPEC_THREADS), argv, 0,
                           static_cast<hipStream_t>(stream)) == hipSuccess ? PBL_OK : PBL_ERR_LAUNCH;
}

}  // namespace

extern "C" {

int pbl_spec_verify_f16(const void* logits, int64_t ld_b, int64_t ld_s, int B, int S, int V, int64_t* ids, int64_t* tokens,
                        int64_t total, int64_t* cursor, uint8_t* unfinished, const int64_t* eos, int n_eos, int64_t pad,
                        int32_t* n_unfinished, int32_t* status, int64_t* const* positions, int L, int64_t* stats, int max_ngram,
                        void* stream) {
    if (!logits || !ids || !tokens || !cursor || !unfinished || !n_unfinished || !status || !stats || B < 1 || S < 1 || V < 1 ||
        total < 1 || n_eos < 0 || (n_eos > 0 && !eos) || L < 0 || (L > 0 && !positions) || max_ngram < 0 || max_ngram > SPEC_MAX_NGRAM ||
        (S > 1 && ld_s < V) || (B > 1 && ld_b < (S > 1 ? (S - 1) * ld_s : 0) + V))
        return PBL_ERR_INVALID_ARG;
    const void* ins[3] = {logits, eos, positions};
    const size_t inb[3] = {size_t((B - 1) * ld_b + (S - 1) * ld_s + V) * 2, size_t(n_eos) * 8, size_t(L) * 8};
    const void* outs[7] = {ids, tokens, cursor, unfinished, n_unfinished, status, stats};
    const size_t outb[7] = {size_t(B) * S * 8, size_t(B) * size_t(total) * 8, 8, size_t(B), 4, 4, PBL_SPEC_STATS_WORDS * 8};
    if (spec_aliased(outs, outb, 7, ins, inb, 3)) return PBL_ERR_INVALID_ARG;
    if (int64_t(B) * S > SPEC_MAX_ROWS || V > SPEC_MAX_V || total > INT32_MAX) return PBL_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint16_t* lg = static_cast<const uint16_t*>(logits);
    void* argv[] = {&lg, &ld_b, &ld_s, &S, &V, &stats};
    if (hipLaunchKernel(reinterpret_cast<const void*>(pbl_spec_argmax_kernel), dim3(B * S), dim3(SPEC_THREADS), argv, 0, st) != hipSuccess)
        return PBL_ERR_LAUNCH;
    SpecArgs a{};
    a.ids = ids; a.tokens = tokens; a.total = total; a.cursor = cursor; a.unfinished = unfinished; a.eos = eos; a.pad = pad;
    a.n_unfinished = n_unfinished; a.status = status; a.positions = positions; a.stats = stats;
    a.B = B; a.S = S; a.n_eos = n_eos; a.L = L; a.max_ngram = max_ngram; a.verify = 1;
    return spec_launch_finish(a, stream);
}

int pbl_ngram_draft(const int64_t* tokens, int64_t total, int B, const int64_t* cursor, const uint8_t* unfinished, int64_t* ids, int S,
                    int max_ngram, void* stream) {
    if (!tokens || !cursor || !unfinished || !ids || B < 1 || S < 1 || total < 1 || max_ngram < 1 || max_ngram > SPEC_MAX_NGRAM)
        return PBL_ERR_INVALID_ARG;
    const void* ins[3] = {tokens, cursor, unfinished};
    const size_t inb[3] = {size_t(B) * size_t(total) * 8, 8, size_t(B)};
    const void* outs[1] = {ids};
    const size_t outb[1] = {size_t(B) * S * 8};
    if (spec_aliased(outs, outb, 1, ins, inb, 3)) return PBL_ERR_INVALID_ARG;
    if (int64_t(B) * S > SPEC_MAX_ROWS || total > INT32_MAX) return PBL_ERR_UNSUPPORTED;
    if (S == 1) return PBL_OK;                             // no draft slots
    SpecArgs a{};
    a.ids = ids; a.tokens = const_cast<int64_t*>(tokens); a.total = total; a.cursor = const_cast<int64_t*>(cursor);
    a.unfinished = const_cast<uint8_t*>(unfinished);
    a.B = B; a.S = S; a.max_ngram = max_ngram; a.verify = 0;
    return spec_launch_finish(a, stream);
}

}  // extern "C"
