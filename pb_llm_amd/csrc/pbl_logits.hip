// pbl_logits.hip -- the logits processors of a decode step (pbl_process_logits_f16), in front of pbl_select_token_f16: repetition
// penalty, no-repeat n-grams and the minimum-length block of the eos ids, in place on the fp16 logits, on the device.
//
// One workgroup of 1024 threads per row.  The row's history h = tokens[b, 0 : col0 + step) is walked 1024 positions per pass; every
// access to the logits is one 2-byte element at an index taken from h, so neither the row stride nor its alignment matters.
//
// Order independence.  The penalty must hit every DISTINCT id of h exactly once, wherever and however often the id occurs.  The
// kernel does not look for "the first occurrence": it reads the ORIGINAL value of logit[h[i]] for every position i into a scratch
// row first (phase A), waits for the whole workgroup, and only then stores penalty(original) to logit[h[i]] for every i (phase B).
// All occurrences of an id have read the same original, so they store the same bits -- the outcome does not depend on which store
// lands last, nor on the pass an occurrence falls into.  A thread reads back only the scratch elements it wrote itself.  The two
// -inf rules store one constant, behind a barrier each: a ban always wins over a penalty.  Nothing is accumulated and no atomic is
// used: the same inputs give the same bits on every run, eager or replayed.
//
// No allocation, no synchronisation, nothing read on the host; the step counter is read on the device and left as it is, so one
// captured graph serves every step.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pbl.h"

namespace {

constexpr int LGT_THREADS = 1024;
constexpr int LGT_MAX_V = 1 << 19;             // pbl_select_token_f16's scope
constexpr int LGT_MAX_NGRAM = 8;
constexpr uint16_t LGT_NINF = 0xfc00u;

struct LgtArgs {
    uint16_t* logits;               // row b at logits + b * ld
    int64_t ld;
    const int64_t* tokens;          // [B, total]
    int64_t total, col0;
    const int64_t* step;
    const int64_t* eos;
    int64_t min_new, min_length;
    uint16_t* scratch;              // [B, total] fp16, or NULL without a penalty
    float penalty;
    int ngram, n_eos, V;
};

__global__ __launch_bounds__(LGT_THREADS) void pbl_process_logits_kernel(LgtArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t step = *a.step;
    int64_t len = a.col0 + step;
    len = len < 0 ? 0 : (len > a.total ? a.total : len);
    uint16_t* row = a.logits + int64_t(b) * a.ld;
    const int64_t* h = a.tokens + int64_t(b) * a.total;
    const int64_t V = a.V;

    if (a.penalty != 1.f) {                    // rule 1: every original first, then every store
        uint16_t* orig = a.scratch + int64_t(b) * a.total;
        for (int64_t i = tid; i < len; i += LGT_THREADS) {
            const int64_t t = h[i];
            if (t >= 0 && t < V) orig[i] = row[t];
        }
        __syncthreads();
        for (int64_t i = tid; i < len; i += LGT_THREADS) {
            const int64_t t = h[i];
            if (t >= 0 && t < V) {
                const float x = float(__builtin_bit_cast(_Float16, orig[i]));
                const float y = x < 0.f ? x * a.penalty : __fdiv_rn(x, a.penalty);
                row[t] = __builtin_bit_cast(uint16_t, _Float16(y));            // round to nearest even
            }
        }
    }
    __syncthreads();

    const int n = a.ngram;
    if (n > 0 && len >= n) {                   // rule 2: a window that repeats the last n - 1 tokens bans the token behind it
        int64_t suffix[LGT_MAX_NGRAM - 1];
#pragma unroll
        for (int j = 0; j < LGT_MAX_NGRAM - 1; ++j) suffix[j] = j < n - 1 ? h[len - (n - 1) + j] : 0;
        for (int64_t i = tid; i + n <= len; i += LGT_THREADS) {
            bool match = true;
#pragma unroll
            for (int j = 0; j < LGT_MAX_NGRAM - 1; ++j)
                if (j < n - 1 && h[i + j] != suffix[j]) match = false;
            const int64_t t = h[i + n - 1];
            if (match && t >= 0 && t < V) row[t] = LGT_NINF;
        }
    }
    __syncthreads();

    if (step < a.min_new || a.col0 + step < a.min_length)                       // rule 3
        for (int j = tid; j < a.n_eos; j += LGT_THREADS) {
            const int64_t t = a.eos[j];
            if (t >= 0 && t < V) row[t] = LGT_NINF;
        }
}

bool lgt_overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && x < y + nb && y < x + na;
}

}  // namespace

extern "C" {

int pbl_process_logits_f16(void* logits, int64_t ld, int B, int V, const int64_t* tokens, int64_t total, int64_t col0,
                           const int64_t* step, float repetition_penalty, int no_repeat_ngram_size, int64_t min_new_tokens,
                           int64_t min_length, const int64_t* eos, int n_eos, void* scratch, void* stream) {
    if (!logits || !tokens || !step || B < 1 || V < 1 || ld < V || total < 1 || col0 < 0 || col0 >= total || n_eos < 0 ||
        (n_eos > 0 && !eos))
        return PBL_ERR_INVALID_ARG;
    if (!(repetition_penalty > 0.f) || no_repeat_ngram_size < 0 || no_repeat_ngram_size > LGT_MAX_NGRAM)
        return PBL_ERR_INVALID_ARG;
    const bool penalise = repetition_penalty != 1.f;
    if (penalise && !scratch) return PBL_ERR_INVALID_ARG;
    if (total >= (int64_t(1) << 31)) return PBL_ERR_UNSUPPORTED;                // (before the byte counts below are formed)
    const void* ins[3] = {tokens, step, eos};
    const size_t inb[3] = {size_t(B) * size_t(total) * 8, 8, size_t(n_eos) * 8};
    const void* outs[2] = {logits, penalise ? scratch : nullptr};
    const size_t outb[2] = {size_t((int64_t(B) - 1) * ld + V) * 2, size_t(B) * size_t(total) * 2};
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 3; ++j)
            if (lgt_overlaps(outs[i], outb[i], ins[j], inb[j])) return PBL_ERR_INVALID_ARG;
    if (lgt_overlaps(outs[0], outb[0], outs[1], outb[1])) return PBL_ERR_INVALID_ARG;
    if (V > LGT_MAX_V) return PBL_ERR_UNSUPPORTED;
    const bool block_eos = n_eos > 0 && (min_new_tokens > 0 || min_length > col0);
    if (!penalise && no_repeat_ngram_size == 0 && !block_eos) return PBL_OK;    // every rule off: nothing to launch
    LgtArgs a{};
    a.logits = static_cast<uint16_t*>(logits);
    a.ld = ld;
    a.tokens = tokens; a.total = total; a.col0 = col0; a.step = step; a.eos = eos;
    a.min_new = min_new_tokens; a.min_length = min_length;
    a.scratch = static_cast<uint16_t*>(scratch);
    a.penalty = repetition_penalty; a.ngram = no_repeat_ngram_size; a.n_eos = n_eos; a.V = V;
    void* argv[] = {&a};
    return hipLaunchKernel(reinterpret_cast<const void*>(pbl_process_logits_kernel), dim3(B), dim3(LGT_THREADS), argv, 0,
                           static_cast<hipStream_t>(stream)) == hipSuccess ? PBL_OK : PBL_ERR_LAUNCH;
}

}  // extern "C"
