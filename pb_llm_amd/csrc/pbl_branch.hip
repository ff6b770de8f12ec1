// pbl_branch.hip -- branch attention over a static KV cache (pbl_branch_attn_f16): pbl_prefill_attn_f16 for the rows of several
// continuations packed behind ONE shared context (scoring.loglikelihood(share_prefix=True)).
//
// The S new rows of a sequence are [ trunk: the context | branch 0 | branch 1 | ... | padding ].  Query row s sees absolute key k iff
//     k <= p + s   and   ( k < p + trunk[b]   or   k >= p + lo[b, s] )
// with lo[b, s] the packed index of the first row of s's own branch (0 for a trunk row, s for a padding row): the context and its own
// continuation, nothing of its siblings.  Everything else is pbl_prefill.hip's: the append, the tiles laid from absolute key row 0,
// the fp16 P relative to m - 14, the fixed order, the advance of *pos.  The kernel is pbl_prefill_attn_kernel with the BranchMask
// policy (pbl_prefill_kernels.h), which adds to the causal test of a score the two comparisons above and nothing else; with lo = 0
// everywhere it computes what the causal instantiation computes, bit for bit, and a row's result depends only on its own q, the keys
// it sees and the tiling.
//
// Key 0.  The online softmax starts from m = -inf and relies on key 0 being seen by every row, so that m is finite from tile 0 on
// (exp2(-inf - -inf) is NaN).  The policy keeps that true for ANY table: lo is clamped to [0, s], p + trunk to [1, max_len].  Callers
// pass trunk >= 1; trunk < 1 at p = 0 behaves as trunk = 1.
//
// Masked keys.  A masked score is -inf whatever the key holds, so P = 0.  0 x NaN is NaN inside an MFMA and one V tile serves rows
// that see a key and rows that do not, so this instantiation stores Inf / NaN value elements into LDS as +0 (rows at or beyond
// min(p + S, max_len) enter as zeros in every instantiation): a key a row does not see contributes exactly nothing.  K is not
// touched: a NaN key gives NaN in the rows that see it.
//
// No tile skipping.  A key tile wholly between p + trunk and the smallest p + lo of a wave's 32 rows is masked for the whole wave, and
// visiting it is an exact no-op (P = 0, rescale factor 1), so a wave could leave it out without changing a bit.  Measured on the
// hellaswag shape (context 64, four branches of 23 rows: one such tile for one wave of one workgroup) it pays nothing -- 31.9 us with
// the skip, 32.5 us without, spreads of 7 - 30 % -- so the kernel visits every tile below the diagonal, as the causal one does.
#include "pbl_prefill_kernels.h"

extern "C" {

int pbl_branch_attn_f16(const void* q, const int64_t* q_stride, const void* k_new, const int64_t* k_stride, const void* v_new,
                        const int64_t* v_stride, void* k_cache, void* v_cache, const int32_t* trunk, const int32_t* lo, int B, int S,
                        int Hq, int Hkv, int D, int max_len, float scaling, int64_t* pos, void* out, uint32_t ldo, void* stream) {
    if (!trunk || !lo) return PBL_ERR_INVALID_ARG;
    const int rc = prefill_check(q, q_stride, k_new, k_stride, v_new, v_stride, k_cache, v_cache, size_t(D) * 2, nullptr, 0, B, S, Hq, Hkv,
                                 D, max_len, pos, out, ldo);
    if (rc == PBL_ERR_INVALID_ARG) return rc;
    {                                                       // the tables are inputs: no output may overlap them
        const size_t cacheb = size_t(B) * Hkv * max_len * size_t(D) * 2;
        const size_t ob = size_t((int64_t(B) * S - 1) * ldo + int64_t(Hq) * D) * 2;
        const void* outs[4] = {k_cache, v_cache, out, pos};
        const size_t outb[4] = {cacheb, cacheb, ob, 8};
        for (int i = 0; i < 4; ++i)
            if (pf_overlaps(outs[i], outb[i], trunk, size_t(B) * 4) || pf_overlaps(outs[i], outb[i], lo, size_t(B) * S * 4))
                return PBL_ERR_INVALID_ARG;
    }
    if (rc != PBL_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (prefill_append(k_new, k_stride, v_new, v_stride, k_cache, v_cache, B, S, Hkv, D, max_len, pos, st) != PBL_OK) return PBL_ERR_LAUNCH;
    PrefillArgsBranch a{};
    a.trunk = trunk;
    a.lo = lo;
    return prefill_attend<BranchMask>(a, q, q_stride, k_cache, v_cache, B, S, Hq, Hkv, D, max_len, scaling, pos, out, ldo, st);
}

}  // extern "C"
