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
// score x scaling x log2 e).  P is rounded to fp16 for the P V product and the denominator is summed from the ROUNDED P.  P, l and
// the accumulator are kept relative to m_p = fl(m - 14), not to the running maximum m: P = exp2(x - m_p), the rescale factor is
// exp2(m_p_old - m_p_new), and acc / l is free of the factor however m - 14 was rounded in each tile.  fp16 is normal down to 2^-14,
// so with the maximum at 1 every weight below 2^-14 of it lost precision and every one below 2^-25 vanished -- behind an attention
// sink that is thousands of keys, all rounded the same way (far outside the float64 bound of the tests; measured in DESIGN.md).
// The offset moves those two edges to 2^-28 and 2^-39.  m - m_p is 14 to within half of fp32's spacing at m (2^-20 for |m| < 16) and
// at most 15 while |m - 14| < 2^25; beyond, where the spacing is 4 or more and the difference could come out as 16, the offset is
// dropped for that tile (m_p = m).  So P <= 2^15 < 65504 for every input, and the fp32 sums stay below 2^31 max |v| at 65536 keys.
// The accumulator is fp32; acc / l is rounded to fp16 once.  A fully masked tile is an exact no-op (p = 0, rescale factor 1), so a query
// row's result depends only on its own q, its keys and the 64-key tiling from row 0 -- not on which rows share its query tile, on S,
// or on how a prompt was chunked.  No atomics, fixed order: bit-stable from run to run, eager or replayed.
//
// The kernels and the launch helpers live in pbl_prefill_kernels.h: the FP8 cache's entry (pbl_kv8.hip) runs the same attention kernel.
#include "pbl_prefill_kernels.h"

extern "C" {

int pbl_prefill_attn_f16(const void* q, const int64_t* q_stride, const void* k_new, const int64_t* k_stride, const void* v_new,
                         const int64_t* v_stride, void* k_cache, void* v_cache, int B, int S, int Hq, int Hkv, int D, int max_len,
                         float scaling, int64_t* pos, void* out, uint32_t ldo, void* stream) {
    const int rc = prefill_check(q, q_stride, k_new, k_stride, v_new, v_stride, k_cache, v_cache, size_t(D) * 2, nullptr, 0, B, S, Hq, Hkv,
                                 D, max_len, pos, out, ldo);
    if (rc != PBL_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);

    if (prefill_append(k_new, k_stride, v_new, v_stride, k_cache, v_cache, B, S, Hkv, D, max_len, pos, st) != PBL_OK) return PBL_ERR_LAUNCH;

    PrefillArgs a{};
    return prefill_attend(a, q, q_stride, k_cache, v_cache, B, S, Hq, Hkv, D, max_len, scaling, pos, out, ldo, st);
}

}  // extern "C"
