// pbl_attn.hip -- decode attention over a static KV cache (pbl_decode_attn_f16).
//
// A decode step of S <= 4 new query rows per sequence attends to the keys [0, pos + s] of its layer's cache
// [B, Hkv, max_len, D] fp16 (HF StaticLayer.keys / .values), where pos is the layer's int64 position read on the device.  The
// key range is split flash-decoding style: workgroup (split, h, b) of pbl_attn_partial_kernel owns `chunk` keys of one query head
// and writes, per query row, the fp32 partial (m, l, acc[D]) of its keys -- empty splits write l = 0.  pbl_attn_combine_kernel then
// merges the partials of every split in split order and rounds the output to fp16 once; its first workgroup advances the position
// by S after everything that reads it has run.  Every reduction runs in a fixed order, so the result is bit-stable from run to run.
//
// K / V rows stream straight into VGPRs (one 16-byte load per lane, D / 8 lanes per row): a memory-bound stream that LDS staging
// would only slow down.  Scores (S x chunk) and the cross-wave reduction of acc go through LDS.  No allocation, no host read of
// the position: one captured graph serves every position.
//
// The kernels and the launch plan live in pbl_attn_kernels.h: the FP8 cache's entry (pbl_kv8.hip) runs the same ones.
#include "pbl_attn_kernels.h"

extern "C" {

size_t pbl_decode_attn_workspace_bytes(int B, int S, int Hq, int D, int max_len) {
    return attn_workspace_bytes(B, S, Hq, D, max_len);
}

int pbl_decode_attn_f16(const void* q, const int64_t* q_stride, const void* k_cache, const void* v_cache, int B, int S, int Hq,
                        int Hkv, int D, int max_len, float scaling, int64_t* pos, void* out, uint32_t ldo, void* ws,
                        size_t ws_bytes, void* stream) {
    AttnArgs a{};
    return attn_run(a, q, q_stride, k_cache, v_cache, size_t(D) * 2, nullptr, nullptr, 0, B, S, Hq, Hkv, D, max_len, scaling, pos, out,
                    ldo, ws, ws_bytes, stream);
}

}  // extern "C"
