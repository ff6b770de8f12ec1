"""-m gpu: pbl_decode_attn_f16 and pbl_rope_append_f16 over the whole range they accept -- caches of 1 to 65536 rows, i.e. every
chunk size of the split plan (chunk = 32 * ceil(max_len / 4096) keys per split, nsplit = ceil(max_len / chunk) <= 128 splits), full
and cut-short last splits, second trips of the score / value / softmax loops and all four rows in flight -- and at the edges of the
cache (positions below 0 and at or beyond max_len).

The criterion is the one of test_gpu_decode_attention.py: within_ulps (4 fp16 ulps of the output's scale per query row and head)
against the float64 ref64, computed on the device.  Cache rows at or beyond pos + S are NaN, so a read past the valid range shows
up in the output; where a test aims at a guard, the cache is a view into a larger allocation that the test owns, so a broken guard
shows up as a NaN or a changed sentinel and never as an access outside the allocation."""
import ctypes as C

import pytest
import torch

from pb_llm_amd import _lib
from pb_llm_amd.runtime import decode_attention_f16, rope_append_f16, rope_f16
from test_decode_epilogues_cpu import cos_sin
from test_gpu_decode_attention import DEV, built, ref64, within_ulps  # noqa: F401  (built: fixture)
from test_gpu_decode_epilogues import qkv_out

pytestmark = pytest.mark.gpu
SHORT = (1, 5, 31, 32, 33, 100)
LONG = (4097, 4132, 8192, 8200, 12288, 20000, 40000, 65535, 65536)       # 4132: tools/bench_generate.py at context 4096
STRUCTURED = (100, 4132, 20000, 65536)
NAN = float("nan")
SENTINEL = 0x5A5A


def plan(max_len, D):
    """(chunk, nsplit, KP): keys per split, splits, and keys per pass of the partial kernel's workgroup (256 lanes, D / 8 per key)"""
    chunk = 32 * -(-max_len // 4096)
    return chunk, -(-max_len // chunk), 256 // (D // 8)


def positions(max_len, S, D):
    """pos = 0, pos = max_len - S, and for the first, a middle and the last split every pos at which that split is the last
    non-empty one and holds n valid keys, n in {1, KP, KP + 1, 4 KP, 4 KP + 1, 65, chunk - 1, chunk} (where that fits): one pass
    of one row in flight, one more key, all four rows in flight, a second trip of the score / value loops, a second trip of the
    softmax loop, and a split one short of full and full"""
    chunk, nsplit, KP = plan(max_len, D)
    ends = {S, max_len}
    for j in {0, nsplit // 2, nsplit - 1}:
        ends |= {j * chunk + n for n in (1, KP, KP + 1, 4 * KP, 4 * KP + 1, 65, chunk - 1, chunk) if 1 <= n <= chunk}
    return sorted(e - S for e in ends if S <= e <= max_len)


def attend(q, k, v, pos, scaling):
    """the kernel over copies of k / v whose rows at or beyond pos + S are NaN"""
    S = q.shape[2]
    kc, vc = k.clone(), v.clone()
    kc[:, :, pos + S:] = NAN
    vc[:, :, pos + S:] = NAN
    p = torch.tensor(pos, dtype=torch.int64, device=DEV)
    out = decode_attention_f16(q, kc, vc, p, scaling)
    assert out.shape == (q.shape[0] * S, q.shape[1] * q.shape[3]) and out.dtype == torch.float16
    assert int(p) == pos + S, "the position advances by S"
    return out


def test_the_lengths_cover_every_chunk_size_and_both_kinds_of_last_split():
    chunks = {plan(L, 64)[0] for L in SHORT + LONG}
    assert chunks == {32, 64, 96, 160, 320, 512}
    assert {plan(L, 64)[1] for L in SHORT + LONG} >= {1, 2, 4, 65, 128}
    for c in (32, 64, 96, 512):                                             # a last split that is full and one cut short by max_len
        assert {L % c == 0 for L in SHORT + LONG if plan(L, 64)[0] == c} == {True, False}, c
    assert positions(4132, 1, 128)[-3:] == [4096 + 16 - 1, 4096 + 17 - 1, 4131] and plan(4132, 128) == (64, 65, 16)


@pytest.mark.parametrize("heads", [(8, 2), (4, 4)])
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("max_len", SHORT + LONG)
def test_decode_attention_over_the_supported_range(max_len, D, B, heads):
    Hq, Hkv = heads
    g = torch.Generator(device=DEV).manual_seed(7 * max_len + D + 10 * B + Hq)
    k = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    v = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    scaling = D ** -0.5
    for S in range(1, min(4, max_len) + 1):
        q = (torch.randn(B, Hq, S, D, generator=g, device=DEV) * 2).half()
        for pos in positions(max_len, S, D):
            within_ulps(attend(q, k, v, pos, scaling), ref64(q, k, v, pos, scaling), D, f"max_len={max_len} S={S} pos={pos}")


# ---------------------------------------------------------------- structured inputs
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("max_len", STRUCTURED)
def test_one_dominant_key(max_len, D):
    """one key whose score is >= 30 above every other: the rows that may see it return its V row (the rest weighs < 65536 e^-30),
    the rows before it must not see it.  Placed in the first split, in a middle split, and at row pos + s for every s: row s's
    own key, which rows < s must not see -- the causal edge inside the S rows"""
    B, Hq, Hkv, S = 1, 8, 2, 4
    chunk, nsplit, _ = plan(max_len, D)
    scaling = D ** -0.5
    g = torch.Generator(device=DEV).manual_seed(max_len + D)
    q = torch.randn(B, Hq, S, D, generator=g, device=DEV).half()
    k0 = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    v = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    q[..., 0] = 8.0                                                           # the dominant key is big * e_0: score 8 big scaling
    k0[..., 0] = 0.0
    others = float((q.double() @ k0.double().repeat_interleave(Hq // Hkv, 1).transpose(-1, -2)).amax()) * scaling
    big = float(int((others + 32) / (8 * scaling)) + 1)
    assert big < 2048 and 8 * big * scaling >= others + 30
    pos = max_len - S
    rows = {min(3, pos), (nsplit // 2) * chunk + min(5, chunk - 1)} | {pos + s for s in range(S)}
    for r in sorted(r for r in rows if r < max_len):
        k = k0.clone()
        k[:, :, r] = 0.0
        k[:, :, r, 0] = big
        out = attend(q, k, v, pos, scaling)
        within_ulps(out, ref64(q, k, v, pos, scaling), D, f"max_len={max_len} dominant key at row {r} vs float64")
        sees = [s for s in range(S) if r <= pos + s]
        vrow = v[:, :, r].repeat_interleave(Hq // Hkv, 1).reshape(B, 1, Hq * D).expand(B, len(sees), Hq * D).reshape(-1, Hq * D)
        within_ulps(out.view(B, S, -1)[:, sees].reshape(-1, Hq * D), vrow, D, f"max_len={max_len} dominant key at row {r} vs its V row")
        for s in range(S):
            if s not in sees:
                assert not torch.equal(out.view(B, S, -1)[:, s], vrow[:B]), f"row {s} saw key {r} > pos + s = {pos + s}"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("max_len", STRUCTURED)
def test_wide_score_range(max_len, D):
    """scaled scores spanning several thousand: whole splits carry weight 0 in the combine and most exp(score - m) inside a split
    underflow"""
    B, Hq, Hkv, S = 1, 8, 2, 4
    chunk = plan(max_len, D)[0]
    scaling = D ** -0.5
    g = torch.Generator(device=DEV).manual_seed(3 * max_len + D)
    q = (torch.randn(B, Hq, S, D, generator=g, device=DEV) * 32).half()
    k = (torch.randn(B, Hkv, max_len, D, generator=g, device=DEV) * 32).half()
    v = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    sc = (q.double() @ k.double().repeat_interleave(Hq // Hkv, 1).transpose(-1, -2)) * scaling
    assert float((sc.amax(-1) - sc.amin(-1)).min()) > 3000, "the inputs do not span what this test is for"
    for pos in sorted({0, min(chunk + 1, max_len - S), (max_len - S) // 2, max_len - S}):
        within_ulps(attend(q, k, v, pos, scaling), ref64(q, k, v, pos, scaling), D, f"max_len={max_len} pos={pos}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("max_len", STRUCTURED)
def test_identical_keys(max_len, D):
    """every key the same: a uniform softmax, the output is the mean of V over rows [0, pos + s]"""
    B, Hq, Hkv, S = 1, 8, 2, 4
    chunk = plan(max_len, D)[0]
    scaling = D ** -0.5
    g = torch.Generator(device=DEV).manual_seed(5 * max_len + D)
    q = (torch.randn(B, Hq, S, D, generator=g, device=DEV) * 2).half()
    k = torch.randn(B, Hkv, 1, D, generator=g, device=DEV).half().expand(B, Hkv, max_len, D).contiguous()
    v = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    means = v.double().cumsum(2) / torch.arange(1, max_len + 1, device=DEV, dtype=torch.float64)[:, None]
    for pos in sorted({0, min(chunk + 1, max_len - S), (max_len - S) // 2, max_len - S}):
        ref = ref64(q, k, v, pos, scaling)
        mean = means[:, :, pos:pos + S].repeat_interleave(Hq // Hkv, 1).transpose(1, 2).reshape(B * S, Hq * D)
        torch.testing.assert_close(ref, mean, rtol=1e-9, atol=1e-12)
        within_ulps(attend(q, k, v, pos, scaling), ref, D, f"max_len={max_len} pos={pos}")


# ---------------------------------------------------------------- what the entry may write
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("max_len", [100, 65536])
def test_workspace_and_output_bounds(max_len, D):
    """the C entry with a workspace of exactly pbl_decode_attn_workspace_bytes inside a buffer of sentinel bytes, and ldo > Hq D
    with sentinel padding columns and a sentinel row before and after the output: no sentinel changes"""
    B, S, Hq, Hkv, PAD = 2, 3, 8, 2, 4096
    L = _lib.lib()
    scaling = D ** -0.5
    g = torch.Generator(device=DEV).manual_seed(11 * max_len + D)
    q = (torch.randn(B, Hq, S, D, generator=g, device=DEV) * 2).half()
    k = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    v = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    need = int(L.pbl_decode_attn_workspace_bytes(B, S, Hq, D, max_len))
    ldo = Hq * D + 40
    for pos in (5, max_len - S):                                              # pos = 5: every split but the first is empty
        ws = torch.full((need + 2 * PAD,), 0xA5, dtype=torch.uint8, device=DEV)
        ob = torch.full((B * S + 2, ldo), SENTINEL, dtype=torch.int16, device=DEV)
        p = torch.tensor(pos, dtype=torch.int64, device=DEV)
        assert (ws.data_ptr() + PAD) % 16 == 0
        rc = L.pbl_decode_attn_f16(q.data_ptr(), (C.c_int64 * 3)(*q.stride()[:3]), k.data_ptr(), v.data_ptr(), B, S, Hq, Hkv, D,
                                   max_len, scaling, p.data_ptr(), ob.data_ptr() + 2 * ldo, ldo, ws.data_ptr() + PAD, need,
                                   torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.PBL_OK
        torch.cuda.synchronize()
        assert bool((ws[:PAD] == 0xA5).all()) and bool((ws[PAD + need:] == 0xA5).all()), "a write outside the workspace"
        assert bool((ob[0] == SENTINEL).all()) and bool((ob[-1] == SENTINEL).all()), "a write before or after the output"
        assert bool((ob[1:-1, Hq * D:] == SENTINEL).all()), "a write into the padding columns"
        got = ob[1:-1, :Hq * D].contiguous().view(torch.float16)
        within_ulps(got, ref64(q, k, v, pos, scaling), D, f"max_len={max_len} pos={pos}")
        assert int(p) == pos + S
        assert L.pbl_decode_attn_f16(q.data_ptr(), (C.c_int64 * 3)(*q.stride()[:3]), k.data_ptr(), v.data_ptr(), B, S, Hq, Hkv, D,
                                     max_len, scaling, p.data_ptr(), ob.data_ptr() + 2 * ldo, ldo, ws.data_ptr() + PAD, need - 1,
                                     torch.cuda.current_stream().cuda_stream) == _lib.PBL_ERR_INVALID_ARG


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("max_len", [100, 4132])
def test_positions_outside_the_cache_are_clamped(max_len, D):
    """the documented behaviour: a negative pos counts as 0, and query row s attends to keys [0, min(pos + s + 1, max_len)).  The
    cache is the first max_len rows of a larger allocation (B = Hkv = 1: a contiguous view) whose later rows are NaN"""
    B, Hq, Hkv, EXTRA = 1, 4, 1, 64
    scaling = D ** -0.5
    g = torch.Generator(device=DEV).manual_seed(13 * max_len + D)
    whole_k = torch.randn(B, Hkv, max_len + EXTRA, D, generator=g, device=DEV).half()
    whole_v = torch.randn(B, Hkv, max_len + EXTRA, D, generator=g, device=DEV).half()
    k, v = whole_k[:, :, :max_len].clone(), whole_v[:, :, :max_len].clone()
    for S in range(1, 5):
        q = (torch.randn(B, Hq, S, D, generator=g, device=DEV) * 2).half()
        for pos in [-3] + list(range(max_len - S + 1, max_len + 2)):
            first = max(pos, 0)
            wk, wv = whole_k.clone(), whole_v.clone()
            wk[:, :, first + S:] = NAN
            wv[:, :, first + S:] = NAN
            wk[:, :, max_len:] = NAN
            wv[:, :, max_len:] = NAN
            kc, vc = wk[:, :, :max_len], wv[:, :, :max_len]
            assert kc.is_contiguous() and kc.data_ptr() == wk.data_ptr()
            p = torch.tensor(pos, dtype=torch.int64, device=DEV)
            out = decode_attention_f16(q, kc, vc, p, scaling)
            assert int(p) == pos + S
            ref = torch.cat([ref64(q[:, :, s:s + 1], k, v, min(first + s, max_len - 1), scaling) for s in range(S)])
            assert bool(torch.isfinite(out).all()), f"max_len={max_len} S={S} pos={pos}: a row beyond the valid keys was read"
            within_ulps(out, ref, D, f"max_len={max_len} S={S} pos={pos}")


def test_captured_step_across_the_64_key_split_boundaries():
    """test_captured_step_is_bit_stable_and_position_independent at max_len = 4132 (chunk 64, 65 splits): one captured step replayed
    over positions 4090 .. 4131 is bit-equal to the eager call"""
    from transformers import LlamaConfig
    B, S, Hq, Hkv, D, L = 1, 1, 8, 2, 128, 4132
    cfg = LlamaConfig(hidden_size=Hq * D, num_attention_heads=Hq, num_key_value_heads=Hkv, max_position_embeddings=8192)
    y, _, _ = qkv_out(B, S, Hq, Hkv, D, 5)
    cos, sin = cos_sin(cfg, [[17]], DEV)
    kc = torch.randn(B, Hkv, L, D, device=DEV).half()
    vc = torch.randn(B, Hkv, L, D, device=DEV).half()
    p = torch.tensor(4100, dtype=torch.int64, device=DEV)

    def step():
        q = rope_append_f16(y, 0, Hq * D, (Hq + Hkv) * D, B, S, Hq, Hkv, D, cos, sin, kc, vc, p)
        return decode_attention_f16(q, kc, vc, p, D ** -0.5)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    p.fill_(4100)
    with torch.cuda.graph(graph):
        out = step()
    for pos in range(4090, 4132):
        p.fill_(pos)
        graph.replay()
        replayed = out.clone()
        p.fill_(pos)
        eager = step()
        assert torch.equal(replayed.view(torch.int16), eager.view(torch.int16)), pos
        assert int(p) == pos + 1
        ref = ref64(rope_f16(y, 0, Hq * D, B, S, Hq, Hkv, D, cos, sin)[0], kc, vc, pos, D ** -0.5)
        within_ulps(replayed, ref, D, f"replayed at pos={pos}")


# ---------------------------------------------------------------- the append at the edges of the cache
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B,S", [(1, 1), (1, 4), (2, 3), (4, 2)])
def test_rope_append_at_the_edges_of_the_cache(B, S, D):
    """positions max_len - S + 1 .. max_len + 1 and pos = -1: rows inside [0, max_len) receive what test_rope_append_equals_hf
    expects, nothing else changes -- the caches lie inside larger allocations with sentinel rows before and after them -- and q
    is written in full, bit-equal to rope_f16"""
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    Hq, Hkv, L, GUARD = 8, 2, 96, 8 * D
    cfg = LlamaConfig(hidden_size=Hq * D, num_attention_heads=Hq, num_key_value_heads=Hkv, max_position_embeddings=131072)
    y, q, k = qkv_out(B, S, Hq, Hkv, D, 17 * B + S + D)
    v = y[:, (Hq + Hkv) * D:].reshape(B, S, Hkv, D).transpose(1, 2)
    n = B * Hkv * L * D

    def guarded():
        whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
        whole[GUARD:GUARD + n] = torch.randn(n, device=DEV).half().view(torch.int16)
        return whole

    def cache_of(whole):
        return whole[GUARD:GUARD + n].view(torch.float16).view(B, Hkv, L, D)

    for pos in [-1] + list(range(L - S + 1, L + 2)):
        cos, sin = cos_sin(cfg, [[abs(pos + s) for s in range(S)]], DEV)
        wk, wv = guarded(), guarded()
        ek, ev = wk.clone(), wv.clone()                                         # what the allocations must hold afterwards
        q_ref, k_ref = apply_rotary_pos_emb(q, k, cos, sin)
        for s in range(S):
            if 0 <= pos + s < L:
                cache_of(ek)[:, :, pos + s] = k_ref[:, :, s]
                cache_of(ev)[:, :, pos + s] = v[:, :, s]
        kc, vc = cache_of(wk), cache_of(wv)
        assert kc.is_contiguous() and kc.data_ptr() % 16 == 0
        p = torch.tensor(pos, dtype=torch.int64, device=DEV)
        got = rope_append_f16(y, 0, Hq * D, (Hq + Hkv) * D, B, S, Hq, Hkv, D, cos, sin, kc, vc, p)
        q_rope = rope_f16(y, 0, Hq * D, B, S, Hq, Hkv, D, cos, sin)[0]
        assert got.shape == q_rope.shape and got.stride() == q_rope.stride()
        assert torch.equal(got.view(torch.int16), q_rope.view(torch.int16)) and torch.equal(got, q_ref)
        for name, w, e in (("k", wk, ek), ("v", wv, ev)):
            diff = (w != e).nonzero().flatten()
            assert len(diff) == 0, f"pos={pos}: the {name} allocation differs at elements {(diff[:4] - GUARD).tolist()} of the cache " \
                                   f"({len(diff)} in all; {n} elements in the cache)"
        assert int(p) == pos
