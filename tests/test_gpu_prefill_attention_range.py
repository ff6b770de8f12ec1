"""-m gpu: pbl_prefill_attn_f16 (and, where the FP8 entry shares a code path, pbl_prefill_attn_kv8) over the whole range the entry
accepts -- caches of up to 65536 rows with the last query row's last key at the first key, one short of the end and the end of a
middle and of the last 64-key tile; positions below 0, across max_len and beyond it; the scalar branches of the loads (q / k_new /
v_new whose base or row stride rules out 16-byte accesses) and of the store (out rows that are not 8-byte aligned); one dominant key
at the tile, wave and lane edges of the causal diagonal, scores spanning thousands, a uniform softmax over 65536 keys; and an
attention sink whose later keys weigh less than 2^-14 of the row's maximum.

The criterion is the one of test_gpu_decode_attention.py: within_ulps (4 fp16 ulps of the output's scale per query row and head)
against the float64 ref64, computed on the device.  Cache rows at or beyond min(pos + S, max_len) are NaN, so a read past the valid
range shows up in the output; where a test aims at a guard, the buffer is a view into a larger allocation that the test owns, so a
broken guard shows up as a NaN or a changed sentinel and never as an access outside the allocation.

The numerics the headers state are pinned by ref_tiled, a float64 restatement of the kernel's loop: 64-key tiles from absolute row 0,
a running maximum m in base-2 scores, P, l and o relative to m_p = m - P_OFFSET -- the row's maximum sits at 2^P_OFFSET, so a weight
reaches fp16's subnormal grid only below 2^-28 of the maximum and vanishes below 2^-39 --, alpha = exp2(m_p_old - m_p_new),
P = fp16(exp2(x - m_p)), l summed from the rounded P, o = o alpha + P V, out = o / l.  ref_tiled(offset=0) is the loop with P's
maximum at 1.0; what that costs in the sink cases of section 5 is measured in DESIGN.md ("P's offset")."""
import ctypes as C
import math

import pytest
import torch

from pb_llm_amd import _lib
from pb_llm_amd.runtime import kv8_dequantize, prefill_attention_f16, prefill_attention_kv8
from test_gpu_decode_attention import DEV, ULPS, built, ref64, within_ulps  # noqa: F401  (built: fixture)
from test_gpu_kv8 import fresh_caches, prefill_case, prefill_inputs, quantized, roundtrip
from test_gpu_prefill_attention import bits, check_case, inputs, position

pytestmark = pytest.mark.gpu
TK = 64                                                                   # keys per tile, laid from absolute key row 0
P_OFFSET = 14                                                             # the kernel's P is exp2(x - m + 14), rounded to fp16
LOG2E = 1.4426950408889634
LENGTHS = (4097, 4132, 8200, 20000, 65536)                                # 4132: tools/bench_generate.py at context 4096
S_LONG = (1, 33, 130)                                                     # 130: two query tiles, the second with two live rows
STRUCTURED = (512, 4132, 65536)
NAN = float("nan")
SENTINEL = 0x5A5A
NAN_SENTINEL = 0x7E5A                                                     # an fp16 NaN with a payload: a read shows, a write shows
INF = float("inf")


def ratio(got, ref, D):
    """max error / bound for the prints next to the assertions (within_ulps states the bound: ULPS fp16 ulps of each (row, head)'s
    scale, floored at fp16's smallest normal; it alone decides)"""
    g, r = got.double().view(got.shape[0], -1, D), ref.double().view(ref.shape[0], -1, D)
    tol = ULPS * torch.exp2(torch.floor(torch.log2(r.abs().amax(-1, keepdim=True).clamp_min(2.0 ** -14))) - 10)
    return float(((g - r).abs() / tol).max())


def attend(q, k, v, pos, scaling):
    """the kernel's output for k / v holding the cache AFTER the append: rows [pos, pos + S) go in as k_new / v_new, the cache
    handed over holds NaN from row pos on; the position and the cache rows below pos + S are checked"""
    S = q.shape[2]
    kc, vc = k.clone(), v.clone()
    kc[:, :, pos:] = NAN
    vc[:, :, pos:] = NAN
    p = position(pos)
    out = prefill_attention_f16(q, k[:, :, pos:pos + S], v[:, :, pos:pos + S], kc, vc, p, scaling)
    assert out.shape == (q.shape[0] * S, q.shape[1] * q.shape[3]) and out.dtype == torch.float16
    assert int(p) == pos + S, "the position advances by S"
    for c, full in ((kc, k), (vc, v)):
        assert torch.equal(bits(c[:, :, :pos + S]), bits(full[:, :, :pos + S])) and bool(torch.isnan(c[:, :, pos + S:]).all())
    return out


def ref64_rows(q, k, v, last, scaling):
    """ref64 for query rows that each have their own last key: row s attends to cache rows [0, last[s]]"""
    B, Hq, S, D = q.shape
    G = Hq // k.shape[1]
    n = int(last.max()) + 1
    k, v = (t[:, :, :n].double().repeat_interleave(G, 1) for t in (k, v))
    sc = q.double() @ k.transpose(-1, -2) * scaling
    allowed = torch.arange(n, device=q.device)[None, :] <= last[:, None]
    return (torch.softmax(sc.masked_fill(~allowed, -INF), -1) @ v).transpose(1, 2).reshape(B * S, Hq * D)


def ref_tiled(q, k, v, pos, scaling, offset=P_OFFSET):
    """the kernel's loop in float64 (the module docstring): everything exact but the rounding of P to fp16"""
    B, Hq, S, D = q.shape
    G = Hq // k.shape[1]
    n = pos + S
    k, v = (t[:, :, :n].double().repeat_interleave(G, 1) for t in (k, v))
    x = q.double() @ k.transpose(-1, -2) * (scaling * LOG2E)
    allowed = torch.arange(n, device=q.device)[None, :] <= (pos + torch.arange(S, device=q.device))[:, None]
    x = x.masked_fill(~allowed, -INF)
    m = torch.full((B, Hq, S, 1), -INF, dtype=torch.float64, device=q.device)
    m_p = m.clone()
    l = torch.zeros_like(m)
    o = torch.zeros(B, Hq, S, D, dtype=torch.float64, device=q.device)
    for k0 in range(0, n, TK):
        xt = x[..., k0:k0 + TK]
        m = torch.maximum(m, xt.amax(-1, keepdim=True))                   # finite from tile 0 on: key 0 is valid for every row
        m_p_new = m - offset                                              # exact here; the kernel's fp32 drops the offset at 2^25
        alpha = torch.exp2(m_p - m_p_new)
        p = torch.exp2(xt - m_p_new).half().double()
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p @ v[:, :, k0:k0 + TK]
        m_p = m_p_new
    return (o / l).transpose(1, 2).reshape(B * S, Hq * D)


# ---------------------------------------------------------------- 1. long caches
def tile_edges(max_len):
    """{tile: the rows 64 t, 64 t + 62, 64 t + 63 that exist} for a middle key tile and the last one: a tile's first key, one short
    of full, and full"""
    last = (max_len - 1) // TK
    return {t: [e for e in (TK * t, TK * t + 62, TK * t + 63) if e < max_len] for t in (last // 2, last)}


def positions(max_len, S):
    """pos = 0, pos = max_len - S, and every pos at which the last query row's last key, pos + S - 1, is a row of tile_edges"""
    ends = {S - 1, max_len - 1}
    for rows in tile_edges(max_len).values():
        ends |= set(rows)
    return sorted(e + 1 - S for e in ends if e + 1 - S >= 0)


def test_the_positions_reach_the_edges_of_a_middle_and_the_last_key_tile_at_every_length():
    for L in LENGTHS:
        last = (L - 1) // TK
        mid = last // 2
        assert 0 < mid < last
        for S in S_LONG:
            pos = positions(L, S)
            assert pos[0] == 0 and pos[-1] == L - S and all(0 <= p <= L - S for p in pos)
            ends = {p + S - 1 for p in pos}
            assert {TK * mid, TK * mid + 62, TK * mid + 63} <= ends, (L, S)
            assert TK * last in ends and L - 1 in ends, (L, S)          # the last tile's first key, and its last one that exists
            assert {e for e in (TK * last + 62, TK * last + 63) if e < L} <= ends, (L, S)
    # the last tile holds 1, 36, 8, 32 and 64 rows; only at 65536 has it a row 62 and a row 63
    assert [(L - 1) % TK + 1 for L in LENGTHS] == [1, 36, 8, 32, 64]
    assert positions(65536, 130)[-3:] == [65536 - 64 + 1 - 130, 65535 - 130, 65536 - 130]
    assert positions(4132, 33) == [0, 2048 - 32, 2110 - 32, 2111 - 32, 4096 - 32, 4132 - 33]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("max_len", LENGTHS)
def test_prefill_attention_over_long_caches(max_len, D):
    B, Hq, Hkv = 1, 4, 2
    base_k, base_v, q, k_new, v_new = inputs(B, Hq, Hkv, D, max_len, max(S_LONG), 7 * max_len + D)
    for S in S_LONG:
        for pos in positions(max_len, S):
            check_case(q[:, :, :S], k_new[:, :, :S], v_new[:, :, :S], base_k, base_v, pos, D ** -0.5,
                       f"max_len={max_len} S={S} pos={pos}", sdpa=False)


@pytest.mark.parametrize("D", [64, 128])
def test_random_inputs_follow_the_tiled_restatement(D):
    """two cases of the grid above against ref_tiled: on random inputs the restatement itself sits 0.1 - 0.2 x the bound from ref64"""
    B, Hq, Hkv, max_len, S = 1, 4, 2, 4132, 130
    k, v, q, _, _ = inputs(B, Hq, Hkv, D, max_len, S, 7 * max_len + D)
    for pos in (positions(max_len, S)[2], max_len - S):
        out = attend(q, k, v, pos, D ** -0.5)
        tiled, ref = ref_tiled(q, k, v, pos, D ** -0.5), ref64(q, k, v, pos, D ** -0.5)
        print(f"[tiled] D={D} pos={pos}: kernel vs ref_tiled {ratio(out, tiled, D):.3f}, kernel vs ref64 {ratio(out, ref, D):.3f}, "
              f"ref_tiled vs ref64 {ratio(tiled, ref, D):.3f} x the bound")
        within_ulps(out, tiled, D, f"D={D} pos={pos} vs ref_tiled")
        within_ulps(out, ref, D, f"D={D} pos={pos} vs float64")


# ---------------------------------------------------------------- 2. clipping and clamped positions
def clip_positions(max_len, S):
    """-3 and max_len - S + 1 .. max_len + 2; thinned for S > 5 to both ends, the middle and the positions around max_len"""
    every = [-3] + list(range(max_len - S + 1, max_len + 3))
    if S <= 5:
        return every
    keep = {-3, max_len - S + 1, max_len - S + 2, max_len - S // 2, max_len - 1, max_len, max_len + 1, max_len + 2}
    return sorted(keep & set(every))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("max_len", [100, 200, 4132])
def test_clipping_and_clamped_positions(max_len, D):
    """the documented behaviour: a negative pos counts as 0 and one beyond max_len as max_len; with first = clamp(pos, 0, max_len),
    cache rows [first, min(first + S, max_len)) receive the new rows, query row s attends to rows [0, min(first + s, max_len - 1)],
    and *pos advances by S unclamped.  The cache is the first max_len rows of a larger allocation (B = Hkv = 1: a contiguous view)
    whose later rows are NaN sentinels"""
    B, Hq, Hkv, EXTRA = 1, 4, 1, 8
    scaling = D ** -0.5
    base_k, base_v, q_all, k_all, v_all = inputs(B, Hq, Hkv, D, max_len, max_len, 13 * max_len + D)
    for S in (s for s in (1, 5, 70, 130, max_len) if s <= max_len):
        q, k_new, v_new = q_all[:, :, :S], k_all[:, :, :S], v_all[:, :, :S]
        pos_set = clip_positions(max_len, S)
        assert {-3, max_len - S + 1, max_len, max_len + 2} <= set(pos_set)
        for pos in pos_set:
            what = f"max_len={max_len} S={S} pos={pos}"
            first = min(max(pos, 0), max_len)
            n = min(S, max_len - first)                                    # rows that fit
            wholes, want = [], []
            for base, new in ((base_k, k_new), (base_v, v_new)):
                w = torch.full((B, Hkv, max_len + EXTRA, D), NAN_SENTINEL, dtype=torch.int16, device=DEV).view(torch.float16)
                w[:, :, :first] = base[:, :, :first]
                w[:, :, first:max_len] = NAN
                wholes.append(w)
                e = base.clone()
                e[:, :, first:first + n] = new[:, :, :n]
                want.append(e)
            kc, vc = (w[:, :, :max_len] for w in wholes)
            assert kc.is_contiguous() and kc.data_ptr() == wholes[0].data_ptr()
            p = position(pos)
            out = prefill_attention_f16(q, k_new, v_new, kc, vc, p, scaling)
            assert out.shape == (B * S, Hq * D)
            assert int(p) == pos + S, f"{what}: the position advances by S, unclamped"
            for w, c, e in zip(wholes, (kc, vc), want):
                assert torch.equal(bits(c[:, :, first:first + n]), bits(e[:, :, first:first + n])), f"{what}: appended rows"
                assert torch.equal(bits(c[:, :, :first]), bits(e[:, :, :first])), f"{what}: rows below the position"
                assert bool(torch.isnan(c[:, :, first + n:]).all()), f"{what}: rows above the appended ones"
                assert bool((w[:, :, max_len:].view(torch.int16) == NAN_SENTINEL).all()), f"{what}: a write behind max_len"
            assert bool(torch.isfinite(out).all()), f"{what}: a row beyond the valid keys was read"
            last = (first + torch.arange(S, device=DEV)).clamp_max(max_len - 1)
            ref = ref64_rows(q, want[0], want[1], last, scaling)
            if S <= 5:                                                     # ... which is ref64 of every row on its own
                single = torch.cat([ref64(q[:, :, s:s + 1], want[0], want[1], int(last[s]), scaling) for s in range(S)])
                torch.testing.assert_close(ref.view(B, S, -1), single.view(S, B, -1).transpose(0, 1), rtol=1e-12, atol=1e-14)
            within_ulps(out, ref, D, what)


# ---------------------------------------------------------------- 3. scalar load and store paths
def off_base(t):
    """t in a view whose base is 2 bytes off 16-byte alignment (a slice [1:] of a flat tensor, reshaped): contiguous strides"""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert flat.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 2 and v.stride() == t.contiguous().stride()
    return v


def odd_rows(t):
    """t in a view whose base is 16-byte aligned and whose row stride, D + 2, is not a multiple of 8 elements"""
    w = torch.empty(*t.shape[:-1], t.shape[-1] + 2, dtype=t.dtype, device=t.device)
    v = w[..., :t.shape[-1]]
    v.copy_(t)
    assert v.data_ptr() % 16 == 0 and v.stride(3) == 1 and v.stride(2) % 8 == 2
    return v


def vector_path(t):
    """csrc/pbl_prefill_kernels.h, pf_vec: every row of t starts on a 16-byte boundary"""
    return t.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in t.stride()[:3])


@pytest.mark.parametrize("relaid", [off_base, odd_rows])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [37, 130])
def test_scalar_loads_equal_vector_loads(S, D, relaid):
    """q, k_new and v_new, one at a time and all three, in a layout that rules out 16-byte loads (q_vec / k_vec / v_vec = 0): the
    output and both caches equal the aligned call's bit for bit"""
    B, Hq, Hkv, L, pos = 2, 4, 2, 256, 9
    base_k, base_v, q, k_new, v_new = inputs(B, Hq, Hkv, D, L, S, 31 * S + D)
    assert all(vector_path(t) for t in (q, k_new, v_new))

    def run(qq, kk, vv):
        kc, vc, p = base_k.clone(), base_v.clone(), position(pos)
        kc[:, :, pos:] = NAN
        vc[:, :, pos:] = NAN
        out = prefill_attention_f16(qq, kk, vv, kc, vc, p, D ** -0.5)
        assert int(p) == pos + S
        return out, kc, vc

    want = run(q, k_new, v_new)
    full_k, full_v = base_k.clone(), base_v.clone()
    full_k[:, :, pos:pos + S] = k_new
    full_v[:, :, pos:pos + S] = v_new
    within_ulps(want[0], ref64(q, full_k, full_v, pos, D ** -0.5), D, "the aligned call vs float64")
    assert torch.equal(bits(want[1][:, :, :pos + S]), bits(full_k[:, :, :pos + S]))
    for which in ("q", "k", "v", "qkv"):
        args = [relaid(t) if c in which else t for c, t in zip("qkv", (q, k_new, v_new))]
        assert [vector_path(t) for t in args] == [c not in which for c in "qkv"]
        for name, a, b in zip(("out", "k cache", "v cache"), run(*args), want):
            assert torch.equal(bits(a), bits(b)), f"{relaid.__name__} {which}: {name} differs from the aligned call's"


@pytest.mark.parametrize("relaid", [off_base, odd_rows])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [37, 130])
def test_scalar_loads_of_the_kv8_append(S, D, relaid):
    """pbl_prefill_append_kv8_kernel's load8 has the same scalar branch: the FP8 entry over k_new / v_new in those layouts returns
    the aligned call's output, bytes and scales, and still equals the fp16 entry (prefill_case)"""
    B, Hq, Hkv, L, pos = 2, 4, 2, 256, 9
    base, q, k_new, v_new, k_rt, v_rt = prefill_inputs(B, Hq, Hkv, D, L, S, 37 * S + D)

    def run(kk, vv):
        kq, ks, vq, vs, _, _ = fresh_caches(base, pos)
        p = position(pos)
        out = prefill_attention_kv8(q, kk, vv, kq, vq, ks, vs, p, D ** -0.5)
        assert int(p) == pos + S
        return bits(out), kq, vq, ks.view(torch.int32), vs.view(torch.int32)

    want = run(k_new, v_new)
    for which in ("k", "v", "kv"):
        kk, vv = (relaid(t) if c in which else t for c, t in zip("kv", (k_new, v_new)))
        assert [vector_path(kk), vector_path(vv)] == [c not in which for c in "kv"]
        for name, a, b in zip(("out", "k bytes", "v bytes", "k scales", "v scales"), run(kk, vv), want):
            assert torch.equal(a, b), f"{relaid.__name__} {which}: {name} differ from the aligned call's"
    prefill_case(base, q, relaid(k_new), relaid(v_new), k_rt, v_rt, pos, D ** -0.5, f"{relaid.__name__} S={S}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [37, 130])
def test_scalar_stores_stay_inside_the_output(S, D):
    """the C entry with out rows that are not 8-byte aligned (o_vec = 0): ldo = Hq D + 2 with out 8-byte aligned, the same with out
    4-byte but not 8-byte aligned, ldo = Hq D + 4 with such an out, and ldo = Hq D + 3 with out on an odd element.  A sentinel row
    before and after the output and the sentinel padding columns keep their bits; the values and the caches are the wrapper's"""
    B, Hq, Hkv, max_len, pos = 2, 4, 2, 256, 9
    L = _lib.lib()
    scaling = D ** -0.5
    base_k, base_v, q, k_new, v_new = inputs(B, Hq, Hkv, D, max_len, S, 41 * S + D)

    def caches():
        kc, vc = base_k.clone(), base_v.clone()
        kc[:, :, pos:] = NAN
        vc[:, :, pos:] = NAN
        return kc, vc

    kc0, vc0 = caches()
    want = prefill_attention_f16(q, k_new, v_new, kc0, vc0, position(pos), scaling)
    rows, width = B * S, Hq * D
    for pad, lead in ((2, 0), (2, 2), (4, 2), (3, 1)):
        ldo = width + pad
        flat = torch.full(((rows + 2) * ldo + 16,), SENTINEL, dtype=torch.int16, device=DEV)
        e0 = ldo + (lead - ldo) % 4                                          # the output's first element: e0 % 4 == lead
        ptr = flat.data_ptr() + 2 * e0
        assert flat.data_ptr() % 16 == 0 and ptr % 8 == 2 * lead and not (ptr % 8 == 0 and ldo % 4 == 0)
        kc, vc = caches()
        p = position(pos)
        strides = [(C.c_int64 * 3)(*t.stride()[:3]) for t in (q, k_new, v_new)]
        rc = L.pbl_prefill_attn_f16(q.data_ptr(), strides[0], k_new.data_ptr(), strides[1], v_new.data_ptr(), strides[2], kc.data_ptr(),
                                    vc.data_ptr(), B, S, Hq, Hkv, D, max_len, scaling, p.data_ptr(), ptr, ldo,
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.PBL_OK
        torch.cuda.synchronize()
        what = f"ldo = Hq D + {pad}, out at element {e0}"
        body = flat[e0:e0 + rows * ldo].view(rows, ldo)
        assert bool((flat[:e0] == SENTINEL).all()) and bool((flat[e0 + rows * ldo:] == SENTINEL).all()), f"{what}: a write outside out"
        assert bool((body[:, width:] == SENTINEL).all()), f"{what}: a write into the padding columns"
        assert torch.equal(body[:, :width].contiguous(), bits(want)), f"{what}: values differ from the vector stores'"
        assert int(p) == pos + S and torch.equal(bits(kc), bits(kc0)) and torch.equal(bits(vc), bits(vc0))


# ---------------------------------------------------------------- 4. structured values
def mid_positions(max_len, S):
    return sorted({0, 65, (max_len - S) // 2, max_len - S})


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("max_len", STRUCTURED)
def test_one_dominant_key(max_len, D):
    """one key whose score is >= 30 above every other: the rows that may see it return its V row (the rest weighs < 65536 e^-30),
    the rows before it must not see it.  Placed at row 0 -- every later tile is rescaled against tile 0 --, at rows 63 and 64, in a
    middle tile, and at row pos + s for s in {0, 31, 32, 127, 128, 129}: row s's own key, the causal diagonal at a wave's first and
    last lane, at the wave edge and at the query-tile edge"""
    B, Hq, Hkv, S = 1, 4, 2, 130
    G = Hq // Hkv
    scaling = D ** -0.5
    g = torch.Generator(device=DEV).manual_seed(max_len + D)
    q = torch.randn(B, Hq, S, D, generator=g, device=DEV).half()
    k0 = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    v = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    q[..., 0] = 8.0                                                           # the dominant key is big * e_0: score 8 big scaling
    k0[..., 0] = 0.0
    others = float((q.double() @ k0.double().repeat_interleave(G, 1).transpose(-1, -2)).amax()) * scaling
    big = float(int((others + 32) / (8 * scaling)) + 1)
    assert big < 2048 and 8 * big * scaling >= others + 30
    pos = max_len - S
    rows = {0, 63, 64, TK * ((max_len - 1) // TK // 2) + 5} | {pos + s for s in (0, 31, 32, 127, 128, 129)}
    assert len(rows) == 10 and max(rows) == max_len - 1
    for r in sorted(rows):
        k = k0.clone()
        k[:, :, r] = 0.0
        k[:, :, r, 0] = big
        out = attend(q, k, v, pos, scaling)
        within_ulps(out, ref64(q, k, v, pos, scaling), D, f"max_len={max_len} dominant key at row {r} vs float64")
        sees = [s for s in range(S) if r <= pos + s]
        vrow = v[:, :, r].repeat_interleave(G, 1).reshape(B, 1, Hq * D)
        within_ulps(out.view(B, S, -1)[:, sees].reshape(-1, Hq * D), vrow.expand(B, len(sees), Hq * D).reshape(-1, Hq * D), D,
                    f"max_len={max_len} dominant key at row {r} vs its V row")
        for s in range(S):
            if s not in sees:
                assert not torch.equal(out.view(B, S, -1)[:, s], vrow[:, 0]), f"row {s} saw key {r} > pos + s = {pos + s}"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("max_len", STRUCTURED)
def test_wide_score_range(max_len, D):
    """scaled scores spanning several thousand over the keys each row sees at the last position: most exp2(x - m) of a tile
    underflow and whole tiles are rescaled to nothing"""
    B, Hq, Hkv, S = 1, 4, 2, 130
    scaling = D ** -0.5
    g = torch.Generator(device=DEV).manual_seed(3 * max_len + D)
    q = (torch.randn(B, Hq, S, D, generator=g, device=DEV) * 32).half()
    k = (torch.randn(B, Hkv, max_len, D, generator=g, device=DEV) * 32).half()
    v = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    sc = (q.double() @ k.double().repeat_interleave(Hq // Hkv, 1).transpose(-1, -2)) * scaling
    seen = torch.arange(max_len, device=DEV)[None, :] <= (max_len - S + torch.arange(S, device=DEV))[:, None]    # at the last position
    span = sc.masked_fill(~seen, -INF).amax(-1) - sc.masked_fill(~seen, INF).amin(-1)
    assert float(span.min()) > 3000, "the inputs do not span what this test is for"
    for pos in mid_positions(max_len, S):
        within_ulps(attend(q, k, v, pos, scaling), ref64(q, k, v, pos, scaling), D, f"max_len={max_len} pos={pos}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("max_len", STRUCTURED)
def test_identical_keys(max_len, D):
    """every key the same: a uniform softmax over up to 65536 keys, the output is the mean of V over rows [0, pos + s]"""
    B, Hq, Hkv, S = 1, 4, 2, 130
    scaling = D ** -0.5
    g = torch.Generator(device=DEV).manual_seed(5 * max_len + D)
    q = (torch.randn(B, Hq, S, D, generator=g, device=DEV) * 2).half()
    k = torch.randn(B, Hkv, 1, D, generator=g, device=DEV).half().expand(B, Hkv, max_len, D).contiguous()
    v = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    means = v.double().cumsum(2) / torch.arange(1, max_len + 1, device=DEV, dtype=torch.float64)[:, None]
    for pos in mid_positions(max_len, S):
        ref = ref64(q, k, v, pos, scaling)
        mean = means[:, :, pos:pos + S].repeat_interleave(Hq // Hkv, 1).transpose(1, 2).reshape(B * S, Hq * D)
        torch.testing.assert_close(ref, mean, rtol=1e-9, atol=1e-12)
        within_ulps(attend(q, k, v, pos, scaling), ref, D, f"max_len={max_len} pos={pos}")


HUGE_KEYS = (-60000., -30000., -9000., -2000., 500., 3000., 9000., 11000., 13000., 17024., 21008., 26000., 33024., 41024., 52000., 65504.)


@pytest.mark.parametrize("D", [64, 128])
def test_scores_beyond_2_to_the_25(D):
    """base-2 scores of up to 2^28, where fp32's spacing is 4 and more and m - 14 cannot be formed: rounded, the difference comes out
    as 12 or 16, and P = exp2(16) would be inf in fp16 and the row NaN.  q = q0 e_0 per head, key j = HUGE_KEYS[j // 32] e_0: 32 tied
    keys per level, levels ascending and 2^19 or more apart in score, so the running maximum moves in every tile and a row's result
    is the mean of V over the keys it sees of its top level (for the head with q0 < 0: of level 0).  The premise is asserted on an
    fp32 restatement of the kernel's scores: some running maxima give fl(m - 14) = m - 16, some m - 12, some m"""
    B, Hq, Hkv, S, max_len = 1, 4, 2, 130, 512
    scaling, pos = D ** -0.5, max_len - S
    q0 = torch.tensor([4096., 16384., 32768., -16384.])
    levels = torch.tensor(HUGE_KEYS).half()
    assert torch.equal(levels.float(), torch.tensor(HUGE_KEYS)) and bool((levels[1:] > levels[:-1]).all()) and len(levels) * 32 == max_len
    x = q0[:, None] * levels.float()[None, :] * (torch.tensor(scaling, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    assert x.dtype == torch.float32 and float(x.abs().max()) > 2.0 ** 28
    tops = torch.cat([x[:3, 1::2].flatten(), x[3, :1]])                    # the maxima the tiles bring: a tile holds two levels
    gaps = set((tops - (tops - 14.0)).tolist())
    assert {16.0, 12.0, 0.0} <= gaps and any(13.5 < g < 14.5 for g in gaps), gaps
    g = torch.Generator(device=DEV).manual_seed(D)
    k = torch.zeros(B, Hkv, max_len, D, dtype=torch.float16, device=DEV)
    k[..., 0] = levels.to(DEV).repeat_interleave(32)
    v = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    q = torch.zeros(B, Hq, S, D, dtype=torch.float16, device=DEV)
    q[..., 0] = q0.to(DEV).half()[None, :, None]
    out = attend(q, k, v, pos, scaling)
    assert bool(torch.isfinite(out).all()), "P overflowed fp16"
    ref = ref64(q, k, v, pos, scaling)
    rows = pos + torch.arange(S, device=DEV)
    first = torch.stack([rows // 32 * 32] * 3 + [torch.zeros_like(rows)])    # [Hq, S]: the first key of the row's top level
    last = torch.stack([rows] * 3 + [rows.clamp_max(31)])
    csum = torch.cat([torch.zeros(B, Hkv, 1, D, dtype=torch.float64, device=DEV), v.double().cumsum(2)], 2).repeat_interleave(Hq // Hkv, 1)
    idx = lambda t: (t[None, :, :, None]).expand(B, Hq, S, D)
    mean = (csum.gather(2, idx(last + 1)) - csum.gather(2, idx(first))) / (last + 1 - first)[None, :, :, None]
    torch.testing.assert_close(ref, mean.transpose(1, 2).reshape(B * S, Hq * D), rtol=1e-9, atol=1e-12)
    within_ulps(out, ref, D, f"D={D}: scores up to 2^28")


# ---------------------------------------------------------------- 5. weights below 2^-14 of the row's maximum: an attention sink
# D -> the integer magnitudes `big` of the sink key.  r = 2^24 exp(-big scaling) is a later key's weight relative to the row's maximum
# in units of 2^-24, fp16's subnormal step: with P's maximum at 1.0 such a weight is rounded to round(r) 2^-24
SINKS = {64: (125, 129, 131, 136, 142),        # r = 2.75, 1.67, 1.30, 0.69, 0.33
         128: (172, 177, 182, 192, 201)}       # r = 4.19, 2.69, 1.73, 0.72, 0.32
EDGE_SINKS = {64: 209, 128: 296}                # 2^38 exp(-big scaling) = 1.24, 1.19: the subnormal step of a P whose maximum is 2^14


def relative_weight(big, D, unit):
    """r = exp(-big scaling) in units of 2^-unit, asserted to lie in [0.3, 6] and 0.1 or more from every boundary k + 1/2 at which
    the rounding of r 2^-unit to a multiple of 2^-unit changes"""
    r = 2.0 ** unit * math.exp(-big * D ** -0.5)
    assert 0.3 <= r <= 6 and abs(r - math.floor(r) - 0.5) >= 0.1, (big, D, unit, r)
    return r


def sink_inputs(max_len, S, D, big, vscale=64.0):
    """q = e_0, key 0 = big e_0 with a zero V row, every other key with coordinate 0 = 0: the sink's score is exactly big scaling and
    every other exactly 0.  The other V rows ~ N(0, vscale^2), so that outputs around r 2^-24 sqrt(max_len) vscale are normal fp16"""
    B, Hq, Hkv = 1, 4, 2
    g = torch.Generator(device=DEV).manual_seed(max_len + D + big)
    k = torch.randn(B, Hkv, max_len, D, generator=g, device=DEV).half()
    v = (torch.randn(B, Hkv, max_len, D, generator=g, device=DEV) * vscale).half()
    k[..., 0] = 0.0
    k[:, :, 0] = 0.0
    k[:, :, 0, 0] = float(big)
    v[:, :, 0] = 0.0
    q = torch.zeros(B, Hq, S, D, dtype=torch.float16, device=DEV)
    q[..., 0] = 1.0
    sc = q.double() @ k.double().repeat_interleave(Hq // Hkv, 1).transpose(-1, -2) * D ** -0.5
    assert bool((sc[..., 0] == big * D ** -0.5).all()) and bool((sc[..., 1:] == 0).all())
    return q, k, v


@pytest.mark.parametrize("D,big", [(D, big) for D in SINKS for big in SINKS[D]])
@pytest.mark.parametrize("max_len", [4132, 65536])
def test_attention_sink_with_weights_below_fp16_s_normal_range(max_len, D, big):
    """(a) the kernel follows ref_tiled, the numerics the headers state; (b) it meets the suite's criterion against float64.
    With P's maximum at 1.0 the later keys' weights would be rounded to round(r) 2^-24 -- all of them the same way, so the error is
    systematic: the print shows how far ref_tiled(offset=0) lies from ref64 (18 .. 494 x the bound)"""
    S, scaling = 33, D ** -0.5
    r = relative_weight(big, D, 24)
    q, k, v = sink_inputs(max_len, S, D, big)
    pos = max_len - S
    out = attend(q, k, v, pos, scaling)
    ref, tiled = ref64(q, k, v, pos, scaling), ref_tiled(q, k, v, pos, scaling)
    scale = ref.abs().view(S, -1, D).amax(-1)
    assert float(scale.min()) >= 2.0 ** -14, "the outputs are not normal fp16 numbers"
    print(f"[sink] max_len={max_len} D={D} big={big} r={r:.3f}: kernel vs ref_tiled {ratio(out, tiled, D):.3f}, kernel vs ref64 "
          f"{ratio(out, ref, D):.3f}, ref_tiled(offset=0) vs ref64 {ratio(ref_tiled(q, k, v, pos, scaling, 0), ref, D):.1f} x the bound; "
          f"output scale {float(scale.min()):.2e} .. {float(scale.max()):.2e}")
    within_ulps(out, tiled, D, f"max_len={max_len} D={D} big={big} (a) vs ref_tiled")
    within_ulps(out, ref, D, f"max_len={max_len} D={D} big={big} (b) vs float64")


@pytest.mark.parametrize("D", [64, 128])
def test_attention_sink_at_the_edge_of_the_offset_p(D):
    """65536 keys whose weights are r 2^-38 of the row's maximum, r = 1.2: with P's maximum at 2^14 they land on fp16's subnormal
    step, 2^-24, and are rounded to round(r) 2^-24.  For these V rows (|sum over keys| stays below 2^17) that is an error below
    0.5 x 2^-38 x 2^17 = 2^-22 on outputs of that size, i.e. under the bound's floor of 4 x 2^-24: (b) holds here although the
    output is all rounding.  This is where the offset's reach ends: weights below 2^-39 of the maximum are dropped"""
    max_len, S, scaling, big = 65536, 33, D ** -0.5, EDGE_SINKS[D]
    r = relative_weight(big, D, 24 + P_OFFSET)
    q, k, v = sink_inputs(max_len, S, D, big)
    assert float(v.double().sum(2).abs().max()) < 2.0 ** 17
    pos = max_len - S
    out = attend(q, k, v, pos, scaling)
    ref, tiled = ref64(q, k, v, pos, scaling), ref_tiled(q, k, v, pos, scaling)
    print(f"[sink edge] D={D} big={big} r={r:.3f}: kernel vs ref_tiled {ratio(out, tiled, D):.3f}, kernel vs ref64 {ratio(out, ref, D):.3f} "
          f"x the bound; max |ref64| {float(ref.abs().max()):.2e}")
    assert float(out.abs().max()) > 0, "the weights were dropped"
    within_ulps(out, tiled, D, f"D={D} big={big} (a) vs ref_tiled")
    within_ulps(out, ref, D, f"D={D} big={big} (b) vs float64")


def test_attention_sink_over_the_fp8_cache_equals_the_fp16_entry():
    """a sink case through the FP8 entry, which runs the same template: big = 128 is an e4m3fn value, so the dequantised cache still
    holds the sink (r = 1.89) and exact zero scores elsewhere; bit-equal to the fp16 entry, which meets (b) over those rows"""
    D, big, max_len, S = 64, 128, 4132, 33
    scaling, pos = D ** -0.5, max_len - S
    relative_weight(big, D, 24)
    q, k, v = sink_inputs(max_len, S, D, big)
    base = (*quantized(k), *quantized(v))
    k16, v16 = kv8_dequantize(base[0], base[1]), kv8_dequantize(base[2], base[3])
    assert torch.equal(k16[:, :, 0], k[:, :, 0]) and bool((k16[..., 0][:, :, 1:] == 0).all()) and bool((v16[:, :, 0] == 0).all())
    k_new, v_new = k[:, :, pos:], v[:, :, pos:]
    assert torch.equal(roundtrip(k_new), k16[:, :, pos:])
    prefill_case(base, q, k_new, v_new, roundtrip(k_new), roundtrip(v_new), pos, scaling, "sink over the FP8 cache")
    within_ulps(attend(q, k16, v16, pos, scaling), ref64(q, k16, v16, pos, scaling), D, "the fp16 entry over the dequantised sink")
