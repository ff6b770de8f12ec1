"""-m gpu: the FP8 KV cache -- pbl_rope_append_kv8 / pbl_decode_attn_kv8 / pbl_prefill_attn_kv8 (runtime.rope_append_kv8,
decode_attention_kv8, prefill_attention_kv8) and DecodeSession / generate with kv_cache="fp8".

Every comparison is exact.  The format's scale is a power of two and a dequantised value is an fp16 value, so each FP8 entry must
return bit for bit what its (already tested) fp16 counterpart returns over a cache holding the dequantised rows; the quantiser itself
is compared byte for byte with the torch reference runtime.kv8_quantize, on the CPU."""
import pytest
import torch

from pb_llm_amd import decoding, harness as H, runtime
from pb_llm_amd.runtime import (decode_attention_f16, decode_attention_kv8, kv8_dequantize, kv8_quantize, prefill_attention_f16,
                                prefill_attention_kv8, rope_append_f16, rope_append_kv8)
from test_decode_epilogues_cpu import cos_sin
from test_gpu_decode_epilogues import ids_of, qkv_out

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BYTE, PAT_BYTE, PAT_SCALE = 0x7f, 0x55, -7.0


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()


def bits(t):
    return t.contiguous().view(torch.int16)


def position(pos):
    return torch.tensor(pos, dtype=torch.int64, device=DEV)


def quantized(x):
    """(bytes, scale) of x by the torch reference, computed on the CPU, on the device"""
    q, s = kv8_quantize(x.cpu())
    return q.to(DEV), s.to(DEV)


def roundtrip(x):
    """kv8_dequantize(kv8_quantize(x)) by the torch reference, computed on the CPU, on x's device"""
    return kv8_dequantize(*kv8_quantize(x.cpu())).to(x.device)


def rows_with_exponents(shape, g, lo=-6, hi=4):
    """randn rows [..., D], each scaled by a random power of two in [2^lo, 2^hi]: rows of a cache then carry different exponents"""
    e = torch.randint(lo, hi + 1, shape[:-1], generator=g, device=DEV)
    return (torch.randn(shape, generator=g, device=DEV) * torch.exp2(e.float())[..., None]).half()


# ---------------------------------------------------------------- 0. the conversion instruction against torch, value by value
def test_quantiser_equals_the_reference_on_every_fp16_value():
    """every finite fp16 value of magnitude <= 448, in rows whose first element is 448 (e = 0: the byte is the conversion of the value
    itself -- normals, subnormals and every tie), and the same rows scaled by 2^-20 (e = -15, the clamp): the bytes and scales that
    pbl_prefill_attn_kv8's append writes equal runtime.kv8_quantize's"""
    D = 128
    allv = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    vals = allv[torch.isfinite(allv) & (allv.abs() <= 448)]
    S = -(-vals.numel() // (D - 1))
    rows = torch.zeros(S, D - 1, dtype=torch.float16).view(-1)
    rows[:vals.numel()] = vals
    k = torch.cat((torch.full((S, 1), 448.0, dtype=torch.float16), rows.view(S, D - 1)), 1)
    v = (k.float() * 2.0 ** -20).half()
    assert S <= 512
    kd, vd = k.to(DEV).view(1, 1, S, D), v.to(DEV).view(1, 1, S, D)
    kc, vc = (torch.full((1, 1, S, D), PAT_BYTE, dtype=torch.uint8, device=DEV) for _ in range(2))
    ks, vs = (torch.full((1, 1, S), PAT_SCALE, device=DEV) for _ in range(2))
    out = prefill_attention_kv8(torch.zeros(1, 1, S, D, dtype=torch.float16, device=DEV), kd, vd, kc, vc, ks, vs, position(0), 0.1)
    assert out is not None
    for name, x, c, s in (("k", k, kc, ks), ("v", v, vc, vs)):
        qb, qs = kv8_quantize(x)
        bad = (c.cpu().view(S, D) != qb).nonzero()
        assert not len(bad), f"{name}: {len(bad)} bytes differ from the reference, first at value {float(x[tuple(bad[0])])!r}"
        assert torch.equal(s.cpu().view(S), qs)
    assert bool((ks == 1.0).all()) and bool((vs == 2.0 ** -15).all())


# ---------------------------------------------------------------- 1. append
def check_append(B, S, D, Hq, Hkv, L, positions, whole_cache=True):
    from transformers import LlamaConfig
    cfg = LlamaConfig(hidden_size=Hq * D, num_attention_heads=Hq, num_key_value_heads=Hkv, max_position_embeddings=131072)
    y, _, _ = qkv_out(B, S, Hq, Hkv, D, 31 * B + S + D)
    k_off, v_off = Hq * D, (Hq + Hkv) * D
    y[0, k_off:k_off + D] = 0                                              # token 0: an all-zero k head (e = -15, every byte 0),
    y[0, k_off + D:k_off + 2 * D] *= 2.0 ** -12                            # a k head scaled by 2^-12 (small exponents),
    y[0, v_off:v_off + D] *= 2.0 ** -20                                    # a v head at the clamp e = -15,
    y[0, v_off + D + 1] = y[0, v_off + D:v_off + 2 * D].abs().max() * 2.0 ** -15      # and an element 2^-15 of its row's amax: a subnormal byte
    kc16, vc16 = (torch.zeros(B, Hkv, L, D, dtype=torch.float16, device=DEV) for _ in range(2))
    kc, vc = (torch.empty(B, Hkv, L, D, dtype=torch.uint8, device=DEV) for _ in range(2))
    ks, vs = (torch.empty(B, Hkv, L, device=DEV) for _ in range(2))
    seen_e, seen_sub = set(), False
    for pos in positions:
        cos, sin = cos_sin(cfg, [[pos + s for s in range(S)]], DEV)
        for t, pat in ((kc, PAT_BYTE), (vc, PAT_BYTE), (ks, PAT_SCALE), (vs, PAT_SCALE)):
            t.fill_(pat)
        p = position(pos)
        q16 = rope_append_f16(y, 0, k_off, v_off, B, S, Hq, Hkv, D, cos, sin, kc16, vc16, p)
        q8 = rope_append_kv8(y, 0, k_off, v_off, B, S, Hq, Hkv, D, cos, sin, kc, vc, ks, vs, p)
        assert int(p) == pos, "the append leaves the position"
        assert q8.shape == q16.shape and q8.stride() == q16.stride() and torch.equal(bits(q8), bits(q16))
        for c16, c, s in ((kc16, kc, ks), (vc16, vc, vs)):
            want_b, want_s = kv8_quantize(c16[:, :, pos:pos + S].cpu())    # of the rows the fp16 entry wrote; compared on the CPU
            got_b, got_s = c[:, :, pos:pos + S].cpu(), s[:, :, pos:pos + S].cpu()
            assert torch.equal(got_b, want_b), f"pos {pos}: bytes"
            assert torch.equal(got_s, want_s), f"pos {pos}: scales"
            seen_e |= set(torch.log2(got_s).flatten().long().tolist())
            seen_sub |= bool((((got_b & 0x78) == 0) & ((got_b & 0x07) != 0)).any())
            c[:, :, pos:pos + S] = PAT_BYTE                                 # every other row and scale is untouched
            s[:, :, pos:pos + S] = PAT_SCALE
            if whole_cache:
                assert bool((c == PAT_BYTE).all()) and bool((s == PAT_SCALE).all()), f"pos {pos}: a row outside [pos, pos + S) changed"
            else:
                assert bool((c[:, -1] == PAT_BYTE).all()) and bool((s[:, -1] == PAT_SCALE).all())
    assert -15 in seen_e and len(seen_e) > 2 and seen_sub, "the inputs did not reach e = -15, several exponents and subnormal bytes"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B,S", [(1, 1), (1, 4), (2, 2), (4, 1)])
def test_rope_append_kv8_equals_the_quantised_fp16_append(B, S, D):
    check_append(B, S, D, 8, 2, 512, (0, 5, 512 - S))


def test_rope_append_kv8_at_65536_rows():
    """the largest cache the entries accept, the last rows of the last head: the byte index reaches 4 * 8 * 65536 * 128 = 2^28"""
    check_append(4, 4, 128, 8, 8, 65536, (65536 - 4,), whole_cache=False)


def test_rope_append_kv8_drops_rows_beyond_max_len():
    from transformers import LlamaConfig
    B, S, Hq, Hkv, D, L = 2, 4, 8, 2, 64, 32
    cfg = LlamaConfig(hidden_size=Hq * D, num_attention_heads=Hq, num_key_value_heads=Hkv, max_position_embeddings=4096)
    y, _, _ = qkv_out(B, S, Hq, Hkv, D, 9)
    cos, sin = cos_sin(cfg, [[30 + s for s in range(S)]], DEV)
    flat = torch.full((2 * B * Hkv * L * D + 4096,), PAT_BYTE, dtype=torch.uint8, device=DEV)      # k, v, then guard bytes
    kc, vc = (flat[i * B * Hkv * L * D:(i + 1) * B * Hkv * L * D].view(B, Hkv, L, D) for i in range(2))
    sflat = torch.full((2 * B * Hkv * L + 64,), PAT_SCALE, device=DEV)
    ks, vs = (sflat[i * B * Hkv * L:(i + 1) * B * Hkv * L].view(B, Hkv, L) for i in range(2))
    assert rope_append_kv8(y, 0, Hq * D, (Hq + Hkv) * D, B, S, Hq, Hkv, D, cos, sin, kc, vc, ks, vs, position(30)) is not None
    for c, s in ((kc, ks), (vc, vs)):
        assert bool((c[:, :, :30] == PAT_BYTE).all()) and bool((s[:, :, :30] == PAT_SCALE).all())
        assert bool((s[:, :, 30:] != PAT_SCALE).all())                     # rows 30 and 31 written, rows 32 and 33 dropped
    assert bool((flat[-4096:] == PAT_BYTE).all()) and bool((sflat[-64:] == PAT_SCALE).all())


# ---------------------------------------------------------------- 2. decode attention
def decode_case(q, kq, ksc, vq, vsc, k16, v16, pos, scaling, what):
    """one call at `pos` over caches whose rows beyond pos + S hold NaN bytes and NaN scales, against decode_attention_f16 over the
    dequantised cache: equal bits, finite, and the position advanced"""
    S = q.shape[2]
    kc, vc, ks, vs = kq.clone(), vq.clone(), ksc.clone(), vsc.clone()
    for c, s in ((kc, ks), (vc, vs)):
        c[:, :, pos + S:] = NAN_BYTE
        s[:, :, pos + S:] = float("nan")
    p8, p16 = position(pos), position(pos)
    got = decode_attention_kv8(q, kc, vc, ks, vs, p8, scaling)
    ref = decode_attention_f16(q, k16, v16, p16, scaling)
    assert got.shape == ref.shape and got.dtype == torch.float16 and got.is_contiguous()
    assert int(p8) == int(p16) == pos + S, f"{what}: the position advances by S"
    assert bool(torch.isfinite(got).all()), f"{what}: a row beyond pos + S was read"
    assert torch.equal(bits(got), bits(ref)), f"{what}: {int((bits(got) != bits(ref)).sum())} values differ from the fp16 entry's"


def decode_inputs(B, Hkv, L, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    kq, ksc = quantized(rows_with_exponents((B, Hkv, L, D), g))
    vq, vsc = quantized(rows_with_exponents((B, Hkv, L, D), g))
    assert len(torch.unique(ksc)) > 4
    return g, kq, ksc, vq, vsc, kv8_dequantize(kq, ksc), kv8_dequantize(vq, vsc)


@pytest.mark.parametrize("heads", [(4, 4), (8, 2)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_decode_attention_kv8_equals_f16_over_the_dequantised_cache(B, D, heads):
    Hq, Hkv = heads
    L = 200                                                                # 7 splits of 32 keys, the last one partial
    g, kq, ksc, vq, vsc, k16, v16 = decode_inputs(B, Hkv, L, D, B * 1000 + D + Hq)
    for S in (1, 2, 3, 4):
        q = (torch.randn(B, Hq, S, D, generator=g, device=DEV) * 2).half()
        for pos in (0, 1, 31, 32, 33, 63, 64, 65, L - S):
            decode_case(q, kq, ksc, vq, vsc, k16, v16, pos, D ** -0.5, f"S={S} pos={pos}")
    qt = torch.randn(B, 2, Hq, D, generator=g, device=DEV).half().transpose(1, 2)     # q as rope_append returns it: strided
    assert not qt.is_contiguous()
    decode_case(qt, kq, ksc, vq, vsc, k16, v16, 70, D ** -0.5, "strided q")


@pytest.mark.parametrize("D", [64, 128])
def test_decode_attention_kv8_with_chunk_64(D):
    """max_len 4100: the chunk is 64 keys (65 splits); positions at the end of the 64th split and at the end of the cache"""
    L = 4100
    g, kq, ksc, vq, vsc, k16, v16 = decode_inputs(1, 1, L, D, 4100 + D)
    for S in (1, 2, 3, 4):
        q = (torch.randn(1, 4, S, D, generator=g, device=DEV) * 2).half()
        for pos in (4095 - S, L - S):
            decode_case(q, kq, ksc, vq, vsc, k16, v16, pos, D ** -0.5, f"S={S} pos={pos}")


def test_kv8_entries_decline_and_raise():
    def z(*shape, dtype=torch.uint8):
        return torch.zeros(*shape, dtype=dtype, device=DEV)

    p = position(0)
    q = z(1, 4, 1, 64, dtype=torch.float16)
    assert decode_attention_kv8(z(1, 4, 1, 96, dtype=torch.float16), z(1, 2, 64, 96), z(1, 2, 64, 96), z(1, 2, 64, dtype=torch.float32),
                                z(1, 2, 64, dtype=torch.float32), p, 0.1) is None                                  # D = 96
    kc, sc = z(1, 2, 64, 64), z(1, 2, 64, dtype=torch.float32)
    assert decode_attention_kv8(z(1, 4, 5, 64, dtype=torch.float16), kc, kc.clone(), sc, sc.clone(), p, 0.1) is None  # S = 5
    assert int(p) == 0
    for bad in ((q, kc.half(), kc.half(), sc, sc.clone()),                 # an fp16 cache
                (q, kc, kc.clone(), sc.half(), sc.half()),                 # fp16 scales
                (q, kc, kc.clone(), sc[:, :, :32], sc[:, :, :32]),         # scales of another length
                (q, kc, kc.clone(), sc.cpu(), sc.cpu())):
        with pytest.raises(ValueError):
            decode_attention_kv8(*bad, p, 0.1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 3. prefill attention
def prefill_inputs(B, Hq, Hkv, D, L, smax, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    base_kq, base_ks = quantized(rows_with_exponents((B, Hkv, L, D), g))
    base_vq, base_vs = quantized(rows_with_exponents((B, Hkv, L, D), g))
    q = (torch.randn(B, Hq, smax, D, generator=g, device=DEV) * 2).half()
    k_new = rows_with_exponents((B, Hkv, smax, D), g)
    v_new = rows_with_exponents((B, Hkv, smax, D), g)
    return (base_kq, base_ks, base_vq, base_vs), q, k_new, v_new, roundtrip(k_new), roundtrip(v_new)


def fresh_caches(base, pos):
    """the FP8 cache with the base rows below pos and NaN bytes / NaN scales from pos on, and the fp16 cache that holds the
    dequantised rows below pos and NaN from pos on"""
    kq, ks, vq, vs = (t.clone() for t in base)
    for c, s in ((kq, ks), (vq, vs)):
        c[:, :, pos:] = NAN_BYTE
        s[:, :, pos:] = float("nan")
    k16, v16 = kv8_dequantize(base[0], base[1]), kv8_dequantize(base[2], base[3])
    k16[:, :, pos:] = float("nan")
    v16[:, :, pos:] = float("nan")
    return kq, ks, vq, vs, k16, v16


def prefill_case(base, q, k_new, v_new, k_rt, v_rt, pos, scaling, what):
    S = q.shape[2]
    kq, ks, vq, vs, k16, v16 = fresh_caches(base, pos)
    p8, p16 = position(pos), position(pos)
    got = prefill_attention_kv8(q, k_new, v_new, kq, vq, ks, vs, p8, scaling)
    ref = prefill_attention_f16(q, k_rt, v_rt, k16, v16, p16, scaling)
    assert got.shape == ref.shape and got.dtype == torch.float16 and got.is_contiguous()
    assert int(p8) == int(p16) == pos + S, f"{what}: the position advances by S"
    assert bool(torch.isfinite(got).all()), what
    assert torch.equal(bits(got), bits(ref)), f"{what}: {int((bits(got) != bits(ref)).sum())} values differ from the fp16 entry's"
    for c, s, c16 in ((kq, ks, k16), (vq, vs, v16)):
        assert torch.equal(bits(kv8_dequantize(c[:, :, :pos + S], s[:, :, :pos + S])), bits(c16[:, :, :pos + S])), f"{what}: cache rows"
        assert bool((c[:, :, pos + S:] == NAN_BYTE).all()) and bool(torch.isnan(s[:, :, pos + S:]).all()), f"{what}: rows above pos + S"


@pytest.mark.parametrize("heads", [(4, 4), (4, 2)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B", [1, 2])
def test_prefill_attention_kv8_equals_f16_over_the_dequantised_cache(B, D, heads):
    Hq, Hkv = heads
    base, q, k_new, v_new, k_rt, v_rt = prefill_inputs(B, Hq, Hkv, D, 384, 200, B * 1000 + D + Hkv)
    for S in (5, 63, 64, 65, 129, 200):
        for pos in (0, 3, 64, 100):
            prefill_case(base, q[:, :, :S], k_new[:, :, :S], v_new[:, :, :S], k_rt[:, :, :S], v_rt[:, :, :S], pos, D ** -0.5,
                         f"S={S} pos={pos}")


@pytest.mark.parametrize("heads", [(4, 4), (4, 2)])
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_attention_kv8_is_chunking_invariant(D, heads):
    Hq, Hkv = heads
    B, S = 2, 200
    base, q, k_new, v_new, _, _ = prefill_inputs(B, Hq, Hkv, D, 384, S, 200 + D + Hkv)

    def run(chunks):
        kq, ks, vq, vs, _, _ = fresh_caches(base, 0)
        p, outs, s0 = position(0), [], 0
        for n in chunks:
            o = prefill_attention_kv8(q[:, :, s0:s0 + n], k_new[:, :, s0:s0 + n], v_new[:, :, s0:s0 + n], kq, vq, ks, vs, p, D ** -0.5)
            outs.append(o.view(B, n, Hq * D))
            s0 += n
        assert int(p) == S
        return torch.cat(outs, 1), (kq, ks, vq, vs)

    one, c1 = run([S])
    three, c3 = run([64, 7, 129])
    for a, b in zip(c1, c3):
        assert torch.equal(a[:, :, :S], b[:, :, :S])
    assert torch.equal(bits(one), bits(three)), "a row's result depends on how the prompt was chunked"


def test_prefill_attention_kv8_clips_at_max_len():
    """pos + S > max_len: rows at or beyond max_len are dropped -- nothing lands in the guard bytes behind the buffers -- and the
    result still equals the fp16 entry's"""
    B, Hq, Hkv, D, L, S, pos = 2, 4, 2, 64, 96, 40, 70
    base, q, k_new, v_new, k_rt, v_rt = prefill_inputs(B, Hq, Hkv, D, L, S, 96)
    n = B * Hkv * L
    flat = torch.full((2 * n * D + 8192,), PAT_BYTE, dtype=torch.uint8, device=DEV)
    sflat = torch.full((2 * n + 128,), PAT_SCALE, device=DEV)
    kq, vq = (flat[i * n * D:(i + 1) * n * D].view(B, Hkv, L, D) for i in range(2))
    ks, vs = (sflat[i * n:(i + 1) * n].view(B, Hkv, L) for i in range(2))
    _, _, _, _, k16, v16 = fresh_caches(base, pos)
    for dst, src in ((kq, base[0]), (ks, base[1]), (vq, base[2]), (vs, base[3])):
        dst[:, :, :pos] = src[:, :, :pos]
    p8, p16 = position(pos), position(pos)
    got = prefill_attention_kv8(q, k_new, v_new, kq, vq, ks, vs, p8, D ** -0.5)
    ref = prefill_attention_f16(q, k_rt, v_rt, k16, v16, p16, D ** -0.5)
    assert int(p8) == int(p16) == pos + S
    assert torch.equal(bits(got), bits(ref))
    assert bool((flat[-8192:] == PAT_BYTE).all()) and bool((sflat[-128:] == PAT_SCALE).all())
    assert torch.equal(bits(kv8_dequantize(kq, ks)), bits(k16)) and torch.equal(bits(kv8_dequantize(vq, vs)), bits(v16))
    assert torch.equal(kq[:, :, :pos], base[0][:, :, :pos]) and torch.equal(vs[:, :, :pos], base[3][:, :, :pos])


# ---------------------------------------------------------------- 4. graph capture
def captured(unit):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        unit()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = unit()
    return graph, out


def test_captured_append_and_decode_attention_serve_every_position():
    from transformers import LlamaConfig
    B, S, Hq, Hkv, D, L = 2, 2, 8, 2, 128, 256
    cfg = LlamaConfig(hidden_size=Hq * D, num_attention_heads=Hq, num_key_value_heads=Hkv, max_position_embeddings=4096)
    y, _, _ = qkv_out(B, S, Hq, Hkv, D, 5)
    cos, sin = cos_sin(cfg, [[17, 18]], DEV)
    g, kq, ksc, vq, vsc, _, _ = decode_inputs(B, Hkv, L, D, 55)
    state0 = [t.clone() for t in (kq, ksc, vq, vsc)]
    p = position(0)

    def step():
        q = rope_append_kv8(y, 0, Hq * D, (Hq + Hkv) * D, B, S, Hq, Hkv, D, cos, sin, kq, vq, ksc, vsc, p)
        return decode_attention_kv8(q, kq, vq, ksc, vsc, p, D ** -0.5)

    graph, out = captured(step)
    for pos in (0, 63, 200):                                               # inside the first split, across a boundary, far on
        for t, t0 in zip((kq, ksc, vq, vsc), state0):
            t.copy_(t0)
        p.fill_(pos)
        graph.replay()
        replayed, cache = out.clone(), [t.clone() for t in (kq, ksc, vq, vsc)]
        assert int(p) == pos + S
        for t, t0 in zip((kq, ksc, vq, vsc), state0):
            t.copy_(t0)
        p.fill_(pos)
        eager = step()
        assert torch.equal(bits(replayed), bits(eager)), pos
        assert all(torch.equal(a, b) for a, b in zip(cache, (kq, ksc, vq, vsc))) and int(p) == pos + S


def test_captured_prefill_serves_every_position():
    B, S, Hq, Hkv, D, L = 2, 70, 4, 2, 64, 384
    base, q, k_new, v_new, _, _ = prefill_inputs(B, Hq, Hkv, D, L, S, 70)
    kq, ks, vq, vs = (t.clone() for t in base)
    p = position(0)

    def call():
        return prefill_attention_kv8(q, k_new, v_new, kq, vq, ks, vs, p, D ** -0.5)

    graph, out = captured(call)
    for pos in (0, 60, 300):
        for t, t0 in zip((kq, ks, vq, vs), base):
            t.copy_(t0)
        p.fill_(pos)
        graph.replay()
        replayed, cache = out.clone(), [t.clone() for t in (kq, ks, vq, vs)]
        for t, t0 in zip((kq, ks, vq, vs), base):
            t.copy_(t0)
        p.fill_(pos)
        eager = call()
        assert int(p) == pos + S and torch.equal(bits(replayed), bits(eager)), pos
        assert all(torch.equal(a, b) for a, b in zip(cache, (kq, ks, vq, vs)))


# ---------------------------------------------------------------- 5. end to end
P, STEPS, VOCAB = 70, 12, 1000


def small_gqa_llama(seed=3):
    """test_gpu_decode_epilogues.gqa_llama with 4 q heads and 2 kv heads of head_dim 64: a packed 2-layer LLaMA, folded"""
    from transformers import LlamaConfig, LlamaForCausalLM
    from oracle import pb_oracle as O
    torch.manual_seed(seed)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      vocab_size=VOCAB, max_position_embeddings=256)
    model = LlamaForCausalLM(cfg).half().eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_(1 + 0.2 * torch.randn_like(p.float()))

    def producer(name, W):
        Wn = W.float().numpy()
        mask = O.ptq_low_mask(Wn, 0.9, "magnitude", None, -1)
        r = O.ptq_rtn(Wn, mask, 8, -1)
        return dict(W_fq=torch.from_numpy(r["W_fq"]), low_mask=torch.from_numpy(mask), hscale=r["hscale"], hzero=r["hzero"])

    model = H.to_pb_(model, H.quantize_dense_(model, producer)).to(DEV)
    assert H.fuse_decode_(model, epilogues=True) == 4
    model.generation_config.eos_token_id = None
    return model


@pytest.fixture(scope="module")
def model():
    return small_gqa_llama()


@pytest.fixture(scope="module")
def seq():
    return ids_of(P + STEPS, 29)                                           # the prompt and the tokens forced on every session


def wrap_fp16_path(mp):
    """the fp16 session as the exact oracle: the HIP prefill attention on, and every row the fp16 entries append replaced by its
    dequantised-quantised value (graph=False sessions only: the position is read on the host)"""
    mp.setattr(decoding, "PREFILL_ATTENTION", True)
    append, prefill = runtime.rope_append_f16, runtime.prefill_attention_f16

    def append_rt(qkv, q_off, k_off, v_off, batch, seq, n_q, n_kv, head_dim, cos, sin, k_cache, v_cache, pos):
        q = append(qkv, q_off, k_off, v_off, batch, seq, n_q, n_kv, head_dim, cos, sin, k_cache, v_cache, pos)
        at = int(pos)
        for c in (k_cache, v_cache):
            c[:, :, at:at + seq] = roundtrip(c[:, :, at:at + seq])
        return q

    def prefill_rt(q, k, v, k_cache, v_cache, pos, scaling):
        return prefill(q, roundtrip(k), roundtrip(v), k_cache, v_cache, pos, scaling)

    mp.setattr(runtime, "rope_append_f16", append_rt)
    mp.setattr(runtime, "prefill_attention_f16", prefill_rt)


def forced_logits(model, seq, **session):
    sess = H.DecodeSession(model, 1, P + STEPS, **session)
    lg = [sess.prefill(seq[:, :P]).clone()]
    for t in range(P, P + STEPS - 1):
        lg.append(sess.step(seq[:, t]).clone())
    return sess, torch.stack(lg, 1)


@pytest.fixture(scope="module")
def oracle_logits(model, seq):
    mp = pytest.MonkeyPatch()
    try:
        wrap_fp16_path(mp)
        _, wrapped = forced_logits(model, seq, graph=False)
    finally:
        mp.undo()
    _, plain = forced_logits(model, seq, graph=False)
    return wrapped, plain


def test_session_logits_equal_the_wrapped_fp16_session(model, seq, oracle_logits):
    from torch.profiler import ProfilerActivity, profile
    wrapped, plain = oracle_logits
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        sess, eager = forced_logits(model, seq, graph=False, kv_cache="fp8")
        torch.cuda.synchronize()
    names = " ".join(e.name for e in prof.events())
    for kern in ("pbl_prefill_append_kv8_kernel", "pbl_rope_append_kv8_kernel", "AttnArgsKv8", "PrefillArgsKv8"):
        assert kern in names, kern
    lay = sess.cache.layers[0]
    assert lay.keys.dtype == torch.uint8 and int(lay.cumulative_length) == P + STEPS - 1 and sess.kv_cache == "fp8"
    assert eager.shape == wrapped.shape == (1, STEPS, VOCAB) and bool(torch.isfinite(eager).all())
    assert torch.equal(bits(eager), bits(wrapped)), "prefill and step logits over the FP8 cache differ from the exact oracle's"
    gsess, graphed = forced_logits(model, seq, graph=True, kv_cache="fp8")
    assert gsess.graph is not None and torch.equal(bits(graphed), bits(eager)), "graph=True differs from graph=False"
    gsess.reset()
    glay = gsess.cache.layers[0]
    assert not glay.keys.any() and not glay.key_scales.any() and int(glay.cumulative_length) == 0 and gsess.pos == 0
    again = [gsess.prefill(seq[:, :P]).clone()] + [gsess.step(seq[:, t]).clone() for t in range(P, P + STEPS - 1)]
    assert torch.equal(bits(torch.stack(again, 1)), bits(eager)), "reset() and the same run give other logits"
    d = float((eager.float() - plain.float()).abs().max())
    print(f"[kv8] max |logits fp8 - logits fp16| = {d:.3e} at max |logit| = {float(plain.float().abs().max()):.3e} "
          f"({P} prompt tokens, {STEPS - 1} steps)")
    assert d == d and d < float("inf")


def generate_pair(model, ids, monkeypatch, **kw):
    got = H.generate(model, ids, max_new_tokens=STEPS, kv_cache="fp8", **kw)
    wrap_fp16_path(monkeypatch)
    ref = H.generate(model, ids, max_new_tokens=STEPS, graph=False, **kw)
    assert got.shape == ref.shape == (1, P + STEPS) and torch.equal(got[:, :P], ids)
    return got, ref


def test_generate_fp8_greedy_equals_the_wrapped_fp16_run(model, seq, monkeypatch):
    got, ref = generate_pair(model, seq[:, :P], monkeypatch)
    assert torch.equal(got, ref)


def test_generate_fp8_sampled_equals_the_wrapped_fp16_run(model, seq, monkeypatch):
    table = torch.rand(STEPS, 1, generator=torch.Generator().manual_seed(11))
    got, ref = generate_pair(model, seq[:, :P], monkeypatch, do_sample=True, temperature=0.9, top_k=40, top_p=0.95, uniforms=table)
    assert torch.equal(got, ref)


def test_generate_fp8_with_prompt_lookup_equals_the_wrapped_fp16_run(model, seq, monkeypatch):
    """a speculative step appends 1 + K rows and later overwrites the rejected ones: what a per-row format must survive"""
    made = []

    class Recorded(decoding.DecodeSession):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(decoding, "DecodeSession", Recorded)
    ids = torch.cat((seq[:, :P // 2], seq[:, :P - P // 2]), 1)             # a prompt that repeats itself: drafts are found
    got, ref = generate_pair(model, ids, monkeypatch, prompt_lookup_num_tokens=3)
    assert torch.equal(got, ref)
    assert [s.kv_cache for s in made] == ["fp8", "fp16"] and all(s.spec is not None and s.spec.K == 3 for s in made)
    assert made[0].speculation_stats() == made[1].speculation_stats()
