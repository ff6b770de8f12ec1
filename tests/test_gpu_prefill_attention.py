"""-m gpu: the HIP causal prefill attention over a static KV cache (pbl_prefill_attn_f16; runtime.prefill_attention_f16) against a
float64 restatement and torch's fp16 SDPA, with exact row selection, chunking, strided inputs, declines and graph replay; and
decoding.PREFILL_ATTENTION in folded LLaMA layers (fuse_decode_(epilogues=True)) under DecodeSession / generate.

Tolerance of the attention output: test_gpu_decode_attention's -- 4 fp16 ulps of each (row, head)'s output scale, against the float64
result over the cache after the append and against torch's fp16 SDPA over the same prefix.  The kernel's tiles are 128 query rows
and 64 key rows: the grid holds 63 / 64 / 65 / 127 / 128 / 129 and 2 * 128 + 1 = 257."""
import pytest
import torch

from pb_llm_amd import decoding, harness as H
from pb_llm_amd.runtime import prefill_attention_f16, rope_f16
from test_decode_epilogues_cpu import cos_sin
from test_gpu_decode_attention import ref64, sdpa16, within_ulps
from test_gpu_decode_epilogues import gqa_llama, ids_of, qkv_out
from test_gpu_decode_prologues import llama

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN = 512
S_GRID = (1, 4, 5, 31, 32, 33, 64, 65, 127, 128, 129, 257, 300)
POS_GRID = (0, 1, 31, 63, 64, 65, 200)
KERNEL = "pbl_prefill_attn_kernel"


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()


def bits(t):
    return t.contiguous().view(torch.int16)


def position(pos):
    return torch.tensor(pos, dtype=torch.int64, device=DEV)


def check_case(q, k_new, v_new, base_k, base_v, pos, scaling, what, sdpa=True):
    """one call at `pos` over a cache whose rows >= pos + S are NaN: the float64 and (unless sdpa=False) SDPA bounds, the position,
    the appended rows' bits, the rows below (unchanged) and above (still NaN)"""
    S, D = q.shape[2], q.shape[3]
    kc, vc = base_k.clone(), base_v.clone()
    kc[:, :, pos + S:] = float("nan")
    vc[:, :, pos + S:] = float("nan")
    p = position(pos)
    out = prefill_attention_f16(q, k_new, v_new, kc, vc, p, scaling)
    assert out.shape == (q.shape[0] * S, q.shape[1] * D) and out.dtype == torch.float16 and out.is_contiguous()
    assert int(p) == pos + S, f"{what}: the position advances by S"
    full_k, full_v = base_k.clone(), base_v.clone()
    full_k[:, :, pos:pos + S] = k_new
    full_v[:, :, pos:pos + S] = v_new
    within_ulps(out, ref64(q, full_k, full_v, pos, scaling), D, f"{what} vs float64")
    if sdpa:
        within_ulps(out, sdpa16(q, full_k, full_v, pos, scaling), D, f"{what} vs SDPA")
    for c, new, base in ((kc, k_new, base_k), (vc, v_new, base_v)):
        assert torch.equal(bits(c[:, :, pos:pos + S]), bits(new)), f"{what}: appended rows"
        assert torch.equal(bits(c[:, :, :pos]), bits(base[:, :, :pos])), f"{what}: rows below pos"
        assert bool(torch.isnan(c[:, :, pos + S:]).all()), f"{what}: rows above pos + S"


def inputs(B, Hq, Hkv, D, L, smax, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    base_k = torch.randn(B, Hkv, L, D, generator=g, device=DEV).half()
    base_v = torch.randn(B, Hkv, L, D, generator=g, device=DEV).half()
    q = (torch.randn(B, Hq, smax, D, generator=g, device=DEV) * 2).half()
    k_new = torch.randn(B, Hkv, smax, D, generator=g, device=DEV).half()
    v_new = torch.randn(B, Hkv, smax, D, generator=g, device=DEV).half()
    return base_k, base_v, q, k_new, v_new


# ---------------------------------------------------------------- 1. grid against float64
@pytest.mark.parametrize("heads", [(4, 4), (8, 2)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B", [1, 3])
def test_prefill_attention_grid(B, D, heads):
    Hq, Hkv = heads
    base_k, base_v, q, k_new, v_new = inputs(B, Hq, Hkv, D, MAX_LEN, max(S_GRID), B * 1000 + D + Hq)
    for S in S_GRID:
        for pos in POS_GRID:
            if pos + S <= MAX_LEN:
                check_case(q[:, :, :S], k_new[:, :, :S], v_new[:, :, :S], base_k, base_v, pos, D ** -0.5, f"S={S} pos={pos}")


@pytest.mark.parametrize("heads", [(4, 4), (8, 2)])
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_attention_at_position_4000(D, heads):
    Hq, Hkv = heads
    base_k, base_v, q, k_new, v_new = inputs(1, Hq, Hkv, D, 4096, 17, 4000 + D + Hq)
    check_case(q, k_new, v_new, base_k, base_v, 4000, D ** -0.5, "S=17 pos=4000")


# ---------------------------------------------------------------- 2. exact row selection
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S,pos,L", [(5, 0, 512), (65, 0, 512), (130, 63, 512), (300, 0, 512), (17, 4000, 4096)])
def test_prefill_attention_selects_rows_exactly(S, pos, L, D):
    """q_s = fp16(64 k_pi(s)) for a random valid key pi(s) of every row: every other key's weight vanishes, so the output must be
    v[pi(s)] bit for bit -- any row, column or k permutation in either product shows.  The premise is asserted on the float64
    reference first: every row's softmax weight outside pi(s), rounded to fp32, is 0.0 and the one at pi(s) is 1.0 (a score
    gap above 104 does that: exp(-104) is below half the smallest fp32 subnormal; in float64 itself such a weight is 1e-46 or less, not
    0.0)."""
    B, Hq, Hkv = 2, 8, 2
    G = Hq // Hkv
    torch.manual_seed(1000 * S + pos + D)
    base_k, base_v, _, k_new, v_new = inputs(B, Hq, Hkv, D, L, S, 7 * S + pos + D)
    # keys uniform in [-sqrt 3, sqrt 3) (unit variance): |k|^2 spreads less than a gaussian row's, which keeps the smallest gap clear
    base_k, k_new = (((torch.rand_like(t, dtype=torch.float32) * 2 - 1) * 3 ** 0.5).half() for t in (base_k, k_new))
    full_k, full_v = base_k.clone(), base_v.clone()
    full_k[:, :, pos:pos + S] = k_new
    full_v[:, :, pos:pos + S] = v_new
    g = torch.Generator(device=DEV).manual_seed(S + D)
    u = torch.rand(B, Hq, S, generator=g, device=DEV)
    pi = (u * (pos + 1 + torch.arange(S, device=DEV))).long().clamp_max(pos + S - 1)        # pi(s) in [0, pos + s]
    assert bool((pi <= pos + torch.arange(S, device=DEV)).all())
    idx = pi[..., None].expand(B, Hq, S, D)
    q = (full_k.repeat_interleave(G, 1).gather(2, idx).float() * 64).half()
    want = full_v.repeat_interleave(G, 1).gather(2, idx)                                      # [B, Hq, S, D]
    scaling = D ** -0.5
    sc = q.double() @ full_k[:, :, :pos + S].double().repeat_interleave(G, 1).transpose(-1, -2) * scaling
    allowed = torch.arange(pos + S, device=DEV)[None, :] <= (pos + torch.arange(S, device=DEV))[:, None]
    sc = sc.masked_fill(~allowed, float("-inf"))
    w32 = torch.softmax(sc, -1).float()
    onehot = torch.zeros_like(w32).scatter_(-1, pi[..., None], 1.0)
    top2 = sc.topk(2, -1).values if pos + S > 1 else None
    if top2 is not None:
        gap = (top2[..., 0] - top2[..., 1])[torch.isfinite(top2[..., 1])]
        print(f"[select] D={D} S={S} pos={pos}: smallest score gap {float(gap.min()):.0f}")
    assert torch.equal(w32, onehot), "the reference's weights are not one-hot at pi"
    kc, vc = base_k.clone(), base_v.clone()
    kc[:, :, pos + S:] = float("nan")
    vc[:, :, pos + S:] = float("nan")
    out = prefill_attention_f16(q, k_new, v_new, kc, vc, position(pos), scaling)
    assert torch.equal(bits(out), bits(want.transpose(1, 2).reshape(B * S, Hq * D)))


# ---------------------------------------------------------------- 3. chunking
@pytest.mark.parametrize("heads", [(4, 4), (8, 2)])
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_attention_is_chunking_invariant(D, heads):
    Hq, Hkv = heads
    B, S = 3, 150
    base_k, base_v, q, k_new, v_new = inputs(B, Hq, Hkv, D, MAX_LEN, S, 150 + D + Hq)

    def run(chunks):
        kc, vc, p, outs, s0 = base_k.clone(), base_v.clone(), position(0), [], 0
        for n in chunks:
            o = prefill_attention_f16(q[:, :, s0:s0 + n], k_new[:, :, s0:s0 + n], v_new[:, :, s0:s0 + n], kc, vc, p, D ** -0.5)
            outs.append(o.view(B, n, Hq * D))
            s0 += n
        assert int(p) == S
        return torch.cat(outs, 1), kc, vc

    one, kc1, vc1 = run([S])
    two, kc2, vc2 = run([70, 80])
    again, _, _ = run([S])
    assert torch.equal(bits(kc1), bits(kc2)) and torch.equal(bits(vc1), bits(vc2))
    assert torch.equal(bits(one), bits(two)), "a row's result depends on how the prompt was chunked"
    assert torch.equal(bits(one), bits(again)), "two runs of the same call differ"


# ---------------------------------------------------------------- 4. strided inputs
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B,S", [(1, 37), (3, 130)])
def test_prefill_attention_takes_the_layer_s_strided_views(B, S, D):
    from transformers import LlamaConfig
    Hq, Hkv, pos = 8, 2, 9
    cfg = LlamaConfig(hidden_size=Hq * D, num_attention_heads=Hq, num_key_value_heads=Hkv, max_position_embeddings=4096)
    y, _, _ = qkv_out(B, S, Hq, Hkv, D, 3 * B + S + D, scale=1.0)
    cos, sin = cos_sin(cfg, [[pos + s for s in range(S)]], DEV)
    q, k = rope_f16(y, 0, Hq * D, B, S, Hq, Hkv, D, cos, sin)
    v = y[:, (Hq + Hkv) * D:].reshape(B, S, Hkv, D).transpose(1, 2)
    assert not v.is_contiguous()
    base_k, base_v, _, _, _ = inputs(B, Hq, Hkv, D, MAX_LEN, 1, S + D)
    res = []
    for qq, kk, vv in ((q, k, v), (q.contiguous(), k.contiguous(), v.contiguous())):
        kc, vc, p = base_k.clone(), base_v.clone(), position(pos)
        res.append((prefill_attention_f16(qq, kk, vv, kc, vc, p, D ** -0.5), kc, vc))
        assert int(p) == pos + S
    for a, b in zip(res[0], res[1]):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(res[0][2][:, :, pos:pos + S]), bits(v))
    within_ulps(res[0][0], ref64(q, res[0][1], res[0][2], pos, D ** -0.5), D, "strided vs float64")


# ---------------------------------------------------------------- 5. declines and errors
def test_prefill_attention_declines_and_errors():
    def z(*shape, dtype=torch.float16, device=DEV):
        return torch.zeros(*shape, dtype=dtype, device=device)

    p = position(3)
    kc, vc = torch.ones(1, 2, 64, 96, dtype=torch.float16, device=DEV), torch.ones(1, 2, 64, 96, dtype=torch.float16, device=DEV)
    assert prefill_attention_f16(z(1, 4, 8, 96), z(1, 2, 8, 96), z(1, 2, 8, 96), kc, vc, p, 0.1) is None            # D = 96
    assert bool((kc == 1).all()) and bool((vc == 1).all()) and int(p) == 3
    kc, vc = torch.ones(1, 3, 64, 64, dtype=torch.float16, device=DEV), torch.ones(1, 3, 64, 64, dtype=torch.float16, device=DEV)
    assert prefill_attention_f16(z(1, 4, 8, 64), z(1, 3, 8, 64), z(1, 3, 8, 64), kc, vc, p, 0.1) is None            # 4 % 3
    assert bool((kc == 1).all()) and bool((vc == 1).all()) and int(p) == 3
    kc, vc = z(1, 2, 64, 64), z(1, 2, 64, 64)
    assert prefill_attention_f16(z(1, 4, 65, 64), z(1, 2, 65, 64), z(1, 2, 65, 64), kc, vc, p, 0.1) is None         # S > max_len
    q, k, v = z(1, 4, 8, 64), z(1, 2, 8, 64), z(1, 2, 8, 64)
    bad = [
        (q.float(), k, v, kc, vc, p),                                                       # dtype
        (q, k.float(), v, kc, vc, p),
        (q.cpu(), k, v, kc, vc, p),                                                         # device
        (q, k, v.cpu(), kc, vc, p),
        (q.transpose(2, 3).contiguous().transpose(2, 3), k, v, kc, vc, p),                  # d stride
        (q, k, v.transpose(2, 3).contiguous().transpose(2, 3), kc, vc, p),
        (q[0], k, v, kc, vc, p),                                                            # rank
        (q, k, v, kc, vc[:, :, :32], p),                                                    # k / v cache shapes differ
        (q, k, v, kc.transpose(1, 2), vc.transpose(1, 2), p),                               # cache not contiguous
        (q, k, v, z(2, 2, 64, 64), z(2, 2, 64, 64), p),                                     # cache batch
        (q, k, v, z(1, 2, 64, 128), z(1, 2, 64, 128), p),                                   # cache head_dim
        (q, z(1, 4, 8, 64), z(1, 4, 8, 64), kc, vc, p),                                     # k / v heads are not the cache's
        (q, k, z(1, 2, 7, 64), kc, vc, p),                                                  # v rows
        (q, k, v, kc.float(), vc.float(), p),                                               # cache dtype
        (q, k, v, kc, vc, p.int()),                                                         # pos dtype
        (q, k, v, kc, vc, p.cpu()),                                                         # pos device
    ]
    for args in bad:
        with pytest.raises(ValueError):
            prefill_attention_f16(*args, 0.1)
    assert int(p) == 3
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. graph capture
def test_prefill_attention_captured_once_serves_every_position():
    B, S, Hq, Hkv, D, L = 2, 8, 8, 2, 128, 256
    base_k, base_v, q, k_new, v_new = inputs(B, Hq, Hkv, D, L, S, 66)
    kc, vc, p = base_k.clone(), base_v.clone(), position(0)

    def call():
        return prefill_attention_f16(q, k_new, v_new, kc, vc, p, D ** -0.5)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    kc.copy_(base_k)
    vc.copy_(base_v)
    p.fill_(60)                                                # the second replay crosses a key-tile boundary
    graph.replay()
    first = out.clone()
    assert int(p) == 68
    graph.replay()
    second = out.clone()
    assert int(p) == 76, "the position advances once per replay"
    replayed_k, replayed_v = kc.clone(), vc.clone()
    kc.copy_(base_k)
    vc.copy_(base_v)
    p.fill_(60)
    assert torch.equal(bits(call()), bits(first)) and torch.equal(bits(call()), bits(second))
    assert int(p) == 76 and torch.equal(bits(kc), bits(replayed_k)) and torch.equal(bits(vc), bits(replayed_v))


# ---------------------------------------------------------------- model level
P, ROWS, STEPS = 37, 2, 8


@pytest.fixture(scope="module", params=["mha", "gqa"])
def epi(request):
    model = llama()[1] if request.param == "mha" else gqa_llama()
    assert H.fuse_decode_(model, epilogues=True) == 4
    model.generation_config.eos_token_id = None
    return model


@pytest.fixture(scope="module")
def seq():
    return ids_of(ROWS * (P + STEPS), 29, ROWS)                # the prompt and the tokens forced on every session


def run_session(model, seq, switch, monkeypatch, impl=None):
    """(session, prefill kernels' names, teacher-forced logits [rows, 1 + STEPS, V]) with decoding.PREFILL_ATTENTION = switch"""
    from torch.profiler import ProfilerActivity, profile
    monkeypatch.setattr(decoding, "PREFILL_ATTENTION", switch)
    was = model.config._attn_implementation
    if impl is not None:
        model.config._attn_implementation = impl
    try:
        sess = H.DecodeSession(model, seq.shape[0], seq.shape[1], graph=False)
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            lg = [sess.prefill(seq[:, :P]).float().clone()]
            torch.cuda.synchronize()
        names = " ".join(e.name for e in prof.events())
        sess.after_prefill = [int(lay.cumulative_length) for lay in sess.cache.layers]
        for t in range(P, P + STEPS):
            lg.append(sess.step(seq[:, t]).float().clone())
    finally:
        model.config._attn_implementation = was
    return sess, names, torch.stack(lg, 1)


@pytest.fixture(scope="module")
def sessions(epi, seq):
    mp = pytest.MonkeyPatch()
    try:
        on = run_session(epi, seq, True, mp)
        off = run_session(epi, seq, False, mp)
        eager = run_session(epi, seq, False, mp, impl="eager")
        sdpa = run_session(epi, seq, False, mp, impl="sdpa")
    finally:
        mp.undo()
    return on, off, eager, sdpa


def test_switch_routes_the_prefill_through_the_kernel(sessions):
    (s_on, k_on, _), (s_off, k_off, _), _, _ = sessions
    assert KERNEL in k_on and "pbl_prefill_append_kernel" in k_on
    assert KERNEL not in k_off
    for sess in (s_on, s_off):
        assert sess.after_prefill == [P] * len(sess.cache.layers) and len(sess.cache.layers) == 2
        assert [int(lay.cumulative_length) for lay in sess.cache.layers] == [P + STEPS] * 2 and sess.pos == P + STEPS
    a, b = s_on.cache.layers[0], s_off.cache.layers[0]
    assert torch.equal(bits(a.keys[:, :, :P]), bits(b.keys[:, :, :P])) and torch.equal(bits(a.values[:, :, :P]), bits(b.values[:, :, :P]))


def test_switch_keeps_the_logits_within_hf_s_own_spread(sessions):
    """prefill logits and 8 decode steps fed the same forced tokens: max |on - off| against 4 x d_ref, the max |logit| difference
    between HF's own two attention implementations (sdpa, eager) on the off path for the same ids"""
    (_, _, on), (_, _, off), (_, _, eager), (_, _, sdpa) = sessions
    assert on.shape == off.shape == (ROWS, 1 + STEPS, 1000) and bool(torch.isfinite(on).all())
    d_ref = float((sdpa - eager).abs().max())
    d = float((on - off).abs().max())
    print(f"[prefill switch] max |on - off| = {d:.3e}, d_ref (sdpa vs eager) = {d_ref:.3e}, max |logit| = {float(off.abs().max()):.3e}")
    assert d <= 4 * d_ref


def test_generate_with_the_switch_on(epi, seq, monkeypatch):
    monkeypatch.setattr(decoding, "PREFILL_ATTENTION", True)
    made = []

    class Recorded(decoding.DecodeSession):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(decoding, "DecodeSession", Recorded)
    ids = seq[:, :P]
    out = H.generate(epi, ids, max_new_tokens=8)                                   # the one-token loop
    assert out.shape == (ROWS, P + 8) and torch.equal(out[:, :P], ids)
    one = ids[:1]
    out = H.generate(epi, one, max_new_tokens=8, prompt_lookup_num_tokens=3)       # the speculative loop
    assert out.shape == (1, P + 8) and torch.equal(out[:, :P], one)
    sess = made[-1]
    assert sess.spec is not None, "the speculative path did not run"
    assert sess.pos == int(sess.cache.layers[0].cumulative_length)
    assert len({int(lay.cumulative_length) for lay in sess.cache.layers}) == 1
