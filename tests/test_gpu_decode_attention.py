"""-m gpu: greedy generation over a static KV cache -- the HIP decode-attention entries (pbl_rope_append_f16 / pbl_decode_attn_f16;
runtime.rope_append_f16 / decode_attention_f16) against a float64 restatement, HF's RoPE and SDPA, and under graph replay; and
harness.DecodeSession / harness.generate on packed LLaMA models with fuse_decode_(epilogues=True) against model.generate.

Tolerance of the attention output: 4 fp16 ulps of the output's scale, i.e. |out - ref| <= 4 * 2^(floor(log2 max|ref|) - 10) per
query row and head, against the float64 result and against torch's fp16 SDPA over the same prefix."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from op_trace import called_ops
from pb_llm_amd import harness as H
from pb_llm_amd.runtime import decode_attention_f16, rope_append_f16, rope_f16
from test_decode_epilogues_cpu import cos_sin
from test_gpu_decode_epilogues import gqa_llama, ids_of, pair, qkv_out
from test_gpu_decode_prologues import llama

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN = 4096
ULPS = 4


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()


def ref64(q, k, v, pos, scaling):
    """float64 softmax(scaling q k^T) v over cache rows [0, pos + s] (causal inside the S rows, GQA): [B S, Hq D]"""
    B, Hq, S, D = q.shape
    G = Hq // k.shape[1]
    k, v = (t[:, :, :pos + S].double().repeat_interleave(G, 1) for t in (k, v))
    sc = q.double() @ k.transpose(-1, -2) * scaling
    allowed = torch.arange(pos + S, device=q.device)[None, :] <= (pos + torch.arange(S, device=q.device))[:, None]
    return (torch.softmax(sc.masked_fill(~allowed, float("-inf")), -1) @ v).transpose(1, 2).reshape(B * S, Hq * D)


def sdpa16(q, k, v, pos, scaling):
    B, Hq, S, D = q.shape
    G = Hq // k.shape[1]
    k, v = (t[:, :, :pos + S].repeat_interleave(G, 1) for t in (k, v))
    allowed = torch.arange(pos + S, device=q.device)[None, :] <= (pos + torch.arange(S, device=q.device))[:, None]
    return F.scaled_dot_product_attention(q, k, v, attn_mask=allowed, scale=scaling).transpose(1, 2).reshape(B * S, Hq * D)


def within_ulps(got, ref, D, what):
    g, r = got.double().view(got.shape[0], -1, D), ref.double().view(ref.shape[0], -1, D)
    scale = r.abs().amax(-1, keepdim=True).clamp_min(2.0 ** -14)
    tol = ULPS * torch.exp2(torch.floor(torch.log2(scale)) - 10)
    err = (g - r).abs()
    assert bool((err <= tol).all()), f"{what}: max error {float((err / tol).max()):.2f} x the bound"


@pytest.mark.parametrize("heads", [(32, 32), (8, 2)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_decode_attention_grid(B, D, heads):
    Hq, Hkv = heads
    g = torch.Generator(device=DEV).manual_seed(B * 1000 + D + Hq)
    base_k = torch.randn(B, Hkv, MAX_LEN, D, generator=g, device=DEV).half()
    base_v = torch.randn(B, Hkv, MAX_LEN, D, generator=g, device=DEV).half()
    scaling = D ** -0.5
    for S in (1, 2, 3, 4):
        q = (torch.randn(B, Hq, S, D, generator=g, device=DEV) * 2).half()
        for pos in (0, 1, 63, 64, 65, 1000, MAX_LEN - S):
            kc, vc = base_k.clone(), base_v.clone()
            kc[:, :, pos + S:] = float("nan")                      # rows beyond pos + S: read them and the output is NaN
            vc[:, :, pos + S:] = float("nan")
            p = torch.tensor(pos, dtype=torch.int64, device=DEV)
            out = decode_attention_f16(q, kc, vc, p, scaling)
            assert out.shape == (B * S, Hq * D) and out.dtype == torch.float16 and out.is_contiguous()
            assert int(p) == pos + S, "the position advances by S"
            within_ulps(out, ref64(q, base_k, base_v, pos, scaling), D, f"S={S} pos={pos} vs float64")
            within_ulps(out, sdpa16(q, base_k, base_v, pos, scaling), D, f"S={S} pos={pos} vs SDPA")
    # q as rope_append_f16 returns it for a fused launch's output (strided, not contiguous)
    qt = torch.randn(B, 2, Hq, D, generator=g, device=DEV).half().transpose(1, 2)
    p = torch.tensor(70, dtype=torch.int64, device=DEV)
    within_ulps(decode_attention_f16(qt, base_k, base_v, p, scaling), ref64(qt, base_k, base_v, 70, scaling), D, "strided q")


def test_decode_attention_declines():
    kc = torch.zeros(1, 2, 64, 96, dtype=torch.float16, device=DEV)
    p = torch.zeros((), dtype=torch.int64, device=DEV)
    assert decode_attention_f16(torch.zeros(1, 4, 1, 96, dtype=torch.float16, device=DEV), kc, kc.clone(), p, 0.1) is None   # D = 96
    kc = torch.zeros(1, 3, 64, 64, dtype=torch.float16, device=DEV)
    assert decode_attention_f16(torch.zeros(1, 4, 1, 64, dtype=torch.float16, device=DEV), kc, kc.clone(), p, 0.1) is None   # 4 % 3
    kc = torch.zeros(1, 2, 64, 64, dtype=torch.float16, device=DEV)
    assert decode_attention_f16(torch.zeros(1, 4, 5, 64, dtype=torch.float16, device=DEV), kc, kc.clone(), p, 0.1) is None   # S = 5
    assert int(p) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B,S", [(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (4, 1)])
def test_rope_append_equals_hf(B, S, D):
    check_rope_append(B, S, D, 8, 2, 512, (0, 5, 512 - S))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B,S", [(1, 1), (4, 4)])
def test_rope_append_equals_hf_at_65536_rows(B, S, D):
    """the largest cache the entries accept, the last rows of its last head: the cache index ((b Hkv + hh) max_len + row) D reaches
    4 * 8 * 65536 * 128 = 2^28 elements"""
    check_rope_append(B, S, D, 8, 8, 65536, (65536 - S - 1, 65536 - S))


def check_rope_append(B, S, D, Hq, Hkv, L, positions):
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    cfg = LlamaConfig(hidden_size=Hq * D, num_attention_heads=Hq, num_key_value_heads=Hkv, max_position_embeddings=131072)
    y, q, k = qkv_out(B, S, Hq, Hkv, D, 31 * B + S + D)
    v = y[:, (Hq + Hkv) * D:].reshape(B, S, Hkv, D).transpose(1, 2)
    for pos in positions:
        cos, sin = cos_sin(cfg, [[pos + s for s in range(S)]], DEV)
        kc0 = torch.randn(B, Hkv, L, D, device=DEV).half()
        vc0 = torch.randn(B, Hkv, L, D, device=DEV).half()
        kc, vc = kc0.clone(), vc0.clone()
        p = torch.tensor(pos, dtype=torch.int64, device=DEV)
        got = rope_append_f16(y, 0, Hq * D, (Hq + Hkv) * D, B, S, Hq, Hkv, D, cos, sin, kc, vc, p)
        q_ref, k_ref = apply_rotary_pos_emb(q, k, cos, sin)
        q_rope = rope_f16(y, 0, Hq * D, B, S, Hq, Hkv, D, cos, sin)[0]
        assert got.shape == q_rope.shape and got.stride() == q_rope.stride()
        assert torch.equal(got.view(torch.int16), q_rope.view(torch.int16))             # rope_f16's q, bit for bit
        assert torch.equal(got, q_ref)
        assert torch.equal(kc[:, :, pos:pos + S].view(torch.int16), k_ref.contiguous().view(torch.int16))
        assert torch.equal(vc[:, :, pos:pos + S].view(torch.int16), v.contiguous().view(torch.int16))
        for c, c0 in ((kc, kc0), (vc, vc0)):                                            # every other row unchanged
            assert torch.equal(c[:, :, :pos], c0[:, :, :pos]) and torch.equal(c[:, :, pos + S:], c0[:, :, pos + S:])
        assert int(p) == pos                                                            # the append leaves the position ...
        decode_attention_f16(got, kc, vc, p, D ** -0.5)
        assert int(p) == pos + S                                                        # ... the attention advances it


def test_captured_step_is_bit_stable_and_position_independent():
    from transformers import LlamaConfig
    B, S, Hq, Hkv, D, L = 1, 1, 8, 2, 128, 256
    cfg = LlamaConfig(hidden_size=Hq * D, num_attention_heads=Hq, num_key_value_heads=Hkv, max_position_embeddings=4096)
    y, _, _ = qkv_out(B, S, Hq, Hkv, D, 5)
    cos, sin = cos_sin(cfg, [[17]], DEV)
    kc = torch.randn(B, Hkv, L, D, device=DEV).half()
    vc = torch.randn(B, Hkv, L, D, device=DEV).half()
    p = torch.tensor(100, dtype=torch.int64, device=DEV)

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
    p.fill_(100)
    with torch.cuda.graph(graph):
        out = step()
    first = None
    for _ in range(100):
        p.fill_(100)
        graph.replay()
        first = out.clone() if first is None else first
        assert torch.equal(out.view(torch.int16), first.view(torch.int16))
    assert int(p) == 101
    for pos in range(0, 70):                                   # across the 32-key split boundaries
        p.fill_(pos)
        graph.replay()
        replayed = out.clone()
        p.fill_(pos)
        eager = step()
        assert torch.equal(replayed.view(torch.int16), eager.view(torch.int16)), pos
        assert int(p) == pos + 1


# ---------------------------------------------------------------- model level
@pytest.fixture(scope="module", params=["mha", "gqa"])
def epi(request):
    plain = llama()[1] if request.param == "mha" else gqa_llama()
    _, e = pair(plain)
    e.generation_config.eos_token_id = None                    # model.generate runs to the length limit unless a test sets eos
    return e


def hf_run(model, ids, n, **kw):
    out = model.generate(ids, do_sample=False, max_new_tokens=n, output_scores=True, return_dict_in_generate=True, **kw)
    return out.sequences, torch.stack(out.scores, 1).float()


def session_logits(model, seq, P, graph=True):
    """teacher-forced logits of a DecodeSession over seq: the prefill of seq[:, :P], then one step per token"""
    sess = H.DecodeSession(model, seq.shape[0], seq.shape[1], graph=graph)
    lg = [sess.prefill(seq[:, :P]).float().clone()]
    for t in range(P, seq.shape[1] - 1):
        lg.append(sess.step(seq[:, t]).float().clone())
    return torch.stack(lg, 1)


def greedy_agreement(model, prompts, n=32, min_steps=16):
    """generate against model.generate: (steps compared, relative teacher-forced logit difference).  The tolerance is measured:
    the largest |session - HF| logit difference on HF's own sequence; tokens must agree up to the first step where HF's top-1 /
    top-2 margin (over the rows) falls below twice that.  A random model has near-ties: of the candidate prompts, the first whose
    HF margins stay clear for min_steps is compared (chosen by HF's run alone), and the caller asserts that one was found"""
    for ids in prompts:
        P = ids.shape[1]
        seq, scores = hf_run(model, ids, n)
        tf = session_logits(model, seq, P)
        diff = float((tf - scores).abs().max())
        rel = diff / float(scores.abs().max())
        top2 = scores.topk(2, -1).values
        margin = (top2[..., 0] - top2[..., 1]).amin(0)
        close = (margin < 2 * diff).nonzero()
        steps = int(close[0]) if len(close) else n
        if steps >= min_steps:
            break
    ours = H.generate(model, ids, max_new_tokens=n)
    assert ours.shape == seq.shape
    assert torch.equal(ours[:, :P + steps], seq[:, :P + steps])
    print(f"[greedy] P={P} rows={ids.shape[0]}: {steps} steps compared, teacher-forced logits rel {rel:.2e} (abs {diff:.2e})")
    return steps, rel


def prompts(P, rows, seed):
    return [ids_of(P * rows, seed + 100 * i, rows) for i in range(6)]


@pytest.mark.parametrize("P,rows", [(3, 1), (9, 1), (2, 2)])
def test_generate_equals_model_generate(epi, P, rows):
    steps, rel = greedy_agreement(epi, prompts(P, rows, 40 + P))
    assert rel < 1e-2
    assert steps >= 16, "near-tie within 16 steps: pick another prompt"


def test_generate_eos_and_padding_equal_hf(epi):
    P, n = 4, 12
    ids = ids_of(2 * P, 77, 2)
    seq, _ = hf_run(epi, ids, n)
    new = seq[:, P:].tolist()
    eos = next(t for t in new[0][2:] if t not in new[1] and t not in new[0][:2])          # row 0 finishes early, row 1 runs on
    k = new[0].index(eos)
    ref = epi.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=eos, pad_token_id=0)
    got = H.generate(epi, ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=0)
    assert got.shape == ref.shape == (2, P + n) and torch.equal(got, ref)
    assert bool((got[0, P + k + 1:] == 0).all())
    eos2 = [eos, new[1][5]]                                                                 # both rows finish: a shorter result
    ref = epi.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=eos2)
    got = H.generate(epi, ids, max_new_tokens=n, eos_token_id=eos2)
    assert got.shape == ref.shape and got.shape[1] < P + n and torch.equal(got, ref)


def test_generate_under_inference_mode_equals_no_grad(epi):
    ids = ids_of(5, 91)
    with torch.no_grad():
        a = H.generate(epi, ids, max_new_tokens=20)
        la = session_logits(epi, a, 5)
    with torch.inference_mode():
        b = H.generate(epi, ids, max_new_tokens=20)
        lb = session_logits(epi, a, 5)
    assert torch.equal(a, b) and torch.equal(la, lb)


def test_folded_step_runs_the_new_kernels_only(epi):
    from torch.profiler import ProfilerActivity, profile
    ids = ids_of(6, 12)
    sess = H.DecodeSession(epi, 1, 16, graph=False)
    sess.prefill(ids[:, :5])
    layer = H.decoder_layers(epi)[0]
    seen = []
    h = layer.register_forward_pre_hook(lambda m, a, k: seen.append((a, k)), with_kwargs=True)
    sess.step(ids[:, 5])
    h.remove()
    args, kwargs = seen[0]
    assert type(kwargs["past_key_values"]).__name__ == "DecodeCache"
    with torch.no_grad():
        ops = called_ops(lambda: layer(*args, **kwargs))
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            layer(*args, **kwargs)
            torch.cuda.synchronize()
    assert not ops & {"aten::index_copy_", "aten::cat", "aten::scaled_dot_product_attention"}, ops & {"aten::index_copy_", "aten::cat",
                                                                                                     "aten::scaled_dot_product_attention"}
    names = " ".join(e.name for e in prof.events())
    for kern in ("pbl_rope_append_kernel", "pbl_attn_partial_kernel", "pbl_attn_combine_kernel"):
        assert kern in names, kern


def step_kernels(model, seq, P):
    """the GPU kernels' names in one eager session step at position P, after a prefill of seq[:, :P]"""
    from torch.profiler import ProfilerActivity, profile
    sess = H.DecodeSession(model, seq.shape[0], seq.shape[1], graph=False)
    sess.prefill(seq[:, :P])
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        sess.step(seq[:, P])
        torch.cuda.synchronize()
    return " ".join(e.name for e in prof.events())


def test_session_across_position_4096_equals_hf_attention():
    """a session of 4120 positions (chunk 64, 65 splits: what tools/bench_generate.py measures at context 4096): 4090 tokens
    prefilled, then teacher-forced steps across position 4096 -- the HIP decode attention against the same model and session
    over HF's StaticLayer and SDPA, at the bound this file applies to session-vs-HF logits"""
    from pb_llm_amd import decoding
    model = gqa_llama(max_positions=4224)
    assert H.fuse_decode_(model, epilogues=True) == 4
    P, n = 4090, 4120
    seq = ids_of(n, 23)
    assert "pbl_attn_partial_kernel" in step_kernels(model, seq, P)
    on = session_logits(model, seq, P)
    was = decoding.DECODE_ATTENTION
    decoding.DECODE_ATTENTION = False
    try:
        off = session_logits(model, seq, P)
        assert "pbl_attn_partial_kernel" not in step_kernels(model, seq, P)
    finally:
        decoding.DECODE_ATTENTION = was
    assert on.shape == off.shape == (1, n - P, 1000) and bool(torch.isfinite(on).all())
    diff = float((on - off).abs().max())
    rel = diff / float(off.abs().max())
    print(f"[long context] P={P}, {n - P - 1} steps across position 4096: logits rel {rel:.2e} (abs {diff:.2e}) against HF's attention")
    assert rel < 1e-2


def test_generate_without_the_kernels_reproduces_hf():
    """the fallback path: a packed model without fuse_decode_, and a bf16 model -- HF's StaticLayer and attention under the session"""
    dense, plain = llama(seed=5)
    plain.generation_config.eos_token_id = None
    steps, rel = greedy_agreement(plain, prompts(6, 1, 55))
    assert steps >= 16 and rel < 1e-2
    b16 = copy.deepcopy(dense).to(torch.bfloat16)
    b16.generation_config.eos_token_id = None
    steps, rel = greedy_agreement(b16, prompts(6, 1, 56))
    assert steps >= 16 and rel < 5e-2
