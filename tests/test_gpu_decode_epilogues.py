"""-m gpu: the decode epilogues -- HF's RoPE in one launch (pbl_rope_f16, runtime.rope_f16), the residual adds in the GEMV's store
(pbl_linear_f16_residual / pbl_linear_f16_swiglu_residual; PBLinear.forward_residual / forward_swiglu(residual=)) and
harness.fuse_decode_(epilogues=True) on a HF LLaMA model.  References: transformers' own functions on the GPU, and the
prologues=True model, which the folded layers must equal bit for bit."""
import copy
import ctypes as C
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pb_llm_amd import _lib, synth
from pb_llm_amd.runtime import rope_f16
from test_decode_epilogues_cpu import cos_sin, rope_config, rope_ref
from test_gpu_decode_prologues import llama, make, swiglu_input

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()


def exact(a, b):
    """equal values (NaN where NaN), equal shape, strides and dtype"""
    assert a.shape == b.shape and a.dtype == b.dtype and a.stride() == b.stride(), (a.shape, b.shape, a.stride(), b.stride())
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


# ---------------------------------------------------------------- RoPE
def qkv_out(B, S, Hq, Hkv, D, seed, scale=30.0):
    """a fused q/k/v launch's output [B S, (Hq + 2 Hkv) D] fp16 and the q / k views LlamaAttention makes of it"""
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(B * S, (Hq + 2 * Hkv) * D, generator=g) * scale).half().to(DEV)

    def heads(a, n):
        return y[:, a:a + n * D].reshape(B, S, n * D).view(B, S, -1, D).transpose(1, 2)

    return y, heads(0, Hq), heads(Hq * D, Hkv)


CASES = [(B, 1) for B in (1, 2, 3, 4)] + [(1, S) for S in (2, 3, 4)] + [(2, 2)]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B,S", CASES)
def test_rope_equals_hf(B, S, D):
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    Hq, Hkv = 8, 2                                                   # GQA
    from transformers import LlamaConfig
    cfg = LlamaConfig(hidden_size=Hq * D, num_attention_heads=Hq, num_key_value_heads=Hkv, max_position_embeddings=131072)
    y, q, k = qkv_out(B, S, Hq, Hkv, D, 10 * B + S + D)
    pos_sets = [[0, 1, 4095, 100000][:S]] if S > 1 else [[p] for p in (0, 1, 4095, 100000)]
    for pos in pos_sets:
        for per_batch in (False, True):                              # position_ids [1, S] (broadcast) and [B, S]
            pid = [[p + b * per_batch for p in pos] for b in range(B if per_batch else 1)]
            cos, sin = cos_sin(cfg, pid, DEV)
            got = rope_f16(y, 0, Hq * D, B, S, Hq, Hkv, D, cos, sin)
            assert got is not None
            ref = apply_rotary_pos_emb(q, k, cos, sin)
            exact(got[0], ref[0])
            exact(got[1], ref[1])


def test_rope_nonfinite_and_llama3_scaling():
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    B, S, Hq, Hkv, D = 1, 4, 4, 2, 128
    cfg = rope_config(scaled=True)
    y, q, k = qkv_out(B, S, Hq, Hkv, D, 7, scale=2e4)
    y[0, 5] = float("inf")
    y[1, D + D // 2 + 3] = float("-inf")
    y[2, 2 * D + 1] = float("nan")
    y[3, Hq * D + 7] = float("nan")                                  # a k head
    cos, sin = cos_sin(cfg, [[0, 1, 4095, 100000]], DEV)
    got = rope_f16(y, 0, Hq * D, B, S, Hq, Hkv, D, cos, sin)
    ref = apply_rotary_pos_emb(q, k, cos, sin)
    exact(got[0], ref[0])
    exact(got[1], ref[1])
    assert torch.isnan(got[0]).any() and torch.isinf(got[0]).any() and torch.isnan(got[1]).any()
    # the numpy restatement agrees too (the kernel's roundings are torch's, not an artefact of both being on the GPU)
    np.testing.assert_array_equal(got[0].cpu().numpy(), rope_ref(q.cpu().numpy(), cos.unsqueeze(1).cpu().numpy(),
                                                                 sin.unsqueeze(1).cpu().numpy()))


def test_rope_declines():
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    B, S, Hq, Hkv = 1, 1, 2, 1
    for D, cos_dim in ((63, 63), (258, 258), (64, 32)):
        y = torch.zeros(1, (Hq + 2 * Hkv) * D, dtype=torch.float16, device=DEV)
        cs = torch.zeros(1, 1, cos_dim, dtype=torch.float16, device=DEV)
        qo = torch.empty(B, Hq, S, D, dtype=torch.float16, device=DEV)
        ko = torch.empty(B, Hkv, S, D, dtype=torch.float16, device=DEV)
        qs, ks = (C.c_int64 * 3)(*qo.stride()[:3]), (C.c_int64 * 3)(*ko.stride()[:3])
        rc = L.pbl_rope_f16(y.data_ptr(), y.shape[1], 0, Hq * D, B, S, Hq, Hkv, D, cs.data_ptr(), cs.data_ptr(), cos_dim, 0, 0,
                            qo.data_ptr(), qs, ko.data_ptr(), ks, st)
        assert rc == _lib.PBL_ERR_UNSUPPORTED, (D, cos_dim)
        assert rope_f16(y, 0, Hq * D, B, S, Hq, Hkv, D, cs, cs) is None
    torch.cuda.synchronize()


# ---------------------------------------------------------------- residual epilogue
@pytest.fixture(scope="module")
def o_proj():
    return make(4096, 4096, 120)


@pytest.fixture(scope="module")
def down():
    return make(4096, 11008, 121)


def residual_rows(M, N, seed):
    """normal rows; row 1 near +-65504 (sums overflow to +-inf); row 2 holds inf / -inf / NaN"""
    g = torch.Generator().manual_seed(seed)
    r = (torch.randn(M, N, generator=g) * 4).half()
    if M > 1:
        r[1, ::3] = 65504.0
        r[1, 1::3] = -65504.0
    if M > 2:
        r[2, 0], r[2, 1], r[2, 2] = float("inf"), float("-inf"), float("nan")
    return r.to(DEV)


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_residual_epilogue_o_proj(o_proj, M):
    lay, _ = o_proj
    x = torch.from_numpy(synth.activations((M, 4096), 130 + M, 1) * np.float16(8)).to(DEV)
    res = residual_rows(M, 4096, M)
    y = lay.forward_residual(x, res)
    assert y is not None
    with torch.no_grad():
        ref = res + lay(x)
    exact(y, ref)
    if M > 1:
        assert torch.isinf(y[1]).any()
    # a 3-D call as LlamaDecoderLayer makes it
    y3 = lay.forward_residual(x.view(M, 1, 4096), res.view(M, 1, 4096))
    exact(y3, ref.view(M, 1, 4096))


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_residual_epilogue_down_swiglu(down, M):
    lay, _ = down
    I = lay.in_features
    gate, up = swiglu_input(M, I, 140 + M)
    gu = torch.from_numpy(np.concatenate([gate, up], 1)).to(DEV)
    res = residual_rows(M, 4096, 10 + M)
    y = lay.forward_swiglu(gu, I, residual=res)
    plain = lay.forward_swiglu(gu, I)
    if plain is None:                                               # more rows than one pass takes at K = 11008: both decline
        assert y is None and M >= 3
        return
    with torch.no_grad():
        ref = res + lay(F.silu(gu[:, :I]) * gu[:, I:])
    exact(y, res + plain)
    exact(y, ref)


def test_residual_epilogue_declines(o_proj):
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    lay, _ = o_proj
    x5 = torch.zeros(5, 4096, dtype=torch.float16, device=DEV)
    r5 = torch.zeros(5, 4096, dtype=torch.float16, device=DEV)
    y5 = torch.empty(5, 4096, dtype=torch.float16, device=DEV)
    ls = lay.packed.layer_struct(None)
    assert L.pbl_linear_f16_residual(C.byref(ls), x5.data_ptr(), r5.data_ptr(), 4096, y5.data_ptr(), 5, st) == _lib.PBL_ERR_UNSUPPORTED
    assert lay.forward_residual(x5, r5) is None
    # column groups
    glay, _ = make(256, 512, 150, groupsize=128)
    assert glay.packed.G > 1
    x = torch.zeros(1, 512, dtype=torch.float16, device=DEV)
    r = torch.zeros(1, 256, dtype=torch.float16, device=DEV)
    assert glay.forward_residual(x, r) is None
    gu = torch.zeros(1, 1024, dtype=torch.float16, device=DEV)
    assert glay.forward_swiglu(gu, 512, residual=r) is None
    # an image-only layer (its blob released to the host)
    ilay, _ = make(256, 512, 151)
    from pb_llm_amd import quant as Q
    if Q._kept_image(ilay.packed) is not None:
        ilay.release_blob_()
        assert ilay.forward_residual(x, r) is None
    # an output overlapping an input, through ctypes
    xs = torch.zeros(1, 4096, dtype=torch.float16, device=DEV)
    assert L.pbl_linear_f16_residual(C.byref(ls), xs.data_ptr(), xs.data_ptr(), 4096, xs.data_ptr(), 1, st) == _lib.PBL_ERR_INVALID_ARG
    torch.cuda.synchronize()


# ---------------------------------------------------------------- model level
def gqa_config(max_positions=256):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=512, intermediate_size=1408, num_hidden_layers=2, num_attention_heads=8,
                       num_key_value_heads=2, vocab_size=1000, max_position_embeddings=max_positions)


def gqa_llama(seed=3, max_positions=256):
    """the 2-layer model of test_gpu_decode_prologues.llama with 8 q heads and 2 kv heads"""
    from transformers import LlamaForCausalLM
    from oracle import pb_oracle as O
    from pb_llm_amd import harness as H
    torch.manual_seed(seed)
    model = LlamaForCausalLM(gqa_config(max_positions)).half().eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_(1 + 0.2 * torch.randn_like(p.float()))

    def producer(name, W):
        Wn = W.float().numpy()
        mask = O.ptq_low_mask(Wn, 0.9, "magnitude", None, -1)
        r = O.ptq_rtn(Wn, mask, 8, -1)
        return dict(W_fq=torch.from_numpy(r["W_fq"]), low_mask=torch.from_numpy(mask), hscale=r["hscale"], hzero=r["hzero"])

    side = H.quantize_dense_(model, producer)
    return H.to_pb_(model, side).to(DEV)


def pair(plain):
    from pb_llm_amd import harness as H
    pro, epi = copy.deepcopy(plain), copy.deepcopy(plain)
    assert H.fuse_decode_(pro, prologues=True) == 4
    assert H.fuse_decode_(epi, prologues=True, epilogues=True) == 4
    return pro, epi


@pytest.fixture(scope="module", params=["mha", "gqa"])
def models(request):
    plain = llama()[1] if request.param == "mha" else gqa_llama()
    pro, epi = pair(plain)
    return plain, pro, epi


def ids_of(n, seed, rows=1):
    return torch.from_numpy((synth.uniform01(n, seed, 1) * 1000).astype(np.int64)).view(rows, -1).to(DEV)


def test_model_folds_and_logs(caplog):
    from pb_llm_amd import harness as H
    plain = gqa_llama()
    epi = copy.deepcopy(plain)
    with caplog.at_level(logging.INFO, logger="pb_llm_amd"):
        assert H.fuse_decode_(epi, epilogues=True) == 4
    assert any("RoPE and the residual adds folded into the decode launches of 2 decoder layers" in r.getMessage() for r in caplog.records)
    assert all("forward" in vars(layer) for layer in epi.model.layers)


def test_model_eager_kv_cache_decode(models):
    plain, pro, epi = models
    ids = ids_of(16, 8, rows=2)
    with torch.no_grad():
        op = pro(ids[:, :5], use_cache=True)
        oe = epi(ids[:, :5], use_cache=True)
        assert torch.equal(op.logits, oe.logits)                 # 10 rows: the unfolded path
        cp, ce = op.past_key_values, oe.past_key_values
        tok = op.logits[:, -1:].argmax(-1)
        for step in range(8):                                    # batch 2: 2 rows per step through the folded layer forward
            op = pro(tok, past_key_values=cp, use_cache=True)
            oe = epi(tok, past_key_values=ce, use_cache=True)
            assert torch.equal(oe.logits, op.logits), step
            cp, ce = op.past_key_values, oe.past_key_values
            tok = op.logits[:, -1:].argmax(-1)
        for layer in range(len(epi.model.layers)):
            assert torch.equal(ce.layers[layer].keys, cp.layers[layer].keys)
            assert torch.equal(ce.layers[layer].values, cp.layers[layer].values)


def test_model_graph_replay(models):
    from pb_llm_amd import harness as H
    plain, pro, epi = models
    ids = ids_of(16, 9)
    gp, ge = H.GraphedForward(pro, ids[:, :1]), H.GraphedForward(epi, ids[:, :1])
    with torch.no_grad():
        for t in range(8):
            tok = ids[:, t:t + 1]
            assert torch.equal(ge.replay(tok).clone(), gp.replay(tok).clone()), t
        first = ge.replay(ids[:, 3:4]).clone()
        for _ in range(100):
            assert torch.equal(ge.replay(ids[:, 3:4]), first)


def count_ops(model, tok):
    from torch.profiler import ProfilerActivity, profile
    with torch.no_grad(), profile(activities=[ProfilerActivity.CPU]) as prof:
        model(tok, use_cache=False)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    return names.count("aten::neg"), names.count("aten::cat")


def test_model_runs_no_torch_rope(models):
    plain, pro, epi = models
    tok = ids_of(2, 11)[:, :1]
    L = len(epi.model.layers)
    # rotate_half's neg and cat run twice per folded layer in the prologues=True model and never in the epilogues=True one; the
    # cat outside the layers (LlamaModel's rotary embedding, the mask) is the same in both
    (pn, pc), (en, ec) = count_ops(pro, tok), count_ops(epi, tok)
    assert (pn, en) == (2 * L, 0)
    assert pc - ec == 2 * L


def test_model_prefill_equals_plain(models):
    plain, pro, epi = models
    ids = ids_of(20, 12)
    with torch.no_grad():
        assert torch.equal(epi(ids, use_cache=False).logits, plain(ids, use_cache=False).logits)


def test_model_groupsize_128_runs_plain():
    from pb_llm_amd import harness as H
    _, gplain = llama(groupsize=128, seed=1)
    ge = copy.deepcopy(gplain)
    H.fuse_decode_(ge, epilogues=True)
    assert not any("forward" in vars(m) for m in ge.modules())
    ids = ids_of(8, 13)
    with torch.no_grad():
        for t in range(3):
            tok = ids[:, t:t + 1]
            assert torch.equal(ge(tok, use_cache=False).logits, gplain(tok, use_cache=False).logits), t


def test_model_state_dict_round_trip(models):
    from pb_llm_amd import harness as H
    plain, pro, epi = models
    sd = epi.state_dict()
    assert list(sd.keys()) == list(pro.state_dict().keys())
    fresh = copy.deepcopy(plain)
    with torch.no_grad():
        for n, p in fresh.named_parameters():
            if "layernorm" in n:
                p.mul_(2)
    H.fuse_decode_(fresh, epilogues=True)
    tok = torch.tensor([[17]], device=DEV)
    with torch.no_grad():
        assert not torch.equal(fresh(tok, use_cache=False).logits, epi(tok, use_cache=False).logits)
        fresh.load_state_dict(sd)
        assert torch.equal(fresh(tok, use_cache=False).logits, epi(tok, use_cache=False).logits)
        assert torch.equal(fresh(tok, use_cache=False).logits, pro(tok, use_cache=False).logits)


def test_model_decode_step_under_inference_mode(models):
    plain, pro, epi = models
    ids = ids_of(8, 14, rows=2)
    with torch.no_grad():
        ref = pro(ids[:, :1], use_cache=False).logits
    with torch.inference_mode():
        out = epi(ids[:, :1], use_cache=False).logits
    assert torch.equal(out, ref)
