"""-m gpu: the decode prologues -- LlamaRMSNorm folded into the fused q/k/v and gate/up GEMV launches (pbl_gemv_f16_fused_norm_host,
runtime.FusedGemv(..., norm=)), silu(gate) * up folded into the down_proj GEMV (pbl_linear_f16_swiglu, PBLinear.forward_swiglu), and
harness.fuse_decode_(prologues=True) on a HF LLaMA model.  References: the float64 restatements of HF's arithmetic
(test_decode_prologues_cpu.py) and the unfused composition on the GPU."""
import copy
import ctypes as C
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pb_oracle as O
from pb_llm_amd import _lib, synth
from pb_llm_amd import quant as Q
from pb_llm_amd.runtime import FusedGemv
from test_decode_prologues_cpu import linear_ref, rmsnorm_ref, silu_mul_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()


def make(N, K, seed, lf=0.95, groupsize=-1):
    """a synthetic PB layer as an fp16 checkpoint holds it (tools/bench_decoder_layer.py) and its W_fq on the fp16 grid"""
    W = synth.llm_weight(N, K, seed=seed)
    mask = O.ptq_low_mask(W, lf, "magnitude", None, groupsize)
    r = O.ptq_rtn(W, mask, 8, groupsize)
    W16 = torch.from_numpy(r["W_fq"]).half()
    lay = Q.PBLinear.from_dense(W16.to(DEV), None, torch.from_numpy(mask).to(DEV), groupsize, r["hscale"], r["hzero"]).to(DEV)
    return lay, W16.double().numpy()


@pytest.fixture(scope="module")
def qkv():
    return [make(4096, 4096, 40 + i) for i in range(3)]


@pytest.fixture(scope="module")
def gate_up():
    return [make(11008, 4096, 50 + i) for i in range(2)]


@pytest.fixture(scope="module")
def down():
    return make(4096, 11008, 60)


def norm_input(K, seed):
    """rows: a normal spread, values near fp16's max, all zero, one inf, one NaN"""
    rows = [synth.activations((1, K), seed, 1)[0] * np.float16(3)]
    big = synth.activations((1, K), seed, 2)[0].astype(np.float32) * 2e4
    big[:: max(K // 7, 1)] = 65504.0
    big[1:: max(K // 5, 1)] = -65504.0
    rows.append(np.clip(big, -65504, 65504).astype(np.float16))
    rows.append(np.zeros(K, np.float16))
    r = synth.activations((1, K), seed, 3)[0].copy(); r[K // 3] = np.inf
    rows.append(r)
    r = synth.activations((1, K), seed, 4)[0].copy(); r[K // 2] = np.nan
    rows.append(r)
    return np.stack(rows)


def norm_weight(K, seed):
    return (1.0 + 0.25 * synth.normal((K,), seed, 9)).astype(np.float16)


def check_rows(y, ref, what):
    y = y.double().cpu().numpy()
    for i in range(y.shape[0]):
        if np.isnan(ref[i]).any():
            assert np.isnan(ref[i]).all() and np.isnan(y[i]).all(), (what, i, "HF gives a NaN row")
        elif not np.abs(ref[i]).max():
            assert not np.abs(y[i]).max(), (what, i, "a zero row gives zeros")
        else:
            rel, ratio = O.parity_errors(y[i], ref[i])
            assert rel < 1e-3 and ratio < 1.0, (what, i, rel, ratio)


def run_norm_case(layers, x16, w16):
    from transformers.models.llama.modeling_llama import LlamaRMSNorm
    packs = [lay.packed for lay, _ in layers]
    fg = FusedGemv(packs, None, DEV)
    x, w = torch.from_numpy(x16).to(DEV), torch.from_numpy(w16).to(DEV)
    outs = fg(x, norm=(w, EPS))
    assert outs is not None, "the RMSNorm prologue declined"
    hn = rmsnorm_ref(x16, w16, EPS, np.float16)
    norm = LlamaRMSNorm(x16.shape[1], eps=EPS).half().to(DEV)
    with torch.no_grad():
        norm.weight.copy_(w)
        unfused = fg(norm(x))
    torch.cuda.synchronize()
    for o, u, (lay, Wd) in zip(outs, unfused, layers):
        assert o.shape == (x16.shape[0], lay.out_features) and o.dtype == torch.float16
        check_rows(o, linear_ref(hn, Wd), "float64 restatement")
        ud = u.double().cpu().numpy()
        check_rows(o, ud, "unfused on the GPU")          # (the normaliser may differ by 1 ulp of fp32: summation order)


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_rmsnorm_prologue_qkv_shape(qkv, M):
    X = norm_input(4096, 70 + M)
    sel = [[0], [0, 1], [1, 2, 3], [0, 1, 3, 4]][M - 1]
    run_norm_case(qkv, X[sel], norm_weight(4096, 7))


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_rmsnorm_prologue_gate_up_shape(gate_up, M):
    X = norm_input(4096, 80 + M)
    sel = [[1], [0, 4], [0, 2, 3], [1, 2, 3, 0]][M - 1]
    run_norm_case(gate_up, X[sel], norm_weight(4096, 8))


@pytest.mark.parametrize("M", [1, 3, 4])
def test_rmsnorm_prologue_scalar_staging_k_not_multiple_of_8(M):
    K = 1001
    layers = [make(96, K, 90), make(160, K, 91)]
    X = norm_input(K, 92)
    run_norm_case(layers, X[[0, 1, 4, 2][:M]], norm_weight(K, 9))


def swiglu_input(M, I, seed):
    g = np.linspace(-30.0, 30.0, I).astype(np.float16)
    gate = np.stack([np.roll(g, 37 * m) for m in range(M)])
    up = (synth.activations((M, I), seed, 5).astype(np.float32) * 2).astype(np.float16)
    return gate, up


@pytest.mark.parametrize("M", [1, 2])
def test_swiglu_prologue_down_shape(down, M):
    lay, Wd = down
    I = lay.in_features
    gate, up = swiglu_input(M, I, 100 + M)
    gu = torch.from_numpy(np.concatenate([gate, up], 1)).to(DEV)
    y = lay.forward_swiglu(gu, I)
    assert y is not None and y.shape == (M, lay.out_features) and y.dtype == torch.float16
    with torch.no_grad():
        yu = lay(F.silu(gu[:, :I]) * gu[:, I:])
    torch.cuda.synchronize()
    check_rows(y, linear_ref(silu_mul_ref(gate, up), Wd), "float64 restatement")
    check_rows(y, yu.double().cpu().numpy(), "unfused on the GPU")
    # non-finite rows: a product that overflows fp16 (silu(20) * 60000), a NaN gate -- as torch gives them
    g2, u2 = gate.copy(), up.copy()
    g2[0, 5], u2[0, 5] = 20.0, 60000.0
    if M > 1:
        g2[1, 9] = np.nan
    gu2 = torch.from_numpy(np.concatenate([g2, u2], 1)).to(DEV)
    t = F.silu(gu2[:, :I]) * gu2[:, I:]
    assert torch.isinf(t[0, 5])
    y2 = lay.forward_swiglu(gu2, I)
    with torch.no_grad():
        yu2 = lay(t)
    torch.cuda.synchronize()
    assert torch.equal(torch.isnan(y2), torch.isnan(yu2)) and torch.equal(torch.isinf(y2), torch.isinf(yu2))
    assert not torch.isfinite(y2[0]).any()
    if M > 1:
        assert torch.isnan(y2[1]).all()
    # a strided gate/up matrix (the fused launch's output is [M, 2 I] with more columns around it): same result
    wide = torch.zeros(M, 2 * I + 64, dtype=torch.float16, device=DEV)
    wide[:, :2 * I] = gu
    assert torch.equal(lay.forward_swiglu(wide, I), y)


# ---------------------------------------------------------------- declines
def test_declines_return_unsupported_through_ctypes(down, qkv):
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    lay, _ = down
    I = lay.in_features
    # more rows than one GEMV pass takes: M = 4 at K = 11008; a row count the matrix-core kernel serves: 12
    for M in (4, 12):
        gu = torch.zeros(M, 2 * I, dtype=torch.float16, device=DEV)
        y = torch.empty(M, lay.out_features, dtype=torch.float16, device=DEV)
        layer = lay.packed.layer_struct(None)
        assert L.pbl_linear_f16_swiglu(C.byref(layer), gu.data_ptr(), 2 * I, I, y.data_ptr(), M, 0, st) == _lib.PBL_ERR_UNSUPPORTED, M
        assert lay.forward_swiglu(gu, I) is None
    # column groups
    glay, _ = make(256, 512, 110, groupsize=128)
    assert glay.packed.G > 1
    gu = torch.zeros(1, 1024, dtype=torch.float16, device=DEV)
    y = torch.empty(1, 256, dtype=torch.float16, device=DEV)
    gl = glay.packed.layer_struct(None)
    assert L.pbl_linear_f16_swiglu(C.byref(gl), gu.data_ptr(), 1024, 512, y.data_ptr(), 1, 0, st) == _lib.PBL_ERR_UNSUPPORTED
    x = torch.zeros(1, 512, dtype=torch.float16, device=DEV)
    w = torch.ones(512, dtype=torch.float16, device=DEV)
    fg = FusedGemv([glay.packed], None, DEV)
    assert L.pbl_gemv_f16_fused_norm_host(C.addressof(fg._structs_host), C.addressof(fg._yoff_host), x.data_ptr(), y.data_ptr(), 1, 1,
                                          256, fg.max_NRB, 512, fg.max_nch, fg.flags, 0, w.data_ptr(), EPS, st) == _lib.PBL_ERR_UNSUPPORTED
    assert fg(x, norm=(w, EPS)) is None
    # more rows than a launch takes (5): the matrix-core / small-batch kernels serve those
    fq = FusedGemv([l_.packed for l_, _ in qkv], None, DEV)
    x5 = torch.zeros(5, 4096, dtype=torch.float16, device=DEV)
    w4 = torch.ones(4096, dtype=torch.float16, device=DEV)
    y5 = torch.empty(5, 3 * 4096, dtype=torch.float16, device=DEV)
    assert L.pbl_gemv_f16_fused_norm_host(C.addressof(fq._structs_host), C.addressof(fq._yoff_host), x5.data_ptr(), y5.data_ptr(), 3, 5,
                                          3 * 4096, fq.max_NRB, 4096, fq.max_nch, fq.flags, 0, w4.data_ptr(), EPS, st) == _lib.PBL_ERR_UNSUPPORTED
    # bad sizes: up overlapping gate, a member with another in_features
    assert L.pbl_linear_f16_swiglu(C.byref(layer), gu.data_ptr(), 2 * I, I - 1, y.data_ptr(), 1, 0, st) == _lib.PBL_ERR_INVALID_ARG
    assert L.pbl_gemv_f16_fused_norm_host(C.addressof(fq._structs_host), C.addressof(fq._yoff_host), x5.data_ptr(), y5.data_ptr(), 3, 1,
                                          3 * 4096, fq.max_NRB, 2048, fq.max_nch, fq.flags, 0, w4.data_ptr(), EPS, st) == _lib.PBL_ERR_INVALID_ARG
    torch.cuda.synchronize()


# ---------------------------------------------------------------- model level
def llama(groupsize=-1, inter=1408, seed=0):
    from transformers import LlamaConfig, LlamaForCausalLM
    from pb_llm_amd import harness as H
    torch.manual_seed(seed)
    cfg = LlamaConfig(hidden_size=512, intermediate_size=inter, num_hidden_layers=2, num_attention_heads=8,
                      num_key_value_heads=8, vocab_size=1000, max_position_embeddings=256)
    model = LlamaForCausalLM(cfg).half().eval()
    with torch.no_grad():                                   # norms that are not all ones: the weight multiply is exercised
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_(1 + 0.2 * torch.randn_like(p.float()))

    def producer(name, W):
        Wn = W.float().numpy()
        mask = O.ptq_low_mask(Wn, 0.9, "magnitude", None, groupsize)
        r = O.ptq_rtn(Wn, mask, 8, groupsize)
        out = dict(W_fq=torch.from_numpy(r["W_fq"]), low_mask=torch.from_numpy(mask), hscale=r["hscale"], hzero=r["hzero"])
        if groupsize > 0:
            out["groupsize"] = groupsize
        return out

    side = H.quantize_dense_(model, producer)
    dense = copy.deepcopy(model).to(DEV)
    plain = H.to_pb_(model, side).to(DEV)
    return dense, plain


def relmax(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / b.abs().max())


def count_ops(model, tok):
    from torch.profiler import ProfilerActivity, profile
    with torch.no_grad(), profile(activities=[ProfilerActivity.CPU]) as prof:
        model(tok, use_cache=False)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    return names.count("aten::rsqrt"), names.count("aten::silu")


@pytest.fixture(scope="module")
def models():
    from pb_llm_amd import harness as H
    dense, plain = llama()
    base = copy.deepcopy(plain)
    assert H.fuse_decode_(base) == 4
    folded = copy.deepcopy(plain)
    return dense, plain, base, folded


def test_model_folded_decode(models, caplog):
    from pb_llm_amd import harness as H
    dense, plain, base, folded = models
    with caplog.at_level(logging.INFO, logger="pb_llm_amd"):
        assert H.fuse_decode_(folded, prologues=True) == 4
    assert any("decode launches of 2 decoder layers" in r.getMessage() for r in caplog.records)
    assert sum(isinstance(m, H._DeferredNorm) for m in folded.modules()) == 4
    assert not isinstance(folded.model.norm, H._DeferredNorm)
    ids = torch.from_numpy((synth.uniform01(64, 7, 1) * 1000).astype(np.int64)).view(1, -1).to(DEV)
    # kernels per token: the folded layers run no rsqrt (only the final norm) and no silu
    L = len(folded.model.layers)
    assert count_ops(base, ids[:, :1]) == (2 * L + 1, L)
    assert count_ops(folded, ids[:, :1]) == (1, 0)
    # graph replay: 8 single tokens against fuse_decode_ alone and the dense fake-quant model; 100 replays bit-stable
    gb, gf = H.GraphedForward(base, ids[:, :1]), H.GraphedForward(folded, ids[:, :1])
    with torch.no_grad():
        for t in range(8):
            tok = ids[:, t:t + 1]
            lf = gf.replay(tok).clone()
            lb = gb.replay(tok).clone()
            ld = dense(tok, use_cache=False).logits
            assert relmax(lf, lb) < 1e-3, t
            assert relmax(lf, ld) < 1e-2, t
        first = gf.replay(ids[:, 3:4]).clone()
        for _ in range(100):
            assert torch.equal(gf.replay(ids[:, 3:4]), first)
        # a prefill (>= 16 rows) is the unfolded model's, bit for bit
        assert torch.equal(folded(ids[:, :20], use_cache=False).logits, plain(ids[:, :20], use_cache=False).logits)


def test_model_folded_eager_kv_cache_decode(models):
    from pb_llm_amd import harness as H
    dense, plain, base, folded = models
    if not any(isinstance(m, H._DeferredNorm) for m in folded.modules()):
        H.fuse_decode_(folded, prologues=True)
    ids = torch.from_numpy((synth.uniform01(16, 8, 1) * 1000).astype(np.int64)).view(2, -1).to(DEV)
    with torch.no_grad():
        ob = base(ids[:, :5], use_cache=True)
        of = folded(ids[:, :5], use_cache=True)
        assert torch.equal(ob.logits, of.logits)                 # 10 rows: the unfolded path
        pb_, pf = ob.past_key_values, of.past_key_values
        tok = ob.logits[:, -1:].argmax(-1)
        for step in range(8):                                    # batch 2: 2 rows per step through the folded launches
            ob = base(tok, past_key_values=pb_, use_cache=True)
            of = folded(tok, past_key_values=pf, use_cache=True)
            assert relmax(of.logits, ob.logits) < 1e-3, step
            pb_, pf = ob.past_key_values, of.past_key_values
            tok = ob.logits[:, -1:].argmax(-1)


def test_model_state_dict_round_trip(models):
    from pb_llm_amd import harness as H
    dense, plain, base, folded = models
    if not any(isinstance(m, H._DeferredNorm) for m in folded.modules()):
        H.fuse_decode_(folded, prologues=True)
    sd = folded.state_dict()
    fresh = copy.deepcopy(plain)
    with torch.no_grad():
        for n, p in fresh.named_parameters():
            if "layernorm" in n:
                p.mul_(2)
    H.fuse_decode_(fresh, prologues=True)
    assert set(fresh.state_dict().keys()) == set(sd.keys())
    tok = torch.tensor([[17]], device=DEV)
    with torch.no_grad():
        assert not torch.equal(fresh(tok, use_cache=False).logits, folded(tok, use_cache=False).logits)
        fresh.load_state_dict(sd)
        assert torch.equal(fresh(tok, use_cache=False).logits, folded(tok, use_cache=False).logits)


def test_model_declined_layers_are_bit_identical(models):
    """bf16 activations and column-group layers fold nothing: logits equal fuse_decode_() alone, bit for bit"""
    from pb_llm_amd import harness as H
    dense, plain, base, folded = models
    ids = torch.from_numpy((synth.uniform01(8, 9, 1) * 1000).astype(np.int64)).view(1, -1).to(DEV)
    a, b = copy.deepcopy(plain).to(torch.bfloat16), copy.deepcopy(plain).to(torch.bfloat16)
    H.fuse_decode_(a)
    H.fuse_decode_(b, prologues=True)
    assert not any(isinstance(m, H._DeferredNorm) for m in b.modules())
    _, gplain = llama(groupsize=128, seed=1)
    ga, gb = copy.deepcopy(gplain), copy.deepcopy(gplain)
    H.fuse_decode_(ga)
    H.fuse_decode_(gb, prologues=True)
    assert not any(isinstance(m, H._DeferredNorm) for m in gb.modules())
    with torch.no_grad():
        for t in range(3):
            tok = ids[:, t:t + 1]
            assert torch.equal(a(tok, use_cache=False).logits, b(tok, use_cache=False).logits), t
            assert torch.equal(ga(tok, use_cache=False).logits, gb(tok, use_cache=False).logits), t


def test_model_swiglu_decline_runs_the_unfused_tail():
    """4 rows at intermediate 11008: down_proj's prologue declines (LDS budget) and the folded MLP runs silu * up in torch and the
    layer -- bit-identical to the unfolded tail on the same gate/up output; the logits stay within 1e-3 of fuse_decode_() alone"""
    from pb_llm_amd import harness as H
    _, plain = llama(inter=11008, seed=2)
    base, folded = copy.deepcopy(plain), copy.deepcopy(plain)
    H.fuse_decode_(base)
    H.fuse_decode_(folded, prologues=True)
    ids = torch.from_numpy((synth.uniform01(8, 10, 1) * 1000).astype(np.int64)).view(4, -1).to(DEV)
    with torch.no_grad():
        mlp = folded.model.layers[0].mlp
        x = torch.randn(4, 1, 512, device=DEV).half()
        xd = folded.model.layers[0].post_attention_layernorm(x)
        assert xd is x                                          # deferred: passed on unchanged
        y = mlp(x)
        gu = mlp.gate_proj._group[0].y_all
        I = 11008
        assert mlp.down_proj.forward_swiglu(gu, I) is None
        assert torch.equal(y.reshape(4, -1), mlp.down_proj(F.silu(gu[:, :I]) * gu[:, I:2 * I]))
        assert relmax(folded(ids[:, :1], use_cache=False).logits, base(ids[:, :1], use_cache=False).logits) < 1e-3
