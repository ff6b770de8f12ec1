"""-m "not gpu": the decode prologues (fuse_decode_(prologues=True); pbl_gemv_f16_fused_norm_host / pbl_linear_f16_swiglu).
The float64 restatements of HF's LlamaRMSNorm / SwiGLU arithmetic the GPU tests (test_gpu_decode_prologues.py) compare against live
here and are checked against transformers' own modules on the host; the new C entries are declared and exported; a host-resident
model folds nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import pb_oracle as O
from pb_llm_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("pbl_gemv_f16_fused_norm_host", "pbl_linear_f16_swiglu")


# ---------------------------------------------------------------- float64 restatements (HF's order of roundings)
def rmsnorm_ref(x, w, eps, dt=np.float16):
    """LlamaRMSNorm.forward in float64 with its roundings to `dt` (the activation dtype): normalise, round to dt, times the weight,
    round once.  x [..., K], w [K] (both representable in dt).  Returns float64 values on dt's grid."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        var = (x * x).mean(-1, keepdims=True)
        h = (x / np.sqrt(var + eps)).astype(dt).astype(np.float64)
        return (np.asarray(w, np.float64) * h).astype(dt).astype(np.float64)


def silu_mul_ref(g, u, dt=np.float16):
    """F.silu(gate) * up on `dt` tensors in float64: silu rounded to dt, the product rounded to dt"""
    g = np.asarray(g, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (g / (1.0 + np.exp(-g))).astype(dt).astype(np.float64)
        return (s * np.asarray(u, np.float64)).astype(dt).astype(np.float64)


def linear_ref(x, W):
    """W_fq @ x in float64 (x [M, K], W [N, K])"""
    return np.asarray(x, np.float64) @ np.asarray(W, np.float64).T


# ---------------------------------------------------------------- the C ABI
def test_new_entries_are_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "pbl.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, re.M), f"{name} not declared in pbl.h"
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name), f"{name} not exported by libpbl.so"
        assert name in open(os.path.join(REPO, "INTEGRATION.md")).read()


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """argument checks come before any device work: NULL pointers are PBL_ERR_INVALID_ARG"""
    L = _lib.lib()
    layer = _lib.PblLayer()
    assert L.pbl_linear_f16_swiglu(None, None, 0, 0, None, 1, 0, None) == _lib.PBL_ERR_INVALID_ARG
    assert L.pbl_linear_f16_swiglu(C.byref(layer), None, 16, 8, None, 1, 0, None) == _lib.PBL_ERR_INVALID_ARG    # (blob NULL)
    assert L.pbl_gemv_f16_fused_norm_host(None, None, None, None, 1, 1, 8, 1, 8, 1, 0, 0, None, 1e-6, None) == _lib.PBL_ERR_INVALID_ARG


# ---------------------------------------------------------------- the restatements against transformers
@pytest.mark.parametrize("K", [64, 300])
def test_rmsnorm_restatement_matches_transformers(K):
    from transformers.models.llama.modeling_llama import LlamaRMSNorm
    rng = np.random.default_rng(K)
    x = (rng.standard_normal((3, K)) * np.array([[1.0], [30.0], [1e-3]])).astype(np.float32)
    norm = LlamaRMSNorm(K, eps=1e-6)
    with torch.no_grad():
        norm.weight.copy_(torch.from_numpy((1 + 0.2 * rng.standard_normal(K)).astype(np.float32)))
        y = norm(torch.from_numpy(x)).double().numpy()
    ref = rmsnorm_ref(x, norm.weight.detach().numpy(), 1e-6, np.float32)
    np.testing.assert_allclose(y, ref, rtol=2e-6, atol=0)
    # a zero row gives zeros; an inf in a row leaves that element NaN (rsqrt(inf) = 0)
    xs = np.zeros((2, K), np.float32); xs[1, 5] = np.inf
    with torch.no_grad():
        yz = norm(torch.from_numpy(xs)).numpy()
    rz = rmsnorm_ref(xs, norm.weight.detach().numpy(), 1e-6, np.float32)
    assert np.array_equal(np.isnan(yz), np.isnan(rz)) and np.all(rz[0] == 0) and np.isnan(rz[1, 5])


def test_mlp_restatement_matches_transformers():
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaMLP
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=64, intermediate_size=176, hidden_act="silu")
    mlp = LlamaMLP(cfg).eval()
    x = torch.randn(3, 64) * 2
    with torch.no_grad():
        y = mlp(x).double().numpy()
    Wg, Wu, Wd = (getattr(mlp, n).weight.detach().numpy() for n in ("gate_proj", "up_proj", "down_proj"))
    xn = x.numpy()
    gate, up = linear_ref(xn, Wg).astype(np.float32), linear_ref(xn, Wu).astype(np.float32)
    ref = linear_ref(silu_mul_ref(gate, up, np.float32), Wd)
    rel, _ = O.parity_errors(y, ref)
    assert rel < 1e-5, rel
    # silu's tails: -inf gate -> NaN (as F.silu), large negative -> -0, overflow of the product -> inf
    g = np.array([-np.inf, -200.0, 30.0, np.nan], np.float32)
    u = np.array([1.0, 1.0, 3e38, 1.0], np.float32)
    t = torch.nn.functional.silu(torch.from_numpy(g)) * torch.from_numpy(u)
    r = silu_mul_ref(g, u, np.float32)
    assert np.array_equal(np.isnan(t.numpy()), np.isnan(r)) and np.isinf(r[2]) and r[1] == 0


# ---------------------------------------------------------------- harness on the host
def test_fuse_decode_prologues_on_a_host_model_folds_nothing(caplog):
    import logging
    from transformers import LlamaConfig, LlamaForCausalLM
    from pb_llm_amd import harness as H
    torch.manual_seed(0)
    model = LlamaForCausalLM(LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                                         num_key_value_heads=4, vocab_size=100, max_position_embeddings=64)).half().eval()

    def producer(name, W):
        Wn = W.float().numpy()
        mask = O.ptq_low_mask(Wn, 0.9, "magnitude", None, -1)
        r = O.ptq_rtn(Wn, mask, 8, -1)
        return dict(W_fq=torch.from_numpy(r["W_fq"]), low_mask=torch.from_numpy(mask), hscale=r["hscale"], hzero=r["hzero"])

    side = H.quantize_dense_(model, producer)
    pb = H.to_pb_(model, side)
    before = [(n, type(m)) for n, m in pb.named_modules()]
    keys = list(pb.state_dict().keys())
    with caplog.at_level(logging.INFO, logger="pb_llm_amd"):
        assert H.fuse_decode_(pb, prologues=True) == 0
    assert [(n, type(m)) for n, m in pb.named_modules()] == before
    assert list(pb.state_dict().keys()) == keys
    assert any("folded into the decode launches of 0 decoder layers" in r.getMessage() for r in caplog.records)
