"""-m "not gpu": the decode epilogues (fuse_decode_(epilogues=True); pbl_linear_f16_residual / pbl_linear_f16_swiglu_residual /
pbl_rope_f16).  The numpy restatements of HF's RoPE and residual-add roundings the GPU tests (test_gpu_decode_epilogues.py) compare
against live here and are checked against transformers' own fp16 ops on the host; the new C entries are declared, exported and
check their arguments before any device work; a host-resident model folds nothing."""
import ctypes as C
import logging
import os
import re

import numpy as np
import pytest
import torch

from oracle import pb_oracle as O
from pb_llm_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("pbl_linear_f16_residual", "pbl_linear_f16_swiglu_residual", "pbl_rope_f16")


# ---------------------------------------------------------------- numpy restatements (torch's fp16 roundings)
def rope_ref(x, cos, sin):
    """HF's apply_rotary_pos_emb on fp16 tensors, one operand: x [..., D], cos / sin broadcastable to it, all fp16.  x * cos and
    rotate_half(x) * sin each rounded to fp16 (the fp32 product of two fp16 values is exact), then the sum in fp32 rounded to fp16."""
    x, cos, sin = (np.asarray(a, np.float16) for a in (x, cos, sin))
    h = x.shape[-1] // 2
    rot = np.concatenate([-x[..., h:], x[..., :h]], -1)
    with np.errstate(invalid="ignore", over="ignore"):
        a = (x.astype(np.float32) * cos.astype(np.float32)).astype(np.float16)
        b = (rot.astype(np.float32) * sin.astype(np.float32)).astype(np.float16)
        return (a.astype(np.float32) + b.astype(np.float32)).astype(np.float16)


def residual_ref(lin, res):
    """HF's `residual + hidden_states` on fp16 tensors: the sum of two fp16 values in fp32, rounded once to fp16"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(lin, np.float16).astype(np.float32) + np.asarray(res, np.float16).astype(np.float32)).astype(np.float16)


def rope_config(scaled: bool):
    from transformers import LlamaConfig
    kw = dict(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=131072)
    if scaled:
        kw.update(rope_theta=500000.0, rope_scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                                     "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
    return LlamaConfig(**kw)


def cos_sin(cfg, positions, device="cpu"):
    """HF's position_embeddings (fp16) for position_ids [B, S]"""
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding
    emb = LlamaRotaryEmbedding(cfg).to(device)
    pid = torch.as_tensor(positions, dtype=torch.int64, device=device)
    return emb(torch.zeros(1, dtype=torch.float16, device=device), pid)


# ---------------------------------------------------------------- the C ABI
def test_new_entries_are_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "pbl.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, re.M), f"{name} not declared in pbl.h"
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name), f"{name} not exported by libpbl.so"
        assert name in doc


def _host_layer(N=64, K=64):
    """a layer descriptor whose blob is a host buffer: every call below must fail its argument checks (none may reach a launch)"""
    buf = (C.c_uint8 * 4096)()
    lay = _lib.PblLayer()
    lay.blob, lay.N, lay.K, lay.G = C.addressof(buf) + (-C.addressof(buf)) % 16, N, K, 1
    return lay, buf


def test_residual_entries_reject_bad_arguments_without_a_gpu():
    L = _lib.lib()
    INV = _lib.PBL_ERR_INVALID_ARG
    lay, keep = _host_layer()
    a = (C.c_uint16 * 1024)()
    b = (C.c_uint16 * 1024)()
    y = (C.c_uint16 * 1024)()
    pa, pb, py = C.addressof(a), C.addressof(b), C.addressof(y)
    assert L.pbl_linear_f16_residual(None, pa, pb, 64, py, 1, None) == INV
    assert L.pbl_linear_f16_residual(C.byref(lay), None, pb, 64, py, 1, None) == INV
    assert L.pbl_linear_f16_residual(C.byref(lay), pa, None, 64, py, 1, None) == INV
    assert L.pbl_linear_f16_residual(C.byref(lay), pa, pb, 64, None, 1, None) == INV
    assert L.pbl_linear_f16_residual(C.byref(lay), pa, pb, 63, py, 1, None) == INV           # ldr < N
    assert L.pbl_linear_f16_residual(C.byref(lay), pa, pb, 64, py, 0, None) == INV           # M < 1
    assert L.pbl_linear_f16_residual(C.byref(lay), pa, pb, 64, pa + 2, 1, None) == INV      # y overlaps x
    assert L.pbl_linear_f16_residual(C.byref(lay), pa, pb, 64, pb, 1, None) == INV          # y is the residual (in place)
    nolay = _lib.PblLayer()
    assert L.pbl_linear_f16_residual(C.byref(nolay), pa, pb, 64, py, 1, None) == INV        # blob NULL
    sw = L.pbl_linear_f16_swiglu_residual
    assert sw(None, pa, 128, 64, pb, 64, py, 1, None) == INV
    assert sw(C.byref(lay), pa, 128, 64, None, 64, py, 1, None) == INV
    assert sw(C.byref(lay), pa, 128, 63, pb, 64, py, 1, None) == INV                         # up overlaps gate
    assert sw(C.byref(lay), pa, 127, 64, pb, 64, py, 1, None) == INV                         # ldx < up_off + K
    assert sw(C.byref(lay), pa, 128, 64, pb, 32, py, 1, None) == INV                         # ldr < N
    assert sw(C.byref(lay), pa, 128, 64, pb, 64, pa + 200, 1, None) == INV                   # y overlaps gate_up
    assert sw(C.byref(lay), pa, 128, 64, pb, 64, pb + 64, 1, None) == INV                    # y overlaps the residual


def test_rope_entry_rejects_bad_arguments_without_a_gpu():
    L = _lib.lib()
    INV = _lib.PBL_ERR_INVALID_ARG
    bufs = [(C.c_uint16 * 4096)() for _ in range(5)]
    qkv, cs, sn, qo, ko = (C.addressof(b) for b in bufs)
    qs, ks = (C.c_int64 * 3)(512, 64, 512), (C.c_int64 * 3)(128, 64, 128)

    def call(**over):
        a = dict(qkv=qkv, ld=768, q_off=0, k_off=512, B=1, S=1, Hq=8, Hkv=2, D=64, cos=cs, sin=sn, cos_dim=64, cos_sb=0, cos_ss=0,
                 q_out=qo, q_ostride=qs, k_out=ko, k_ostride=ks)
        a.update(over)
        return L.pbl_rope_f16(a["qkv"], a["ld"], a["q_off"], a["k_off"], a["B"], a["S"], a["Hq"], a["Hkv"], a["D"], a["cos"], a["sin"],
                              a["cos_dim"], a["cos_sb"], a["cos_ss"], a["q_out"], a["q_ostride"], a["k_out"], a["k_ostride"], None)

    for k in ("qkv", "cos", "sin", "q_out", "k_out", "q_ostride", "k_ostride"):
        assert call(**{k: None}) == INV, k
    for k in ("B", "S", "Hq", "Hkv", "D", "cos_dim"):
        assert call(**{k: 0}) == INV, k
    assert call(cos_sb=-1) == INV
    assert call(q_ostride=(C.c_int64 * 3)(512, -64, 512)) == INV
    assert call(ld=639) == INV                                   # the k heads end past a row of qkv
    assert call(q_off=300) == INV                                # the q heads end past a row of qkv
    assert call(q_out=qkv + 16) == INV                           # an output overlapping qkv
    assert call(k_out=qo + 2 * 500) == INV                       # the two outputs overlapping
    assert call(q_out=cs) == INV                                 # an output overlapping cos
    assert call(k_out=sn) == INV                                 # ... or sin


# ---------------------------------------------------------------- the restatements against transformers
@pytest.mark.parametrize("scaled", [False, True])
def test_rope_restatement_matches_transformers(scaled):
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    cfg = rope_config(scaled)
    D = cfg.hidden_size // cfg.num_attention_heads
    positions = [[0, 1, 4095, 100000, 131071]]
    cos, sin = cos_sb = cos_sin(cfg, positions)
    assert cos.dtype == torch.float16 and cos.shape == (1, 5, D)
    g = torch.Generator().manual_seed(3 + scaled)
    q = (torch.randn(1, 4, 5, D, generator=g) * 40).half()
    k = (torch.randn(1, 2, 5, D, generator=g) * 40).half()
    q[0, 1, 2, 3] = float("inf")
    q[0, 2, 0, D // 2 + 1] = float("nan")
    q[0, 3, 4, 0] = 65504.0
    qe, ke = apply_rotary_pos_emb(q, k, *cos_sb)
    rq = rope_ref(q.numpy(), cos.unsqueeze(1).numpy(), sin.unsqueeze(1).numpy())
    rk = rope_ref(k.numpy(), cos.unsqueeze(1).numpy(), sin.unsqueeze(1).numpy())
    np.testing.assert_array_equal(qe.numpy(), rq)                # (NaN positions equal; values bit-for-bit on the fp16 grid)
    np.testing.assert_array_equal(ke.numpy(), rk)
    assert np.isnan(rq).any() and np.isinf(rq).any()


def test_residual_restatement_matches_torch():
    g = torch.Generator().manual_seed(5)
    lin = (torch.randn(4, 300, generator=g) * 1e3).half()
    res = (torch.randn(4, 300, generator=g) * 1e3).half()
    lin[0, :8] = 65504.0
    res[0, :8] = torch.tensor([65504.0, 8.0, 32.0, -65504.0, 1e-3, -65504.0, float("inf"), float("nan")])
    lin[1, 3] = float("-inf")
    res[1, 3] = float("inf")                                     # -inf + inf = NaN
    t = res + lin
    r = residual_ref(lin.numpy(), res.numpy())
    np.testing.assert_array_equal(t.numpy(), r)
    assert np.isinf(r[0, 0]) and r[0, 1] == 65504.0 and np.isnan(r[1, 3])


# ---------------------------------------------------------------- harness on the host
def test_fuse_decode_epilogues_on_a_host_model_folds_nothing(caplog):
    from transformers import LlamaConfig, LlamaForCausalLM
    from pb_llm_amd import harness as H
    torch.manual_seed(0)
    model = LlamaForCausalLM(LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                                         num_key_value_heads=2, vocab_size=100, max_position_embeddings=64)).half().eval()

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
        assert H.fuse_decode_(pb, prologues=True, epilogues=True) == 0
    assert [(n, type(m)) for n, m in pb.named_modules()] == before
    assert list(pb.state_dict().keys()) == keys
    assert not any("forward" in vars(m) for m in pb.modules())          # every layer keeps LlamaDecoderLayer.forward
    assert any("RoPE and the residual adds folded into the decode launches of 0 decoder layers" in r.getMessage() for r in caplog.records)
