"""-m "not gpu": the prefill attention's declarations, scope table, argument checks (pbl_prefill_attn_f16 returns before any device
work) and the decoding.PREFILL_ATTENTION switch on the host, where a folded layer keeps HF's path."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from pb_llm_amd import _lib, decoding, fusion, runtime

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_exported_and_built():
    hdr = open(os.path.join(REPO, "include", "pbl.h")).read()
    assert re.search(r"^int\s+pbl_prefill_attn_f16\s*\(", hdr, re.M), "pbl_prefill_attn_f16 not declared in pbl.h"
    assert "pbl_prefill_attn_f16" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "pbl_prefill_attn_f16"), "pbl_prefill_attn_f16 not exported by libpbl.so"
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert '"pbl_prefill.hip"' in entry and os.path.exists(os.path.join(REPO, "pb_llm_amd", "csrc", "pbl_prefill.hip"))


def test_prefill_attention_ok_follows_its_scope():
    ok = runtime.prefill_attention_ok
    assert ok(1, 128, 32, 32, 128, 4096) and ok(3, 5, 8, 2, 64, 512) and ok(1, 1, 4, 4, 64, 1) and ok(64, 512, 8, 8, 128, 512)
    assert not ok(1, 8, 4, 2, 96, 64)                          # head_dim
    assert not ok(1, 8, 4, 3, 64, 64)                          # n_q % n_kv
    assert not ok(1, 65, 4, 2, 64, 64)                         # seq > max_len
    assert not ok(1, 0, 4, 2, 64, 64) and not ok(0, 8, 4, 2, 64, 64) and not ok(1, 8, 4, 0, 64, 64)
    assert not ok(65536, 8, 4, 2, 64, 64) and not ok(1, 8, 65536, 1, 64, 64)                 # the grid
    assert not ok(64, 8, 64, 64, 128, 1 << 22)                 # B Hkv max_len D > 2^40


def test_prefill_attention_raises_on_host_or_non_fp16_tensors():
    def z(*shape, dtype=torch.float16):
        return torch.zeros(*shape, dtype=dtype)

    q, k, v, kc, vc, p = z(1, 4, 8, 64), z(1, 2, 8, 64), z(1, 2, 8, 64), z(1, 2, 64, 64), z(1, 2, 64, 64), z(1, dtype=torch.int64)
    with pytest.raises(ValueError):
        runtime.prefill_attention_f16(q, k, v, kc, vc, p, 0.125)                   # on the host
    with pytest.raises(ValueError):
        runtime.prefill_attention_f16(q.float(), k.float(), v.float(), kc, vc, p, 0.125)
    with pytest.raises(ValueError):
        runtime.prefill_attention_f16(q.bfloat16(), k, v, kc, vc, p, 0.125)


def test_entry_checks_its_arguments_before_any_device_work():
    L = _lib.lib()
    INV, MIS, UNS = _lib.PBL_ERR_INVALID_ARG, _lib.PBL_ERR_MISALIGNED, _lib.PBL_ERR_UNSUPPORTED
    bufs = [(C.c_uint16 * 40000)() for _ in range(6)]
    q, k, v, kc, vc, out = (C.addressof(b) + (-C.addressof(b)) % 16 for b in bufs)
    pos = (C.c_int64 * 1)()
    qs, ks = (C.c_int64 * 3)(2048, 512, 64), (C.c_int64 * 3)(1024, 512, 64)

    def call(**over):
        a = dict(q=q, q_stride=qs, k=k, k_stride=ks, v=v, v_stride=ks, kc=kc, vc=vc, B=1, S=8, Hq=4, Hkv=2, D=64, max_len=64,
                 scaling=0.125, pos=C.addressof(pos), out=out, ldo=256)
        a.update(over)
        return L.pbl_prefill_attn_f16(a["q"], a["q_stride"], a["k"], a["k_stride"], a["v"], a["v_stride"], a["kc"], a["vc"], a["B"],
                                      a["S"], a["Hq"], a["Hkv"], a["D"], a["max_len"], a["scaling"], a["pos"], a["out"], a["ldo"], None)

    for name in ("q", "q_stride", "k", "k_stride", "v", "v_stride", "kc", "vc", "pos", "out"):
        assert call(**{name: None}) == INV, name
    for name in ("B", "S", "Hq", "Hkv", "D", "max_len"):
        assert call(**{name: 0}) == INV, name
    assert call(q_stride=(C.c_int64 * 3)(2048, -512, 64)) == INV
    assert call(v_stride=(C.c_int64 * 3)(1024, 512, -64)) == INV
    assert call(ldo=255) == INV                                  # ldo < Hq D
    assert call(S=65) == INV                                     # S > max_len
    assert call(B=1 << 12, Hkv=1 << 12, Hq=1 << 12, max_len=1 << 12, D=128, ldo=1 << 19) == INV      # B Hkv max_len D = 2^43
    assert call(out=q + 64) == INV                               # out overlaps q
    assert call(kc=k) == INV and call(vc=v + 32) == INV          # a cache overlaps an input
    assert call(vc=kc + 16) == INV                               # the caches overlap
    assert call(out=kc) == INV                                   # out overlaps a cache
    assert call(pos=out + 8) == INV                              # pos inside out
    assert call(kc=kc + 2) == MIS and call(vc=vc + 8) == MIS
    assert call(D=96, ldo=384) == UNS                            # head_dim
    assert call(Hq=4, Hkv=3) == UNS                              # Hkv does not divide Hq
    assert pos[0] == 0


def test_switch_is_off_by_default():
    assert decoding.PREFILL_ATTENTION is False


def test_folded_layer_on_the_host_keeps_hf_s_path(monkeypatch):
    """a decoder layer with the folded forward installed, on the CPU with a DecodeCache: with the switch on it still runs
    LlamaDecoderLayer.forward -- the same output and the same cache as with the switch off"""
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaDecoderLayer, LlamaRotaryEmbedding
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                      vocab_size=100, max_position_embeddings=64)
    cfg._attn_implementation = "eager"
    layer = LlamaDecoderLayer(cfg, 0).eval()
    layer.input_layernorm = fusion._DeferredNorm(layer.input_layernorm)
    layer.post_attention_layernorm = fusion._DeferredNorm(layer.post_attention_layernorm)
    layer.forward = types.MethodType(fusion._folded_layer_forward, layer)
    B, S = 2, 6
    x = torch.randn(B, S, 256)
    pid = torch.arange(S)[None]
    pe = LlamaRotaryEmbedding(cfg)(x, pid)
    mask = torch.zeros(B, 1, S, 16).masked_fill(torch.arange(16)[None, :] > torch.arange(S)[:, None], torch.finfo(torch.float32).min)
    called = []
    monkeypatch.setattr(runtime, "prefill_attention_f16", lambda *a, **k: called.append(1))

    def run(switch):
        monkeypatch.setattr(decoding, "PREFILL_ATTENTION", switch)
        cache = decoding._decode_cache_class()(cfg, B, 16, "cpu", torch.float32)
        with torch.no_grad():
            y = layer(x, attention_mask=mask, position_ids=pid, past_key_values=cache, use_cache=True, position_embeddings=pe)
        return (y[0] if isinstance(y, tuple) else y), cache.layers[0]

    (on, c_on), (off, c_off) = run(True), run(False)
    with torch.no_grad():
        cache = decoding._decode_cache_class()(cfg, B, 16, "cpu", torch.float32)
        ref = LlamaDecoderLayer.forward(layer, x, attention_mask=mask, position_ids=pid, past_key_values=cache, use_cache=True,
                                        position_embeddings=pe)
    ref = ref[0] if isinstance(ref, tuple) else ref
    assert not called
    assert torch.equal(on, off) and torch.equal(on, ref) and bool(torch.isfinite(on).all())
    assert torch.equal(c_on.keys, c_off.keys) and torch.equal(c_on.values, c_off.values) and bool(c_on.keys[:, :, :S].any())
    assert int(c_on.cumulative_length) == int(c_off.cumulative_length) == S
