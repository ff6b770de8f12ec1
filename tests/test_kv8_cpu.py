"""-m "not gpu": the FP8 KV cache on the host -- the three entries' declarations, runtime.kv8_ok's scope table, the C entries' argument
checks (each returns before any device work), the torch reference of the row format (runtime.kv8_quantize / kv8_dequantize) and the
ValueErrors of DecodeSession(..., kv_cache=) and generate(..., kv_cache=)."""
import ctypes as C
import os
import re

import pytest
import torch

from pb_llm_amd import _lib, decoding, harness as H, runtime

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pbl_rope_append_kv8", "pbl_decode_attn_kv8", "pbl_prefill_attn_kv8")
INV, MIS, UNS = _lib.PBL_ERR_INVALID_ARG, _lib.PBL_ERR_MISALIGNED, _lib.PBL_ERR_UNSUPPORTED


def test_entries_are_declared_exported_and_built():
    hdr = open(os.path.join(REPO, "include", "pbl.h")).read()
    for name in ENTRIES:
        assert re.search(rf"^int\s+{name}\s*\(", hdr, re.M), f"{name} not declared in pbl.h"
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name), f"{name} not exported by libpbl.so"
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert '"pbl_kv8.hip"' in entry and os.path.exists(os.path.join(REPO, "pb_llm_amd", "csrc", "pbl_kv8.hip"))


def test_kv8_ok_follows_its_scope():
    ok = runtime.kv8_ok
    assert ok(1, 1, 32, 32, 128, 4096) and ok(4, 4, 8, 2, 64, 65536) and ok(2, 200, 4, 2, 64, 384) and ok(1, 1, 4, 4, 64, 1)
    assert not ok(1, 1, 4, 2, 96, 64) and not ok(1, 1, 4, 2, 256, 64)             # head_dim
    assert not ok(5, 1, 4, 2, 64, 64) and not ok(0, 1, 4, 2, 64, 64)              # batch
    assert not ok(1, 1, 4, 3, 64, 64) and not ok(1, 1, 4, 0, 64, 64)              # n_q % n_kv
    assert not ok(1, 65, 4, 2, 64, 64) and not ok(1, 0, 4, 2, 64, 64)             # seq
    assert not ok(1, 1, 4, 2, 64, 65537)                                          # max_len


# ---------------------------------------------------------------- the C entries
def _buffers(n=8):
    bufs = [(C.c_uint16 * 40000)() for _ in range(n)]
    return bufs, [C.addressof(b) + (-C.addressof(b)) % 16 for b in bufs]


def test_rope_append_kv8_checks_its_arguments_before_any_device_work():
    L = _lib.lib()
    bufs, (qkv, cos, sin, q, kc, vc, ks, vs) = _buffers()
    pos = (C.c_int64 * 1)()
    qst = (C.c_int64 * 3)(512, 64, 256)

    def call(**over):
        a = dict(qkv=qkv, ld=512, q_off=0, k_off=256, v_off=384, B=1, S=2, Hq=4, Hkv=2, D=64, cos=cos, sin=sin, cos_dim=64, cos_sb=0,
                 cos_ss=64, q=q, qst=qst, kc=kc, vc=vc, ks=ks, vs=vs, max_len=64, pos=C.addressof(pos))
        a.update(over)
        return L.pbl_rope_append_kv8(a["qkv"], a["ld"], a["q_off"], a["k_off"], a["v_off"], a["B"], a["S"], a["Hq"], a["Hkv"], a["D"],
                                     a["cos"], a["sin"], a["cos_dim"], a["cos_sb"], a["cos_ss"], a["q"], a["qst"], a["kc"], a["vc"],
                                     a["ks"], a["vs"], a["max_len"], a["pos"], None)

    for name in ("qkv", "cos", "sin", "q", "qst", "kc", "vc", "ks", "vs", "pos"):
        assert call(**{name: None}) == INV, name
    for name in ("B", "S", "Hq", "Hkv", "D", "max_len", "cos_dim"):
        assert call(**{name: 0}) == INV, name
    assert call(qst=(C.c_int64 * 3)(512, -64, 256)) == INV and call(cos_ss=-1) == INV
    assert call(ld=511) == INV                                   # the v heads end beyond a row
    assert call(q=qkv + 64) == INV and call(kc=cos) == INV and call(vs=sin + 16) == INV      # an output overlaps an input
    assert call(vc=kc + 64) == INV and call(vs=ks + 16) == INV and call(ks=kc + 128) == INV  # outputs overlap each other
    assert call(ks=ks + 2) == MIS and call(vs=vs + 1) == MIS
    assert call(D=96, ld=1024, cos_dim=96) == UNS                # head_dim
    assert call(S=5, ld=512) == UNS                              # rows
    assert call(B=5) == UNS
    assert call(Hq=4, Hkv=3, ld=1024, k_off=256, v_off=448) == UNS
    assert pos[0] == 0


def test_decode_attn_kv8_checks_its_arguments_before_any_device_work():
    L = _lib.lib()
    bufs, (q, kc, vc, ks, vs, out, ws, _) = _buffers()
    pos = (C.c_int64 * 1)()
    qs = (C.c_int64 * 3)(512, 64, 256)

    def call(**over):
        a = dict(q=q, q_stride=qs, kc=kc, vc=vc, ks=ks, vs=vs, B=1, S=2, Hq=4, Hkv=2, D=64, max_len=64, scaling=0.125,
                 pos=C.addressof(pos), out=out, ldo=256, ws=ws, ws_bytes=80000)
        a.update(over)
        return L.pbl_decode_attn_kv8(a["q"], a["q_stride"], a["kc"], a["vc"], a["ks"], a["vs"], a["B"], a["S"], a["Hq"], a["Hkv"], a["D"],
                                     a["max_len"], a["scaling"], a["pos"], a["out"], a["ldo"], a["ws"], a["ws_bytes"], None)

    assert L.pbl_decode_attn_workspace_bytes(1, 2, 4, 64, 64) <= 80000
    for name in ("q", "q_stride", "kc", "vc", "ks", "vs", "pos", "out", "ws"):
        assert call(**{name: None}) == INV, name
    for name in ("B", "S", "Hq", "Hkv", "D", "max_len"):
        assert call(**{name: 0}) == INV, name
    assert call(q_stride=(C.c_int64 * 3)(512, -64, 256)) == INV
    assert call(ldo=255) == INV and call(ws_bytes=64) == INV
    assert call(out=q + 64) == INV and call(out=kc) == INV and call(out=ks + 16) == INV and call(out=vs) == INV
    assert call(ws=vc) == INV and call(ws=ks) == INV
    assert call(kc=kc + 2) == MIS and call(ws=ws + 4) == MIS and call(ks=ks + 2) == MIS
    assert call(D=96, ldo=384) == UNS and call(S=5) == UNS and call(B=5, ws_bytes=10 ** 6, ws=None) == INV
    assert call(Hq=4, Hkv=3) == UNS
    assert pos[0] == 0


def test_prefill_attn_kv8_checks_its_arguments_before_any_device_work():
    L = _lib.lib()
    bufs, (q, k, v, kc, vc, ks, vs, out) = _buffers()
    pos = (C.c_int64 * 1)()
    qs, kst = (C.c_int64 * 3)(2048, 512, 64), (C.c_int64 * 3)(1024, 512, 64)

    def call(**over):
        a = dict(q=q, q_stride=qs, k=k, k_stride=kst, v=v, v_stride=kst, kc=kc, vc=vc, ks=ks, vs=vs, B=1, S=8, Hq=4, Hkv=2, D=64,
                 max_len=64, scaling=0.125, pos=C.addressof(pos), out=out, ldo=256)
        a.update(over)
        return L.pbl_prefill_attn_kv8(a["q"], a["q_stride"], a["k"], a["k_stride"], a["v"], a["v_stride"], a["kc"], a["vc"], a["ks"],
                                      a["vs"], a["B"], a["S"], a["Hq"], a["Hkv"], a["D"], a["max_len"], a["scaling"], a["pos"], a["out"],
                                      a["ldo"], None)

    for name in ("q", "q_stride", "k", "k_stride", "v", "v_stride", "kc", "vc", "ks", "vs", "pos", "out"):
        assert call(**{name: None}) == INV, name
    for name in ("B", "S", "Hq", "Hkv", "D", "max_len"):
        assert call(**{name: 0}) == INV, name
    assert call(q_stride=(C.c_int64 * 3)(2048, -512, 64)) == INV and call(v_stride=(C.c_int64 * 3)(1024, 512, -64)) == INV
    assert call(ldo=255) == INV and call(S=65) == INV
    assert call(out=q + 64) == INV and call(kc=k) == INV and call(vc=v + 32) == INV and call(ks=q) == INV
    assert call(vc=kc + 16) == INV and call(out=kc) == INV and call(vs=ks + 16) == INV and call(ks=out + 16) == INV
    assert call(pos=out + 8) == INV and call(pos=vs + 8) == INV
    assert call(kc=kc + 2) == MIS and call(vc=vc + 8) == MIS and call(vs=vs + 2) == MIS
    assert call(D=96, ldo=384) == UNS and call(Hq=4, Hkv=3) == UNS
    assert pos[0] == 0


def test_wrappers_raise_on_host_or_wrongly_typed_tensors():
    q = torch.zeros(1, 4, 1, 64, dtype=torch.float16)
    kc, sc, p = torch.zeros(1, 2, 64, 64, dtype=torch.uint8), torch.zeros(1, 2, 64), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError):
        runtime.decode_attention_kv8(q, kc, kc.clone(), sc, sc.clone(), p, 0.125)                   # on the host
    with pytest.raises(ValueError):
        runtime.prefill_attention_kv8(q, q[:, :2], q[:, :2], kc, kc.clone(), sc, sc.clone(), p, 0.125)


# ---------------------------------------------------------------- the format's torch reference
def _e(scale):
    return torch.log2(scale).to(torch.int64).tolist()


def test_kv8_quantize_obeys_the_rule_on_the_edge_rows():
    """amax 0, 2^-20, exactly 448 * 2^e, just above it, and 6e4: the smallest e with amax <= 448 * 2^e in [-15, 7]"""
    D = 64
    rows = torch.zeros(9, D, dtype=torch.float16)
    amax = [0.0, 2.0 ** -20, 448.0, 448.25, 448.0 * 4, 448.0 * 4 + 1, 448.0 * 2.0 ** -10, 6e4, 448.0 * 2.0 ** -15]
    for i, a in enumerate(amax):
        rows[i, 5] = -a
        rows[i, 9] = a / 2
    q, scale = runtime.kv8_quantize(rows)
    assert q.dtype == torch.uint8 and q.shape == rows.shape and scale.dtype == torch.float32 and scale.shape == (9,)
    assert _e(scale) == [-15, -15, 0, 1, 2, 3, -10, 7, -15]
    assert torch.equal(scale, torch.exp2(torch.log2(scale).round()))                    # powers of two
    for i, a in enumerate(amax):
        e = _e(scale)[i]
        a16 = float(rows[i, 5].abs())
        assert (a16 <= 448 * 2.0 ** e or e == 7) and (e == -15 or a16 > 448 * 2.0 ** (e - 1))       # 6e4 > 57344: clamped at e = 7
    want = (rows.float() / scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(q, want)
    assert q[2, 5] == 0xfe and q[4, 5] == 0xfe and q[7, 5] == 0xfe and (q[0] & 0x7f).eq(0).all()  # -448 where amax = 448 * 2^e, and where it saturates
    assert not bool(((q & 0x7f) == 0x7f).any()), "no byte is NaN"
    over = torch.full((1, D), 65504.0, dtype=torch.float16)                             # beyond 57344: saturates at +-448, e = 7
    q, scale = runtime.kv8_quantize(over)
    assert _e(scale) == [7] and bool((q == 0x7e).all())


def test_kv8_roundtrip_is_exact_in_fp16_and_idempotent():
    """rows of N(0, sigma^2) from 1e-6 to 6e4: every dequantised value is an fp16 value (the fp32 product converts exactly), the row
    error is at most half an e4m3 ulp of the row's scale range (1/16 of amax), and quantising a dequantised row gives the row back.
    (Bytes and scale themselves may differ on the second pass -- a row whose amax was rounded down to exactly 448 * 2^(e-1) then
    takes e - 1 -- the values do not.)"""
    g = torch.Generator().manual_seed(7)
    for sigma in (1e-6, 1e-4, 1e-2, 1.0, 30.0, 1e3, 6e4):
        x = (torch.randn(256, 128, generator=g) * sigma).clamp(-65504, 65504).half()
        q, scale = runtime.kv8_quantize(x)
        assert int(torch.log2(scale).min()) >= -15 and int(torch.log2(scale).max()) <= 7
        assert not bool(((q & 0x7f) == 0x7f).any())
        d = runtime.kv8_dequantize(q, scale)
        assert d.dtype == torch.float16
        exact = q.view(torch.float8_e4m3fn).double() * scale[:, None].double()
        assert torch.equal(d.double(), exact), f"sigma {sigma}: a dequantised value is not an fp16 value"
        amax = x.double().abs().amax(-1, keepdim=True)
        sat = (amax > 57344).squeeze(-1)
        err = (d.double() - x.double()).abs()
        floor = 2.0 ** -25                                                               # half the smallest dequantised step (2^-9 2^-15)
        assert bool((err[~sat] <= torch.maximum(amax[~sat] / 16, torch.tensor(floor, dtype=torch.float64))).all()), sigma
        q2, scale2 = runtime.kv8_quantize(d)
        assert torch.equal(runtime.kv8_dequantize(q2, scale2), d), f"sigma {sigma}: not idempotent"


def test_kv8_reference_handles_inf_and_nan_rows():
    x = torch.zeros(3, 64, dtype=torch.float16)
    x[0, 1], x[0, 2] = float("inf"), 3.0
    x[1, 1], x[1, 2] = float("nan"), 3.0
    x[2] = float("nan")
    q, scale = runtime.kv8_quantize(x)
    assert _e(scale) == [7, -7, -15]
    assert q[0, 1] == 0x7e and (q[1, 1] & 0x7f) == 0x7f and q[1, 2] == runtime.kv8_quantize(x[1:2, 2:3].expand(1, 64))[0][0, 0]


# ---------------------------------------------------------------- DecodeSession / generate
def tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
                      vocab_size=50, max_position_embeddings=64)
    return LlamaForCausalLM(cfg).eval()


def test_session_refuses_an_unfolded_model_and_an_unknown_format():
    model = tiny_llama()
    with pytest.raises(ValueError, match="folded layer"):
        H.DecodeSession(model, 1, 16, kv_cache="fp8")
    with pytest.raises(ValueError, match="fp4"):
        H.DecodeSession(model, 1, 16, kv_cache="fp4")
    sess = H.DecodeSession(model, 1, 16, graph=False)                                      # the default is the fp16 cache, as before
    assert sess.kv_cache == "fp16" and sess.cache.layers[0].keys.dtype == model.dtype


def test_refusal_names_the_first_condition_that_fails(monkeypatch):
    import types
    from pb_llm_amd import fusion
    model = tiny_llama()
    for lay in model.model.layers:                                                          # folded as far as the check can see
        lay.forward = types.MethodType(fusion._folded_layer_forward, lay)
    assert "fp16" in decoding._kv8_refusal(model, 1, 16)                                    # an fp32 model
    model = model.half()
    assert decoding._kv8_refusal(model, 1, 16) is None
    assert "batch" in decoding._kv8_refusal(model, 5, 16)
    assert "max_length" in decoding._kv8_refusal(model, 1, 65537)
    model.config.head_dim = 96
    assert "head_dim" in decoding._kv8_refusal(model, 1, 16)


def test_fp8_cache_layers_on_the_host():
    """the layer class: uint8 rows and fp32 scales of the right shapes, half the fp16 cache's bytes plus 4 per row; update() raises;
    reset() zeroes bytes, scales and the position"""
    model = tiny_llama()
    cache = H.DecodeCache(model.config, 2, 32, "cpu", torch.float16, kv_cache="fp8")
    ref = H.DecodeCache(model.config, 2, 32, "cpu", torch.float16)
    lay, lay16 = cache.layers[0], ref.layers[0]
    assert lay.keys.dtype == lay.values.dtype == torch.uint8 and lay.keys.shape == lay16.keys.shape == (2, 1, 32, 64)
    assert lay.key_scales.dtype == torch.float32 and lay.key_scales.shape == lay.value_scales.shape == (2, 1, 32)
    nbytes = sum(t.numel() * t.element_size() for t in (lay.keys, lay.values, lay.key_scales, lay.value_scales))
    assert nbytes == 2 * 2 * 32 * (64 + 4) and nbytes * 64 * 2 == lay16.keys.numel() * 2 * 2 * (64 + 4)
    assert decoding._kv8_cache_layer(cache, 0) is lay and decoding._kv8_cache_layer(ref, 0) is None
    assert decoding._decode_cache_layer(cache, 0, 2, 1, 64) is None and int(cache.get_seq_length()) == 0
    with pytest.raises(RuntimeError, match="FP8 KV cache"):
        cache.update(torch.zeros(2, 1, 1, 64), torch.zeros(2, 1, 1, 64), 0)
    lay.keys.fill_(3), lay.key_scales.fill_(2.0), lay.value_scales.fill_(2.0), lay.cumulative_length.fill_(5)
    assert int(cache.get_seq_length()) == 5
    cache.reset()
    assert not lay.keys.any() and not lay.key_scales.any() and not lay.value_scales.any() and int(lay.cumulative_length) == 0
    with pytest.raises(ValueError, match="fp4"):
        H.DecodeCache(model.config, 2, 32, "cpu", torch.float16, kv_cache="fp4")


def test_folded_layer_over_an_fp8_cache_raises_off_its_hip_paths():
    """a folded layer on the CPU with an FP8 cache: RuntimeError before anything runs, not LlamaDecoderLayer.forward's failure inside update()"""
    import types
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding
    from pb_llm_amd import fusion
    model = tiny_llama()
    layer = model.model.layers[0]
    layer.input_layernorm = fusion._DeferredNorm(layer.input_layernorm)
    layer.post_attention_layernorm = fusion._DeferredNorm(layer.post_attention_layernorm)
    layer.forward = types.MethodType(fusion._folded_layer_forward, layer)
    cache = H.DecodeCache(model.config, 1, 16, "cpu", torch.float16, kv_cache="fp8")
    x, pid = torch.randn(1, 2, 128), torch.arange(2)[None]
    pe = LlamaRotaryEmbedding(model.config)(x, pid)
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP paths only"):
        layer(x, position_ids=pid, past_key_values=cache, use_cache=True, position_embeddings=pe)
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP paths only"):
        layer(x.repeat(1, 4, 1), position_ids=pid, past_key_values=cache, use_cache=True, position_embeddings=None)
    assert int(cache.layers[0].cumulative_length) == 0


def test_generate_raises_where_the_call_is_handed_over():
    model = tiny_llama()
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="kv_cache"):
        H.generate(model, ids, max_new_tokens=2, kv_cache="fp8")                            # a model off the GPU
    with pytest.raises(ValueError, match="kv_cache"):
        H.generate(model, ids, max_new_tokens=2, kv_cache="fp8", num_beams=2)
    with pytest.raises(ValueError, match="fp4"):
        H.generate(model, ids, max_new_tokens=2, kv_cache="fp4")
    out = H.generate(model, ids, max_new_tokens=2, pad_token_id=0)                          # the default is handed over as before
    assert out.shape == (1, 6)
