"""-m "not gpu": greedy generation over a static KV cache (harness.DecodeSession / harness.generate; pbl_rope_append_f16 and
pbl_decode_attn_f16).  The float64 restatement of the split decode attention that the GPU tests (test_gpu_decode_attention.py)
compare against lives here and is checked against a direct softmax(Q K^T) V; the new C entries are declared, exported and decline
unsupported shapes before any device work; the length / eos / pad resolution of generate and the session's host-side bookkeeping
are checked on CPU models."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from pb_llm_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("pbl_rope_append_f16", "pbl_decode_attn_workspace_bytes", "pbl_decode_attn_f16")


# ---------------------------------------------------------------- the float64 restatement
def decode_attn_ref(q, k, v, pos, scaling, chunk=32):
    """float64 decode attention as the kernel splits it: q [B, Hq, S, D], k / v [B, Hkv, max_len, D]; query row s of head h attends
    to rows [0, pos + s] of kv head h // (Hq / Hkv).  Per split of `chunk` keys the partial (m, l, acc), then their merge in split
    order.  Returns [B * S, Hq * D] float64."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    B, Hq, S, D = q.shape
    G = Hq // k.shape[1]
    out = np.zeros((B, S, Hq, D))
    for b in range(B):
        for h in range(Hq):
            for s in range(S):
                n = pos + s + 1
                M, L, acc = -np.inf, 0.0, np.zeros(D)
                for k0 in range(0, n, chunk):
                    kk, vv = k[b, h // G, k0:min(n, k0 + chunk)], v[b, h // G, k0:min(n, k0 + chunk)]
                    sc = kk @ q[b, h, s] * scaling
                    m = sc.max()
                    p = np.exp(sc - m)
                    Mn = max(M, m)
                    acc = acc * np.exp(M - Mn) + (p @ vv) * np.exp(m - Mn)
                    L = L * np.exp(M - Mn) + p.sum() * np.exp(m - Mn)
                    M = Mn
                out[b, s, h] = acc / L
    return out.reshape(B * S, Hq * D)


def direct_attn(q, k, v, pos, scaling):
    """softmax(scaling Q K^T + causal mask) V in float64 torch, GQA by repeating the kv heads"""
    q, k, v = (torch.as_tensor(np.asarray(a, np.float64)) for a in (q, k, v))
    B, Hq, S, D = q.shape
    G = Hq // k.shape[1]
    k, v = k[:, :, :pos + S].repeat_interleave(G, 1), v[:, :, :pos + S].repeat_interleave(G, 1)
    sc = q @ k.transpose(-1, -2) * scaling
    allowed = torch.arange(pos + S)[None, :] <= (pos + torch.arange(S))[:, None]
    sc = sc.masked_fill(~allowed, float("-inf"))
    return (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B * S, Hq * D).numpy()


@pytest.mark.parametrize("B,S,Hq,Hkv,D,pos", [(1, 1, 4, 4, 16, 0), (2, 3, 4, 2, 8, 70), (1, 4, 6, 3, 16, 31), (3, 2, 2, 1, 8, 5),
                                              (1, 1, 2, 2, 8, 64)])
def test_restatement_matches_direct_softmax(B, S, Hq, Hkv, D, pos):
    rng = np.random.default_rng(B * 100 + S * 10 + pos)
    L = pos + S + 7
    q = rng.standard_normal((B, Hq, S, D)) * 2
    k, v = rng.standard_normal((B, Hkv, L, D)), rng.standard_normal((B, Hkv, L, D))
    np.testing.assert_allclose(decode_attn_ref(q, k, v, pos, D ** -0.5), direct_attn(q, k, v, pos, D ** -0.5), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("chunk", [64, 96, 512])
@pytest.mark.parametrize("B,S,Hq,Hkv,D", [(1, 1, 2, 2, 8), (2, 4, 4, 2, 16)])
def test_restatement_matches_direct_softmax_at_the_larger_chunks(B, S, Hq, Hkv, D, chunk):
    """the chunk sizes the GPU tests rely on beyond 32, at positions past one chunk: a split boundary inside the S rows, one key
    into the second split, and several splits with a cut-short last one"""
    rng = np.random.default_rng(chunk + 10 * B + S)
    for pos in (chunk - 2, chunk, 2 * chunk + chunk // 2 + 3):
        L = pos + S + 7
        q = rng.standard_normal((B, Hq, S, D)) * 2
        k, v = rng.standard_normal((B, Hkv, L, D)), rng.standard_normal((B, Hkv, L, D))
        np.testing.assert_allclose(decode_attn_ref(q, k, v, pos, D ** -0.5, chunk), direct_attn(q, k, v, pos, D ** -0.5),
                                   rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------- the split plan
def split_plan(max_len):
    """(chunk, nsplit) of pbl_decode_attn_f16: keys per split and splits"""
    chunk = 32 * -(-max_len // 4096)
    return chunk, -(-max_len // chunk)


def test_split_plan_over_every_supported_length():
    L = _lib.lib()
    shapes = [(1, 1, 8, 128), (4, 4, 32, 64), (2, 3, 4, 128)]
    for max_len in range(1, 65537):
        chunk, nsplit = split_plan(max_len)
        assert chunk <= 512 and nsplit <= 128 and chunk * nsplit >= max_len, max_len
        for B, S, Hq, D in shapes:
            assert L.pbl_decode_attn_workspace_bytes(B, S, Hq, D, max_len) == B * Hq * S * nsplit * (2 + D) * 4, (max_len, B, S, Hq, D)
    assert split_plan(4096) == (32, 128) and split_plan(4097) == (64, 65) and split_plan(65536) == (512, 128)


def test_decode_attention_declines_65537_rows_before_any_launch():
    from pb_llm_amd import runtime as R
    L = _lib.lib()
    rows, D = 65537, 64
    keep = [(C.c_uint16 * (rows * D + 8))() for _ in range(2)] + [(C.c_uint16 * (1 << 15))() for _ in range(3)]   # k, v; q, out, ws
    kc, vc, q, out, ws = (C.addressof(b) + (-C.addressof(b)) % 16 for b in keep)
    pos = (C.c_int64 * 1)(0)
    need = L.pbl_decode_attn_workspace_bytes(1, 1, 1, D, rows)
    assert 0 < need <= (1 << 16) - 16
    assert L.pbl_decode_attn_f16(q, (C.c_int64 * 3)(D, D, D), kc, vc, 1, 1, 1, 1, D, rows, 0.125, C.addressof(pos), out, D, ws, need,
                                 None) == _lib.PBL_ERR_UNSUPPORTED
    assert pos[0] == 0
    assert R.decode_attention_ok(1, 1, 1, 1, D, 65536) and not R.decode_attention_ok(1, 1, 1, 1, D, rows)


# ---------------------------------------------------------------- the C ABI
def test_new_entries_are_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "pbl.h")).read()
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"^(int|size_t)\s+" + name + r"\s*\(", hdr, re.M), f"{name} not declared in pbl.h"
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name), f"{name} not exported by libpbl.so"
    for name in ("pbl_rope_append_f16", "pbl_decode_attn_f16"):
        assert name in doc


def _bufs(n=6, elems=1 << 16):
    keep = [(C.c_uint16 * elems)() for _ in range(n)]
    return keep, [C.addressof(b) + (-C.addressof(b)) % 16 for b in keep]


def test_rope_append_declines_before_any_launch():
    L = _lib.lib()
    keep, (qkv, cs, qo, kc, vc, ps) = _bufs()
    pos = (C.c_int64 * 1)(0)

    def call(**over):
        a = dict(ld=768, q_off=0, k_off=512, v_off=640, B=1, S=1, Hq=8, Hkv=2, D=64, cos_dim=64, qst=(512, 64, 512), kc=kc, vc=vc, L=64,
                 pos=C.addressof(pos))
        a.update(over)
        return L.pbl_rope_append_f16(qkv, a["ld"], a["q_off"], a["k_off"], a["v_off"], a["B"], a["S"], a["Hq"], a["Hkv"], a["D"], cs, cs,
                                     a["cos_dim"], 0, 0, qo, (C.c_int64 * 3)(*a["qst"]), a["kc"], a["vc"], a["L"], a["pos"], None)

    UNS, INV = _lib.PBL_ERR_UNSUPPORTED, _lib.PBL_ERR_INVALID_ARG
    assert call(D=96, cos_dim=96, ld=1152, k_off=768, v_off=960) == UNS
    assert call(S=5) == UNS
    assert call(B=5) == UNS
    assert call(Hq=6, Hkv=4, ld=896, k_off=384, v_off=640) == UNS           # 6 % 4 kv heads
    # bad arguments, each on an unsupported shape as well: a missed check answers UNSUPPORTED instead of launching on host memory
    bad = dict(S=5)
    assert call(pos=None, **bad) == INV
    assert call(kc=None, **bad) == INV
    assert call(L=0, **bad) == INV
    assert call(vc=kc, **bad) == INV                                        # k and v cache overlapping
    assert call(v_off=700, **bad) == INV                                    # the v heads end past a row of qkv


def test_decode_attention_declines_before_any_launch():
    L = _lib.lib()
    keep, (q, kc, vc, out, ws, _) = _bufs()
    pos = (C.c_int64 * 1)(0)

    def call(**over):
        a = dict(B=1, S=1, Hq=4, Hkv=2, D=64, L=64, ldo=256, ws=ws, ws_bytes=1 << 17, out=out, pos=C.addressof(pos))
        a.update(over)
        return L.pbl_decode_attn_f16(q, (C.c_int64 * 3)(256, 64, 64), kc, vc, a["B"], a["S"], a["Hq"], a["Hkv"], a["D"], a["L"], 0.125,
                                     a["pos"], a["out"], a["ldo"], a["ws"], a["ws_bytes"], None)

    UNS, INV = _lib.PBL_ERR_UNSUPPORTED, _lib.PBL_ERR_INVALID_ARG
    assert call(D=96, ldo=384) == UNS
    assert call(S=5) == UNS
    assert call(B=5) == UNS
    assert call(Hq=6, Hkv=4, ldo=384) == UNS
    bad = dict(S=5)                                                         # (as above: never a launchable shape)
    assert call(pos=None, **bad) == INV
    assert call(ldo=255, **bad) == INV
    assert call(ws_bytes=16, **bad) == INV                                  # smaller than pbl_decode_attn_workspace_bytes
    assert call(out=kc, **bad) == INV                                       # the output overlapping the cache
    assert L.pbl_decode_attn_workspace_bytes(1, 1, 4, 64, 64) == 4 * 2 * (2 + 64) * 4   # 64 keys: 2 splits of 32
    assert L.pbl_decode_attn_workspace_bytes(0, 1, 4, 64, 64) == 0


def test_runtime_wrappers_check_their_arguments():
    from pb_llm_amd import runtime as R
    assert R.decode_attention_ok(4, 4, 32, 8, 128, 4096) and not R.decode_attention_ok(1, 5, 8, 8, 64, 64)
    assert not R.decode_attention_ok(1, 1, 6, 4, 64, 64) and not R.decode_attention_ok(1, 1, 8, 8, 96, 64)
    q = torch.zeros(1, 8, 1, 64, dtype=torch.float16)
    with pytest.raises(ValueError):
        R.decode_attention_f16(q, torch.zeros(1, 2, 16, 64, dtype=torch.float16), torch.zeros(1, 2, 16, 64, dtype=torch.float16),
                               torch.zeros((), dtype=torch.int64), 0.125)                       # host tensors
    with pytest.raises(ValueError):
        R.rope_append_f16(torch.zeros(1, 768, dtype=torch.float16), 0, 512, 640, 1, 1, 8, 2, 64, None, None, None, None, None)


# ---------------------------------------------------------------- generate / DecodeSession on the host
def tiny_llama(seed=0, **kw):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=97, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=64, **kw)
    return LlamaForCausalLM(cfg).eval()


@pytest.mark.parametrize("kw,total", [(dict(max_new_tokens=3), 8), (dict(max_length=9), 9), (dict(max_length=30, max_new_tokens=2), 7),
                                      (dict(), 25)])
def test_generation_limits_follow_model_generate(kw, total):
    import warnings
    from pb_llm_amd import harness as H
    model = tiny_llama()
    ids = torch.randint(0, 97, (2, 5), generator=torch.Generator().manual_seed(1))
    got, eos, pad = H._generation_limits(model, 5, **kw)
    assert got == total
    assert eos == [model.generation_config.eos_token_id] and pad == eos[0]          # pad defaults to eos, as in HF
    model.generation_config.eos_token_id = None                                      # (HF then runs to the length limit)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert model.generate(ids, do_sample=False, **kw).shape[1] == total


def test_generation_limits_edge_cases():
    from pb_llm_amd import harness as H
    model = tiny_llama()
    assert H._generation_limits(model, 50)[0] == 64                                  # default 20 new tokens, capped by the positions
    with pytest.raises(ValueError):
        H._generation_limits(model, 5, max_length=5)                                 # model.generate refuses it too
    with pytest.raises(ValueError):
        H._generation_limits(model, 5, max_new_tokens=0)
    assert H._generation_limits(model, 5, max_new_tokens=2, eos_token_id=[7, 9])[1:] == ([7, 9], 7)
    assert H._generation_limits(model, 5, max_new_tokens=2, eos_token_id=7, pad_token_id=0)[1:] == ([7], 0)
    model.generation_config.eos_token_id = None
    assert H._generation_limits(model, 5, max_new_tokens=2)[1:] == ([], None)


def test_generate_hands_host_padded_and_sampling_calls_to_model_generate():
    from pb_llm_amd import harness as H
    model = tiny_llama()
    ids = torch.randint(0, 97, (2, 6), generator=torch.Generator().manual_seed(2))
    ref = model.generate(ids, do_sample=False, max_new_tokens=4)
    assert torch.equal(H.generate(model, ids, max_new_tokens=4), ref)               # a host model: model.generate itself
    calls = []
    orig = model.generate

    def spy(*a, **k):
        calls.append(k)
        return orig(*a, **k)

    model.generate = spy
    mask = torch.ones_like(ids)
    mask[1, 0] = 0
    H.generate(model, ids, max_new_tokens=2, attention_mask=mask)
    H.generate(model, ids, max_new_tokens=2, do_sample=True, top_k=1)
    H.generate(model, ids, max_new_tokens=2, num_beams=2)
    assert [c.get("attention_mask") is mask for c in calls] == [True, False, False]
    assert calls[1]["do_sample"] is True and calls[1]["top_k"] == 1 and calls[2]["num_beams"] == 2


def test_decode_session_on_the_host_equals_a_full_forward():
    """the session's cache, 4D mask and positions (graph=False, HF's StaticLayer path on the host): the logits of a prefill and of
    each step equal those of one forward over the whole sequence, and the host count enforces max_length"""
    from pb_llm_amd import harness as H
    model = tiny_llama(3)
    ids = torch.randint(0, 97, (2, 9), generator=torch.Generator().manual_seed(4))
    full = model(ids, use_cache=False).logits
    sess = H.DecodeSession(model, 2, 9, graph=False)
    assert type(sess.cache).__name__ == "DecodeCache" and sess.cache.layers[0].keys.shape == (2, 2, 9, 16)
    torch.testing.assert_close(sess.prefill(ids[:, :6]), full[:, 5], rtol=1e-4, atol=1e-5)
    for t in range(6, 9):
        torch.testing.assert_close(sess.step(ids[:, t]), full[:, t], rtol=1e-4, atol=1e-5)
    assert sess.pos == 9 and int(sess.cache.layers[1].cumulative_length) == 9
    with pytest.raises(ValueError):
        sess.step(ids[:, 0])
    sess.reset()
    assert sess.pos == 0 and int(sess.cache.layers[0].cumulative_length) == 0 and not sess.cache.layers[0].keys.any()
    torch.testing.assert_close(sess.prefill(ids[:, :3]), full[:, 2], rtol=1e-4, atol=1e-5)
    with pytest.raises(ValueError):
        sess.prefill(ids[:1, :2])                                                    # one row: the session has two
