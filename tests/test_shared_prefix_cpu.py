"""-m "not gpu": scoring.loglikelihood(share_prefix=True) on the host -- the packing plan against a hand-written expectation, the
masked path (a 4-D branch mask handed to HF's attention, the route of every model that is not folded fp16 on the GPU) against the
unshared path on a tiny fp32 LLaMA, the unchanged default, and pbl_branch_attn_f16's declaration and argument checks (the entry
returns before any device work)."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from pb_llm_amd import _lib, decoding, fusion, harness, runtime, scoring

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# max_length = 16.  A: four requests behind [7, 7] (continuations of 3, 1, 9 and 1 tokens); B: two behind [1, 2, 3] (1 and 2); one
# request alone; G: three behind an 8-token context with 5 tokens each -- 8 + 3 * 4 = 20 packed rows do not fit, two of them (16) do;
# T: a 14-token context whose 4-token continuation lm-eval's truncation would touch (18 > 17), and a second request behind it that
# is then alone
A, B, G, T = [7, 7], [1, 2, 3], list(range(20, 28)), list(range(50, 64))
REQUESTS = [
    (A, [10, 11, 12]),                  # 0
    ([9], [1]),                         # 1   alone
    (B, [4]),                           # 2
    (A, [13]),                          # 3
    (G, [30, 31, 32, 33, 34]),          # 4
    (A, list(range(40, 49))),           # 5
    (B, [5, 6]),                        # 6
    (G, [35, 36, 37, 38, 39]),          # 7
    (T, [1, 2, 3, 4]),                  # 8   truncated
    (A, [14]),                          # 9
    (G, [60, 61, 62, 63, 64]),          # 10  what is left of G
    (T, [5, 6]),                        # 11  alone once 8 is gone
]
PAD = 99


def test_plan_matches_the_hand_written_layout():
    plan = scoring.shared_prefix_plan(REQUESTS, 6, 16, pad_token_id=PAD)
    assert plan.unshared == [1, 8, 10, 11]
    assert len(plan.batches) == 2
    b0, b1 = plan.batches
    # batch 0: G's two requests (16 rows, the longest) and A's four (12 rows, padded by 4): 6 requests
    assert b0.tokens == [G + [30, 31, 32, 33] + [35, 36, 37, 38],
                         A + [10, 11] + list(range(40, 48)) + [PAD] * 4]
    assert b0.position_ids == [list(range(8)) + [8, 9, 10, 11] + [8, 9, 10, 11],
                               [0, 1] + [2, 3] + list(range(2, 10)) + [0] * 4]
    assert b0.trunk == [8, 2]
    assert b0.lo == [[0] * 8 + [8] * 4 + [12] * 4,
                     [0, 0] + [2, 2] + [4] * 8 + [12, 13, 14, 15]]
    assert b0.requests == [(4, 0, [7, 8, 9, 10, 11]), (7, 0, [7, 12, 13, 14, 15]),
                           (0, 1, [1, 2, 3]), (3, 1, [1]), (5, 1, [1, 4, 5, 6, 7, 8, 9, 10, 11]), (9, 1, [1])]
    # batch 1: B
    assert b1.tokens == [[1, 2, 3, 5]] and b1.position_ids == [[0, 1, 2, 3]] and b1.trunk == [3] and b1.lo == [[0, 0, 0, 3]]
    assert b1.requests == [(2, 0, [2]), (6, 0, [2, 3])]


@pytest.mark.parametrize("bs", [1, 2, 4, 6, 100])
def test_plan_holds_every_request_once_in_whole_groups(bs):
    plan = scoring.shared_prefix_plan(REQUESTS, bs, 16)
    seen = list(plan.unshared)
    last = None
    for b in plan.batches:
        L = len(b.tokens[0])
        assert all(len(row) == L for rows in (b.tokens, b.position_ids, b.lo) for row in rows) and len(b.trunk) == len(b.tokens)
        assert L <= 16 and (last is None or L <= last), "batches run longest first and fit max_length"
        last = L
        groups = {}
        for i, j, rows in b.requests:
            ctx, cont = REQUESTS[i]
            seen.append(i)
            groups.setdefault(j, []).append(i)
            assert len(rows) == len(cont) and b.trunk[j] == len(ctx) and b.tokens[j][:len(ctx)] == ctx
            assert rows[0] == len(ctx) - 1, "the last trunk row scores the first continuation token"
            assert [b.tokens[j][r] for r in rows[1:]] == cont[:-1], "a branch row holds the token before the one it scores"
            assert [b.position_ids[j][r] for r in rows] == list(range(len(ctx) - 1, len(ctx) - 1 + len(cont)))
            assert all(b.lo[j][r] == rows[1] for r in rows[1:]) and rows[1:] == list(range(rows[1], rows[1] + len(cont) - 1)) \
                if len(cont) > 1 else True
        assert all(len(g) >= 2 for g in groups.values()), "a packed sequence shares its context between two or more requests"
        assert len(groups) == len(b.tokens) and (len(b.requests) <= bs or len(groups) == 1)
        for j, trunk in enumerate(b.trunk):
            used = trunk + sum(len(REQUESTS[i][1]) - 1 for i in groups[j])
            assert b.lo[j][:trunk] == [0] * trunk and b.lo[j][used:] == list(range(used, L)), "trunk rows lo = 0, padding rows lo = s"
    assert sorted(seen) == list(range(len(REQUESTS))), "every request exactly once"
    assert plan.unshared == [1, 8, 10, 11], "the fall-backs do not depend on the batch size"


def test_plan_raises_what_the_unshared_path_raises():
    with pytest.raises(ValueError, match="empty context"):
        scoring.shared_prefix_plan([([], [1, 2])], 1, 16)
    with pytest.raises(ValueError, match="empty continuation"):
        scoring.shared_prefix_plan([([1], [])], 1, 16)
    with pytest.raises(ValueError, match="longer than max_length"):
        scoring.shared_prefix_plan([([1], list(range(17)))], 1, 16)
    with pytest.raises(ValueError, match="at least 1"):
        scoring.shared_prefix_plan(REQUESTS, 0, 16)


def tiny(impl):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      vocab_size=1000, max_position_embeddings=64, attn_implementation=impl)
    return LlamaForCausalLM(cfg).float().eval()


def grouped_requests(seed, vocab=1000):
    """groups of 1, 2 and 4 behind contexts of 37, 5 and 20 tokens (continuations of 1, 2, 5 and 9 tokens), a group of three whose
    packed length exceeds max_length = 64 and one request longer than max_length + 1, shuffled"""
    import numpy as np
    rng = np.random.default_rng(seed)
    reqs = []
    for ctx_len, conts in ((37, (1, 5, 9, 3)), (5, (2, 1)), (20, (7,)), (50, (9, 9, 9)), (60, (9,))):
        ctx = rng.integers(0, vocab, ctx_len).tolist()
        reqs += [(ctx, rng.integers(0, vocab, n).tolist()) for n in conts]
    return [reqs[i] for i in rng.permutation(len(reqs))]


@pytest.mark.parametrize("impl", ["eager", "sdpa"])
def test_masked_path_equals_the_unshared_path(impl):
    model = tiny(impl)
    reqs = grouped_requests(5)
    # a continuation the model itself decodes behind a shared context: its flag is True on both paths
    ctx = reqs[0][0]
    seq = list(ctx)
    with torch.no_grad():
        for _ in range(3):
            seq.append(int(model(torch.tensor([seq])).logits[0, -1].argmax()))
    reqs += [(ctx, seq[len(ctx):]), (ctx, [seq[len(ctx)]])]
    forwards = []
    hook = model.get_decoder().register_forward_hook(lambda *a: forwards.append(1))
    try:
        for bs in (1, 4, 16):
            plain = scoring.loglikelihood(model, reqs, batch_size=bs)
            forwards[:] = []
            shared = scoring.loglikelihood(model, reqs, batch_size=bs, share_prefix=True)
            plan = scoring.shared_prefix_plan(reqs, bs, 64)
            n_unshared = -(-len(plan.unshared) // bs)
            assert len(forwards) == len(plan.batches) + n_unshared, "one forward per packed batch"
            forwards[:] = []
            assert len(shared) == len(reqs)
            worst = max(abs(a[0] - b[0]) for a, b in zip(plain, shared))
            print(f"[shared prefix, {impl}, batch_size {bs}] max |shared - unshared| = {worst:.3e} over {len(reqs)} requests")
            for i, ((ps, pg), (ss, sg)) in enumerate(zip(plain, shared)):
                assert isinstance(ss, float) and isinstance(sg, bool)
                assert abs(ps - ss) <= 1e-4, (impl, bs, i, ps, ss)
                assert pg == sg, (impl, bs, i)
            assert shared[-2][1] is True and shared[-1][1] is True and not all(g for _, g in shared)
    finally:
        hook.remove()


def test_default_is_the_unshared_path():
    model = tiny("sdpa")
    reqs = grouped_requests(6)
    assert scoring.loglikelihood(model, reqs, batch_size=3) == scoring.loglikelihood(model, reqs, batch_size=3, share_prefix=False)
    assert harness.loglikelihood is scoring.loglikelihood and scoring.BRANCH_ATTENTION is True
    called = []
    plan = scoring.shared_prefix_plan
    try:
        scoring.shared_prefix_plan = lambda *a, **k: called.append(1) or plan(*a, **k)
        scoring.loglikelihood(model, reqs[:3], batch_size=3)
        assert not called
        harness.loglikelihood(model, reqs[:3], batch_size=3, share_prefix=True)
        assert called == [1]
    finally:
        scoring.shared_prefix_plan = plan


def test_vocab_limit_and_errors_on_the_shared_path():
    model = tiny("eager")
    reqs = [([1, 2, 3], [4, 5]), ([1, 2, 3], [6]), ([1, 2, 3], [7, 950])]
    got = scoring.loglikelihood(model, reqs[:2], batch_size=2, vocab_limit=900, share_prefix=True)
    want = scoring.loglikelihood(model, reqs[:2], batch_size=2, vocab_limit=900)
    assert all(abs(a[0] - b[0]) <= 1e-4 and a[1] == b[1] for a, b in zip(got, want))
    with pytest.raises(RuntimeError, match="outside"):
        scoring.loglikelihood(model, reqs, batch_size=3, vocab_limit=900, share_prefix=True)
    with pytest.raises(ValueError, match="empty continuation"):
        scoring.loglikelihood(model, [([1], [2]), ([1], [])], share_prefix=True)


# ---------------------------------------------------------------- the entry and its plumbing, without a GPU
def test_entry_is_declared_exported_built_and_documented():
    hdr = open(os.path.join(REPO, "include", "pbl.h")).read()
    assert re.search(r"^int\s+pbl_branch_attn_f16\s*\(", hdr, re.M) and "trunk >= 1" in hdr
    assert "pbl_branch_attn_f16" in _lib.EXPORTS and hasattr(_lib.lib(), "pbl_branch_attn_f16")
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert '"pbl_branch.hip"' in entry and os.path.exists(os.path.join(REPO, "pb_llm_amd", "csrc", "pbl_branch.hip"))
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "share_prefix" in open(os.path.join(REPO, doc)).read(), doc


def test_entry_checks_its_arguments_before_any_device_work():
    L = _lib.lib()
    INV, MIS, UNS = _lib.PBL_ERR_INVALID_ARG, _lib.PBL_ERR_MISALIGNED, _lib.PBL_ERR_UNSUPPORTED
    bufs = [(C.c_uint16 * 40000)() for _ in range(6)]
    q, k, v, kc, vc, out = (C.addressof(b) + (-C.addressof(b)) % 16 for b in bufs)
    pos, trunk, lo = (C.c_int64 * 1)(), (C.c_int32 * 1)(), (C.c_int32 * 8)()
    qs, ks = (C.c_int64 * 3)(2048, 512, 64), (C.c_int64 * 3)(1024, 512, 64)

    def call(**over):
        a = dict(q=q, q_stride=qs, k=k, k_stride=ks, v=v, v_stride=ks, kc=kc, vc=vc, trunk=C.addressof(trunk), lo=C.addressof(lo), B=1,
                 S=8, Hq=4, Hkv=2, D=64, max_len=64, scaling=0.125, pos=C.addressof(pos), out=out, ldo=256)
        a.update(over)
        return L.pbl_branch_attn_f16(a["q"], a["q_stride"], a["k"], a["k_stride"], a["v"], a["v_stride"], a["kc"], a["vc"], a["trunk"],
                                     a["lo"], a["B"], a["S"], a["Hq"], a["Hkv"], a["D"], a["max_len"], a["scaling"], a["pos"], a["out"],
                                     a["ldo"], None)

    for name in ("q", "q_stride", "k", "k_stride", "v", "v_stride", "kc", "vc", "pos", "out", "trunk", "lo"):
        assert call(**{name: None}) == INV, name
    for name in ("B", "S", "Hq", "Hkv", "D", "max_len"):
        assert call(**{name: 0}) == INV, name
    assert call(ldo=255) == INV and call(S=65) == INV
    assert call(out=q + 64) == INV and call(kc=k) == INV and call(vc=kc + 16) == INV and call(pos=out + 8) == INV
    assert call(lo=out + 64) == INV and call(trunk=kc + 128) == INV and call(lo=vc) == INV      # a table inside an output
    assert call(trunk=C.addressof(pos)) == INV and call(lo=C.addressof(pos) + 4) == INV
    assert call(kc=kc + 2) == MIS
    assert call(D=96, ldo=384) == UNS and call(Hq=4, Hkv=3) == UNS
    assert pos[0] == 0


def test_wrapper_scope_and_host_tensors():
    assert runtime.branch_attention_ok(2, 200, 8, 2, 128, 512) and not runtime.branch_attention_ok(1, 8, 4, 2, 96, 64)
    assert not runtime.branch_attention_ok(1, 65, 4, 2, 64, 64)

    def z(*shape, dtype=torch.float16):
        return torch.zeros(*shape, dtype=dtype)

    q, k, v, kc, vc, p = z(1, 4, 8, 64), z(1, 2, 8, 64), z(1, 2, 8, 64), z(1, 2, 64, 64), z(1, 2, 64, 64), z(1, dtype=torch.int64)
    with pytest.raises(ValueError):
        runtime.branch_attention_f16(q, k, v, kc, vc, p, 0.125, z(1, dtype=torch.int32), z(1, 8, dtype=torch.int32))   # on the host


def test_decode_cache_carries_no_branch_table_by_default_and_a_host_layer_with_one_raises():
    """a folded layer over a cache with a branch table takes the HIP branch attention or raises: on the host it raises, and without
    the table the same call runs LlamaDecoderLayer.forward as before"""
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
    x, pid = torch.randn(1, 6, 256), torch.arange(6)[None]
    pe = LlamaRotaryEmbedding(cfg)(x, pid)
    mask = torch.zeros(1, 1, 6, 16).masked_fill(torch.arange(16)[None, :] > torch.arange(6)[:, None], torch.finfo(torch.float32).min)
    cache = decoding._decode_cache_class()(cfg, 1, 16, "cpu", torch.float32)
    assert cache.branch is None and decoding._cache_branch(cache) is None and decoding._cache_branch(None) is None
    with torch.no_grad():
        layer(x, attention_mask=mask, position_ids=pid, past_key_values=cache, use_cache=True, position_embeddings=pe)
        cache.reset()
        cache.branch = (torch.ones(1, dtype=torch.int32), torch.zeros(1, 6, dtype=torch.int32))
        with pytest.raises(RuntimeError, match="branch"):
            layer(x, attention_mask=mask, position_ids=pid, past_key_values=cache, use_cache=True, position_embeddings=pe)
    assert int(cache.layers[0].cumulative_length) == 0
