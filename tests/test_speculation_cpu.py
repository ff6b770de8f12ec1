"""-m "not gpu": prompt-lookup speculative decoding (pbl_spec_verify_f16 / pbl_ngram_draft; runtime.spec_verify_f16 / ngram_draft;
DecodeSession.begin_speculation; harness.generate with prompt_lookup_num_tokens).  The invariants of the numpy restatement the GPU
tests compare against (spec_ref.py), the C entries' declarations and their refusals before any device work, and generate's routing
of the two new arguments: the hand-over and clamp rules, with the session replaced by a recorder."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from pb_llm_amd import _lib
from spec_ref import SpecState, argmax_ref, cut_ref, draft_ref, one_token_loop, speculative_loop, verify_ref
from test_decode_attention_cpu import tiny_llama

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the restatement
def toy_lm(vocab, period, seed):
    """a deterministic "greedy model": the next token is a function of the last two tokens, with a loop of `period` tokens that it
    falls into now and then -- so that n-gram drafts are sometimes right and sometimes wrong"""
    table = np.random.default_rng(seed).integers(0, vocab, (vocab, vocab))

    def next_token(hist):
        a, b = (int(hist[-2]), int(hist[-1])) if len(hist) > 1 else (0, int(hist[-1]))
        if (a + b) % 3 == 0:
            return (b + 1) % period                                             # a cycle 0, 1, .., period - 1
        return int(table[a, b])

    return next_token


@pytest.mark.parametrize("B,K", [(1, 0), (1, 1), (1, 3), (2, 1), (4, 0)])
@pytest.mark.parametrize("max_ngram", [1, 2, 4])
def test_emitting_with_any_drafts_equals_emitting_token_by_token(B, K, max_ngram):
    accepted = 0
    for seed in range(6):
        rng = np.random.default_rng(100 * seed + B)
        lm = toy_lm(11, 2 + seed % 3, seed)
        prompt = rng.integers(0, 11, (B, 5))
        total = 5 + 40 + seed
        for eos in ((), (3,), (3, 7)):
            ref = one_token_loop(lm, prompt, total, eos, pad=9)
            got, stats, ns = speculative_loop(lm, prompt, total, K, max_ngram, eos, pad=9)
            assert np.array_equal(cut_ref(got, 5, eos), cut_ref(ref, 5, eos)), (seed, eos)
            assert all(0 <= n <= K for n in ns) and stats[0] == len(ns)
            assert stats[2] == stats[0] + stats[1]                               # tokens == steps + accepted (+ 1: the first token)
            accepted += int(stats[1])

            def noise(st, rng=rng):                                              # ANY drafts give the same tokens
                st.ids[:, 1:] = rng.integers(0, 11, st.ids[:, 1:].shape)

            got, _, _ = speculative_loop(lm, prompt, total, K, max_ngram, eos, pad=9, drafter=noise)
            assert np.array_equal(cut_ref(got, 5, eos), cut_ref(ref, 5, eos)), (seed, eos, "random drafts")
    assert accepted > 0 or K == 0, "the toy model never confirmed a draft: the test would not exercise acceptance"


@pytest.mark.parametrize("S", [1, 2, 4])
def test_a_perfect_draft_is_accepted_whole_and_a_wrong_slot_cuts_it(S):
    am = np.array([[5, 6, 7, 8][:S]])
    for wrong in range(S):                                                       # wrong == S - 1 + 1 .. : slot j of the drafts is wrong
        ids = np.array([[4, 5, 6, 7][:S]])
        if wrong < S - 1:
            ids[0, 1 + wrong] = 99
        st = SpecState(ids, np.zeros((1, 20), np.int64), 3, np.ones(1, bool), np.full(2, 2 + S, np.int64))
        n = verify_ref(st, am)
        assert n == wrong and st.cursor == 3 + n + 1 and st.tokens[0, 3:3 + n + 1].tolist() == am[0, :n + 1].tolist()
        assert st.ids[0, 0] == am[0, n] and (st.positions == 2 + n + 1).all() and st.stats.tolist() == [1, n, n + 1]
        assert (st.tokens[0, 3 + n + 1:] == 0).all()


def test_rows_share_the_minimum_and_a_finished_row_does_not_hold_it_back():
    am = np.array([[5, 6], [7, 8]])
    st = SpecState(np.array([[4, 5], [6, 0]]), np.zeros((2, 9), np.int64), 2, np.ones(2, bool), np.full(1, 3, np.int64))
    assert verify_ref(st, am, pad=1) == 0                                        # row 1 rejects: one token for both
    assert st.tokens[:, 2].tolist() == [5, 7] and st.cursor == 3 and st.positions[0] == 2
    st = SpecState(np.array([[4, 5], [6, 0]]), np.zeros((2, 9), np.int64), 2, np.array([True, False]), np.full(1, 3, np.int64))
    assert verify_ref(st, am, pad=1) == 1                                        # row 1 had finished: it receives pad
    assert st.tokens[:, 2:4].tolist() == [[5, 6], [1, 1]] and st.ids[:, 0].tolist() == [6, 1] and st.count == 1


def test_eos_inside_the_run_clamping_and_the_finished_no_op():
    am = np.array([[5, 6, 7, 8]])
    for slot in range(4):
        st = SpecState(np.array([[4, 5, 6, 7]]), np.full((1, 12), -7, np.int64), 2, np.ones(1, bool), np.full(1, 5, np.int64))
        assert verify_ref(st, am, eos=(am[0, slot],), pad=0) == 3
        assert st.tokens[0, 2:6].tolist() == [5, 6, 7, 8][:slot + 1] + [0] * (3 - slot) and not st.unfinished[0] and st.count == 0
    st = SpecState(np.array([[4, 5, 6, 7]]), np.full((1, 12), -7, np.int64), 10, np.ones(1, bool), np.full(1, 13, np.int64))
    assert verify_ref(st, am) == 3 and st.cursor == 12 and st.tokens[0, 10:].tolist() == [5, 6] and st.stats.tolist() == [1, 1, 2]
    before = st.copy()
    assert verify_ref(st, am) == -1                                              # the cursor has reached total: a no-op
    assert np.array_equal(st.tokens, before.tokens) and np.array_equal(st.ids, before.ids) and st.cursor == 12
    assert (st.positions == before.positions - 4).all() and st.stats.tolist() == [1, 1, 2] and st.status == 0
    st = SpecState(np.array([[4, 5]]), np.zeros((1, 12), np.int64), 4, np.zeros(1, bool), np.full(3, 9, np.int64))
    assert verify_ref(st, am[:, :2]) == -1 and (st.positions == 7).all() and st.cursor == 4 and st.count == 0


def drafts(hist, K, max_ngram, unfinished=True, last=None):
    h = np.array([hist], np.int64)
    st = SpecState(np.array([[hist[-1] if last is None else last] + [-1] * K]), h, len(hist), np.array([unfinished]), np.zeros(0, np.int64))
    draft_ref(st, max_ngram)
    return st.ids[0, 1:].tolist()


def test_draft_rules():
    assert drafts([1, 2, 3, 9, 1, 2, 3], 3, 3) == [9, 1, 2]                      # the copy starts after the match
    assert drafts([5, 7, 7], 3, 2) == [7, 7, 7]                                  # period 1: the copy overlaps itself (LZ77)
    assert drafts([5, 1, 2, 1, 2], 3, 2) == [1, 2, 1]                            # period 2
    assert drafts([1, 2, 8, 1, 2, 9, 1, 2], 2, 2) == [9, 1]                      # the LATEST occurrence wins, not the first
    assert drafts([1, 2, 8, 5, 2, 9, 1, 2], 2, 2) == [8, 5]                      # the longest N first: (1, 2) at 0, not the later 2 alone
    assert drafts([1, 2, 8, 5, 2, 9, 1, 2], 2, 1) == [9, 1]                      # max_ngram = 1: that later 2
    assert drafts([1, 2, 8, 5, 2, 9, 3, 2], 2, 2) == [9, 3]                      # no 2-gram match: N = 1
    assert drafts([1, 2, 3, 4], 3, 4) == [4, 4, 4]                               # no match: the last token
    assert drafts([4], 2, 2) == [4, 4] and drafts([4, 4], 2, 2) == [4, 4]        # length 1: nothing earlier; length 2: e = 1
    assert drafts([1, 2, 1, 2], 2, 2, unfinished=False) == [2, 2]                # a finished row drafts its last token
    assert drafts([1, 2, 3, 1, 2, 3], 1, 4) == [1]                               # N = 3 is the longest that fits (N <= e < len)


def test_argmax_rule():
    rows = np.array([[1, 3, 3, 2], [0, -0.0, -1, 0], [1, np.inf, np.nan, np.nan], [-np.inf] * 4], np.float16)
    assert argmax_ref(rows).tolist() == [1, 0, 2, 0]
    assert argmax_ref(rows).tolist() == torch.argmax(torch.from_numpy(rows).float(), -1).tolist()


# ---------------------------------------------------------------- the C ABI
def test_entries_are_declared_exported_and_documented():
    hdr = open(os.path.join(REPO, "include", "pbl.h")).read()
    for name in ("pbl_spec_verify_f16", "pbl_ngram_draft"):
        assert re.search(rf"^int\s+{name}\s*\(", hdr, re.M), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
        for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
            assert name in open(os.path.join(REPO, doc)).read(), (name, doc)
    assert f"#define PBL_SPEC_STATS_WORDS {_lib.PBL_SPEC_STATS_WORDS}" in hdr
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert "pbl_spec.hip" in entry


def test_entries_decline_before_any_launch():
    L = _lib.lib()
    V = (1 << 19) + 8                                   # never a launchable shape: a missed check answers UNSUPPORTED, not a launch
    logits = (C.c_uint16 * (4 * V))()
    tokens = (C.c_int64 * 64)()
    small = [(C.c_int64 * 8)() for _ in range(8)]
    ids, cursor, unf, eos, cnt, status, table, stats = (C.addressof(b) for b in small)

    def verify(**over):
        a = dict(logits=C.addressof(logits), ld_b=2 * V, ld_s=V, B=2, S=2, V=V, ids=ids, tokens=C.addressof(tokens), total=8, cursor=cursor,
                 unf=unf, eos=eos, n_eos=1, pad=0, cnt=cnt, status=status, table=table, L=2, stats=stats, ngram=2)
        a.update(over)
        return L.pbl_spec_verify_f16(a["logits"], a["ld_b"], a["ld_s"], a["B"], a["S"], a["V"], a["ids"], a["tokens"], a["total"],
                                     a["cursor"], a["unf"], a["eos"], a["n_eos"], a["pad"], a["cnt"], a["status"], a["table"], a["L"],
                                     a["stats"], a["ngram"], None)

    UNS, INV = _lib.PBL_ERR_UNSUPPORTED, _lib.PBL_ERR_INVALID_ARG
    assert verify() == UNS
    assert verify(eos=None, n_eos=0, table=None, L=0, ngram=0) == UNS            # no eos, no layers, no drafting: all may be absent
    assert verify(B=1, S=5, V=100) == UNS and verify(B=3, S=2, V=100, ld_b=200, ld_s=100) == UNS          # more than 4 rows
    for name in ("logits", "ids", "tokens", "cursor", "unf", "cnt", "status", "stats"):
        assert verify(**{name: None}) == INV, name
    assert verify(eos=None) == INV and verify(table=None) == INV                 # n_eos = 1 without ids, L = 2 without a table
    for bad in (dict(B=0), dict(S=0), dict(V=0), dict(total=0), dict(n_eos=-1), dict(L=-1), dict(ngram=5), dict(ngram=-1),
                dict(ld_s=V - 1), dict(ld_b=2 * V - 1)):
        assert verify(**bad) == INV, bad
    assert verify(tokens=C.addressof(logits)) == INV                             # an output over an input
    assert verify(ids=eos) == INV and verify(stats=table) == INV
    assert verify(ids=C.addressof(tokens)) == INV and verify(cnt=status) == INV  # two outputs over each other

    def draft(**over):
        a = dict(tokens=C.addressof(tokens), total=8, B=2, cursor=cursor, unf=unf, ids=ids, S=3, ngram=2)   # 6 elements in ids
        a.update(over)
        return L.pbl_ngram_draft(a["tokens"], a["total"], a["B"], a["cursor"], a["unf"], a["ids"], a["S"], a["ngram"], None)

    assert draft() == UNS and draft(B=1, S=5) == UNS
    for name in ("tokens", "cursor", "unf", "ids"):
        assert draft(**{name: None}) == INV, name
    for bad in (dict(B=0), dict(S=0), dict(total=0), dict(ngram=0), dict(ngram=5), dict(ids=C.addressof(tokens)), dict(ids=cursor)):
        assert draft(**bad) == INV, bad
    assert draft(S=1) == _lib.PBL_OK                                             # no draft slots: nothing to launch


def test_runtime_wrappers_check_their_arguments():
    from pb_llm_amd import runtime as R
    assert R.spec_verify_ok(1, 4, 128256) and R.spec_verify_ok(2, 2, 7) and R.spec_verify_ok(4, 1, 1 << 19)
    assert not R.spec_verify_ok(1, 5, 100) and not R.spec_verify_ok(3, 2, 100) and not R.spec_verify_ok(1, 1, (1 << 19) + 1)
    assert not R.spec_verify_ok(0, 1, 100) and not R.spec_verify_ok(1, 0, 100)
    z = lambda *s, dt=torch.int64: torch.zeros(*s, dtype=dt)
    with pytest.raises(ValueError):                                              # host tensors
        R.spec_verify_f16(torch.zeros(1, 2, 100, dtype=torch.float16), z(1, 2), z(1, 8), z(1), z(1, dt=torch.bool), z(1, dt=torch.int32),
                          z(1, dt=torch.int32), z(2), z(8))
    with pytest.raises(ValueError):
        R.ngram_draft(z(1, 8), z(1), z(1, dt=torch.bool), z(1, 2))


# ---------------------------------------------------------------- generate: routing of the two new arguments
class FakeIds:
    """what generate reads of input_ids before it builds a session, claiming to be on the GPU"""
    is_cuda, dtype, device = True, torch.long, "cpu"

    def __init__(self, B, P):
        self.shape = (B, P)

    def dim(self):
        return 2


class Recorder:
    """stands where DecodeSession stands: records what generate asks for"""
    made = []

    def __init__(self, model, batch, max_length, graph=True):
        self.batch, self.max_length, self.calls = batch, max_length, []
        self.sel = type("Sel", (), {"done": 0})()
        self.logits_dtype = model.get_input_embeddings().weight.dtype
        Recorder.made.append(self)

    def prefill(self, ids):
        return torch.zeros(self.batch, 97, dtype=self.logits_dtype)

    def begin_speculation(self, prompt, total, **kw):
        self.calls.append(("begin_speculation", total, {k: v for k, v in kw.items() if k != "logits"}))

    def run_speculation(self, poll_every):
        self.calls.append(("run_speculation", poll_every))

    def speculation_result(self):
        return "speculated"

    def begin_selection(self, prompt, total, **kw):
        self.calls.append(("begin_selection", total))

    def select(self, logits):
        pass

    def run_selection(self, n, poll_every):
        self.calls.append(("run_selection", n, poll_every))

    def selection_result(self):
        return "selected"


@pytest.fixture
def recorded(monkeypatch):
    from pb_llm_amd import decoding
    Recorder.made = []
    monkeypatch.setattr(decoding, "DecodeSession", Recorder)
    model = tiny_llama().half()                                                  # max_position_embeddings = 64
    model.generate = lambda *a, **k: ("handed over", k)
    return decoding, model


def test_generate_clamps_the_drafts_to_the_four_rows_of_a_launch(recorded):
    decoding, model = recorded
    for B, lookup, K in ((1, 10, 3), (1, 2, 2), (1, 1, 1), (2, 10, 1), (2, 1, 1)):
        out = decoding.generate(model, FakeIds(B, 5), max_new_tokens=20, prompt_lookup_num_tokens=lookup, eos_token_id=3, poll_every=5)
        s = Recorder.made[-1]
        assert out == "speculated" and (s.batch, s.max_length) == (B, 24 + K)    # K positions of slack beyond total - 1
        assert s.calls == [("begin_speculation", 25, dict(draft_tokens=K, max_ngram=2, eos=[3], pad=3)), ("run_speculation", 5)]
    for ngram, N in ((1, 1), (3, 3), (4, 4), (9, 4)):
        decoding.generate(model, FakeIds(1, 5), max_new_tokens=20, prompt_lookup_num_tokens=3, max_matching_ngram_size=ngram)
        assert Recorder.made[-1].calls[0][2]["max_ngram"] == N
    for bad in (dict(prompt_lookup_num_tokens=0), dict(prompt_lookup_num_tokens=2, max_matching_ngram_size=-1)):
        with pytest.raises(ValueError):
            decoding.generate(model, FakeIds(1, 5), max_new_tokens=20, **bad)


def test_generate_keeps_the_one_token_loop_where_speculation_does_not_apply(recorded):
    decoding, model = recorded

    def plain(model, B=1, **kw):
        out = decoding.generate(model, FakeIds(B, 5), **kw)
        s = Recorder.made[-1]
        return out, s.max_length, [c[0] for c in s.calls]

    assert plain(model, max_new_tokens=20) == ("selected", 24, ["begin_selection", "run_selection"])       # today's call
    assert plain(model, max_new_tokens=20, max_matching_ngram_size=3)[1:] == (24, ["begin_selection", "run_selection"])
    assert plain(model, B=3, max_new_tokens=20, prompt_lookup_num_tokens=4)[1:] == (24, ["begin_selection", "run_selection"])   # K = 0
    assert plain(model, B=4, max_new_tokens=20, prompt_lookup_num_tokens=4)[1:] == (24, ["begin_selection", "run_selection"])
    # total - 1 + K = 58 + 3 + 3 = 64 fits max_position_embeddings = 64; one token more does not
    assert plain(model, max_new_tokens=57, prompt_lookup_num_tokens=3)[1:] == (64, ["begin_speculation", "run_speculation"])
    assert plain(model, max_new_tokens=58, prompt_lookup_num_tokens=3)[1:] == (62, ["begin_selection", "run_selection"])
    single = tiny_llama()                                                        # fp32 logits: the selection stays in torch, as today
    single.generate = model.generate
    n = len(Recorder.made)
    with pytest.raises(AttributeError, match="step"):                            # ... i.e. the loop over DecodeSession.step
        decoding.generate(single, FakeIds(1, 5), max_new_tokens=20, prompt_lookup_num_tokens=3)
    assert len(Recorder.made) == n + 1 and Recorder.made[-1].max_length == 24 and Recorder.made[-1].calls == []


def test_generate_hands_sampling_and_host_models_over_with_the_new_arguments(recorded):
    decoding, model = recorded
    kw = dict(max_new_tokens=4, prompt_lookup_num_tokens=3, max_matching_ngram_size=2)
    out, got = decoding.generate(model, FakeIds(1, 5), do_sample=True, **kw)
    assert out == "handed over" and got == dict(do_sample=True, **kw) and not Recorder.made
    ids = torch.zeros(1, 5, dtype=torch.long)                                    # a host tensor: model.generate's assisted loop
    out, got = decoding.generate(model, ids, **kw)
    assert out == "handed over" and got == kw and not Recorder.made
    out, got = decoding.generate(model, FakeIds(1, 5), num_beams=2, **kw)
    assert out == "handed over" and got == dict(num_beams=2, **kw) and not Recorder.made


# ---------------------------------------------------------------- the session's loop on a host model, the kernels restated
@pytest.fixture
def restated(monkeypatch):
    """runtime's three device entries replaced by the restatement over host tensors: what remains under test is decoding.py -- the
    unit, the pointer table, the polls, the length guard, the cut of the result -- and HF's StaticLayer path under the rollback"""
    from pb_llm_amd import decoding
    layers = {}

    def verify(logits, ids, tokens, cursor, unfinished, count, status, positions, stats, eos=None, pad=0, max_ngram=0):
        pos = [layers[p] for p in positions.tolist()]
        st = SpecState(ids.numpy(), tokens.numpy(), int(cursor), unfinished.numpy(), np.array([int(p) for p in pos], np.int64))
        verify_ref(st, argmax_ref(logits.detach().float().numpy()), () if eos is None else eos.tolist(), pad, max_ngram)
        cursor.fill_(st.cursor)
        count.fill_(st.count)
        stats[:3] += torch.from_numpy(st.stats)
        for p, v in zip(pos, st.positions):
            p.fill_(int(v))
        return True

    def draft(tokens, cursor, unfinished, ids, max_ngram=2):
        draft_ref(SpecState(ids.numpy(), tokens.numpy(), int(cursor), unfinished.numpy(), np.zeros(0, np.int64)), max_ngram)
        return True

    def select(logits, step, unfinished, tokens, col0, next_ids, count, status, eos=None, pad=0, **kw):
        tok = torch.from_numpy(argmax_ref(logits.detach().float().numpy()))
        tok = torch.where(unfinished, tok, torch.full_like(tok, pad))
        if eos is not None:
            unfinished &= ~torch.isin(tok, eos)
        tokens[:, col0 + int(step)] = tok
        next_ids.copy_(tok.view_as(next_ids))
        count.fill_(int(unfinished.sum()))
        return True

    monkeypatch.setattr(decoding.runtime, "spec_verify_f16", verify)
    monkeypatch.setattr(decoding.runtime, "ngram_draft", draft)
    monkeypatch.setattr(decoding.runtime, "select_token_f16", select)

    def session(model, ids, total, K, **kw):
        sess = decoding.DecodeSession(model, ids.shape[0], total - 1 + K, graph=False)
        for lay in sess.cache.layers:
            layers[lay.cumulative_length.data_ptr()] = lay.cumulative_length
        sess.begin_speculation(ids, total, draft_tokens=K, logits=sess.prefill(ids).half(), **kw)
        return sess

    return session


@pytest.mark.parametrize("B,K", [(1, 3), (1, 1), (2, 1), (1, 0)])
def test_session_loop_on_a_host_model_equals_model_generate(restated, B, K):
    model = tiny_llama(seed=3)
    model.generation_config.eos_token_id = None
    P, n = 5, 24
    ids = torch.randint(0, 97, (B, P), generator=torch.Generator().manual_seed(10 + B))
    with torch.no_grad():
        G = model.generate(ids, do_sample=False, max_new_tokens=n)
    assert G.shape == (B, P + n)
    for poll in (1, 8):
        sess = restated(model, ids, P + n, K)
        assert sess.run_speculation(poll) == n and torch.equal(sess.speculation_result(), G), poll
        st = sess.speculation_stats()
        assert st["tokens"] == n == 1 + st["steps"] + st["accepted"] and sess.pos == P + n - 1
        with pytest.raises(ValueError, match="max_length"):                      # the generation is over
            sess.step_speculate()
    if K:                                                                        # forced drafts: right ones, and wrong at slot j
        for j in range(K):
            sess = restated(model, ids, P + n, K)
            c, steps = P + 1, 0
            while c + K < P + n:
                d = G[:, c:c + K].clone()
                bad = steps % 2 == 1
                if bad:
                    d[-1, j] = (d[-1, j] + 1) % 97
                before = sess.speculation_stats()["accepted"]
                sess.step_speculate(d)
                assert sess.speculation_stats()["accepted"] - before == (j if bad else K), (j, c)
                c += j + 1 if bad else K + 1
                steps += 1
            sess.run_speculation()
            assert torch.equal(sess.speculation_result(), G), j
    eos = int(G[0, P + 6])                                                       # eos / pad: the result is cut or padded as HF's
    with torch.no_grad():
        ref = model.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=eos, pad_token_id=1)
    for poll in (1, 8):
        sess = restated(model, ids, P + n, K, eos=[eos], pad=1)
        sess.run_speculation(poll)
        assert torch.equal(sess.speculation_result(), ref), poll
