"""-m gpu: prompt-lookup speculative decoding -- pbl_spec_verify_f16 / pbl_ngram_draft (runtime.spec_verify_f16 / ngram_draft) against
the numpy restatement of spec_ref.py (exact integer equality) and under graph replay; DecodeSession.begin_speculation /
step_speculate / run_speculation and harness.generate(prompt_lookup_num_tokens=) on the packed LLaMA models of
test_gpu_decode_attention.py against the one-token loop and model.generate.

Token criterion at model level: a step of 1 + K rows and a step of one row round differently, so the tolerance is MEASURED -- the
largest teacher-forced logit difference between (1 + K)-row steps and one-row steps of a session over the same sequence -- and the
tokens must agree up to the first step whose top-1 / top-2 margin in the one-row run falls below twice that difference.  The prompt
is chosen by the one-row run alone (the candidate whose smallest margin is largest); at least 16 steps must be compared.  Against
model.generate the bound is the sum of that difference and the session's measured difference to HF's own logits: the one-token loop
itself equals model.generate only up to the latter (test_gpu_decode_attention.py: greedy_agreement)."""
import math

import numpy as np
import pytest
import torch

from pb_llm_amd import harness as H
from pb_llm_amd.runtime import ngram_draft, spec_verify_f16
from spec_ref import SpecState, argmax_ref, draft_ref, verify_ref
from test_gpu_decode_attention import built, epi, hf_run, prompts  # noqa: F401  (built / epi: fixtures)
from test_gpu_decode_epilogues import ids_of
from test_gpu_sampling import Sel, count_ops, teacher_forced
from test_sampling_cpu import rows16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = [(1, 1), (1, 2), (1, 4), (2, 2), (4, 1)]


# ---------------------------------------------------------------- the kernels against the restatement
def logits_view(rows: np.ndarray, layout: str) -> torch.Tensor:
    """rows [B, S, V] as the kernel's input: 'contig' a contiguous tensor, 'sliced' the view base[:, -S:, 3:3 + V] of a wider NaN-filled
    buffer (rows that start off a 16-byte boundary; reading outside a row finds a NaN, which would win the arg-max)"""
    B, S, V = rows.shape
    t = torch.from_numpy(rows).to(DEV)
    if layout == "contig":
        return t
    base = torch.full((B, S + 2, V + 24), float("nan"), dtype=torch.float16, device=DEV)
    base[:, -S:, 3:3 + V] = t
    return base[:, -S:, 3:3 + V]


class Spec:
    """a SpecState on the device: the layers' positions are tensors of their own, as StaticLayer.cumulative_length is"""

    def __init__(self, st: SpecState):
        t = lambda a, dt=torch.long: torch.tensor(np.asarray(a), dtype=dt, device=DEV)
        self.ids, self.tokens, self.unfinished = t(st.ids), t(st.tokens), t(st.unfinished, torch.bool)
        self.state = t([st.cursor, -7])
        self.cursor, self.count = self.state[:1], self.state[1:].view(torch.int32)[:1]
        self.status = t([st.status], torch.int32)
        self.stats = torch.zeros(8, dtype=torch.long, device=DEV)
        self.stats[:3] = t(st.stats)
        self.layers = [torch.tensor(int(p), dtype=torch.long, device=DEV) for p in st.positions]
        self.table = t([p.data_ptr() for p in self.layers])

    def verify(self, logits, eos=(), pad=0, max_ngram=0):
        e = torch.tensor(list(eos), dtype=torch.long, device=DEV) if len(eos) else None
        assert spec_verify_f16(logits, self.ids, self.tokens, self.cursor, self.unfinished, self.count, self.status, self.table,
                               self.stats, eos=e, pad=pad, max_ngram=max_ngram) is True

    def draft(self, max_ngram):
        assert ngram_draft(self.tokens, self.cursor, self.unfinished, self.ids, max_ngram) is True

    def tensors(self):
        return [self.ids, self.tokens, self.state, self.unfinished, self.status, self.stats] + self.layers

    def read(self) -> SpecState:
        return SpecState(self.ids.cpu().numpy(), self.tokens.cpu().numpy(), int(self.cursor), self.unfinished.cpu().numpy(),
                         np.array([int(p) for p in self.layers], np.int64), int(self.count), int(self.status),
                         self.stats[:3].cpu().numpy())

    def argmaxes(self):
        return self.stats[4:4 + self.ids.numel()].cpu().numpy().reshape(self.ids.shape)


def same(got: SpecState, ref: SpecState, what=""):
    for f in ("ids", "tokens", "unfinished", "positions", "stats"):
        assert np.array_equal(getattr(got, f), getattr(ref, f)), f"{what}: {f}\n{getattr(got, f)}\nexpected\n{getattr(ref, f)}"
    assert (got.cursor, got.count, got.status) == (ref.cursor, ref.count, ref.status), \
        f"{what}: cursor / count / status {(got.cursor, got.count, got.status)} expected {(ref.cursor, ref.count, ref.status)}"


def select_greedy(view: torch.Tensor) -> np.ndarray:
    """pbl_select_token_f16's greedy token of every row of the [B, S, V] view, batch entry by batch entry (a 2-D strided view each)"""
    out = []
    for b in range(view.shape[0]):
        sel = Sel(view.shape[1], 1)
        sel(view[b])
        out.append(sel.tokens[:, 0].cpu().numpy())
    return np.stack(out)


def check(st: SpecState, rows: np.ndarray, layout: str, eos=(), pad=0, max_ngram=0, what=""):
    """one verify call on the device against the restatement; the kernel's arg-maxes against the restatement's and select_token_f16's"""
    view = logits_view(rows, layout)
    dev = Spec(st)
    dev.verify(view, eos, pad, max_ngram)
    am = argmax_ref(rows)
    assert np.array_equal(dev.argmaxes(), am), f"{what}: arg-max {dev.argmaxes()} expected {am}"
    assert np.array_equal(select_greedy(view), am), what
    ref = st.copy()
    n = verify_ref(ref, am, eos, pad, max_ngram)
    same(dev.read(), ref, what)
    return n, ref


def state_for(am: np.ndarray, n_b, V: int, total=40, cursor=9, L=3, seed=0) -> SpecState:
    """a state whose drafts force n_b[b] accepted drafts in row b: slot n_b[b] holds a wrong token"""
    B, S = am.shape
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, S), np.int64)
    ids[:, 0] = rng.integers(0, V, B)
    ids[:, 1:] = am[:, :-1]
    for b in range(B):
        if n_b[b] < S - 1:
            ids[b, 1 + n_b[b]] = (am[b, n_b[b]] + 1) % V if V > 1 else -1
    tokens = np.full((B, total), -7, np.int64)
    tokens[:, :cursor] = rng.integers(0, V, (B, cursor))
    tokens[:, cursor - 1] = ids[:, 0]
    return SpecState(ids, tokens, cursor, np.ones(B, bool), np.full(L, cursor - 1 + S, np.int64))


@pytest.mark.parametrize("layout", ["contig", "sliced"])
@pytest.mark.parametrize("V", [7, 4097, 50257, 128256])
@pytest.mark.parametrize("B,S", GRID)
def test_verify_and_draft_equal_the_restatement(B, S, V, layout):
    rows = rows16(V, 3, 11 * V + 5 * B + S, B * S).reshape(B, S, V)
    am = argmax_ref(rows)
    for shift in range(S):                                                   # n_b from 0 to S - 1, different per row
        n_b = [(b + shift) % S for b in range(B)]
        n, ref = check(state_for(am, n_b, V, seed=shift), rows, layout, max_ngram=2, what=f"n_b = {n_b}")
        assert n == min(n_b) and ref.cursor == 9 + n + 1 and (ref.positions == ref.cursor - 1).all()


def test_ties_nan_and_inf_rows():
    V = 50257
    cases = []
    for idx in ([511, 512], [1023, 1024], [8191, 8192, 40000], [V - 1], [4, V - 1], [0], [7], [8], [V - 9, V - 8]):   # lanes, waves, passes
        r = np.full(V, -3.0, np.float16)
        r[idx] = 2.5
        cases.append((r, idx[0]))
    r = rows16(V, 3, 1)[0]
    r[[30000, 41]] = np.nan                                                  # a NaN counts as the maximum, the lowest of them
    r[5] = np.inf
    cases.append((r, 41))
    r = rows16(V, 3, 2)[0]
    r[[100, 4000]] = np.inf
    r[7] = -np.inf
    cases.append((r, 100))
    cases.append((np.full(V, -np.inf, np.float16), 0))                       # nothing finite: index 0
    r = np.full(V, -np.inf, np.float16)
    r[V - 2] = -65504.0
    cases.append((r, V - 2))
    z = np.zeros(V, np.float16)
    z[0], z[3] = -0.0, 0.0                                                   # -0 equals +0
    cases.append((z, 0))
    for layout in ("contig", "sliced"):
        for i in range(0, len(cases), 4):
            chunk = cases[i:i + 4]
            rows = np.stack([c[0] for c in chunk])[None]                     # B = 1, S = len(chunk)
            am = argmax_ref(rows)
            assert am[0].tolist() == [c[1] for c in chunk] == torch.argmax(torch.from_numpy(rows[0]).float(), -1).tolist()
            check(state_for(am, [len(chunk) - 1], V), rows, layout, what=f"cases {i}.. {layout}")


@pytest.mark.parametrize("B,S", [(1, 4), (2, 2), (1, 2)])
def test_eos_at_each_slot_of_the_accepted_run(B, S):
    V = 4097
    rows = rows16(V, 3, 77 + B, B * S).reshape(B, S, V)
    am = argmax_ref(rows)
    for b in range(B):
        for slot in range(S):
            st = state_for(am, [S - 1] * B, V, seed=slot)
            n, ref = check(st, rows, "sliced", eos=(int(am[b, slot]), V + 3), pad=5, max_ngram=2, what=f"eos at row {b} slot {slot}")
            assert n == S - 1 and not ref.unfinished[b] and (ref.tokens[b, 9 + slot + 1:9 + S] == 5).all()
            assert ref.ids[b, 0] == (5 if slot < S - 1 else am[b, slot])
            if B == 1:                                                       # every row has finished: the next call is the no-op
                assert ref.count == 0
                n2, ref2 = check(ref, rows, "sliced", eos=(int(am[b, slot]),), pad=5, max_ngram=2, what="after the last row finished")
                assert n2 == -1 and np.array_equal(ref2.tokens, ref.tokens) and np.array_equal(ref2.ids, ref.ids)
                assert (ref2.positions == ref.positions - S).all() and ref2.cursor == ref.cursor


def test_a_finished_row_beside_a_running_one():
    V = 4097
    rows = rows16(V, 3, 5, 4).reshape(2, 2, V)
    am = argmax_ref(rows)
    st = state_for(am, [1, 0], V)                                            # row 1 would reject its draft, but it has finished
    st.unfinished[1] = False
    n, ref = check(st, rows, "contig", eos=(V + 1,), pad=3, max_ngram=2)
    assert n == 1 and ref.tokens[1, 9:11].tolist() == [3, 3] and ref.ids[1].tolist() == [3, 3] and ref.count == 1
    st = state_for(am, [1, 0], V)                                            # both running: the minimum
    assert check(st, rows, "contig", eos=(V + 1,), pad=3, max_ngram=2)[0] == 0


@pytest.mark.parametrize("L", [1, 32])
def test_the_cursor_near_total_the_no_op_and_every_layer_position(L):
    V, S = 4097, 4
    rows = rows16(V, 3, 9, S).reshape(1, S, V)
    am = argmax_ref(rows)
    for left in range(0, S + 2):                                             # columns left before the call
        st = state_for(am, [S - 1], V, total=9 + left, cursor=9, L=L)
        n, ref = check(st, rows, "sliced", max_ngram=2, what=f"{left} columns left")
        if left == 0:                                                        # finished: nothing written, all S positions taken back
            assert n == -1 and np.array_equal(ref.tokens, st.tokens) and np.array_equal(ref.ids, st.ids) and ref.cursor == 9
            assert (ref.positions == st.positions - S).all() and ref.stats.tolist() == [0, 0, 0] and ref.status == 0
        else:
            assert n == S - 1 and ref.cursor == 9 + min(left, S) and ref.stats.tolist() == [1, min(left, S) - 1, min(left, S)]
    st = state_for(am, [1], V, L=L)
    n, ref = check(st, rows, "contig", what="one draft accepted")
    assert n == 1 and ref.cursor == 11 and (ref.positions == 10).all() and len(ref.positions) == L


def history(n, plant, tail, seed):
    """n tokens without accidental repeats (a running counter above the vocabulary of `tail`), ending with `tail`, with copies of
    the tail's last len(t) tokens planted so that they END at the positions in `plant` ({end: tokens})"""
    h = np.arange(1000, 1000 + n, dtype=np.int64)
    for e, t in plant.items():
        h[e - len(t):e] = t
    h[n - len(tail):] = tail
    return h


DRAFT_CASES = [                                                              # (history length, {end: planted tokens}, tail)
    (1, {}, [5]), (2, {}, [5, 6]), (2, {}, [6, 6]), (3, {2: [3, 4]}, [4]),
    (1025, {}, [1, 2, 3, 4]),                                                # no match
    (1025, {64: [1, 2, 3, 4]}, [1, 2, 3, 4]), (1025, {65: [3, 4]}, [1, 2, 3, 4]), (1025, {1021: [4]}, [1, 2, 3, 4]),
    (1025, {63: [1, 2, 3, 4], 66: [2, 3, 4], 1020: [3, 4]}, [1, 2, 3, 4]),   # the longest first, across lanes 62 .. 65
    (5000, {1024: [1, 2, 3, 4], 1026: [1, 2, 3, 4], 2049: [1, 2, 3, 4]}, [1, 2, 3, 4]),      # several: the latest; pass boundaries
    (5000, {1025: [3, 4], 4096: [4], 4996: [4]}, [1, 2, 3, 4]),
    (5000, {4: [1, 2, 3, 4]}, [1, 2, 3, 4]), (5000, {3: [2, 3, 4]}, [1, 2, 3, 4]),
    (5000, {}, [7, 7, 7, 7, 7]), (5000, {}, [1, 2, 1, 2, 1, 2]),             # loops of period 1 and 2: the copy overlaps itself
    (65536, {1024: [2, 3, 4], 65000: [3, 4], 40000: [1, 2, 3, 4]}, [1, 2, 3, 4]),
]


@pytest.mark.parametrize("B,S", [(1, 4), (1, 2), (2, 2)])
def test_drafts_equal_the_restatement(B, S):
    for i, (n, plant, tail) in enumerate(DRAFT_CASES):
        if len(tail) > n or any(e > n - 1 for e in plant):
            continue
        for max_ngram in (1, 2, 3, 4):
            tokens = np.full((B, n + 3), -7, np.int64)
            for b in range(B):                                               # row 1: the same history moved by one token
                tokens[b, :n] = history(n, plant if b == 0 else {e - 1: t for e, t in plant.items() if e - 1 - len(t) >= 0}, tail, i)
            ids = np.full((B, S), -1, np.int64)
            ids[:, 0] = tokens[:, n - 1]
            st = SpecState(ids, tokens, n, np.ones(B, bool), np.zeros(0, np.int64))
            dev = Spec(st)
            dev.draft(max_ngram)
            ref = st.copy()
            draft_ref(ref, max_ngram)
            assert np.array_equal(dev.ids.cpu().numpy(), ref.ids), f"case {i} max_ngram {max_ngram}: {dev.ids.tolist()} expected {ref.ids.tolist()}"
            assert np.array_equal(dev.tokens.cpu().numpy(), tokens) and int(dev.cursor) == n
    st = SpecState(np.array([[2, -1], [8, -1]]), np.array([[1, 2, 1, 2], [9, 8, 9, 8]]), 4, np.array([False, True]), np.zeros(0, np.int64))
    dev = Spec(st)
    dev.draft(2)
    assert dev.ids.tolist() == [[2, 2], [8, 9]]                              # a finished row drafts its last token, the other one looks up


@pytest.mark.parametrize("B,S", [(1, 4), (2, 2)])
def test_captured_unit_is_bit_stable_and_equal_to_eager(B, S):
    V, total = 32000, 60
    rows = rows16(V, 3, 40 + B, B * S).reshape(B, S, V)
    am = argmax_ref(rows)
    view = logits_view(rows, "sliced")
    st = state_for(am, [S - 1] * B, V, total=total, cursor=9, L=4)
    st.tokens[:, 9:] = 0
    dev = Spec(st)
    eos = torch.tensor([V + 1], dtype=torch.long, device=DEV)
    call = lambda: spec_verify_f16(view, dev.ids, dev.tokens, dev.cursor, dev.unfinished, dev.count, dev.status, dev.table, dev.stats,
                                   eos=eos, pad=0, max_ngram=2)
    start = [t.clone() for t in dev.tensors()]

    def restore():
        for t, v in zip(dev.tensors(), start):
            t.copy_(v)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    first = None
    for _ in range(100):                                                     # the same state: bit-identical outputs
        restore()
        graph.replay()
        state = [t.clone() for t in dev.tensors()]
        first = state if first is None else first
        assert all(torch.equal(a, b) for a, b in zip(state, first))
    restore()
    ref = st.copy()
    for step in range(total):                                                # replayed over a changing state, into the no-op ...
        for p in dev.layers:
            p.add_(S)                                                        # (the forward pass)
        graph.replay()
        ref.positions += S
        verify_ref(ref, am, (V + 1,), 0, 2)
        if step % 7 == 0 or step > total - 4:
            same(dev.read(), ref, f"replay {step}")
    assert int(dev.cursor) == total
    replayed = [t.clone() for t in dev.tensors()]
    restore()
    for _ in range(total):                                                   # ... equals the eager calls
        for p in dev.layers:
            p.add_(S)
        call()
    assert all(torch.equal(a, b) for a, b in zip(dev.tensors(), replayed))


# ---------------------------------------------------------------- model level
def multi_row_logits(model, seq, P, S):
    """teacher-forced fp16 logits of a session that feeds seq in steps of S rows after the prefill of seq[:, :P]: index i holds
    the logits that follow column P - 1 + i (index 0: the prefill), as test_gpu_sampling.teacher_forced returns them"""
    sess = H.DecodeSession(model, seq.shape[0], seq.shape[1] + S, graph=False)
    lg = [sess.prefill(seq[:, :P]).clone()[:, None]]
    for t in range(P, seq.shape[1] - S, S):
        sess._advance(S)
        out = model(seq[:, t:t + S], attention_mask=sess._mask(S), past_key_values=sess.cache, use_cache=True, logits_to_keep=S)
        lg.append(out.logits[:, -S:].clone())
    return torch.cat(lg, 1)


_PLAIN = {}


def plain_run(model, rows, P, n, seed):
    """the one-row run that everything is compared with: of 6 candidate prompts the one whose smallest top-1 / top-2 margin over the
    n steps is largest (chosen by the plain run alone).  Returns (prompt, plain tokens G, its teacher-forced logits, margins [n]);
    computed once per model and batch and shared by the tests"""
    key = (id(model), rows, P, n, seed)
    if key not in _PLAIN:
        _PLAIN[key] = _plain_run(model, rows, P, n, seed)
    return _PLAIN[key]


def _plain_run(model, rows, P, n, seed):
    best = None
    with torch.no_grad():
        for ids in prompts(P, rows, seed):
            G = H.generate(model, ids, max_new_tokens=n)
            lg = teacher_forced(model, G, ids.shape[1])
            top2 = lg.float().topk(2, -1).values
            margin = (top2[..., 0] - top2[..., 1]).amin(0)
            if best is None or float(margin.min()) > float(best[3].min()):
                best = (ids, G, lg, margin)
    return best


def agreed_steps(model, G, lg, margin, P, K):
    """(steps to compare, the measured difference): the largest teacher-forced logit difference between (1 + K)-row and one-row
    steps over G, and the first step whose one-row margin is below twice that"""
    with torch.no_grad():
        multi = multi_row_logits(model, G, P, 1 + K)
    m = multi.shape[1]
    diff = float((multi.float() - lg[:, :m].float()).abs().max())
    close = (margin < 2 * diff).nonzero()
    steps = int(close[0]) if len(close) else margin.shape[0]
    print(f"[speculation] K={K} rows={G.shape[0]}: (1+K)-row against one-row teacher-forced logits abs {diff:.3e} "
          f"(rel {diff / float(lg.float().abs().max()):.2e}); {steps} steps compared, smallest margin {float(margin.min()):.3e}")
    return steps, diff


@pytest.mark.parametrize("rows,K", [(1, 1), (1, 3), (2, 1)])
def test_generate_with_prompt_lookup_equals_greedy_generate(epi, rows, K, monkeypatch):
    n = 32
    begun, begin = [], H.DecodeSession.begin_speculation
    monkeypatch.setattr(H.DecodeSession, "begin_speculation", lambda self, *a, **kw: (begun.append(kw["draft_tokens"]), begin(self, *a, **kw))[1])
    ids, G, lg, margin = plain_run(epi, rows, 6, n, 60 + rows)
    P = ids.shape[1]
    steps, diff = agreed_steps(epi, G, lg, margin, P, K)
    assert steps >= 16, "near-tie within 16 steps of the best of 6 prompts"
    got = H.generate(epi, ids, max_new_tokens=n, prompt_lookup_num_tokens=K if K < 3 else 10)
    assert begun == [K], "generate did not take the speculative path"
    assert got.shape == G.shape and torch.equal(got[:, :P + steps], G[:, :P + steps])
    # against model.generate the session's own difference to HF's attention comes on top (what greedy_agreement in
    # test_gpu_decode_attention.py measures, on HF's sequence): the two differences add, and HF's margins count as well
    hf, scores = hf_run(epi, ids, n)
    diff_hf = float((teacher_forced(epi, hf, P).float() - scores).abs().max())
    top2 = scores.topk(2, -1).values
    close = (torch.minimum(margin, (top2[..., 0] - top2[..., 1]).amin(0)) < 2 * (diff + diff_hf)).nonzero()
    steps_hf = int(close[0]) if len(close) else n
    print(f"[speculation] against model.generate: session against HF abs {diff_hf:.3e}; {steps_hf} steps compared")
    assert steps_hf >= 16 and torch.equal(got[:, :P + steps_hf], hf[:, :P + steps_hf])
    kw = dict(max_new_tokens=n, prompt_lookup_num_tokens=K, max_matching_ngram_size=3)
    a = H.generate(epi, ids, **kw)
    assert torch.equal(a, H.generate(epi, ids, graph=False, **kw))
    eos = int(a[0, P + 9])                                                   # an id the run produces: the result is cut or padded
    b = H.generate(epi, ids, eos_token_id=eos, pad_token_id=1, poll_every=1, **kw)
    assert torch.equal(b, H.generate(epi, ids, eos_token_id=eos, pad_token_id=1, poll_every=8, **kw))
    assert torch.equal(b, H.generate(epi, ids, eos_token_id=eos, pad_token_id=1, poll_every=8, graph=False, **kw))
    assert b.shape[1] <= P + n and bool((b[0, P:] == eos).any())


def forced_session(model, ids, total, K):
    sess = H.DecodeSession(model, ids.shape[0], total - 1 + K, graph=True)
    sess.begin_speculation(ids, total, draft_tokens=K, max_ngram=2)
    return sess


def drafts_from(G, c, K, total):
    """the plain result's tokens at columns [c, c + K) (zeros beyond the end)"""
    d = torch.zeros(G.shape[0], K, dtype=torch.long, device=G.device)
    m = max(0, min(K, total - c))
    d[:, :m] = G[:, c:c + m]
    return d


@pytest.mark.parametrize("rows,K", [(1, 3), (1, 1), (2, 1)])
def test_forced_drafts_acceptance_and_rollback(epi, rows, K):
    ids, G, lg, margin = plain_run(epi, rows, 6, 32, 60 + rows)
    P = ids.shape[1]
    steps, _ = agreed_steps(epi, G, lg, margin, P, K)
    assert steps >= 16
    n, V = steps, lg.shape[-1]
    total = P + n
    with torch.no_grad():
        # every draft right: ceil((n - 1) / (K + 1)) steps, K accepted in each full one
        sess = forced_session(epi, ids, total, K)
        c, taken = P + 1, 0
        while c < total:
            sess.step_speculate(drafts_from(G, c, K, total))
            taken += 1
            w = min(K + 1, total - c)
            st = sess.speculation_stats()
            assert st == dict(steps=taken, accepted=st["accepted"], tokens=1 + taken + st["accepted"]) and st["tokens"] == c + w - P
            assert st["accepted"] == taken * K if w == K + 1 else st["accepted"] == (taken - 1) * K + w - 1
            c += w
        assert taken == math.ceil((n - 1) / (K + 1))
        assert torch.equal(sess.speculation_result(), G[:, :total])
        with pytest.raises(ValueError):                                      # the generation is over: the length guard is truthful
            sess.step_speculate()
        # a draft corrupted at slot j accepts exactly j, and every later token still equals G (the cache position was rolled
        # back, the stale rows of the rejected drafts are never attended)
        for j in range(K):
            for at in (0, 2):                                                # in the first step, and after two clean ones
                sess = forced_session(epi, ids, total, K)
                c, taken = P + 1, 0
                while c < total:
                    d = drafts_from(G, c, K, total)
                    bad = taken == at and c + K < total
                    if bad:
                        d[-1, j] = (d[-1, j] + 1) % V                        # the last row alone: the other row shares its fate
                    before = sess.speculation_stats()
                    sess.step_speculate(d)
                    after = sess.speculation_stats()
                    w = min(K + 1, total - c)
                    assert after["accepted"] - before["accepted"] == (j if bad else w - 1), (j, at, c)
                    c += j + 1 if bad else w
                    taken += 1
                assert torch.equal(sess.speculation_result(), G[:, :total]), (j, at)
                st = sess.speculation_stats()
                assert st["tokens"] == n == 1 + st["steps"] + st["accepted"]
        # n-gram drafts of its own: any acceptance pattern, the same tokens, the same identity
        sess = forced_session(epi, ids, total, K)
        assert sess.run_speculation() == n and torch.equal(sess.speculation_result(), G[:, :total])
        st = sess.speculation_stats()
        assert st["tokens"] == n == 1 + st["steps"] + st["accepted"]


def test_eos_and_padding_equal_hf(epi):
    P, n = 4, 12
    ids = ids_of(2 * P, 77, 2)
    seq, _ = hf_run(epi, ids, n)
    new = seq[:, P:].tolist()
    eos = next(t for t in new[0][2:] if t not in new[1] and t not in new[0][:2])          # row 0 finishes early, row 1 runs on
    ref = epi.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=eos, pad_token_id=0)
    for poll in (1, 8):
        got = H.generate(epi, ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=0, poll_every=poll, prompt_lookup_num_tokens=2)
        assert got.shape == ref.shape == (2, P + n) and torch.equal(got, ref), poll
    eos2 = [eos, new[1][5]]                                                                 # both rows finish: a shorter result
    ref = epi.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=eos2)
    for poll in (1, 3, 8):
        got = H.generate(epi, ids, max_new_tokens=n, eos_token_id=eos2, poll_every=poll, prompt_lookup_num_tokens=2)
        assert got.shape == ref.shape and got.shape[1] < P + n and torch.equal(got, ref), poll
    one = ids[:1]                                                                           # one row, three drafts per step
    ref = epi.generate(one, do_sample=False, max_new_tokens=n, eos_token_id=eos, pad_token_id=0)
    got = H.generate(epi, one, max_new_tokens=n, eos_token_id=eos, pad_token_id=0, prompt_lookup_num_tokens=3)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("with_eos", [False, True])
def test_the_loop_stays_on_the_device(epi, with_eos):
    ids = ids_of(5, 33)
    n, K, poll = 40, 3, 4
    sess = H.DecodeSession(epi, 1, 5 + n - 1 + K, graph=True)
    sess.begin_speculation(ids, 5 + n, draft_tokens=K, max_ngram=2, eos=[1001] if with_eos else (), pad=0)
    sess.step_speculate()                                                    # the capture happens here
    polls, calls, step = sess.spec.polls, [], sess.step_speculate
    sess.step_speculate = lambda: (calls.append(1), step())[1]
    ops = count_ops(lambda: sess.run_speculation(poll))
    polls = sess.spec.polls - polls
    for op in ("aten::argmax", "aten::sort", "aten::isin", "aten::eq", "aten::index_copy_", "aten::mm"):
        assert op not in ops, op
    reads = max(ops.get("aten::_local_scalar_dense", 0) + ops.get("aten::_to_copy", 0),             # the poll's .tolist(), as an op ...
                sum(v for k, v in ops.items() if k.startswith("Memcpy DtoH")))                       # ... and as a copy
    assert 1 <= reads <= polls, (reads, polls)
    steps = sess.speculation_stats()["steps"]
    assert len(calls) == steps - 1 and polls <= steps, "a surplus step: one that emitted nothing"
    out = sess.speculation_result()
    assert out.shape == (1, 5 + n)
    with torch.no_grad():
        assert torch.equal(out, H.generate(epi, ids, max_new_tokens=n, prompt_lookup_num_tokens=K))
    eager = H.DecodeSession(epi, 1, 12, graph=False)                         # the same unit, launch by launch, under the profiler
    eager.begin_speculation(ids, 9, draft_tokens=K)
    names = count_ops(eager.step_speculate)
    assert any("pbl_spec_argmax_kernel" in name for name in names) and any("pbl_spec_finish_kernel" in name for name in names)
    assert not {"aten::argmax", "aten::sort", "aten::isin"} & set(names)
