"""-m gpu: token selection on the device -- pbl_select_token_f16 (runtime.select_token_f16) against the float64 restatement of
test_sampling_cpu.py (kept set, token, greedy mode, bookkeeping, graph replay), and harness.generate with do_sample=True on the
packed LLaMA models of test_gpu_decode_attention.py.

Token criterion: the kernel's token t is in the restatement's kept set and prefix[t - 1] - delta W <= u W <= prefix[t] + delta W,
delta = 64 * 2^-24 (derived in test_sampling_cpu.py, not measured).  A distinct value whose float64 M(v) lies within delta of
1 - top_p may go either way, so the kept-set tests first assert, from the restatement alone, that their rows have slack > delta."""
import math

import numpy as np
import pytest
import torch

from pb_llm_amd import harness as H
from pb_llm_amd.runtime import select_token_f16
from test_gpu_decode_attention import built, epi, hf_run, prompts  # noqa: F401  (built / epi: fixtures)
from test_gpu_decode_epilogues import ids_of
from test_sampling_cpu import DELTA, PARAMS, U_LAST, rows16, select_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def strided(rows: np.ndarray, layout: str) -> torch.Tensor:
    """the rows as a [B, V] view with a row stride: 'vec' 16-byte aligned rows (the vector loads), 'odd' rows that start 6 bytes
    off (the scalar loads), 'last' the view out.logits[:, -1] of a [B, 2, V] tensor"""
    B, V = rows.shape
    t = torch.from_numpy(rows).to(DEV)
    if layout == "last":
        base = torch.full((B, 2, V), float("nan"), dtype=torch.float16, device=DEV)
        base[:, -1] = t
        return base[:, -1]
    base = torch.full((B, V + 24), float("nan"), dtype=torch.float16, device=DEV)
    off = 0 if layout == "vec" else 3
    base[:, off:off + V] = t
    return base[:, off:off + V]


class Sel:
    """the device state of a selection and one call per step"""

    def __init__(self, B, total, col0=0, eos=None, unfinished=None, step=0):
        self.B, self.col0 = B, col0
        self.tokens = torch.full((B, total), -7, dtype=torch.long, device=DEV)
        self.step = torch.tensor([step], dtype=torch.long, device=DEV)
        self.unfinished = torch.ones(B, dtype=torch.bool, device=DEV) if unfinished is None else torch.tensor(unfinished, device=DEV)
        self.next_ids = torch.full((B, 1), -7, dtype=torch.long, device=DEV)
        self.count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.eos = None if eos is None else torch.tensor(eos, dtype=torch.long, device=DEV)

    def __call__(self, logits, T=1.0, k=0, p=1.0, u=None, pad=0, kept=None):
        assert select_token_f16(logits, self.step, self.unfinished, self.tokens, self.col0, self.next_ids, self.count, self.status,
                                temperature=T, top_k=k, top_p=p, uniforms=u, eos=self.eos, pad=pad, kept=kept) is True


def u_table(n, B, seed):
    u = np.random.default_rng(seed).random((n, B)).astype(np.float32)
    u[0], u[1] = 0.0, U_LAST
    return np.minimum(u, np.float32(U_LAST))


def check_tokens(ref, toks, us, what):
    """every token of `toks` (one per uniform in `us`) against the restatement `ref` of its row"""
    prefix, W = ref["prefix"], ref["W"]
    for t, u in zip(toks.tolist(), us.tolist()):
        assert 0 <= t < len(prefix) and ref["kept"][t], f"{what}: token {t} (u = {u}) is not in the kept set"
        lo = prefix[t - 1] if t else 0.0
        assert lo - DELTA * W <= u * W <= prefix[t] + DELTA * W, \
            f"{what}: u W = {u * W!r} outside [{lo!r}, {prefix[t]!r}] of token {t} by more than delta W = {DELTA * W:.3e}"


@pytest.mark.parametrize("T,k,p", PARAMS)
@pytest.mark.parametrize("V,B,layout", [(1000, 1, "odd"), (1000, 4, "vec"), (32000, 1, "last"), (32000, 2, "vec"), (32000, 4, "odd"),
                                        (128256, 1, "vec"), (128256, 2, "last"), (128256, 4, "vec")])
@pytest.mark.parametrize("sigma", [1, 3])
def test_kept_set_and_tokens_equal_the_restatement(sigma, V, B, layout, T, k, p):
    for seed in range(7 * V + 31 * B + sigma, 7 * V + 31 * B + sigma + 4000, 100):    # chosen by the restatement alone: the first
        rows = rows16(V, sigma, seed, B)                                                # seed whose rows keep clear of 1 - top_p
        refs = [select_ref(r, T, k, p) for r in rows]
        if min(r["slack"] for r in refs) > DELTA:
            break
    assert min(r["slack"] for r in refs) > DELTA, "no seed found: a value's mass lies within delta of 1 - top_p"
    logits = strided(rows, layout)
    n = 64
    us = u_table(n, B, V + B)
    sel = Sel(B, n)
    kept = torch.zeros(B, V, dtype=torch.uint8, device=DEV)
    ut = torch.from_numpy(us).to(DEV)
    for _ in range(n):
        sel(logits, T, k, p, ut, kept=kept)
    assert int(sel.step) == n and int(sel.status) == 0 and int(sel.count) == B
    got = kept.cpu().numpy().astype(bool)
    toks = sel.tokens.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], refs[b]["kept"]), \
            f"row {b}: kept sets differ at {np.flatnonzero(got[b] != refs[b]['kept'])[:8]} ({got[b].sum()} vs {refs[b]['kept'].sum()} kept)"
        check_tokens(refs[b], toks[b], us[:, b], f"row {b}")
    assert torch.equal(sel.next_ids[:, 0], sel.tokens[:, -1])


def test_limits_ties_and_the_whole_table_of_uniforms():
    V = 5000
    row = rows16(V, 2, 99)
    best = int(np.argmax(row[0]))
    logits = strided(row, "vec")
    us = u_table(64, 1, 3)
    ut = torch.from_numpy(us).to(DEV)
    for T, k, p in ((1.0, 1, 1.0), (0.8, 0, 1e-6)):                          # top_k = 1, top_p -> 0+: the argmax for every u
        sel = Sel(1, 64)
        for _ in range(64):
            sel(logits, T, k, p, ut)
        assert bool((sel.tokens == best).all())
    flat = torch.zeros(1, 128256, dtype=torch.float16, device=DEV)          # one value 128256 times: every token kept, w = 1 each
    sel = Sel(1, 64)
    kept = torch.zeros(1, 128256, dtype=torch.uint8, device=DEV)
    for _ in range(64):
        sel(flat, 0.7, 50, 0.9, ut, kept=kept)
    assert bool(kept.all())
    check_tokens(select_ref(np.zeros(128256, np.float16), 0.7, 50, 0.9), sel.tokens[0].cpu().numpy(), us[:, 0], "flat row")
    ties = np.full((1, 4096), -3.0, np.float16)
    ties[0, [5, 77, 4000]] = 2.5                                             # top_k = 2 keeps all three; -inf never wins
    ties[0, 9] = -np.inf
    sel = Sel(1, 64)
    kept = torch.zeros(1, 4096, dtype=torch.uint8, device=DEV)
    for _ in range(64):
        sel(strided(ties, "odd"), 1.0, 2, 1.0, ut, kept=kept)
    assert kept[0].nonzero().flatten().tolist() == [5, 77, 4000]
    assert set(sel.tokens[0].tolist()) == {5, 77, 4000}
    check_tokens(select_ref(ties[0], 1.0, 2, 1.0), sel.tokens[0].cpu().numpy(), us[:, 0], "ties")


@pytest.mark.parametrize("V,B", [(1000, 3), (32000, 1), (128256, 4), (262144, 1)])
def test_greedy_mode(V, B):
    rows = rows16(V, 3, V + B, B)
    for r in rows:
        assert int((r == r.max()).sum()) == 1
    for layout in ("vec", "odd"):
        logits = strided(rows, layout)
        sel = Sel(B, 3, col0=1)
        kept = torch.zeros(B, V, dtype=torch.uint8, device=DEV)
        sel(logits, kept=kept)
        ref = torch.argmax(logits.float(), -1)
        assert torch.equal(sel.tokens[:, 1], ref) and torch.equal(sel.next_ids[:, 0], ref)
        assert bool((sel.tokens[:, [0, 2]] == -7).all()) and int(sel.step) == 1 and int(sel.count) == B and int(sel.status) == 0
        assert torch.equal(kept.sum(1).cpu(), torch.ones(B, dtype=torch.long)) and bool(kept[torch.arange(B), ref].all())
    tie = rows.copy()
    for b in range(B):
        tie[b, [V - 1, 17 + b, V // 2]] = tie[b].max() + 1                   # constructed ties: the lowest index
        tie[b, 3] = -np.inf
    sel = Sel(B, 1)
    sel(strided(tie, "vec"))
    assert sel.tokens[:, 0].tolist() == [17 + b for b in range(B)]
    zero = np.zeros((1, V), np.float16)
    zero[0, 5] = -0.0                                                        # -0 equals +0: index 0, as torch.argmax
    zero[0, 0] = 0.0
    sel = Sel(1, 1)
    sel(strided(zero, "vec"))
    assert sel.tokens[0, 0].item() == int(torch.argmax(torch.from_numpy(zero).float())) == 0
    nan = rows.copy()
    nan[:, 40] = np.nan                                                      # a NaN counts as the maximum; no status in greedy mode
    nan[:, 30] = np.inf
    sel = Sel(B, 1)
    sel(strided(nan, "odd"))
    assert sel.tokens[:, 0].tolist() == [40] * B == torch.argmax(torch.from_numpy(nan).float(), -1).tolist() and int(sel.status) == 0


def test_nan_and_inf_rows_set_the_status_word_when_sampling():
    rows = rows16(2000, 2, 4, 3)
    rows[1, 100] = np.inf
    rows[2, 7] = np.nan
    u = torch.full((1, 3), 0.5, device=DEV)
    sel = Sel(3, 1)
    sel(strided(rows, "vec"), 0.7, 50, 0.9, u)
    assert int(sel.status) == 1
    assert sel.tokens[1:, 0].tolist() == [100, 7]                            # the fallback: rule 5
    check_tokens(select_ref(rows[0], 0.7, 50, 0.9), sel.tokens[0].cpu().numpy(), np.array([0.5]), "clean row")
    sel = Sel(1, 1)
    sel(strided(rows[:1], "vec"), 0.7, 50, 0.9, u[:, :1].contiguous())
    assert int(sel.status) == 0
    sel = Sel(1, 2, step=2)                                                  # a step beyond the result: nothing written, bit 1
    sel(strided(rows[:1], "vec"))
    assert int(sel.status) == 2 and bool((sel.tokens == -7).all()) and int(sel.step) == 3


def test_bookkeeping():
    B, V = 3, 3000
    rows = rows16(V, 2, 11, B)
    top = np.argmax(rows, 1).tolist()
    logits = strided(rows, "vec")
    sel = Sel(B, 8, col0=2, eos=[top[1], V + 5], unfinished=[True, True, False], step=3)
    sel(logits, pad=9)
    assert sel.tokens[:, 5].tolist() == [top[0], top[1], 9] == sel.next_ids[:, 0].tolist()     # row 2 had finished: pad
    assert sel.unfinished.tolist() == [True, False, False] and int(sel.count) == 1 and int(sel.step) == 4   # row 1 drew an eos id
    untouched = sel.tokens.clone()
    untouched[:, 5] = -7
    assert bool((untouched == -7).all())
    sel(logits, pad=9)                                                       # the next step: column 6, row 1 padded now
    assert sel.tokens[:, 6].tolist() == [top[0], 9, 9] and int(sel.count) == 1 and int(sel.step) == 5
    one = Sel(1, 4, eos=[top[0]])                                            # one row: the count and the step in the same launch
    one(logits[:1], pad=2)
    assert one.tokens[0].tolist() == [top[0], -7, -7, -7] and int(one.count) == 0 and int(one.step) == 1 and not bool(one.unfinished[0])
    one(logits[:1], pad=2)
    assert one.tokens[0].tolist() == [top[0], 2, -7, -7] and one.next_ids.item() == 2
    # step t uses row t of u: two rows of u over the same logits give the two restatement tokens
    u = torch.tensor([[0.05] * B, [0.93] * B], device=DEV)
    sel = Sel(B, 2)
    sel(logits, 1.0, 0, 1.0, u)
    sel(logits, 1.0, 0, 1.0, u)
    for b in range(B):
        ref = select_ref(rows[b], 1.0, 0, 1.0)
        check_tokens(ref, sel.tokens[b].cpu().numpy(), np.array([0.05, 0.93], np.float32), f"row {b}")
        assert sel.tokens[b, 0] != sel.tokens[b, 1]


@pytest.mark.parametrize("B", [1, 2])
def test_captured_selection_is_bit_stable_and_step_independent(B):
    V, n = 32000, 24
    rows = rows16(V, 3, 70 + B, B)
    logits = strided(rows, "last")
    u = torch.from_numpy(u_table(n, B, 8)).to(DEV)
    sel = Sel(B, n, eos=[V + 1])
    kept = torch.zeros(B, V, dtype=torch.uint8, device=DEV)
    call = lambda: sel(logits, 0.7, 50, 0.9, u, kept=kept)
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
    for _ in range(100):                                                     # the same inputs: bit-identical outputs
        sel.step.fill_(5)
        sel.tokens.fill_(-7)
        graph.replay()
        state = (sel.tokens.clone(), sel.next_ids.clone(), kept.clone(), sel.count.clone(), sel.step.clone())
        first = state if first is None else first
        assert all(torch.equal(a, b) for a, b in zip(state, first))
    assert int(sel.step) == 6 and int(sel.status) == 0
    sel.step.fill_(0)
    for _ in range(n):                                                       # replayed over a changing step ...
        graph.replay()
    replayed = sel.tokens.clone()
    assert int(sel.step) == n
    sel.step.fill_(0)
    sel.tokens.fill_(-7)
    for _ in range(n):                                                       # ... equals the eager calls
        call()
    assert torch.equal(replayed, sel.tokens)
    for b in range(B):
        check_tokens(select_ref(rows[b], 0.7, 50, 0.9), replayed[b].cpu().numpy(), u[:, b].cpu().numpy(), f"row {b}")


# ---------------------------------------------------------------- model level
def teacher_forced(model, seq, P):
    """the session's own fp16 logits at every generated position of seq: [B, n, V]"""
    sess = H.DecodeSession(model, seq.shape[0], seq.shape[1], graph=True)
    lg = [sess.prefill(seq[:, :P]).clone()]
    for t in range(P, seq.shape[1] - 1):
        lg.append(sess.step(seq[:, t]).clone())
    return torch.stack(lg, 1)


def test_top_k_1_sampling_equals_greedy_up_to_an_exact_tie(epi):
    n = 32
    for ids in prompts(4, 2, 300):
        P = ids.shape[1]
        greedy = H.generate(epi, ids, max_new_tokens=n)
        top2 = teacher_forced(epi, greedy, P).float().topk(2, -1).values
        tie = (top2[..., 0] == top2[..., 1]).any(0).nonzero()               # top-k keeps every tie of the k-th value
        steps = int(tie[0]) if len(tie) else n
        if steps >= 16:
            break
    assert steps >= 16, "an exact top-1 / top-2 tie within 16 steps of every candidate prompt"
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        got = H.generate(epi, ids, max_new_tokens=n, do_sample=True, top_k=1)
        assert got.shape == greedy.shape and torch.equal(got[:, :P + steps], greedy[:, :P + steps]), seed


def test_sampled_tokens_satisfy_the_criterion_on_the_sessions_own_logits(epi):
    n, B = 24, 2
    ids = ids_of(2 * 5, 410, B)
    P = ids.shape[1]
    U = torch.from_numpy(u_table(n, B, 12)).to(DEV)
    T, k, p = 0.7, 50, 0.9
    seq = H.generate(epi, ids, max_new_tokens=n, do_sample=True, temperature=T, top_k=k, top_p=p, uniforms=U)
    assert seq.shape == (B, P + n) and torch.equal(seq[:, :P], ids)
    lg = teacher_forced(epi, seq, P).cpu().numpy()                          # the logits the loop saw (two sessions: bit-equal)
    new = seq[:, P:].cpu().numpy()
    Un = U.cpu().numpy()
    for b in range(B):
        for t in range(n):
            check_tokens(select_ref(lg[b, t], T, k, p), new[b, t:t + 1], Un[t, b:b + 1], f"row {b} step {t}")
    assert torch.equal(H.generate(epi, ids, max_new_tokens=n, do_sample=True, temperature=T, top_k=k, top_p=p, uniforms=U, graph=False), seq)


def test_seeds_generators_and_graph_modes(epi):
    ids = ids_of(6, 77)
    kw = dict(max_new_tokens=24, do_sample=True, temperature=1.5, top_k=0, top_p=0.95)
    torch.manual_seed(5)
    a = H.generate(epi, ids, **kw)
    torch.manual_seed(5)
    b = H.generate(epi, ids, **kw)
    torch.manual_seed(5)
    c = H.generate(epi, ids, graph=False, **kw)
    torch.manual_seed(6)
    d = H.generate(epi, ids, **kw)
    assert torch.equal(a, b) and torch.equal(a, c) and not torch.equal(a, d)
    g = lambda seed: torch.Generator(device=DEV).manual_seed(seed)
    e = H.generate(epi, ids, generator=g(9), **kw)
    assert torch.equal(e, H.generate(epi, ids, generator=g(9), **kw)) and not torch.equal(e, H.generate(epi, ids, generator=g(10), **kw))
    host = H.generate(epi, ids, generator=torch.Generator().manual_seed(9), **kw)        # a host generator draws on the host
    assert host.shape == e.shape
    d0 = H.generate(epi, ids, max_new_tokens=8, do_sample=True)                          # the defaults of model.generate: top_k 50
    assert d0.shape == (1, 14)
    with pytest.raises(ValueError):
        H.generate(epi, ids, uniforms=torch.rand(3, 1, device=DEV), **kw)                # fewer rows than new tokens


def test_eos_pad_and_early_stop_do_not_depend_on_poll_every(epi):
    P, n = 4, 12
    ids = ids_of(2 * P, 77, 2)
    seq, _ = hf_run(epi, ids, n)
    new = seq[:, P:].tolist()
    eos = next(t for t in new[0][2:] if t not in new[1] and t not in new[0][:2])          # row 0 finishes early, row 1 runs on
    ref = epi.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=eos, pad_token_id=0)
    for poll in (1, 8):
        got = H.generate(epi, ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=0, poll_every=poll)
        assert got.shape == ref.shape == (2, P + n) and torch.equal(got, ref), poll
    eos2 = [eos, new[1][5]]                                                                 # both rows finish: a shorter result
    ref = epi.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=eos2)
    for poll in (1, 3, 8):
        got = H.generate(epi, ids, max_new_tokens=n, eos_token_id=eos2, poll_every=poll)
        assert got.shape == ref.shape and got.shape[1] < P + n and torch.equal(got, ref), poll
    U = torch.from_numpy(u_table(n, 2, 5)).to(DEV)
    kw = dict(max_new_tokens=n, do_sample=True, temperature=0.9, top_k=20, top_p=0.9, uniforms=U)
    free = H.generate(epi, ids, **kw)
    stop = [int(free[0, P + 3]), int(free[1, P + 6])]                                       # ids the sampled run produces
    a, b = (H.generate(epi, ids, eos_token_id=stop, pad_token_id=1, poll_every=poll, **kw) for poll in (1, 8))
    assert torch.equal(a, b) and a.shape[1] <= P + 7
    hit = torch.isin(a[:, P:], torch.tensor(stop, device=DEV))
    assert bool(hit.any(1).all())
    for r in range(2):
        k = int(hit[r].int().argmax())
        assert torch.equal(a[r, :P + k + 1], free[r, :P + k + 1]) and bool((a[r, P + k + 1:] == 1).all())


def count_ops(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    return {n: names.count(n) for n in set(names)}


@pytest.mark.parametrize("poll", [4, 8])
@pytest.mark.parametrize("with_eos", [False, True])
def test_the_loop_stays_on_the_device(epi, with_eos, poll):
    ids = ids_of(5, 33)
    n = 40
    U = torch.rand(n, 1, device=DEV)
    sess = H.DecodeSession(epi, 1, 5 + n, graph=True)
    sess.begin_selection(ids, 5 + n, eos=[1001] if with_eos else (), pad=0, uniforms=U, temperature=0.7, top_k=50, top_p=0.9)
    sess.select(sess.prefill(ids))
    sess.sel.done = 1
    assert sess.run_selection(3, poll) == 4                                  # the capture happens here
    ops = count_ops(lambda: sess.run_selection(32, poll))
    assert sess.sel.done == 36
    for op in ("aten::argmax", "aten::sort", "aten::multinomial", "aten::isin", "aten::cumsum", "aten::topk", "aten::softmax"):
        assert op not in ops, op
    reads = ops.get("aten::_local_scalar_dense", 0)
    assert reads <= math.ceil(32 / poll) if with_eos else reads == 0, reads
    out = sess.selection_result()
    assert out.shape == (1, 5 + 36)
    eager = H.DecodeSession(epi, 1, 8, graph=False)                          # the same unit, launch by launch, under the profiler
    eager.begin_selection(ids, 8, uniforms=U, temperature=0.7, top_k=50, top_p=0.9)
    eager.select(eager.prefill(ids))
    names = count_ops(eager.step_select)
    assert any("pbl_select_token_kernel" in name for name in names), "the selection kernel is not in the profile"
    assert not {"aten::argmax", "aten::sort", "aten::multinomial", "aten::cumsum"} & set(names)
