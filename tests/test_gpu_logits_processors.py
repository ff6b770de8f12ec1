"""-m gpu: the logits processors on the device -- pbl_process_logits_f16 (runtime.process_logits_f16) against process_ref of
test_logits_processors_cpu.py bit for bit (fp16 bits, -inf included), captured and replayed; pbl_select_token_minp_f16 against
pbl_select_token_f16 (min_p = 0) and against select_ref_minp (min_p > 0); harness.generate with repetition_penalty /
no_repeat_ngram_size / min_new_tokens / min_p on the packed LLaMA models of test_gpu_decode_attention.py.

min_p criterion: the kernel's kept mask equals the restatement's on rows that have no value with |exp(s - max s) / min_p - 1| <= BAND
= 2^-16 (derived in test_logits_processors_cpu.py, not measured) and whose top-p slack exceeds DELTA (test_sampling_cpu.py); the
tests first assert, from the restatement alone, that their rows are such rows."""

import numpy as np
import pytest
import torch

from pb_llm_amd import _lib
from pb_llm_amd import harness as H
from pb_llm_amd.runtime import process_logits_f16, select_token_f16
from test_gpu_decode_attention import built, epi, prompts  # noqa: F401  (built / epi: fixtures)
from test_gpu_decode_epilogues import ids_of
from test_gpu_sampling import Sel, check_tokens, count_ops, teacher_forced, u_table
from test_logits_processors_cpu import BAND, MINP_PARAMS, process_ref, select_ref_minp
from test_sampling_cpu import DELTA, PARAMS, rows16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LONG = 3000                       # a history of more than one pass of the workgroup's 1024 threads


def guarded(rows: np.ndarray, layout: str):
    """(view, base): the rows as a [B, V] view inside a base tensor that holds NaN everywhere else -- 'vec' 16-byte aligned rows,
    'odd' rows that start 6 bytes off, 'last' the view out.logits[:, -1] of a [B, 2, V] tensor"""
    B, V = rows.shape
    t = torch.from_numpy(rows).to(DEV)
    if layout == "last":
        base = torch.full((B, 2, V), float("nan"), dtype=torch.float16, device=DEV)
        base[:, -1] = t
        return base[:, -1], base
    base = torch.full((B, V + 24), float("nan"), dtype=torch.float16, device=DEV)
    off = 0 if layout == "vec" else 3
    base[:, off:off + V] = t
    return base[:, off:off + V], base


def guards_intact(view, base):
    if base.dim() == 3:
        return bool(torch.isnan(base[:, 0]).all())
    V = view.shape[1]
    off = view.storage_offset() - base.storage_offset()
    return bool(torch.isnan(base[:, :off]).all()) and bool(torch.isnan(base[:, off + V:]).all())


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def make_history(row16, L, n, seed):
    """a history of L ids for the row.  L = LONG: one id at positions 0 and L - 1 (two passes apart, penalised once), the top token
    behind a copy of the last n - 1 tokens (penalised and banned), another such copy in front of the id V (a ban that is skipped),
    the second token elsewhere (penalised only), and the ids -1 and V.  Short histories: random ids, the top token first."""
    rng = np.random.default_rng(seed)
    V = row16.size
    order = np.argsort(row16.astype(np.float32))[::-1]
    h = rng.integers(0, V, L).astype(np.int64)
    if L >= 1:
        h[0] = order[0]
    if L == LONG:
        h[L - (n - 1):] = h[100:100 + n - 1] if n > 1 else h[L:]
        h[100 + n - 1] = order[0]
        h[200:200 + n - 1] = h[L - (n - 1):]
        h[200 + n - 1] = V
        h[50] = order[1]
        h[1500], h[1501] = -1, V
        h[0] = h[L - 1]
    return h


def run_process(rows, layout, hists, total, col0, theta, n, eos=None, min_new=0, min_length=0, step=None):
    """one call over `rows` with one history per row (equal lengths) -- returns the processed bits [B, V]; checks the guards, the
    tokens and the step"""
    B, V = rows.shape
    L = len(hists[0])
    view, base = guarded(rows, layout)
    junk = int(np.argsort(rows[0].astype(np.float32))[-3])                 # beyond the history: an id whose penalty would show
    tokens = torch.full((B, total), junk, dtype=torch.long, device=DEV)
    for b in range(B):
        tokens[b, :L] = torch.from_numpy(hists[b])
    before = tokens.clone()
    step_t = torch.tensor([L - col0 if step is None else step], dtype=torch.long, device=DEV)
    step0 = int(step_t)
    eos_t = None if eos is None else torch.tensor(eos, dtype=torch.long, device=DEV)
    scratch = torch.empty(B, total, dtype=torch.float16, device=DEV) if theta != 1.0 else None
    assert process_logits_f16(view, tokens, col0, step_t, repetition_penalty=theta, no_repeat_ngram_size=n, min_new_tokens=min_new,
                              min_length=min_length, eos=eos_t, scratch=scratch) is True
    torch.cuda.synchronize()
    assert guards_intact(view, base), "a store outside the row"
    assert torch.equal(tokens, before) and int(step_t) == step0
    return bits(view)


@pytest.mark.parametrize("V,layout,B", [(1000, "odd", 1), (1000, "odd", 3), (32000, "vec", 2), (32000, "vec", 4), (32000, "last", 1),
                                        (32000, "last", 3)])
def test_kernel_equals_process_ref_bit_for_bit(V, layout, B):
    rows = rows16(V, 3, 9 * V + B, B)
    total = LONG + 8
    for n in range(1, 9):
        theta = (1.3, 0.7, 2.0, 1.0)[n % 4]                                  # theta < 1 and "off" included
        for L in sorted({0, 1, max(n - 2, 0), n - 1, LONG}):
            hists = [make_history(rows[b], L, n, 100 * n + 10 * b + L) for b in range(B)]
            col0 = min(L // 2, total - 1)
            got = run_process(rows, layout, hists, total, col0, theta, n)
            for b in range(B):
                ref = process_ref(rows[b], hists[b], theta, n)
                assert np.array_equal(got[b], ref.view(np.uint16)), \
                    f"n={n} L={L} row {b}: bits differ at {np.flatnonzero(got[b] != ref.view(np.uint16))[:8]}"
                if L == LONG:                                                # the case holds what it claims
                    assert np.isneginf(ref[int(np.argmax(rows[b].astype(np.float32)))]), "the top token is not banned"
                    assert hists[b][0] == hists[b][L - 1] and (hists[b] == -1).any() and (hists[b] == V).any()


def test_eos_is_blocked_exactly_while_the_minimum_holds_and_the_step_is_clamped():
    V, B, total, col0 = 1000, 2, 64, 10
    rows = rows16(V, 3, 41, B)
    hists = [np.random.default_rng(b).integers(0, V, total).astype(np.int64) for b in range(B)]
    eos = [int(np.argmax(rows[0].astype(np.float32))), 17, V + 3, -5]

    def check(step, min_new, min_length, theta=1.0, n=0):
        L = min(max(col0 + step, 0), total)
        got = run_process(rows, "odd", hists, total, col0, theta, n, eos=eos, min_new=min_new, min_length=min_length, step=step)
        blocked = step < min_new or col0 + step < min_length
        for b in range(B):
            ref = process_ref(rows[b], hists[b][:L], theta, n, eos, blocked)
            assert np.array_equal(got[b], ref.view(np.uint16)), (step, min_new, min_length, b)
        return blocked

    assert check(5, 6, 0) and not check(6, 6, 0) and check(0, 1, 0)             # step < min_new_tokens
    assert check(5, 0, 16) and not check(6, 0, 16) and not check(6, 0, 3)       # col0 + step < min_length
    assert check(5, 6, 0, theta=1.3, n=2) and not check(6, 6, 0, theta=1.3, n=2)
    assert not check(10 ** 6, 6, 0, theta=1.3, n=3)                             # beyond the buffer: the whole buffer is the history
    assert check(-10 ** 6, 6, 0, theta=1.3, n=3)                                # before it: an empty history (and step < min_new)


def test_captured_processing_follows_the_step_and_is_bit_stable():
    V, B, total, col0 = 32000, 2, LONG + 8, 5
    rows = rows16(V, 3, 58, B)
    hists = [make_history(rows[b], LONG, 3, 7 + b) for b in range(B)]
    pristine, _ = guarded(rows, "last")
    work, base = guarded(rows, "last")
    tokens = torch.zeros(B, total, dtype=torch.long, device=DEV)
    for b in range(B):
        tokens[b, :LONG] = torch.from_numpy(hists[b])
    step = torch.tensor([0], dtype=torch.long, device=DEV)
    eos = torch.tensor([3, 999], dtype=torch.long, device=DEV)
    scratch = torch.empty(B, total, dtype=torch.float16, device=DEV)

    def call():
        work.copy_(pristine)
        assert process_logits_f16(work, tokens, col0, step, repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=40,
                                  eos=eos, scratch=scratch) is True

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    step.fill_(LONG - col0)
    first = None
    for _ in range(100):                                                     # the same inputs: bit-identical outputs
        graph.replay()
        out = work.clone()
        first = out if first is None else first
        assert torch.equal(out.view(torch.int16), first.view(torch.int16))
    for b in range(B):
        assert np.array_equal(bits(first)[b], process_ref(rows[b], hists[b], 1.3, 3).view(np.uint16))
    steps = [0, 1, 2, 37, 39, 40, 41, 1100, LONG - col0]
    replayed = []
    for t in steps:                                                          # replayed over a changing step ...
        step.fill_(t)
        graph.replay()
        replayed.append(work.clone())
    assert int(step) == steps[-1] and guards_intact(work, base)
    for t, r in zip(steps, replayed):                                        # ... equals the eager calls and the restatement
        step.fill_(t)
        call()
        assert torch.equal(work.view(torch.int16), r.view(torch.int16)), t
        ref = process_ref(rows[0], hists[0][:col0 + t], 1.3, 3, [3, 999], t < 40)
        assert np.array_equal(bits(r)[0], ref.view(np.uint16)), t


# ---------------------------------------------------------------- min_p in the selection
def old_entry(logits, sel, T, k, p, u, kept):
    """pbl_select_token_f16 itself, through the C ABI"""
    B, V = logits.shape
    rc = _lib.lib().pbl_select_token_f16(
        logits.data_ptr(), logits.stride(0) if B > 1 else V, B, V, T, k, p, None if u is None else u.data_ptr(),
        0 if u is None else u.shape[0], sel.step.data_ptr(), None, 0, 0, sel.unfinished.data_ptr(), sel.tokens.data_ptr(), sel.tokens.shape[1],
        sel.col0, sel.next_ids.data_ptr(), sel.count.data_ptr(), sel.status.data_ptr(), kept.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    assert rc == 0


@pytest.mark.parametrize("T,k,p", PARAMS)
def test_min_p_zero_is_the_old_entry_bit_for_bit(T, k, p):
    for V, B, layout in ((32000, 2, "vec"), (1000, 3, "odd")):
        rows = rows16(V, 3, V + B, B)
        logits, _ = guarded(rows, layout)
        n = 16
        u = torch.from_numpy(u_table(n, B, 4)).to(DEV)
        for table in (u, None):
            new, old = Sel(B, n), Sel(B, n)
            kn, ko = (torch.zeros(B, V, dtype=torch.uint8, device=DEV) for _ in range(2))
            for _ in range(n):
                new(logits, T, k, p, table, kept=kn)                         # runtime.select_token_f16: the min_p entry with 0
                old_entry(logits, old, T, k, p, table, ko)
            for a, b in ((new.tokens, old.tokens), (new.next_ids, old.next_ids), (kn, ko), (new.count, old.count), (new.step, old.step),
                         (new.status, old.status)):
                assert torch.equal(a, b)
            assert int(new.step) == n


@pytest.mark.parametrize("T,k,p,min_p", MINP_PARAMS)
@pytest.mark.parametrize("V,B,layout", [(1000, 1, "odd"), (32000, 2, "vec"), (128256, 1, "last")])
def test_min_p_kept_set_and_tokens_equal_the_restatement(V, B, layout, T, k, p, min_p):
    for seed in range(3 * V + B, 3 * V + B + 4000, 100):                      # chosen by the restatement alone
        rows = rows16(V, 3 if V > 1000 else 2, seed, B)
        refs = [select_ref_minp(r, T, k, p, min_p) for r in rows]
        if min(r["band"] for r in refs) > BAND and min(r["slack"] for r in refs) > DELTA:
            break
    assert min(r["band"] for r in refs) > BAND and min(r["slack"] for r in refs) > DELTA, "no seed found"
    logits, _ = guarded(rows, layout)
    n = 48
    us = u_table(n, B, V + B)
    ut = torch.from_numpy(us).to(DEV)
    sel = Sel(B, n)
    kept = torch.zeros(B, V, dtype=torch.uint8, device=DEV)
    for _ in range(n):
        assert select_token_f16(logits, sel.step, sel.unfinished, sel.tokens, 0, sel.next_ids, sel.count, sel.status, temperature=T,
                                top_k=k, top_p=p, uniforms=ut, kept=kept, min_p=min_p) is True
    assert int(sel.step) == n and int(sel.status) == 0
    got = kept.cpu().numpy().astype(bool)
    toks = sel.tokens.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], refs[b]["kept"]), \
            f"row {b}: kept sets differ at {np.flatnonzero(got[b] != refs[b]['kept'])[:8]} ({got[b].sum()} vs {refs[b]['kept'].sum()} kept)"
        if k == 0 and p == 1.0:
            assert 1 <= refs[b]["kept"].sum() < V                            # min_p alone: it did remove tokens
        check_tokens(refs[b], toks[b], us[:, b], f"row {b}")


# ---------------------------------------------------------------- model level
KW = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=6)


def processed_rows(model, seq, P, eos, theta, n, min_new):
    """process_ref of the session's own teacher-forced logits at every generated position of seq: fp16 [B, steps, V]"""
    lg = teacher_forced(model, seq, P).cpu().numpy()
    s = seq.cpu().numpy()
    out = np.empty_like(lg)
    for b in range(lg.shape[0]):
        for t in range(lg.shape[1]):
            out[b, t] = process_ref(lg[b, t], s[b, :P + t], theta, n, eos, t < min_new)
    return out


def early_eos(model, ids, n):
    """an id that the unconstrained greedy run of row 0 emits at its third new token: without min_new_tokens the row would end there"""
    free = H.generate(model, ids, max_new_tokens=n, repetition_penalty=1.3, no_repeat_ngram_size=2)
    return int(free[0, ids.shape[1] + 2])


def test_greedy_generate_applies_the_processors_on_the_device(epi, monkeypatch):
    n = 24
    ids = ids_of(2 * 5, 410, 2)
    P = ids.shape[1]
    eos = early_eos(epi, ids, n)
    calls = []
    monkeypatch.setattr(epi, "generate", lambda *a, **k: calls.append(k), raising=False)
    seq = H.generate(epi, ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=0, **KW)
    assert torch.equal(seq[:, :P], ids) and seq.shape[1] >= P + 7            # eos is blocked for six tokens
    new = seq[:, P:].cpu().numpy()
    assert eos not in new[:, :6]
    rows = processed_rows(epi, seq, P, [eos], 1.3, 2, 6)
    for b in range(2):
        done = False
        for t in range(new.shape[1]):
            want = 0 if done else int(np.argmax(rows[b, t].astype(np.float32)))   # the arg-max, lowest index on ties
            assert new[b, t] == want, f"row {b} step {t}: {new[b, t]} != {want}"
            done = done or want == eos
    assert torch.equal(H.generate(epi, ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=0, graph=False, **KW), seq)
    fp8 = H.generate(epi, ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=0, kv_cache="fp8", **KW)
    assert fp8.shape[0] == 2 and P + 7 <= fp8.shape[1] <= P + n and not bool((fp8[:, P:P + 6] == eos).any())
    saved = epi.generation_config.repetition_penalty
    epi.generation_config.repetition_penalty = 1.3                           # the model's own config counts as the argument does
    try:
        assert torch.equal(H.generate(epi, ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=0, no_repeat_ngram_size=2,
                                      min_new_tokens=6), seq)
    finally:
        epi.generation_config.repetition_penalty = saved
    assert not calls, "model.generate was called"


def test_sampled_generate_applies_the_processors_and_min_p(epi, monkeypatch):
    n, B = 24, 2
    ids = ids_of(2 * 5, 410, B)
    P = ids.shape[1]
    U = torch.from_numpy(u_table(n, B, 12)).to(DEV)
    T, k, p, min_p = 0.7, 50, 0.9, 0.1
    calls = []
    monkeypatch.setattr(epi, "generate", lambda *a, **kw: calls.append(kw), raising=False)
    kw = dict(max_new_tokens=n, do_sample=True, temperature=T, top_k=k, top_p=p, min_p=min_p, uniforms=U, eos_token_id=999, pad_token_id=0, **KW)
    seq = H.generate(epi, ids, **kw)
    assert torch.equal(seq[:, :P], ids) and seq.shape[1] >= P + 7
    new = seq[:, P:].cpu().numpy()
    rows = processed_rows(epi, seq, P, [999], 1.3, 2, 6)
    Un = U.cpu().numpy()
    in_band = 0
    for b in range(B):
        done = False
        for t in range(new.shape[1]):
            if done:
                assert new[b, t] == 0
                continue
            ref = select_ref_minp(rows[b, t], T, k, p, min_p)
            if ref["band"] > BAND:                                            # every step goes through check_tokens
                check_tokens(ref, new[b, t:t + 1], Un[t, b:b + 1], f"row {b} step {t}")
            else:                                                             # a value inside min_p's band (decided by the restatement
                in_band += 1                                                  # alone) may stay or go: the token must pass check_tokens
                errors = []                                                   # against one of the two restatements that differ by it
                for mp in (min_p * (1 - 2 * BAND), min_p * (1 + 2 * BAND)):
                    try:
                        check_tokens(select_ref_minp(rows[b, t], T, k, p, mp), new[b, t:t + 1], Un[t, b:b + 1], f"row {b} step {t}")
                    except AssertionError as e:
                        errors.append(str(e))
                assert len(errors) < 2, f"in-band step fails with the value kept and with it removed: {errors}"
            assert np.isfinite(rows[b, t][new[b, t]]), f"row {b} step {t}: a banned token"
            done = new[b, t] == 999
    print(f"[sampled generate] {in_band} of {new.size} steps have a value inside the min_p band")
    assert torch.equal(H.generate(epi, ids, graph=False, **kw), seq)
    assert H.generate(epi, ids, kv_cache="fp8", **kw).shape[0] == B
    assert not calls, "model.generate was called"


def test_greedy_generate_equals_model_generate_up_to_a_near_tie(epi):
    n = 32
    steps = 0
    for ids in prompts(4, 2, 300):
        P = ids.shape[1]
        eos = early_eos(epi, ids, n)
        got = H.generate(epi, ids, max_new_tokens=n, eos_token_id=eos, pad_token_id=0, **KW)
        rows = processed_rows(epi, got, P, [eos], 1.3, 2, 6).astype(np.float32)
        top2 = np.sort(rows, -1)[..., -2:]
        spacing = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(top2[..., 1]), 2.0 ** -14))) - 10)
        near = ((top2[..., 1] - top2[..., 0]) <= 2 * spacing).any(0)
        steps = int(np.flatnonzero(near)[0]) if near.any() else rows.shape[1]
        if steps >= 16:
            break
    assert steps >= 16, "a processed top-2 gap within two fp16 spacings inside 16 steps of every candidate prompt"
    ref = epi.generate(ids, do_sample=False, max_new_tokens=n, eos_token_id=eos, pad_token_id=0, **KW)
    m = min(P + steps, got.shape[1], ref.shape[1])
    assert m >= P + 7 and torch.equal(got[:, :m], ref[:, :m])


def profiled(fn):
    """count_ops, with the profiler's results -- reference cycles that only the collector frees -- released here, at a quiet point,
    not by a collection in the middle of a later test's forward or capture"""
    import gc
    ops = count_ops(fn)
    torch.cuda.synchronize()
    gc.collect()
    return ops


def unit_kernels(model, ids, **begin):
    """kernel and op counts of one eager decode-and-select unit of a session begun with `begin`"""
    sess = H.DecodeSession(model, ids.shape[0], ids.shape[1] + 4, graph=False)
    sess.begin_selection(ids, ids.shape[1] + 4, **begin)
    sess.select(sess.prefill(ids))
    return profiled(sess.step_select)


def test_the_loop_stays_on_the_device_with_processors(epi):
    ids = ids_of(5, 33)
    n = 40
    U = torch.rand(n, 1, device=DEV)
    sess = H.DecodeSession(epi, 1, 5 + n, graph=True)
    sess.begin_selection(ids, 5 + n, eos=[1001], pad=0, uniforms=U, temperature=0.7, top_k=50, top_p=0.9, repetition_penalty=1.1,
                         no_repeat_ngram_size=3, min_new_tokens=4, min_p=0.05)
    sess.select(sess.prefill(ids))
    sess.sel.done = 1
    assert sess.run_selection(3, 8) == 4                                     # the capture happens here
    ops = profiled(lambda: sess.run_selection(32, 8))
    assert sess.sel.done == 36
    for op in ("aten::argmax", "aten::sort", "aten::multinomial", "aten::isin", "aten::cumsum", "aten::topk", "aten::softmax",
               "aten::gather", "aten::scatter", "aten::scatter_", "aten::where", "aten::masked_fill", "aten::unfold"):
        assert op not in ops, op
    assert ops.get("aten::_local_scalar_dense", 0) <= 4
    names = unit_kernels(epi, ids, uniforms=U, temperature=0.7, top_k=50, top_p=0.9, repetition_penalty=1.1, no_repeat_ngram_size=3, min_p=0.05)
    assert sum(c for name, c in names.items() if "pbl_process_logits_kernel" in name) >= 1, "the processing kernel is not in the profile"
    assert any("pbl_select_token_kernel" in name for name in names)
    assert not {"aten::argmax", "aten::sort", "aten::multinomial", "aten::cumsum", "aten::gather", "aten::scatter"} & set(names)


def test_all_processors_off_launches_what_a_plain_selection_launches(epi):
    ids = ids_of(5, 33)
    U = torch.rand(8, 1, device=DEV)
    gpu = lambda ops: {name: c for name, c in ops.items() if "(" in name}     # kernels carry their signature; ops and runtime calls do not
    for sampling in (dict(), dict(uniforms=U, temperature=0.7, top_k=50, top_p=0.9)):
        plain = gpu(unit_kernels(epi, ids, **sampling))                      # the arguments of a selection before this feature
        off = gpu(unit_kernels(epi, ids, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, min_length=0, min_p=0.0,
                               eos=[7], **sampling))
        idle = gpu(unit_kernels(epi, ids, min_new_tokens=3, min_length=9, **sampling))      # a minimum without an eos id: nothing to block
        on = gpu(unit_kernels(epi, ids, repetition_penalty=1.2, **sampling))
        assert any("pbl_select_token_kernel" in name for name in plain)
        assert not any("pbl_process_logits" in name for name in plain) and plain == off == idle
        extra = {name: c - plain.get(name, 0) for name, c in on.items() if c != plain.get(name, 0)}
        assert len(extra) == 1 and all("pbl_process_logits_kernel" in name and c >= 1 for name, c in extra.items()), extra
