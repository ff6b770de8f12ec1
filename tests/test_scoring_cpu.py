"""Token scoring without a GPU: score_ref -- the float64 restatement of pbl_score_tokens_f16's rules (include/pbl.h), which the GPU
tests compare the kernel against -- checked against torch.log_softmax / torch.argmax; the C ABI; and scoring.loglikelihood / _batches
on a tiny fp32 LLaMA on the CPU (the torch fallback)."""
import ctypes as C
import logging
import math
import os
import re

import numpy as np
import pytest
import torch

from pb_llm_amd import _lib, scoring

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = -100
ULP = 2.0 ** -24


def bound(V, lse=0.0, xt=0.0):
    """|kernel - float64| per row: the relative error of an fp32 sum in which one of 256 lanes adds at most ceil(V / 256) terms with
    one rescale each, followed by a merge tree, plus four fp32 ulps of the larger operand of the final subtraction"""
    big = max(1.0, abs(float(lse)), abs(float(xt)))
    return (2 * math.ceil(V / 256) + 32) * ULP + 4 * ULP * big


def span_sum_order(values, counted):
    """the fp64 sum of values[counted] in the kernel's order: 64 partials, partial j adds positions j, j + 64, ... in order, then a
    xor butterfly (32, 16, ... 1)"""
    values = np.asarray(values, np.float64)
    part = np.zeros(64, np.float64)
    for j in range(64):
        for i in range(j, len(values), 64):
            if counted[i]:
                part[j] = part[j] + values[i]
    idx = np.arange(64)
    with np.errstate(invalid="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            part = part + part[idx ^ off]
    return part[0]


def score_ref(rows_fp16, targets, ignore_index=IGNORE, spans=None):
    """float64 restatement: dict(logprob [T] f64, greedy [T] bool, lse [T] f64 (NaN for rows that score NaN), xt [T] f64, status,
    span_sum / span_greedy / span_count [R])"""
    rows = np.asarray(rows_fp16)
    assert rows.dtype == np.float16 and rows.ndim == 2
    T, V = rows.shape
    targets = np.asarray(targets, np.int64)
    logprob, greedy = np.zeros(T, np.float64), np.zeros(T, bool)
    lse, xt = np.full(T, np.nan), np.zeros(T, np.float64)
    status = 0
    for t in range(T):
        tg = int(targets[t])
        if tg == ignore_index:
            continue
        if not 0 <= tg < V:
            logprob[t] = np.nan
            status |= 1
            continue
        x = rows[t].astype(np.float64)
        nan = np.isnan(x)
        argmax = int(np.flatnonzero(nan)[0]) if nan.any() else int(np.argmax(x))          # (-0 == +0; the first maximum)
        greedy[t] = argmax == tg
        xt[t] = x[tg]
        if nan.any() or np.isposinf(x).any() or not np.isfinite(x).any():
            logprob[t] = np.nan
            continue
        m = x.max()
        with np.errstate(divide="ignore"):
            lse[t] = m + np.log(np.exp(x - m).sum())
        logprob[t] = x[tg] - lse[t]                                                        # (-inf for a -inf target)
    out = dict(logprob=logprob, greedy=greedy, lse=lse, xt=xt)
    if spans is not None:
        spans = np.asarray(spans, np.int64).reshape(-1, 2)
        R = len(spans)
        out["span_sum"], out["span_greedy"], out["span_count"] = np.zeros(R), np.ones(R, bool), np.zeros(R, np.int32)
        for r, (b, e) in enumerate(spans.tolist()):
            if b < 0 or e > T or b > e:
                out["span_sum"][r], out["span_greedy"][r] = np.nan, False
                status |= 2
                continue
            counted = targets[b:e] != ignore_index
            out["span_sum"][r] = span_sum_order(logprob[b:e], counted)
            out["span_greedy"][r] = bool(greedy[b:e][counted].all())
            out["span_count"][r] = int(counted.sum())
    out["status"] = status
    return out


def normal16(T, V, sigma, seed):
    return (np.random.default_rng(seed).standard_normal((T, V)) * sigma).astype(np.float16)


def special_rows():
    """[(name, row fp16 [V], targets to score)]: the rows whose results are exact (NaN-ness, infinities and flags, no tolerance)"""
    inf = np.inf
    out = []
    out.append(("all -inf", np.full(100, -inf, np.float16), [0, 57]))
    r = normal16(1, 3000, 1, 1)[0]; r[1234] = inf
    out.append(("one +inf", r, [1234, 0]))
    r = normal16(1, 3000, 1, 2)[0]; r[2999] = np.nan
    out.append(("one NaN", r, [2999, 5]))
    r = normal16(1, 3000, 1, 3)[0]; r[77] = np.nan; r[78] = inf; r[2100] = np.nan
    out.append(("NaN and +inf", r, [77, 78, 2100]))
    out.append(("all equal", np.full(1000, 1.5, np.float16), [0, 1]))
    r = normal16(1, 1003, 1, 4)[0]; r[1002] = 9.0
    out.append(("maximum at V - 1, V % 8 != 0", r, [1002, 1001]))
    r = -np.abs(normal16(1, 500, 1, 5)[0]) - np.float16(1); r[3] = -0.0; r[9] = 0.0
    out.append(("-0 before +0", r, [3, 9]))
    r = -np.abs(normal16(1, 500, 1, 6)[0]) - np.float16(1); r[3] = 0.0; r[9] = -0.0
    out.append(("+0 before -0", r, [3, 9]))
    r = np.full(4096, -65504, np.float16); r[::3] = 65504
    out.append(("65504 and -65504", r, [0, 1, 4095]))
    r = normal16(1, 2500, 1, 7)[0]; r[2049] = -inf
    out.append(("finite row, -inf target", r, [2049, 2048]))
    r = normal16(1, 5000, 1, 8)[0]; r[:2048] = -inf
    out.append(("first 2048 -inf", r, [0, 2047, 2048, 4999]))
    r = np.full(7, -inf, np.float16); r[4] = 2.0
    out.append(("V = 7, one finite", r, [4, 0]))
    r = np.full(5000, -inf, np.float16); r[4999] = -3.0
    out.append(("one finite at the end", r, [4999, 0]))
    return out


# ---------------------------------------------------------------- the restatement against torch
@pytest.mark.parametrize("name,row,targets", special_rows(), ids=[s[0] for s in special_rows()])
def test_score_ref_equals_torch_on_special_rows(name, row, targets):
    rows = np.repeat(row[None], len(targets), 0)
    ref = score_ref(rows, targets)
    lsm = torch.log_softmax(torch.from_numpy(row).float(), -1)
    am = int(torch.argmax(torch.from_numpy(row).float()))
    for i, tg in enumerate(targets):
        want, got = float(lsm[tg]), float(ref["logprob"][i])
        assert math.isnan(want) == math.isnan(got), (name, tg, want, got)
        if math.isinf(want) or math.isinf(got):
            assert want == got, (name, tg, want, got)
        elif not math.isnan(want):
            assert abs(want - got) <= bound(len(row), ref["lse"][i], ref["xt"][i]), (name, tg, want, got)
        assert bool(ref["greedy"][i]) == (am == tg), (name, tg, am)
    assert ref["status"] == 0


@pytest.mark.parametrize("V,sigma", [(1, 1), (7, 30), (1000, 1), (32000, 30)])
def test_score_ref_equals_torch_on_normal_rows(V, sigma):
    rows = normal16(3, V, sigma, V + sigma)
    targets = np.array([0, V - 1, V // 2])
    ref = score_ref(rows, targets, spans=[[0, 3], [1, 1]])
    lsm = torch.log_softmax(torch.from_numpy(rows).double(), -1)
    want = lsm[torch.arange(3), torch.from_numpy(targets)].numpy()
    assert np.abs(want - ref["logprob"]).max() < 1e-12 * max(1.0, np.abs(want).max())
    assert np.array_equal(ref["greedy"], torch.from_numpy(rows).float().argmax(-1).numpy() == targets)
    assert ref["span_sum"][0] == pytest.approx(want.sum(), rel=1e-14) and ref["span_count"].tolist() == [3, 0]
    assert ref["span_sum"][1] == 0 and ref["span_greedy"][1]


def test_score_ref_targets_and_spans():
    rows = normal16(6, 50, 1, 9)
    targets = np.array([3, IGNORE, 50, -1, IGNORE, 49])
    ref = score_ref(rows, targets, spans=[[0, 6], [1, 2], [4, 4], [5, 7], [-1, 2], [3, 2], [0, 2]])
    assert ref["status"] == 3
    assert ref["logprob"][1] == 0 and ref["logprob"][4] == 0 and not ref["greedy"][[1, 2, 3, 4]].any()
    assert np.isnan(ref["logprob"][[2, 3]]).all() and np.isfinite(ref["logprob"][[0, 5]]).all()
    assert np.isnan(ref["span_sum"][0]) and ref["span_count"].tolist() == [4, 0, 0, 0, 0, 0, 1]
    assert ref["span_sum"][1] == 0 and ref["span_greedy"][1] and ref["span_sum"][2] == 0 and ref["span_greedy"][2]
    assert np.isnan(ref["span_sum"][[3, 4, 5]]).all() and not ref["span_greedy"][[3, 4, 5]].any()
    assert ref["span_sum"][6] == ref["logprob"][0]


# ---------------------------------------------------------------- the C ABI
def test_entry_is_declared_exported_and_documented():
    hdr = open(os.path.join(REPO, "include", "pbl.h")).read()
    assert re.search(r"^int\s+pbl_score_tokens_f16\s*\(", hdr, re.M)
    assert "pbl_score_tokens_f16" in _lib.EXPORTS and hasattr(_lib.lib(), "pbl_score_tokens_f16")
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "pbl_score_tokens_f16" in open(os.path.join(REPO, doc)).read(), doc


def test_entry_rejects_bad_arguments_before_any_launch():
    """every call below must fail its argument checks: the pointers are host buffers, none may reach a launch"""
    L = _lib.lib()
    T, V, R = 4, 64, 2
    logits = (C.c_uint16 * (T * V))()
    targets, spans = (C.c_int64 * T)(), (C.c_int64 * (2 * R))()
    logprob, greedy, status = (C.c_float * T)(), (C.c_uint8 * T)(), (C.c_int32 * 1)()
    ssum, sgr, scnt = (C.c_double * R)(), (C.c_uint8 * R)(), (C.c_int32 * R)()
    a = C.addressof

    def call(**kw):
        p = dict(logits=a(logits), ld=V, T=T, V=V, targets=a(targets), logprob=a(logprob), greedy=a(greedy), spans=a(spans), R=R,
                 ssum=a(ssum), sgr=a(sgr), scnt=a(scnt), status=a(status))
        p.update(kw)
        return L.pbl_score_tokens_f16(p["logits"], p["ld"], p["T"], p["V"], p["targets"], IGNORE, p["logprob"], p["greedy"], p["spans"],
                                      p["R"], p["ssum"], p["sgr"], p["scnt"], p["status"], None)

    for kw in (dict(logits=None), dict(targets=None), dict(logprob=None), dict(status=None), dict(spans=None), dict(ssum=None),
               dict(sgr=None), dict(scnt=None), dict(greedy=None), dict(T=0), dict(V=0), dict(R=-1), dict(ld=V - 1),
               dict(logprob=a(logits)), dict(greedy=a(targets)), dict(ssum=a(spans)), dict(sgr=a(greedy)), dict(scnt=a(status)),
               dict(status=a(logprob)), dict(logprob=a(logits) + 2 * (T * V - 1))):
        assert call(**kw) == _lib.PBL_ERR_INVALID_ARG, kw
    assert call(V=(1 << 20) + 1, ld=(1 << 20) + 1) == _lib.PBL_ERR_UNSUPPORTED


# ---------------------------------------------------------------- loglikelihood on the CPU (the torch fallback)
@pytest.fixture(scope="module")
def tiny():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=1000, max_position_embeddings=64)
    return LlamaForCausalLM(cfg).float().eval()


def requests_of(seed, lengths, vocab=1000):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, vocab, c).tolist(), rng.integers(0, vocab, n).tolist()) for c, n in lengths]


LENGTHS = [(5, 3), (12, 1), (1, 7), (30, 10), (3, 3), (20, 2), (60, 9), (8, 8), (2, 1)]     # (60, 9): longer than max_length + 1


def unbatched(model, ctx, cont, max_length):
    """one request, no batching and no padding: lm-eval's slice, log_softmax, gather, argmax"""
    full = (list(ctx) + list(cont))[-(max_length + 1):]
    with torch.no_grad():
        lsm = torch.log_softmax(model(torch.tensor([full[:-1]])).logits[0].float(), -1)
    rows = lsm[len(full) - 1 - len(cont):]
    tg = torch.tensor(full[-len(cont):])
    return float(rows.gather(1, tg[:, None]).sum()), bool((rows.argmax(-1) == tg).all())


def test_loglikelihood_equals_unbatched_scoring_for_every_batch_size(tiny):
    reqs = requests_of(1, LENGTHS)
    want = [unbatched(tiny, c, n, 64) for c, n in reqs]
    cut = unbatched(tiny, (reqs[6][0] + reqs[6][1])[-65:-9], reqs[6][1], 64)      # request 6 keeps its last 65 tokens
    assert want[6] == cut
    for bs in (1, 3, 8):
        got = scoring.loglikelihood(tiny, reqs, batch_size=bs)
        assert len(got) == len(reqs)
        for i, ((ws, wg), (gs, gg)) in enumerate(zip(want, got)):
            assert abs(ws - gs) <= 1e-5 * max(1.0, abs(ws)), (bs, i, ws, gs)
            assert wg == gg and isinstance(gs, float) and isinstance(gg, bool), (bs, i)
    short = scoring.loglikelihood(tiny, reqs, batch_size=3, max_length=16)
    for i, (c, n) in enumerate(reqs):
        ws, wg = unbatched(tiny, c, n, 16)
        assert abs(ws - short[i][0]) <= 1e-5 * max(1.0, abs(ws)) and wg == short[i][1], i


def test_loglikelihood_flags_greedy_continuations(tiny):
    ctx = [5, 17, 900, 3]
    seq = list(ctx)
    with torch.no_grad():
        for _ in range(4):
            seq.append(int(tiny(torch.tensor([seq])).logits[0, -1].argmax()))
    other = list(seq[4:])
    other[2] = (other[2] + 1) % 1000
    got = scoring.loglikelihood(tiny, [(ctx, seq[4:]), (ctx, other)], batch_size=2)
    assert got[0][1] is True and got[1][1] is False and got[0][0] > got[1][0]


def test_loglikelihood_raises(tiny):
    with pytest.raises(ValueError, match="empty context"):
        scoring.loglikelihood(tiny, [([], [1, 2])])
    with pytest.raises(ValueError, match="empty continuation"):
        scoring.loglikelihood(tiny, [([1], [])])
    with pytest.raises(ValueError, match="longer than max_length"):
        scoring.loglikelihood(tiny, [([1], list(range(65)))])
    with pytest.raises(ValueError, match="longer than max_length"):
        scoring.loglikelihood(tiny, [([1], [1, 2, 3])], max_length=2)
    assert len(scoring.loglikelihood(tiny, [([1], list(range(64)))])) == 1          # max_length tokens: allowed
    with pytest.raises(RuntimeError, match="outside"):
        scoring.loglikelihood(tiny, [([1, 2], [3, 950])], vocab_limit=900)


def test_fallback_is_logged_once(tiny, caplog):
    scoring._fallback_logged = False
    with caplog.at_level(logging.INFO, logger="pb_llm_amd"):
        scoring.loglikelihood(tiny, requests_of(2, LENGTHS[:4]), batch_size=2)
        scoring.token_logprobs(tiny, torch.tensor([[1, 2, 3, 4]]))
    said = [r for r in caplog.records if "scored by torch" in r.getMessage()]
    assert len(said) == 1 and said[0].levelno == logging.INFO and "float32 logits on cpu" in said[0].getMessage()


def test_token_logprobs_and_modes_on_the_cpu(tiny):
    ids = torch.from_numpy(np.random.default_rng(3).integers(0, 1000, (2, 9)))
    with torch.no_grad():
        lsm = torch.log_softmax(tiny(ids).logits.float(), -1)
    want = lsm[:, :-1].gather(2, ids[:, 1:, None])[..., 0]
    for ctx in (torch.no_grad, torch.inference_mode):
        with ctx():
            lp, gr = scoring.token_logprobs(tiny, ids)
        assert lp.shape == (2, 8) and gr.shape == (2, 8) and gr.dtype == torch.bool
        assert float((lp - want).abs().max()) <= 1e-5
        assert torch.equal(gr, lsm[:, :-1].argmax(-1) == ids[:, 1:])
    lp9, _ = scoring.token_logprobs(tiny, ids % 900, vocab_limit=900)
    with torch.no_grad():
        w9 = torch.log_softmax(tiny(ids % 900).logits[..., :900].float(), -1)[:, :-1].gather(2, (ids % 900)[:, 1:, None])[..., 0]
    assert float((lp9 - w9).abs().max()) <= 1e-5


# ---------------------------------------------------------------- _batches
@pytest.mark.parametrize("bs", [1, 4, 100])
def test_batches_are_longest_first_right_padded_and_complete(bs):
    reqs = requests_of(4, LENGTHS)
    seen, last = [], None
    for input_ids, targets, spans, idx in scoring._batches(reqs, bs, 64, pad_token_id=7):
        b, L = input_ids.shape
        assert b == len(idx) <= bs and targets.shape == (b * L,) and spans.shape == (b, 2)
        assert input_ids.dtype == targets.dtype == spans.dtype == torch.int64
        for j, i in enumerate(idx):
            full = (reqs[i][0] + reqs[i][1])[-65:]
            inp, n = full[:-1], len(reqs[i][1])
            assert last is None or len(reqs[i][0]) + n <= last
            last = len(reqs[i][0]) + n
            assert input_ids[j, :len(inp)].tolist() == inp and (input_ids[j, len(inp):] == 7).all()
            assert spans[j].tolist() == [j * L + len(inp) - n, j * L + len(inp)]
            row = targets.view(b, L)[j]
            assert row[len(inp) - n:len(inp)].tolist() == reqs[i][1]
            assert (row[:len(inp) - n] == IGNORE).all() and (row[len(inp):] == IGNORE).all()
        assert L == len((reqs[idx[0]][0] + reqs[idx[0]][1])[-65:]) - 1               # the batch's first request is its longest
        seen += idx
    assert sorted(seen) == list(range(len(reqs)))
