"""Token scoring on the GPU: pbl_score_tokens_f16 (runtime.score_tokens_f16) against score_ref, the float64 restatement of
test_scoring_cpu -- a grid of shapes, layouts and value ranges, the rows and targets whose results are exact, spans, determinism,
capture, the no-copy contract -- and scoring.token_logprobs / loglikelihood / harness.perplexity(fused=True) on the packed, folded
2-layer LLaMA of test_gpu_decode_attention."""
import functools
import math

import numpy as np
import pytest
import torch

from pb_llm_amd import decoding as D, harness as H, scoring
from pb_llm_amd.runtime import score_tokens_f16
from test_gpu_decode_attention import built, epi  # noqa: F401  (fixtures)
from test_gpu_decode_epilogues import ids_of
from test_gpu_sampling import strided
from test_scoring_cpu import IGNORE, LENGTHS, bound, normal16, requests_of, score_ref, span_sum_order, special_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("vec", "odd", "last")


def dev(a, dtype=torch.int64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def run(logits, targets, spans=None, ignore_index=IGNORE):
    out = score_tokens_f16(logits, dev(targets), None if spans is None else dev(spans).view(-1, 2), ignore_index)
    assert out is not None
    return out


def check_rows(got, ref, V, what):
    """logprob within the per-row bound of the restatement (NaN-ness and infinities exactly), greedy exactly"""
    lp, gr = got[0].cpu().numpy().astype(np.float64), got[1].cpu().numpy()
    assert gr.dtype == bool and np.array_equal(gr, ref["greedy"]), f"{what}: greedy differs at rows {np.flatnonzero(gr != ref['greedy'])[:8]}"
    for t, r in enumerate(ref["logprob"]):
        if math.isnan(r) or math.isinf(r):
            assert (math.isnan(lp[t]) and math.isnan(r)) or lp[t] == r, f"{what}: row {t} scores {lp[t]}, the restatement {r}"
        else:
            tol = bound(V, ref["lse"][t], ref["xt"][t])
            assert abs(lp[t] - r) <= tol, f"{what}: row {t}: |{lp[t]!r} - {r!r}| = {abs(lp[t] - r):.3e} > {tol:.3e}"


def check_spans(got, ref, V, targets, spans, what, ignore_index=IGNORE):
    """span_sum: exactly the fp64 sum, in the kernel's stated order, of the fp32 logprobs it returned, and within the rows' summed
    bounds of the restatement; span_greedy and span_count exactly"""
    lp = got[0].cpu().numpy()
    ssum, sgr, scnt = got[2].cpu().numpy(), got[3].cpu().numpy(), got[4].cpu().numpy()
    assert ssum.dtype == np.float64 and sgr.dtype == bool and scnt.dtype == np.int32
    assert np.array_equal(sgr, ref["span_greedy"]) and np.array_equal(scnt, ref["span_count"]), what
    targets = np.asarray(targets)
    for r, (b, e) in enumerate(np.asarray(spans).reshape(-1, 2).tolist()):
        want = ref["span_sum"][r]
        if math.isnan(want) or math.isinf(want):
            assert (math.isnan(ssum[r]) and math.isnan(want)) or ssum[r] == want, f"{what}: span {r} sums to {ssum[r]}, the restatement {want}"
            continue
        counted = targets[b:e] != ignore_index
        assert ssum[r] == span_sum_order(lp[b:e], counted), f"{what}: span {r} is not the fp64 sum of the returned log-probs"
        tol = sum(bound(V, ref["lse"][t], ref["xt"][t]) for t in range(b, e) if counted[t - b])
        assert abs(ssum[r] - want) <= tol, f"{what}: span {r}: |{ssum[r]!r} - {want!r}| > {tol:.3e}"


# ---------------------------------------------------------------- the grid
@functools.lru_cache(maxsize=None)
def grid_case(V, T, sigma):
    rows = normal16(T, V, sigma, 1000 * sigma + 7 * T + V % 997)
    targets = np.random.default_rng(V + T).integers(0, V, T)
    targets[0], targets[-1] = 0, V - 1
    if T > 3:
        targets[T // 2] = V // 2
        targets[5] = targets[41] = IGNORE
        targets[9] = int(rows[9].argmax())
    spans = np.array([[0, T], [0, T // 2], [T // 2, T]])
    return rows, targets, spans, score_ref(rows, targets, spans=spans)


GRID = [(V, T) for V in (1, 7, 8, 1000, 32000, 128256, 1 << 20) for T in (1, 3, 65) if T <= 3 or V < 128256]   # T <= 3 at the two largest


@pytest.mark.parametrize("sigma", [1, 30])
@pytest.mark.parametrize("V,T", GRID)
def test_grid_equals_the_restatement(V, T, sigma):
    rows, targets, spans, ref = grid_case(V, T, sigma)
    assert ref["status"] == 0 and np.isfinite(ref["logprob"]).all()
    for layout in LAYOUTS:
        got = run(strided(rows, layout), targets, spans)
        what = f"V={V} T={T} sigma={sigma} {layout}"
        check_rows(got, ref, V, what)
        check_spans(got, ref, V, targets, spans, what)
        assert int(got[5]) == 0, what


def test_rows_past_2_to_31_elements():
    """row 1 starts 2^31 + 8 elements after row 0: the row offset is 64-bit arithmetic"""
    V, ld = 1000, (1 << 31) + 8
    rows = normal16(2, V, 3, 5)
    base = torch.empty(ld + V, dtype=torch.float16, device=DEV)
    view = base.as_strided((2, V), (ld, 1))
    view.copy_(torch.from_numpy(rows))
    targets = np.array([17, 999])
    check_rows(run(view, targets), score_ref(rows, targets), V, "ld = 2^31 + 8")


# ---------------------------------------------------------------- rows whose results are exact
@pytest.mark.parametrize("name,row,targets", special_rows(), ids=[s[0] for s in special_rows()])
def test_special_rows(name, row, targets):
    rows = np.repeat(row[None], len(targets), 0)
    spans = [[0, len(targets)]]
    ref = score_ref(rows, targets, spans=spans)
    for layout in LAYOUTS:
        got = run(strided(rows, layout), targets, spans)
        check_rows(got, ref, len(row), f"{name} {layout}")
        check_spans(got, ref, len(row), targets, spans, f"{name} {layout}")
        assert int(got[5]) == 0


def test_every_special_row_in_one_call_next_to_normal_rows():
    """the special rows of one width side by side: a row's result does not depend on its neighbours"""
    V = 3000
    rows = normal16(8, V, 2, 11)
    rows[1, 5] = np.nan
    rows[2, :] = -np.inf
    rows[3, 2999] = np.inf
    rows[5, :] = 0.25
    rows[6, :2048] = -np.inf
    targets = np.array([1, 5, 0, 2999, 7, 0, 3, 2999])
    ref = score_ref(rows, targets)
    for layout in LAYOUTS:
        check_rows(run(strided(rows, layout), targets), ref, V, layout)


# ---------------------------------------------------------------- targets
def test_ignored_and_out_of_range_targets():
    V, T = 1003, 8
    rows = normal16(T, V, 3, 21)
    targets = np.array([0, V - 1, IGNORE, V, 500, -1, IGNORE, int(rows[7].argmax())])
    spans = [[0, 3], [4, 5], [2, 3], [6, 8], [3, 4]]
    ref = score_ref(rows, targets, spans=spans)
    assert ref["status"] == 1
    for layout in LAYOUTS:
        got = run(strided(rows, layout), targets, spans)
        check_rows(got, ref, V, layout)
        check_spans(got, ref, V, targets, spans, layout)
        lp, gr = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert lp[2] == 0 and lp[6] == 0 and np.isnan(lp[[3, 5]]).all() and not gr[[2, 3, 5, 6]].any() and gr[7]
        assert int(got[5]) == 1
    clean = run(strided(rows, "vec"), np.where((targets == V) | (targets == -1), 3, targets))
    dirty = run(strided(rows, "vec"), targets)
    keep = [0, 1, 2, 4, 6, 7]                                       # every other row of the same call is unaffected
    assert torch.equal(clean[0][keep].view(torch.int32), dirty[0][keep].view(torch.int32)) and int(clean[5]) == 0
    other = run(strided(rows, "vec"), np.where(targets == IGNORE, -5, targets), ignore_index=-5)     # another ignore_index
    assert torch.equal(other[0].view(torch.int32), dirty[0].view(torch.int32)) and torch.equal(other[1], dirty[1])


# ---------------------------------------------------------------- spans
def test_spans():
    V, T = 1000, 150
    rows = normal16(T, V, 2, 31)
    targets = np.random.default_rng(32).integers(0, V, T)
    greedy_rows = np.arange(100, 110)
    targets[greedy_rows] = rows[greedy_rows].astype(np.float64).argmax(-1)
    targets[60:70] = IGNORE
    targets[20] = IGNORE
    good = [[0, T], [0, 50], [50, 100], [100, 150], [30, 130], [40, 41], [77, 77], [0, 0], [T, T], [60, 70], [100, 110], [15, 25]]
    ref = score_ref(rows, targets, spans=good)
    assert ref["span_greedy"].tolist() == [False] * 6 + [True] * 5 + [False] and ref["span_count"].tolist() == [139, 49, 40, 50, 90, 1, 0, 0, 0, 0, 10, 9]
    got = run(strided(rows, "vec"), targets, good)
    check_rows(got, ref, V, "spans")
    check_spans(got, ref, V, targets, good, "spans")
    assert int(got[5]) == 0
    one = run(strided(rows, "odd"), targets, [[0, T]])                   # R = 1 over all rows (another layout: other chunks, other bits)
    assert one[2].shape == (1,) and one[3].shape == (1,) and one[4].shape == (1,)
    check_spans(one, score_ref(rows, targets, spans=[[0, T]]), V, targets, [[0, T]], "one span")
    bad = good[:3] + [[-1, 5], [10, T + 1], [9, 8]] + good[3:]
    refb = score_ref(rows, targets, spans=bad)
    assert refb["status"] == 2
    gotb = run(strided(rows, "vec"), targets, bad)
    check_spans(gotb, refb, V, targets, bad, "bad spans")
    assert int(gotb[5]) == 2
    ok = [0, 1, 2] + list(range(6, 15))
    assert torch.equal(gotb[2][ok].view(torch.int64), got[2].view(torch.int64))          # the other spans are unaffected
    none = run(strided(rows, "vec"), targets)
    assert none[2] is None and none[3] is None and none[4] is None
    assert torch.equal(none[0].view(torch.int32), got[0].view(torch.int32))


# ---------------------------------------------------------------- determinism and capture
def test_two_calls_are_bit_equal_and_a_captured_call_follows_new_logits():
    V, T = 32000, 33
    rows, rows2 = normal16(T, V, 3, 41), normal16(T, V, 3, 42)
    targets = np.random.default_rng(43).integers(0, V, T)
    static = strided(rows, "vec")
    tg, sp = dev(targets), dev([[0, T], [5, 20]])

    def unit():
        return score_tokens_f16(static, tg, sp)

    def bits(out):
        return [out[0].view(torch.int32).clone(), out[1].clone(), out[2].view(torch.int64).clone(), out[3].clone(), out[4].clone(), out[5].clone()]

    first, second = bits(unit()), bits(unit())
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    graph, out = D._capture_graph(unit, torch.device(DEV))
    graph.replay()
    assert all(torch.equal(a, b) for a, b in zip(first, bits(out)))
    static.copy_(torch.from_numpy(rows2))
    graph.replay()
    replayed = bits(out)
    eager = bits(unit())
    assert all(torch.equal(a, b) for a, b in zip(eager, replayed))
    assert not torch.equal(first[0], replayed[0])
    check_rows(out, score_ref(rows2, targets), V, "replayed")


# ---------------------------------------------------------------- no copy of the logits
def test_views_of_a_2048_token_window_are_scored_without_a_copy():
    T, V = 2047, 32000
    g = torch.Generator(device=DEV).manual_seed(5)
    logits = torch.randn(1, T + 1, V, generator=g, device=DEV).mul_(3).half()
    targets = torch.randint(0, V - 1, (T,), generator=g, device=DEV)
    spans = dev([[0, T]])
    pick = [0, 1, 1000, 2046]
    for view, width in ((logits[0, :-1], V), (logits[0, :-1, :V - 1], V - 1)):
        assert view.data_ptr() == logits.data_ptr()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        out = score_tokens_f16(view, targets, spans)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
        assert grown < T * width, f"{grown} bytes allocated: half an fp16 copy of the logits is {T * width}"
        rows = view[pick].cpu().numpy()
        ref = score_ref(rows, targets[pick].cpu().numpy())
        sub = (out[0][pick], out[1][pick])
        check_rows(sub, ref, width, f"width {width}")
        assert int(out[5]) == 0 and int(out[4][0]) == T
        assert float(out[2][0]) == span_sum_order(out[0].cpu().numpy(), np.ones(T, bool))


# ---------------------------------------------------------------- declines and errors
def test_declines_and_errors():
    big = torch.zeros(1, (1 << 20) + 1, dtype=torch.float16, device=DEV)
    assert score_tokens_f16(big, dev([0])) is None
    assert score_tokens_f16(big[:, :1 << 20], dev([0])) is not None
    ok = torch.zeros(4, 64, dtype=torch.float16, device=DEV)
    tg = dev([0, 1, 2, 3])
    with pytest.raises(ValueError):
        score_tokens_f16(ok.float(), tg)
    with pytest.raises(ValueError):
        score_tokens_f16(ok.as_strided((4, 64), (32, 1)), tg)                     # ld < V
    with pytest.raises(ValueError):
        score_tokens_f16(ok.as_strided((4, 64), (0, 1)), tg)
    with pytest.raises(ValueError):
        score_tokens_f16(ok.t(), dev(range(64)))                                  # column stride 4
    with pytest.raises(ValueError):
        score_tokens_f16(ok, tg[:3])
    with pytest.raises(ValueError):
        score_tokens_f16(ok, tg.int())
    with pytest.raises(ValueError):
        score_tokens_f16(ok, tg.cpu())
    with pytest.raises(ValueError):
        score_tokens_f16(ok, tg, dev([0, 4]))                                     # spans must be [R, 2]
    with pytest.raises(ValueError):
        score_tokens_f16(ok.cpu(), tg.cpu())
    with pytest.raises(ValueError):
        score_tokens_f16(ok[None], tg)


# ---------------------------------------------------------------- model level
def model_rows(model, ids, vocab_limit=None):
    with torch.no_grad():
        return model(ids).logits[..., :vocab_limit].flatten(0, 1).cpu().numpy()


def test_model_token_logprobs(epi):
    ids = ids_of(80, 51, rows=2)
    B, T = ids.shape
    targets = np.full((B, T), IGNORE)
    targets[:, :-1] = ids[:, 1:].cpu().numpy()
    ref = score_ref(model_rows(epi, ids), targets.reshape(-1))
    for ctx in (torch.no_grad, torch.inference_mode):
        with ctx():
            lp, gr = H.token_logprobs(epi, ids)
        assert lp.shape == (B, T - 1) and lp.dtype == torch.float32 and gr.dtype == torch.bool
        full_lp, full_gr = torch.zeros(B, T, device=DEV), torch.zeros(B, T, dtype=torch.bool, device=DEV)
        full_lp[:, :-1], full_gr[:, :-1] = lp, gr
        check_rows((full_lp.view(-1), full_gr.view(-1)), ref, 1000, ctx.__name__)
    ids9 = ids % 900
    t9 = np.full((B, T), IGNORE)
    t9[:, :-1] = ids9[:, 1:].cpu().numpy()
    ref9 = score_ref(model_rows(epi, ids9, 900), t9.reshape(-1))
    lp, gr = scoring.token_logprobs(epi, ids9, vocab_limit=900)
    full_lp, full_gr = torch.zeros(B, T, device=DEV), torch.zeros(B, T, dtype=torch.bool, device=DEV)
    full_lp[:, :-1], full_gr[:, :-1] = lp, gr
    check_rows((full_lp.view(-1), full_gr.view(-1)), ref9, 900, "vocab_limit=900")
    with pytest.raises(RuntimeError):
        scoring.token_logprobs(epi, ids9 + 100, vocab_limit=900)


@pytest.mark.parametrize("k", [1, 4])
def test_model_loglikelihood(epi, k):
    reqs = requests_of(61, LENGTHS[:8] + [(250, 20)])                # the last one is longer than max_length + 1 = 257
    ctx = [3, 14, 15, 92]
    with torch.no_grad():                                            # one continuation that the model itself decoded
        seq = H.generate(epi, torch.tensor([ctx], device=DEV), max_new_tokens=3)[0].tolist()
    reqs[4] = (ctx, seq[4:])
    got = H.loglikelihood(epi, reqs, batch_size=k)
    assert len(got) == 9 and all(isinstance(s, float) and isinstance(g, bool) for s, g in got)
    seen = []
    for input_ids, targets, spans, idx in scoring._batches(reqs, k, 256, 0):
        ref = score_ref(model_rows(epi, input_ids.to(DEV)), targets.numpy(), spans=spans.numpy())
        for j, i in enumerate(idx):
            b, e = spans[j].tolist()
            tol = sum(bound(1000, ref["lse"][t], ref["xt"][t]) for t in range(b, e))
            assert e - b == len(reqs[i][1]) and abs(got[i][0] - ref["span_sum"][j]) <= tol, (k, i, got[i][0], ref["span_sum"][j], tol)
            assert got[i][1] == bool(ref["span_greedy"][j]), (k, i)
        seen += idx
    assert sorted(seen) == list(range(9))
    assert not all(g for _, g in got)


def test_model_perplexity_fused(epi):
    ids = ids_of(256, 71)
    plain = H.perplexity(epi, ids, 64)
    fused = H.perplexity(epi, ids, 64, fused=True)
    lse = 0.0
    for i in range(4):
        w = ids[:, 64 * i:64 * (i + 1)]
        ref = score_ref(model_rows(epi, w)[:-1], w[0, 1:].cpu().numpy())
        lse = max(lse, float(np.abs(ref["lse"]).max()))
    tol = math.expm1(2 * bound(1000, lse))
    print(f"[perplexity] plain {plain!r} fused {fused!r} rel {abs(fused - plain) / plain:.3e} (tolerance {tol:.3e}, |lse| <= {lse:.2f})")
    assert abs(fused - plain) / plain <= tol
    with torch.inference_mode():
        assert abs(H.perplexity(epi, ids, 64, fused=True) - plain) / plain <= tol
