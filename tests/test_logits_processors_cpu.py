"""-m "not gpu": the logits processors on the device (pbl_process_logits_f16, pbl_select_token_minp_f16; harness.generate with
repetition_penalty / no_repeat_ngram_size / min_new_tokens / min_length / min_p).  The restatement that the GPU tests
(test_gpu_logits_processors.py) compare against lives here -- process_ref for the three processors, select_ref_minp for min_p -- and is
checked against HF's own processor classes; the C entries are declared, exported, documented and refuse bad arguments before any
device work; the resolution of the five parameters is checked against what model.generate itself builds."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import torch

from pb_llm_amd import _lib
from test_decode_attention_cpu import tiny_llama
from test_sampling_cpu import rows16, select_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 2.0 ** -16                 # of exp(s - max s) / min_p around 1: s and max s carry one fp32 rounding each (|s| < 64: at most 2^-19
                                  # each), the subtraction another, so the exponent's argument is off by at most 1.5 * 2^-18; expf adds a
                                  # few ulp (2^-23 each).  2^-16 leaves more than a factor of two (derived, not measured)
MINP_PARAMS = [(1.0, 0, 1.0, 0.05), (0.7, 50, 0.9, 0.1), (1.3, 0, 0.95, 0.02), (1.0, 0, 1.0, 0.5)]


# ---------------------------------------------------------------- the restatement
def process_ref(row16, hist, theta=1.0, n=0, eos=(), block_eos=False):
    """Rules 1-3 of pbl_process_logits_f16 on one row of fp16 logits over the history `hist` (a sequence of ids): the penalty in
    fp32 (x < 0 ? x theta : x / theta, IEEE division) once per distinct id and rounded to fp16, then -inf for every token that
    would complete an n-gram the history already holds, then -inf for the eos ids while block_eos.  Ids outside [0, V) are skipped.
    Returns the processed fp16 row."""
    out = np.array(row16, np.float16)
    V, h = out.size, [int(t) for t in hist]
    if theta != 1.0:
        ids = np.array(sorted({t for t in h if 0 <= t < V}), np.int64)
        x = out[ids].astype(np.float32)
        with np.errstate(over="ignore"):
            out[ids] = np.where(x < 0, x * np.float32(theta), x / np.float32(theta)).astype(np.float16)
    if n > 0 and len(h) >= n:
        suffix = h[len(h) - (n - 1):]
        for i in range(len(h) - n + 1):
            if h[i:i + n - 1] == suffix and 0 <= h[i + n - 1] < V:
                out[h[i + n - 1]] = -np.inf
    if block_eos:
        for t in eos:
            if 0 <= int(t) < V:
                out[int(t)] = -np.inf
    return out


def select_ref_minp(logits16, T, k, p, min_p, u=None):
    """select_ref with rule 4 behind top-k and top-p: a kept token stays iff exp(s - max s) >= min_p.  Adds `band`: the smallest
    |exp(s - max s) / min_p - 1| over the row (inf with min_p = 0) -- a value inside BAND may go either way in fp32 --, and
    `open_block`: top-p's boundary value is shared by several tokens that min_p does not remove (HF cuts such a block of ties at an
    arbitrary place, rule 3 of pbl_select_token_f16 keeps it whole: test_sampling_cpu.py; only there can the two kept sets differ
    for a reason that is not min_p's)."""
    r = select_ref(logits16, T, k, p)
    if min_p <= 0:
        return dict(select_ref(logits16, T, k, p, u), band=np.inf, open_block=False)
    s = (np.asarray(logits16, np.float16).astype(np.float32) / np.float32(T)).astype(np.float64)
    ratio = np.exp(s - s.max())
    kept = r["kept"] & (ratio >= min_p)
    w = np.where(kept, ratio, 0.0)
    prefix = np.cumsum(w)
    W = float(prefix[-1])
    token = None
    if u is not None:
        above = np.flatnonzero(prefix > u * W)
        token = int(above[0]) if len(above) else int(np.flatnonzero(kept)[-1])
    low = s[r["kept"]].min()
    open_block = p < 1 and int((s[r["kept"]] == low).sum()) > 1 and bool(np.exp(low - s.max()) >= min_p)
    return dict(kept=kept, token=token, prefix=prefix, W=W, slack=r["slack"], band=float(np.abs(ratio / min_p - 1).min()),
                open_block=open_block)


def history(row16, length, n, seed):
    """a history of `length` ids for a row: random ids, the row's top tokens among them (twice each, far apart), and its last
    n - 1 tokens copied from an earlier place so that the n-gram rule bans the token behind that place -- one of the top tokens"""
    rng = np.random.default_rng(seed)
    V = row16.size
    h = rng.integers(0, V, length)
    top = np.argsort(row16.astype(np.float32))[::-1][:4]
    h[[3, length // 2]] = top[0]
    h[[7, length - 9]] = top[1]
    h[11] = top[2]
    if n > 1 and length >= 40:
        h[length - (n - 1):] = h[20:20 + n - 1]
        h[20 + n - 1] = top[seed % 4]
    return h


# ---------------------------------------------------------------- against HF's processors
def hf_processed(rows16, hists, theta, n, eos, prompt_len, min_new):
    """HF's three processors on the fp32 copy of the rows (one history per row, equal lengths), in model.generate's order"""
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)
    scores = torch.from_numpy(rows16.astype(np.float32))
    ids = torch.from_numpy(np.asarray(hists, np.int64))
    if theta != 1.0:
        scores = RepetitionPenaltyLogitsProcessor(float(theta))(ids, scores)
    if n > 0:
        scores = NoRepeatNGramLogitsProcessor(n)(ids, scores)
    if min_new > 0:
        scores = MinNewTokensLengthLogitsProcessor(prompt_len, min_new, list(eos))(ids, scores)
    return scores.numpy()


@pytest.mark.parametrize("theta", [1.1, 1.3, 2.0])
@pytest.mark.parametrize("sigma", [1, 3])
def test_restatement_equals_hf_processors_rounded_to_fp16(sigma, theta):
    V, L, n, R = 32000, 140, 3, 300
    rows = rows16(V, sigma, 77 + sigma, R)
    hists = [history(rows[r], L, n, r) for r in range(R)]
    eos = [int(np.argmax(rows[0])), 5]
    near = 0
    for block, min_new in ((slice(0, 150), 0), (slice(150, 300), 8)):       # the second half: 140 - 136 = 4 new tokens < 8, eos blocked
        hf = hf_processed(rows[block], hists[block], theta, n, eos, 136, min_new)
        hf16 = hf.astype(np.float16)
        for j, r in enumerate(range(block.start, block.stop)):
            ref = process_ref(rows[r], hists[r], theta, n, eos, block_eos=min_new > 0)
            assert np.array_equal(ref.view(np.uint16), hf16[j].view(np.uint16)), \
                f"row {r}: bits differ at {np.flatnonzero(ref.view(np.uint16) != hf16[j].view(np.uint16))[:8]}"
            assert np.isneginf(ref).sum() >= 1 and (ref != rows[r]).sum() >= 3        # a ban and the penalties took place
            top2 = np.sort(hf[j])[-2:]
            spacing = 2.0 ** (np.floor(np.log2(abs(float(top2[1])))) - 10)
            if top2[1] - top2[0] > 2 * spacing:
                assert int(np.argmax(ref.astype(np.float32))) == int(np.argmax(hf[j])), f"row {r}: the arg-max differs"
            else:
                near += 1
    print(f"[process_ref vs HF] sigma={sigma} theta={theta}: {near} of {R} rows excluded as near ties")
    assert near <= R // 10, f"{near} of {R} rows are near ties"


def test_restatement_limits():
    row = rows16(500, 2, 3)[0]
    assert np.array_equal(process_ref(row, [], 1.3, 3, [4], False).view(np.uint16), row.view(np.uint16))      # an empty history
    one = process_ref(row, [7, 7, 7, -1, 500], 2.0)                                                        # once per distinct id
    x = np.float32(row[7])
    assert one[7] == np.float16(x * np.float32(2) if x < 0 else x / np.float32(2)) and (np.delete(one, 7) == np.delete(row, 7)).all()
    assert np.isneginf(process_ref(row, [1, 2, 3], 1.0, 1)[[1, 2, 3]]).all()                                # n = 1: every id
    assert not np.isneginf(process_ref(row, [1, 2], 1.0, 3)).any()                                         # len = n - 1: no window
    banned = process_ref(row, [1, 2, 9, 4, 1, 2], 1.0, 3)
    assert np.flatnonzero(np.isneginf(banned)).tolist() == [9]
    both = process_ref(row, [1, 2, 9, 4, 1, 2], 0.5, 3)                                                    # penalised and banned
    assert np.isneginf(both[9]) and both[1] != row[1]
    assert np.flatnonzero(np.isneginf(process_ref(row, [1], 1.0, 0, [4, 600, -2], True))).tolist() == [4]


def hf_kept_minp(row16, T, k, p, min_p):
    from transformers.generation.logits_process import MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    scores = torch.from_numpy(row16.astype(np.float32))[None]
    if T != 1.0:
        scores = TemperatureLogitsWarper(T)(None, scores)
    if k:
        scores = TopKLogitsWarper(k)(None, scores)
    if p < 1.0:
        scores = TopPLogitsWarper(p)(None, scores)
    return torch.isfinite(MinPLogitsWarper(min_p)(None, scores))[0].numpy()


@pytest.mark.parametrize("T,k,p,min_p", MINP_PARAMS)
@pytest.mark.parametrize("sigma", [1, 3])
def test_min_p_keeps_what_hf_keeps(sigma, T, k, p, min_p):
    used, seed, in_band, open_blocks = 0, 5000 * sigma, 0, 0
    while used < 50:
        row = rows16(32000, sigma, seed)[0]
        seed += 1
        ref = select_ref_minp(row, T, k, p, min_p)
        if ref["band"] <= BAND:                          # decided by the restatement alone
            in_band += 1
        elif ref["open_block"]:                          # top-p's tie rule, not min_p's: see select_ref_minp
            open_blocks += 1
        else:
            used += 1
            assert np.array_equal(ref["kept"], hf_kept_minp(row, T, k, p, min_p)), f"seed {seed - 1}"
            assert ref["kept"][np.argmax(row)]
        # the band holds a grid point of spacing >= 2^-11 / T with probability under 2 * 2^-16 * 2^11 T = T / 16 per row: at most a
        # quarter of the rows; an open block is the rule where top-p cuts inside the bulk of the row and min_p lies below the cut
        assert in_band <= 5 + (used + in_band + open_blocks) // 4, f"{in_band} rows inside the band"
        assert seed < 5000 * sigma + 400, f"{open_blocks} rows with an open block of ties at top-p's boundary, {in_band} inside the band"
    print(f"[min_p vs HF] sigma={sigma} T={T} k={k} p={p} min_p={min_p}: 50 rows used, {in_band} skipped inside the band, "
          f"{open_blocks} skipped for an open block of ties at top-p's boundary")
    assert p < 1 or open_blocks == 0
    zero = select_ref_minp(row, T, k, p, 0.0, 0.3)
    plain = select_ref(row, T, k, p, 0.3)
    assert np.array_equal(zero["kept"], plain["kept"]) and zero["token"] == plain["token"]


# ---------------------------------------------------------------- the C ABI
def test_entries_are_declared_exported_and_documented():
    hdr = open(os.path.join(REPO, "include", "pbl.h")).read()
    for name in ("pbl_process_logits_f16", "pbl_select_token_minp_f16"):
        assert re.search(rf"^int\s+{name}\s*\(", hdr, re.M), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
        for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
            assert name in open(os.path.join(REPO, doc)).read(), (name, doc)
    import __graft_entry__ as g
    assert any(s.endswith("pbl_logits.hip") for s in g._lib_sources()[0])


def test_process_logits_declines_before_any_launch():
    L = _lib.lib()
    V = (1 << 19) + 8                                   # never a launchable shape: a missed check answers UNSUPPORTED, not a launch
    logits = (C.c_uint16 * (2 * V))()
    tokens = (C.c_int64 * 16)()
    scratch = (C.c_uint16 * 16)()
    step, eos = (C.c_int64 * 1)(), (C.c_int64 * 2)()

    def call(**over):
        a = dict(logits=C.addressof(logits), ld=V, B=2, V=V, tokens=C.addressof(tokens), total=8, col0=2, step=C.addressof(step), theta=1.2,
                 n=3, min_new=4, min_length=0, eos=C.addressof(eos), n_eos=2, scratch=C.addressof(scratch))
        a.update(over)
        return L.pbl_process_logits_f16(a["logits"], a["ld"], a["B"], a["V"], a["tokens"], a["total"], a["col0"], a["step"], a["theta"], a["n"],
                                        a["min_new"], a["min_length"], a["eos"], a["n_eos"], a["scratch"], None)

    UNS, INV = _lib.PBL_ERR_UNSUPPORTED, _lib.PBL_ERR_INVALID_ARG
    assert call() == UNS
    assert call(eos=None, n_eos=0) == UNS and call(theta=1.0, scratch=None) == UNS          # what may be NULL
    assert call(total=1 << 31, col0=2) == UNS
    for name in ("logits", "tokens", "step", "scratch"):
        assert call(**{name: None}) == INV, name
    assert call(eos=None) == INV                                                             # n_eos = 2 without ids
    for bad in (dict(B=0), dict(V=0), dict(ld=V - 1), dict(total=0), dict(col0=8), dict(col0=-1), dict(n_eos=-1), dict(n=-1), dict(n=9),
                dict(theta=0.0), dict(theta=-1.0), dict(theta=float("nan"))):
        assert call(**bad) == INV, bad
    assert call(tokens=C.addressof(logits)) == INV                                           # the output over an input
    assert call(step=C.addressof(logits) + 64) == INV
    assert call(scratch=C.addressof(tokens)) == INV
    assert call(scratch=C.addressof(logits)) == INV                                          # the two outputs over each other


def test_select_token_minp_declines_before_any_launch():
    L = _lib.lib()
    V = (1 << 19) + 8
    logits = (C.c_uint16 * (2 * V))()
    u = (C.c_float * 64)()
    tokens = (C.c_int64 * 64)()
    small = [(C.c_int64 * 8)() for _ in range(6)]
    step, eos, unf, nxt, cnt, status = (C.addressof(b) for b in small)

    def call(min_p, **over):
        a = dict(logits=C.addressof(logits), tokens=C.addressof(tokens), T=0.7, col0=2)
        a.update(over)
        return L.pbl_select_token_minp_f16(a["logits"], V, 2, V, a["T"], 50, 0.9, min_p, C.addressof(u), 4, step, eos, 1, 0, unf, a["tokens"],
                                           8, a["col0"], nxt, cnt, status, None, None)

    UNS, INV = _lib.PBL_ERR_UNSUPPORTED, _lib.PBL_ERR_INVALID_ARG
    assert call(0.0) == call(0.05) == call(1.0) == UNS
    for bad in (-0.1, 1.5, float("nan")):
        assert call(bad) == INV, bad
    assert call(0.1, logits=None) == INV and call(0.1, T=0.0) == INV and call(0.1, col0=8) == INV      # the old checks hold
    assert call(0.1, tokens=C.addressof(logits)) == INV


def test_runtime_wrappers_check_their_arguments():
    from pb_llm_amd import runtime as R
    assert R.process_logits_ok(1, 32000) and R.process_logits_ok(4, 1 << 19, 4096) and not R.process_logits_ok(1, (1 << 19) + 1)
    assert not R.process_logits_ok(0, 100) and not R.process_logits_ok(1, 100, 1 << 31)
    z = lambda *s, dt=torch.int64: torch.zeros(*s, dtype=dt)
    with pytest.raises(ValueError):                                           # host tensors
        R.process_logits_f16(torch.zeros(2, 100, dtype=torch.float16), z(2, 8), 0, z(1), repetition_penalty=1.2,
                             scratch=z(2, 8, dt=torch.float16))
    with pytest.raises(ValueError):
        R.select_token_f16(torch.zeros(2, 100, dtype=torch.float16), z(1), z(2, dt=torch.bool), z(2, 8), 0, z(2), z(1, dt=torch.int32),
                           z(1, dt=torch.int32), min_p=0.1)


# ---------------------------------------------------------------- generate on the host; parameter resolution
def test_generate_on_a_host_model_hands_the_processors_over():
    from pb_llm_amd import harness as H
    model = tiny_llama()
    ids = torch.randint(0, 97, (2, 6), generator=torch.Generator().manual_seed(2))
    calls = []
    orig = model.generate
    model.generate = lambda *a, **k: (calls.append(k), orig(*a, **k))[1]
    out = H.generate(model, ids, max_new_tokens=3, repetition_penalty=1.2)
    assert out.shape == (2, 9) and calls[0] == dict(max_new_tokens=3, repetition_penalty=1.2)
    H.generate(model, ids, max_new_tokens=3, do_sample=True, min_p=0.1, no_repeat_ngram_size=2, min_new_tokens=2, eos_token_id=5)
    assert calls[1] == dict(max_new_tokens=3, do_sample=True, min_p=0.1, no_repeat_ngram_size=2, min_new_tokens=2, eos_token_id=5)
    with pytest.raises(ValueError, match="uniforms"):
        H.generate(model, ids, max_new_tokens=3, do_sample=True, repetition_penalty=1.2, uniforms=torch.rand(3, 2))
    assert len(calls) == 2


def hf_processor_params(model, ids, **kw):
    """(repetition_penalty, no_repeat_ngram_size, min_new_tokens, min_length, min_p) of the processors model.generate builds for
    do_sample=True with an eos id (1.0 / 0 / 0 / 0 / 0.0 where it builds none)"""
    from transformers.generation import logits_process as LP
    seen = []
    orig = model._get_logits_processor

    def spy(*a, **k):
        out = orig(*a, **k)
        seen.append(list(out))
        return out

    model._get_logits_processor = spy
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model.generate(ids, do_sample=True, max_new_tokens=12, eos_token_id=5, pad_token_id=0, **kw)
    finally:
        del model._get_logits_processor
    got = [1.0, 0, 0, 0, 0.0]
    for proc in seen[0]:
        if isinstance(proc, LP.RepetitionPenaltyLogitsProcessor):
            got[0] = float(proc.penalty)
        elif isinstance(proc, LP.NoRepeatNGramLogitsProcessor):
            got[1] = int(proc.ngram_size)
        elif isinstance(proc, LP.MinNewTokensLengthLogitsProcessor):
            got[2] = int(proc.min_new_tokens)
        elif isinstance(proc, LP.MinLengthLogitsProcessor):
            got[3] = int(proc.min_length)
        elif isinstance(proc, LP.MinPLogitsWarper):
            got[4] = float(proc.min_p)
        else:
            assert isinstance(proc, (LP.TemperatureLogitsWarper, LP.TopKLogitsWarper, LP.TopPLogitsWarper)), type(proc).__name__
    return tuple(got)


def test_processor_params_follow_model_generate():
    from pb_llm_amd import harness as H
    from pb_llm_amd import decoding as D
    model = tiny_llama()
    ids = torch.randint(0, 97, (1, 4), generator=torch.Generator().manual_seed(3))
    P = ids.shape[1]
    resolve = lambda **kw: D._processor_params(model, P, **kw)
    assert resolve() == hf_processor_params(model, ids) == (1.0, 0, 0, 0, 0.0)                 # transformers' defaults: all off
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=6, min_p=0.05)
    assert resolve(**kw) == hf_processor_params(model, ids, **kw) == (1.3, 3, 6, P + 6, 0.05)  # min_new_tokens sets min_length
    kw = dict(min_length=9, repetition_penalty=0.8)
    assert resolve(**kw) == hf_processor_params(model, ids, **kw) == (0.8, 0, 0, 9, 0.0)
    gc = model.generation_config
    gc.repetition_penalty, gc.no_repeat_ngram_size, gc.min_length, gc.min_p = 1.1, 2, 7, 0.1     # the model's own config
    assert resolve() == hf_processor_params(model, ids) == (1.1, 2, 0, 7, 0.1)
    kw = dict(repetition_penalty=1.5, min_p=0.2)                                                # an argument wins over the config
    assert resolve(**kw) == hf_processor_params(model, ids, **kw) == (1.5, 2, 0, 7, 0.2)
    assert "_processor_params" in H.generate.__doc__


# ---------------------------------------------------------------- generate: routing of the processor arguments
@pytest.fixture
def routed(monkeypatch):
    """test_speculation_cpu's Recorder in DecodeSession's place, keeping what begin_selection is given"""
    from pb_llm_amd import decoding
    from test_speculation_cpu import Recorder

    class KwRecorder(Recorder):
        def begin_selection(self, prompt, total, **kw):
            self.calls.append(("begin_selection", total, kw))

    Recorder.made = []
    monkeypatch.setattr(decoding, "DecodeSession", KwRecorder)
    model = tiny_llama().half()                                                  # max_position_embeddings = 64
    model.generation_config.eos_token_id = None
    model.generate = lambda *a, **k: ("handed over", k)
    return decoding, model, Recorder


def processors_of(kw):
    return tuple(kw[k] for k in ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "min_length", "min_p"))


def test_prompt_lookup_that_is_not_speculated_runs_without_processors(routed):
    """K = 0 (three or four rows, or no slack below max_position_embeddings): the one-token loop, and max_matching_ngram_size must not
    reach it as a no-repeat n-gram size"""
    from test_speculation_cpu import FakeIds
    decoding, model, Recorder = routed
    for B, kw in ((3, dict(max_new_tokens=20, prompt_lookup_num_tokens=4, max_matching_ngram_size=3)),
                  (4, dict(max_new_tokens=20, prompt_lookup_num_tokens=4)),
                  (1, dict(max_new_tokens=58, prompt_lookup_num_tokens=3, max_matching_ngram_size=4)),
                  (1, dict(max_new_tokens=20, max_matching_ngram_size=3)),
                  (1, dict(max_new_tokens=20))):
        assert decoding.generate(model, FakeIds(B, 5), **kw) == "selected", kw
        name, _, got = Recorder.made[-1].calls[0]
        assert name == "begin_selection" and processors_of(got) == (1.0, 0, 0, 0, 0.0), (kw, got)


def test_generate_routes_the_processor_arguments(routed):
    from test_speculation_cpu import FakeIds
    decoding, model, Recorder = routed
    ids = FakeIds(1, 5)
    kw = dict(max_new_tokens=20, eos_token_id=3, repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=4)
    assert decoding.generate(model, ids, **kw) == "selected"
    assert processors_of(Recorder.made[-1].calls[0][2]) == (1.2, 3, 4, 9, 0.0)           # min_new_tokens sets min_length = P + 4
    assert decoding.generate(model, ids, do_sample=True, min_p=0.1, no_repeat_ngram_size=8, max_new_tokens=20) == "selected"
    assert processors_of(Recorder.made[-1].calls[0][2]) == (1.0, 8, 0, 0, 0.1)
    n = len(Recorder.made)
    for over in (dict(no_repeat_ngram_size=9),                                           # beyond the kernel's window
                 dict(no_repeat_ngram_size=2, prompt_lookup_num_tokens=3),              # the verify kernel takes the raw arg-max
                 dict(repetition_penalty=1.1, prompt_lookup_num_tokens=3),
                 dict(min_new_tokens=4, eos_token_id=3, prompt_lookup_num_tokens=3),
                 dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(no_repeat_ngram_size=-1),      # HF raises for these
                 dict(min_p=0.1)):                                                      # a sampling argument without do_sample
        out, got = decoding.generate(model, ids, max_new_tokens=20, **over)
        assert out == "handed over" and got == dict(max_new_tokens=20, **over), over
    out, got = decoding.generate(model, ids, max_new_tokens=20, do_sample=True, min_p=1.5)
    assert out == "handed over" and got["min_p"] == 1.5
    assert len(Recorder.made) == n, "a session was built for a call that is handed over"
    # a minimum length without an eos id processes nothing (HF builds no processor): prompt lookup still speculates
    assert decoding.generate(model, ids, max_new_tokens=20, min_new_tokens=4, prompt_lookup_num_tokens=3) == "speculated"
    model.generation_config.repetition_penalty = 1.3                                      # the model's own config counts
    out, got = decoding.generate(model, ids, max_new_tokens=20, prompt_lookup_num_tokens=3)
    assert out == "handed over" and got == dict(max_new_tokens=20, prompt_lookup_num_tokens=3)
    assert decoding.generate(model, ids, max_new_tokens=20) == "selected"
    assert processors_of(Recorder.made[-1].calls[0][2])[0] == 1.3
    single = tiny_llama()                                                                 # fp32 logits: the kernel takes fp16
    single.generate = model.generate
    out, got = decoding.generate(single, ids, max_new_tokens=20, repetition_penalty=1.2)
    assert out == "handed over" and got == dict(max_new_tokens=20, repetition_penalty=1.2)
