"""-m gpu: pbl_select_token_f16 at the limits it states -- vocabularies below 1000 words (several of the 16 wave segments empty),
2^19 words (the bound at which the 2^44-scaled weights still sum inside 64 bits), 2^19 + 1 (declined), and more rows than the 64
lanes of the finish kernel.  State, criterion, restatement, parameters and delta are those of test_gpu_sampling.py and
test_sampling_cpu.py, unchanged; no temperature beyond PARAMS (delta was derived for their score ranges)."""
import numpy as np
import pytest
import torch

from pb_llm_amd.runtime import SELECT_MAX_VOCAB, select_token_f16
from test_gpu_decode_attention import built  # noqa: F401  (fixture)
from test_gpu_sampling import DEV, Sel, check_tokens, strided, u_table
from test_sampling_cpu import DELTA, PARAMS, U_LAST, rows16, select_ref

pytestmark = pytest.mark.gpu
N_STEPS = 64


def clear_rows(V, sigma, B, seed0, T, k, p):
    """the rows of the first seed (chosen by the restatement alone) that keep clear of 1 - top_p by more than delta, and their
    restatements"""
    for seed in range(seed0, seed0 + 4000, 100):
        rows = rows16(V, sigma, seed, B)
        refs = [select_ref(r, T, k, p) for r in rows]
        if min(r["slack"] for r in refs) > DELTA:
            break
    assert min(r["slack"] for r in refs) > DELTA, "no seed found: a value's mass lies within delta of 1 - top_p"
    return rows, refs


def run_steps(logits, B, V, T, k, p, us):
    sel = Sel(B, N_STEPS)
    kept = torch.zeros(B, V, dtype=torch.uint8, device=DEV)
    ut = torch.from_numpy(us).to(DEV)
    for _ in range(N_STEPS):
        sel(logits, T, k, p, ut, kept=kept)
    assert int(sel.step) == N_STEPS and int(sel.status) == 0 and int(sel.count) == B
    assert torch.equal(sel.next_ids[:, 0], sel.tokens[:, -1])
    return kept.cpu().numpy().astype(bool), sel.tokens.cpu().numpy()


@pytest.mark.parametrize("T,k,p", PARAMS)
@pytest.mark.parametrize("V", [1, 2, 7, 9, 100, 127, 129])
@pytest.mark.parametrize("sigma", [1, 3])
def test_small_vocabularies(sigma, V, T, k, p):
    for B in (1, 3):                                                       # one row: the vector loads wherever the row is aligned
        rows, refs = clear_rows(V, sigma, B, 7 * V + 31 * B + sigma, T, k, p)
        us = u_table(N_STEPS, B, V + B)
        for layout in ("vec", "odd", "last"):
            got, toks = run_steps(strided(rows, layout), B, V, T, k, p, us)
            for b in range(B):
                assert np.array_equal(got[b], refs[b]["kept"]), f"B={B} {layout} row {b}: kept {np.flatnonzero(got[b])} vs {np.flatnonzero(refs[b]['kept'])}"
                check_tokens(refs[b], toks[b], us[:, b], f"B={B} {layout} row {b}")
            if V == 1:
                assert not toks.any(), "one word: token 0 for every u"


def test_flat_row_of_2_to_the_19_words():
    """every token kept, w = 2^44 each: the total weight is 2^63, the largest the kernel's 64-bit sums are stated to hold"""
    V = SELECT_MAX_VOCAB
    assert V == 1 << 19
    flat = np.zeros((1, V), np.float16)
    us = u_table(N_STEPS, 1, 19)
    assert us[0, 0] == 0.0 and us[1, 0] == np.float32(U_LAST)
    for T, k, p in ((0.7, 50, 0.9), (1.0, 0, 1.0)):
        got, toks = run_steps(strided(flat, "vec"), 1, V, T, k, p, us)
        assert got.all()
        check_tokens(select_ref(flat[0], T, k, p), toks[0], us[:, 0], f"flat row, T={T} k={k} p={p}")


@pytest.mark.parametrize("T,k,p", [(0.7, 50, 0.9), (1.0, 0, 0.9), (1.0, 0, 1.0)])
def test_random_row_of_2_to_the_19_words(T, k, p):
    V = SELECT_MAX_VOCAB
    rows, refs = clear_rows(V, 3, 1, 19, T, k, p)
    us = u_table(N_STEPS, 1, 20)
    for layout in ("vec", "odd"):
        got, toks = run_steps(strided(rows, layout), 1, V, T, k, p, us)
        assert np.array_equal(got[0], refs[0]["kept"]), \
            f"{layout}: kept sets differ at {np.flatnonzero(got[0] != refs[0]['kept'])[:8]} ({got[0].sum()} vs {refs[0]['kept'].sum()} kept)"
        check_tokens(refs[0], toks[0], us[:, 0], layout)


def test_one_word_more_than_2_to_the_19_is_declined():
    V = SELECT_MAX_VOCAB + 1
    logits = torch.zeros(2, V, dtype=torch.float16, device=DEV)
    logits[:, 5] = 1.0
    u = torch.full((1, 2), 0.5, device=DEV)
    for uniforms in (None, u):
        sel = Sel(2, 3, step=1)
        assert select_token_f16(logits, sel.step, sel.unfinished, sel.tokens, 0, sel.next_ids, sel.count, sel.status,
                                temperature=0.7, top_k=50, top_p=0.9, uniforms=uniforms) is None
        torch.cuda.synchronize()
        assert bool((sel.tokens == -7).all()) and bool((sel.next_ids == -7).all()) and int(sel.step) == 1
        assert int(sel.status) == 0 and int(sel.count) == -7 and bool(sel.unfinished.all())


@pytest.mark.parametrize("B", [5, 64, 65])
def test_greedy_rows_beyond_one_wave_of_the_finish_kernel(B):
    V, pad = 1000, 7
    rows = rows16(V, 3, 500 + B, B)
    for r in rows:
        assert int((r == r.max()).sum()) == 1
    top = np.argmax(rows, 1)
    before = [b % 3 != 0 for b in range(B)]                                # finished rows among unfinished ones, on both sides of lane 63
    eos = [int(top[1]), int(top[B - 1]), V + 5]                           # row 1 (unfinished) draws an eos id now
    for layout in ("vec", "odd"):
        logits = strided(rows, layout)
        sel = Sel(B, 4, col0=1, eos=eos, unfinished=before, step=1)
        sel(logits, pad=pad)
        ref = torch.argmax(logits.float(), -1)
        was = torch.tensor(before, device=DEV)
        now = was & ~torch.isin(ref, torch.tensor(eos, device=DEV))
        assert not bool(now[1]) and 0 < int(now.sum()) < int(was.sum())
        assert torch.equal(sel.tokens[:, 2][was], ref[was]), "an unfinished row's token is torch.argmax"
        assert bool((sel.tokens[:, 2][~was] == pad).all()), "a finished row receives the pad id"
        assert torch.equal(sel.next_ids[:, 0], sel.tokens[:, 2]) and bool((sel.tokens[:, [0, 1, 3]] == -7).all())
        assert torch.equal(sel.unfinished, now) and int(sel.count) == int(now.sum())
        assert int(sel.step) == 2 and int(sel.status) == 0
