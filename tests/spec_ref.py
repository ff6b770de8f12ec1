"""numpy restatement of the control plane of prompt-lookup speculative decoding (include/pbl.h: pbl_spec_verify_f16, pbl_ngram_draft),
written from the rules, not from the kernels; test_speculation_cpu.py checks its invariants, test_gpu_speculation.py the kernels
against it (exact integer equality)."""
from dataclasses import dataclass, field

import numpy as np


def argmax_ref(rows: np.ndarray) -> np.ndarray:
    """rule 1 for fp16 rows [..., V]: the lowest index among the maxima, -0 equals +0, a NaN counts as the maximum (numpy's argmax has
    exactly these rules: the first NaN if there is one, else the first maximum by value)"""
    return np.argmax(rows.astype(np.float32), axis=-1).astype(np.int64)


@dataclass
class SpecState:
    """everything pbl_spec_verify_f16 mutates, on the host"""
    ids: np.ndarray                 # [B, S]
    tokens: np.ndarray              # [B, total]
    cursor: int
    unfinished: np.ndarray          # [B] bool
    positions: np.ndarray           # [L]
    count: int = -1
    status: int = 0
    stats: np.ndarray = field(default_factory=lambda: np.zeros(3, np.int64))

    def copy(self):
        return SpecState(self.ids.copy(), self.tokens.copy(), int(self.cursor), self.unfinished.copy(), self.positions.copy(),
                         self.count, self.status, self.stats.copy())


def draft_ref(st: SpecState, max_ngram: int) -> None:
    """pbl_ngram_draft: ids[b][1:] from the history tokens[b, :cursor]"""
    B, S = st.ids.shape
    n = min(max(st.cursor, 0), st.tokens.shape[1])
    for b in range(B):
        h = st.tokens[b, :n].tolist()
        e = 0
        if st.unfinished[b]:
            for N in range(max_ngram, 0, -1):
                ends = [i for i in range(N, n) if h[i - N:i] == h[n - N:n]]      # N <= e < len: an EARLIER occurrence
                if ends:
                    e = ends[-1]
                    break
        ext = list(h)
        for j in range(S - 1):
            ext.append(ext[e + j] if e else int(st.ids[b, 0]))
            st.ids[b, 1 + j] = ext[-1]


def verify_ref(st: SpecState, am: np.ndarray, eos=(), pad: int = 0, max_ngram: int = 0) -> int:
    """pbl_spec_verify_f16 on the arg-maxes am [B, S]; returns n (-1 for the no-op of rule 5)"""
    B, S = st.ids.shape
    total = st.tokens.shape[1]
    live = [b for b in range(B) if st.unfinished[b]]
    c = st.cursor
    if c < 1 or c > total:
        st.status |= 2
    if c < 1 or c >= total or not live:
        st.positions -= S
        st.count = len(live)
        return -1
    n = S - 1
    for b in live:
        nb = 0
        while nb < S - 1 and st.ids[b, nb + 1] == am[b, nb]:
            nb += 1
        n = min(n, nb)
    w = min(n + 1, total - c)
    for b in range(B):
        for j in range(w):
            tok = int(am[b, j]) if st.unfinished[b] else pad
            if st.unfinished[b] and tok in eos:
                st.unfinished[b] = False
            st.tokens[b, c + j] = tok
        st.ids[b, 0] = st.tokens[b, c + w - 1]
    st.cursor = c + w
    st.count = int(st.unfinished.sum())
    st.stats += np.array([1, w - 1, w])
    st.positions -= S - 1 - n
    if max_ngram >= 1 and S > 1:
        draft_ref(st, max_ngram)
    return n


def one_token_loop(next_token, prompt: np.ndarray, total: int, eos=(), pad: int = 0) -> np.ndarray:
    """the loop speculation must reproduce: one greedy token per row and step, eos / pad as pbl_select_token_f16 books them; runs to
    `total` columns (generate cuts the result after the column at which the last row finished)"""
    B, P = prompt.shape
    tokens = np.zeros((B, total), np.int64)
    tokens[:, :P] = prompt
    unfinished = np.ones(B, bool)
    for c in range(P, total):
        if not unfinished.any():
            break
        for b in range(B):
            tok = next_token(tokens[b, :c]) if unfinished[b] else pad
            if unfinished[b] and tok in eos:
                unfinished[b] = False
            tokens[b, c] = tok
    return tokens


def cut_ref(tokens: np.ndarray, P: int, eos=()) -> np.ndarray:
    """what generate returns of a result buffer: cut after the column at which the last row finished"""
    done = 0
    for row in tokens[:, P:]:
        hits = [i for i, t in enumerate(row.tolist()) if t in eos]
        done = max(done, hits[0] + 1 if hits else len(row))
    return tokens[:, :P + done]


def speculative_loop(next_token, prompt: np.ndarray, total: int, K: int, max_ngram: int, eos=(), pad: int = 0, drafter=None):
    """the session's loop on the host: the first token, the first drafts, then steps of 1 + K rows whose arg-maxes come from
    next_token over the row's history extended by the drafts.  drafter(state): overwrite the n-gram drafts (any drafts do).
    Returns (tokens, stats, steps' n)"""
    B, P = prompt.shape
    tokens = np.zeros((B, total), np.int64)
    tokens[:, :P] = prompt
    st = SpecState(np.zeros((B, 1 + K), np.int64), tokens, P, np.ones(B, bool), np.full(3, P, np.int64))
    for b in range(B):
        tok = next_token(tokens[b, :P])
        st.unfinished[b] = tok not in eos
        tokens[b, P] = st.ids[b, 0] = tok
    st.cursor = P + 1
    draft_ref(st, max_ngram)
    ns = []
    while st.cursor < total and st.unfinished.any():
        if drafter is not None:
            drafter(st)
        st.positions += 1 + K                                                    # the forward pass
        am = np.zeros((B, 1 + K), np.int64)
        for b in range(B):
            hist = st.tokens[b, :st.cursor].tolist()                             # ends with ids[b][0]
            for s in range(1 + K):
                am[b, s] = next_token(np.array(hist + st.ids[b, 1:1 + s].tolist()))
        ns.append(verify_ref(st, am, eos, pad, max_ngram))
        # (a run clamped at `total` leaves the positions of its unwritten tokens behind: the generation is over)
        assert st.cursor == total or (st.positions == st.cursor - 1).all(), "the cache holds every emitted token but the last"
    return st.tokens, st.stats, ns
