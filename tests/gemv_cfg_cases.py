"""The case table of tests/test_gpu_gemv_configs.py and the builder of its layers (test infrastructure; plain numpy, no GPU).

pbl_gemv_kernel<MB, WPB, SF, SPLIT, XB, XP> is instantiated per launch from the record count (16 rows each) and from
P = ceil(K / 512); libpbl's pbl_gemv_route is the authority on which (SPLIT, WPB) a shape gets, and test_gemv_routes_cpu.py asks
it for every row below -- the `split` / `wpb` / `via` columns here are what the table CLAIMS to reach, checked there, so a retuned
threshold fails that test instead of silently thinning the GPU grid.

  via "P"        the split is capped by the panel count (2 at P = 1, 4 at P = 2 or 3, 8 from P = 4): few records
  via "records"  the split is set by the record count (4 from 2048 records, 2 from 4096, 1 from 8192) at a P that would allow more

SPLIT = 1 with WPB = 1 does not exist (fewer than 8192 records always split, more run 4 waves per workgroup): no row.

`rich` rows carry a bias, exception entries (one of them in the last record) and an N that is not a multiple of 16; there is one
per SPLIT value and family.  The layers are built directly on the format's grid (random signs on per-row hi / lo, random 8-bit
codes at about 5 % random positions), never through the oracle's quantiser: a 131067-row layer is set up in seconds.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class Case:
    name: str
    Ns: tuple          # out_features of every member (one entry: a single-layer case)
    K: int
    split: int         # what the case claims to reach ...
    wpb: int
    via: str           # ... and through which of pick_split's two limits ("P" / "records")
    rich: bool = False

    @property
    def P(self) -> int:
        return (self.K + 511) // 512

    @property
    def max_NRB(self) -> int:
        return max((n + 15) // 16 for n in self.Ns)

    @property
    def records(self) -> int:
        """what the split rule counts: the layer's records, or members x the largest member's"""
        return self.max_NRB * len(self.Ns)

    @property
    def large(self) -> bool:
        return self.records >= 1024


SINGLE = [
    Case("s2_p1", (40,), 512, 2, 2, "P"),
    Case("s2_p1_rich", (33,), 203, 2, 2, "P", rich=True),            # K % 8 != 0: every staging path's scalar form
    Case("s4_p2_rich", (100,), 1000, 4, 4, "P", rich=True),
    Case("s4_p3", (48,), 1408, 4, 4, "P"),
    Case("s8_p4", (48,), 2048, 8, 8, "P"),
    Case("s8_p9_rich", (33,), 4104, 8, 8, "P", rich=True),
    Case("s4_records", (32768,), 520, 4, 4, "records"),
    Case("s2_records", (65536,), 520, 2, 2, "records"),
    Case("s1_wpb4_rich", (131067,), 64, 1, 4, "records", rich=True),
]

FUSED = [
    Case("f2_p1_rich", (96, 150), 512, 2, 2, "P", rich=True),
    Case("f4_p2_rich", (96, 157), 1001, 4, 4, "P", rich=True),        # K % 8 != 0
    Case("f4_p2", (256, 64, 64), 1024, 4, 4, "P"),
    Case("f8_p4_rich", (256, 64, 61), 2048, 8, 8, "P", rich=True),
    Case("f4_records", (16384, 4096, 4096), 520, 4, 4, "records"),
    Case("f2_records", (32768, 8192), 520, 2, 2, "records"),
    Case("f1_wpb4_rich", (65536, 8192, 8187), 64, 1, 4, "records", rich=True),
]

# every configuration the grid must reach, per family: (split, wpb) -> the `via` values wanted
WANTED = {(8, 8): {"P"}, (4, 4): {"P", "records"}, (2, 2): {"P", "records"}, (1, 4): {"records"}}

SALIENT_FRACTION = 0.05


def build_member(N: int, K: int, seed: int, sal_f16: bool, rich: bool) -> dict:
    """One layer on the format's grid.  Returns W [N, K] fp32 (what the blob must decode to), hi, lo, sscale, szero [N], the
    salient mask [N, K] uint8, bias [N] fp32 or None, and the (row, col) of the exception entries.

    Binarized weights: per-row levels mu +- alpha with alpha in [0.005, 0.015]; salient weights: sscale (q - 128) with codes
    q != 128 and sscale in [2e-4, 4e-4], i.e. within +-0.051.  sal_f16: levels and salient values on fp16's grid (an fp16
    checkpoint), else on fp32's.  A unit-variance activation row then gives |y| of a few units at the largest K of the table,
    which the residual tests rely on (see test_gpu_gemv_configs.py)."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.005, 0.015, N).astype(np.float32)
    mu = rng.uniform(-0.002, 0.002, N).astype(np.float32)
    hi, lo = mu + alpha, mu - alpha
    ss = rng.uniform(2e-4, 4e-4, N).astype(np.float32)
    sz = np.full(N, 128.0, np.float32)
    if sal_f16:
        hi, lo = hi.astype(np.float16).astype(np.float32), lo.astype(np.float16).astype(np.float32)
    sal = rng.random((N, K), dtype=np.float32) < SALIENT_FRACTION
    W = np.where(rng.integers(0, 2, (N, K), dtype=np.uint8).astype(bool), hi[:, None], lo[:, None]).astype(np.float32)
    q = rng.integers(0, 255, (N, K), dtype=np.uint8).astype(np.float32)
    q += q >= 128                                                        # 0 .. 255 without 128
    vals = ss[:, None] * (q - sz[:, None])                               # fp32, the packer's own expression
    if sal_f16:
        vals = vals.astype(np.float16).astype(np.float32)
    W[sal] = vals[sal]
    del q, vals
    bias, exc = None, []
    if rich:
        bias = rng.normal(0.0, 0.5, N).astype(np.float32)
        n_exc = 2 + seed % 4                                             # 2 .. 5, as tests/test_gpu_pack.py makes them:
        for e in range(n_exc):                                           # values on neither level nor the code grid
            r, c = ((7 * e) % N, (131 * e + 5) % K) if e else (N - 1, K - 1)     # (the first one sits in the last record)
            v = np.float32(0.123 + 0.01 * e)
            W[r, c] = np.float32(np.float16(v)) if sal_f16 else v
            exc.append((r, c))
    return dict(W=W, hi=hi, lo=lo, ss=ss, sz=sz, sal=sal.astype(np.uint8), bias=bias, exc=exc)


def seed_of(case: Case, member: int, sal_f16: bool) -> int:
    """a stable seed per (case, member, form)"""
    return 1000 * (SINGLE + FUSED).index(case) + 10 * member + int(sal_f16)
