"""The grouped launches of tests/test_gpu_gemv_persistent.py and tools/record_gemv_golden.py (test infrastructure; numpy only, no
GPU): a few distinct layers on the format's grid (gemv_cfg_cases.build_member), replicated to the members of one
pbl_gemv_f16_grouped launch as bench.py replicates its weight sets, each member at its own device address.

Both launches reach the throughput route (SPLIT = 1, 4 waves per workgroup): that needs max_NRB x members >= 8192, and 128 records
(2048 rows) x 64 members is the smallest such launch.  The members differ in K (512, 640 -- no multiple of a 512-column panel --,
1024) and in N (2048, 2040, 1000), so workgroups past a member's own record count exit, the last record of a member has rows past
N, and neighbouring members stage x of different lengths.  Two sets carry 20 % and 30 % salient weights instead of 5 %: their
records hold about 210 and 165 salient chunks, i.e. 4 and 3 rounds of 64 lanes (an even and an odd number of trips through the
kernel's two-round loop, the last round cut short); the others fit one round.

  MIXED  68 members, 5 sets: fp32 grid plain / with bias and exception entries / with a bias only / small, and one fp16-checkpoint
         (PBL_FLAG_SAL_F16) set -- the launch runs the SF instantiation.  32 groups of 4 records x 68 = 2176 work items.
  PLAIN  64 members, the 4 fp32-grid sets -- the headline (non-SF) instantiation.  32 x 64 = 2048 work items, the fewest a
         throughput launch can have.

Activations: member i multiplies x number i % (2 x sets), so every weight set meets two inputs and neighbouring members -- also the
two neighbouring sets of equal K -- never share one.  (weight set, x) repeat after 2 x sets members: a fixture holds that many
members' outputs and the test compares every member of the launch with it."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from gemv_cfg_cases import build_member


@dataclass(frozen=True)
class SetSpec:
    N: int
    K: int
    sal_f16: bool
    rich: bool            # bias + exception entries (build_member)
    bias_only: bool
    seed: int
    extra_sal: float = 0.0   # further salient weights on top of build_member's 5 %, as a fraction of all weights


@dataclass(frozen=True)
class Launch:
    name: str
    sets: tuple
    members: int

    @property
    def max_NRB(self):
        return max((s.N + 15) // 16 for s in self.sets)

    @property
    def P(self):
        return (max(s.K for s in self.sets) + 511) // 512

    @property
    def items(self):
        """work items of the launch: groups of 4 records of the largest member x members"""
        return (self.max_NRB + 3) // 4 * self.members

    @property
    def period(self):
        """members after which (weight set, x) repeat"""
        return 2 * len(self.sets)

    def set_of(self, member):
        return member % len(self.sets)


A = SetSpec(2048, 1024, False, False, False, 9101, extra_sal=0.15)      # ~210 salient chunks per record: 4 rounds of 64
B = SetSpec(2040, 640, False, True, False, 9102)
C = SetSpec(1000, 512, True, False, False, 9103)
D = SetSpec(2048, 512, False, False, True, 9104, extra_sal=0.25)        # ~165 chunks: 3 rounds, the last one cut short
E = SetSpec(1000, 512, False, False, False, 9105)

MIXED = Launch("mixed68", (A, B, C, D, E), 68)
PLAIN = Launch("plain64", (A, B, D, E), 64)
LAUNCHES = (MIXED, PLAIN)
MS = (1, 4)


def build_set(s: SetSpec) -> dict:
    """build_member's dict for one set (W, hi, lo, ss, sz, sal, bias, exc); bias_only sets get a bias of their own"""
    d = build_member(s.N, s.K, s.seed, s.sal_f16, s.rich)
    if s.extra_sal:
        # more salient weights, on the code grid as build_member's are: sscale (q - 128), q != 128
        assert not s.sal_f16 and not s.rich
        rng = np.random.default_rng(s.seed + 3)
        more = (rng.random((s.N, s.K), dtype=np.float32) < s.extra_sal) & (d["sal"] == 0)
        q = rng.integers(0, 255, (s.N, s.K), dtype=np.uint8).astype(np.float32)
        q += q >= 128
        d["W"][more] = (d["ss"][:, None] * (q - d["sz"][:, None]))[more]
        d["sal"][more] = 1
    if s.bias_only:
        d["bias"] = np.random.default_rng(s.seed + 7).normal(0.0, 0.5, s.N).astype(np.float32)
    return d


def activations(K: int, M: int, j: int) -> np.ndarray:
    """x number j for a member of K columns, [M, K] fp16; the M = 1 input is row 0 of the M = 4 input"""
    from pb_llm_amd import synth
    return synth.activations((4, K), 7700 + j, 3)[:M].copy()


def fixture_name(launch: Launch, M: int) -> str:
    return f"gemv_grouped_{launch.name}_m{M}_parent_de42e4d"


SENTINEL = -1536.0                                      # exact in fp16; no output of these launches comes near it
GAP = 37                                                # elements between two members' outputs in the sentinel-filled buffer


def pack_sets(launch: Launch):
    """[(build_set's dict, host PackedWeight)] per set of the launch"""
    from pb_llm_amd.packing import pack_dense
    out = []
    for s in launch.sets:
        d = build_set(s)
        out.append((d, pack_dense(d["W"], d["hi"], d["lo"], d["ss"], d["sz"], d["sal"], sal_f16=s.sal_f16)))
    return out


def build_group(launch: Launch, packed_sets, M: int, dev):
    """The launch as a GroupedGemv on `dev` with its inputs in place: every member a fresh device copy of its set's blob, x number
    i % period per member, and the outputs redirected into ONE sentinel-filled buffer with GAP elements in front of, between and
    behind the members' [M, N] blocks.  Returns (group, buffer, keep) -- keep: the mask of buffer elements no member owns."""
    import torch
    from pb_llm_amd.runtime import GroupedGemv
    ids = [launch.set_of(i) for i in range(launch.members)]
    packed = [packed_sets[k][1].to(dev) for k in ids]
    assert len({p.blob.data_ptr() for p in packed}) == launch.members
    biases = [None if packed_sets[k][0]["bias"] is None else torch.from_numpy(packed_sets[k][0]["bias"]) for k in ids]
    g = GroupedGemv(packed, biases, M=M, device=dev)
    for i, t in enumerate(g.x):
        t.copy_(torch.from_numpy(activations(launch.sets[ids[i]].K, M, i % launch.period)))
    offs, cur = [], GAP
    for p in packed:
        offs.append(cur)
        cur += M * p.N + GAP
    buf = torch.full((cur,), SENTINEL, dtype=torch.float16, device=dev)
    keep = torch.ones(cur, dtype=torch.bool, device=dev)
    g.y = []
    for o, p in zip(offs, packed):
        g.y.append(buf[o:o + M * p.N].view(M, p.N))
        keep[o:o + M * p.N] = False
    g._y_ptrs = torch.tensor([t.data_ptr() for t in g.y], dtype=torch.int64, device=dev)
    return g, buf, keep
