"""The launches of tests/test_gpu_gemv_lookahead.py (and, through --cases, of tools/record_gemv_golden.py): the panel and salient
round counts at which the decode GEMV's lookahead loops begin, wrap and end (test infrastructure; numpy only, no GPU).

The one-token code-mode instantiations of pbl_gemv_kernel walk a record's 512-column panels over a ring of three tile register
sets: whole trips of three panels while every request exists (p0 + 4 < P), then a second loop for the last one to four panels.
The salient chunks go in rounds of 64 over two register sets, two rounds per trip.  gemv_persistent_cases.py holds 1 and 2 panels
and 1, 3 and 4 rounds; the ring's edges lie elsewhere.

  RING    one grouped launch on the throughput route (SPLIT = 1, 4 waves per workgroup; 128 records x 64 members = 8192): N = 2048,
          five sets of K = 1536, 2048, 2304 (no multiple of 512), 3584 and 4096, i.e. 3, 4, 5, 7 and 8 panels -- the second loop
          alone for one whole trip (3) and for a trip and a panel (4), one whole trip of the first loop followed by 2 and by 4
          panels of the second (5, 7), and two trips of the first loop, i.e. its back edge, followed by 2 panels (8: the
          benchmark's shape) -- whose records hold 2, 5, 6, 7 and 4 salient rounds (even and odd numbers of them).
          test_lookahead_cases_cpu.py asserts the counts from every record's table entry, so a retuned packer or density cannot
          thin the coverage silently.
  SPLITS  two single layers on the SPLIT = 8 route (N = 64: 4 records; K = 11008 and 12800 at build_member's 5 % salients): 22 and
          25 panels, which a wave walks at stride 8 -- 3 and 4 panels for wave 0 --, and 9 and 11 salient rounds, of which wave 0
          (at 11: waves 0 to 2) takes a second one.

Activations, members, the sentinel-filled output buffer and the packing are gemv_persistent_cases'."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from gemv_persistent_cases import GAP, SENTINEL, Launch, SetSpec, activations, build_group, build_set, pack_sets  # noqa: F401

# per set: K, the further salient fraction on top of build_member's 5 %, and the rounds of 64 chunks EVERY record then holds.  A
# record's chunk count is about K f + 15.5 (16 rows, each with a cut-short last chunk) with a spread of a few chunks; the fractions
# put it in the middle of the 64-chunk window of the wanted round count: 92, 288, 352 and 416 chunks.
W3 = SetSpec(2048, 1536, False, False, False, 9201)                         # 3 panels, 2 rounds
W4 = SetSpec(2048, 2048, False, False, True, 9202, extra_sal=0.0872)        # 4 panels, 5 rounds; a bias
W5 = SetSpec(2048, 2304, False, False, False, 9203, extra_sal=0.1009)       # 5 panels (the last one half empty), 6 rounds
W7 = SetSpec(2048, 3584, False, False, False, 9204, extra_sal=0.0648)       # 7 panels, 7 rounds
W8 = SetSpec(2048, 4096, False, False, False, 9205)                         # 8 panels, 4 rounds (about 215 chunks)
PANELS = {W3: 3, W4: 4, W5: 5, W7: 7, W8: 8}
ROUNDS = {W3: 2, W4: 5, W5: 6, W7: 7, W8: 4}

RING = Launch("ring64", (W3, W4, W5, W7, W8), 64)
LAUNCHES = (RING,)
MS = (1, 4)
COMMIT = "1b8b0df"                                      # the commit whose library recorded the fixtures
SIDECAR = "gemv_lookahead_parent.json"


def fixture_name(launch: Launch, M: int) -> str:
    return f"gemv_lookahead_{launch.name}_m{M}_parent_{COMMIT}"


@dataclass(frozen=True)
class Split:
    name: str
    N: int
    K: int
    seed: int

    @property
    def P(self):
        return (self.K + 511) // 512


SPLITS = (Split("split_k11008", 64, 11008, 9301), Split("split_k12800", 64, 12800, 9302))
SPLIT_WAVES = 8                                         # what pbl_gemv_route answers for them (asserted by the CPU test)


def split_fixture_name(s: Split, M: int) -> str:
    return f"gemv_lookahead_{s.name}_m{M}_parent_{COMMIT}"


def build_split(s: Split):
    """(build_member's dict, host PackedWeight) of one single-layer case"""
    from gemv_cfg_cases import build_member
    from pb_llm_amd.packing import pack_dense
    d = build_member(s.N, s.K, s.seed, False, False)
    return d, pack_dense(d["W"], d["hi"], d["lo"], d["ss"], d["sz"], d["sal"], sal_f16=False)


def run_split(packed_dev, x, M: int):
    """pbl_linear_f16 of one packed layer (on the device) into a sentinel-filled buffer with GAP elements in front of and behind the
    [M, N] block.  Returns (y -- a view into the buffer --, buffer, keep)."""
    import ctypes as C

    import torch
    from pb_llm_amd import _lib
    dev = packed_dev.blob.device
    n = M * packed_dev.N
    buf = torch.full((n + 2 * GAP,), SENTINEL, dtype=torch.float16, device=dev)
    keep = torch.ones(n + 2 * GAP, dtype=torch.bool, device=dev)
    keep[GAP:GAP + n] = False
    y = buf[GAP:GAP + n].view(M, packed_dev.N)
    _lib.check(_lib.lib().pbl_linear_f16(C.byref(packed_dev.layer_struct(None)), x.data_ptr(), y.data_ptr(), M, 0,
                                         torch.cuda.current_stream(dev).cuda_stream), "linear_f16")
    return y, buf, keep


def record_counts(blob: np.ndarray):
    """(chunks, exception entries) of every record, from the blob's record table"""
    from oracle import pb_format_ref
    h = pb_format_ref.read_header(blob)
    pos, NRB = h["rb_off_pos"], h["NRB"]
    info = blob[pos: pos + 16 * NRB].view(np.uint32).reshape(NRB, 4)
    return (info[:, 1] + info[:, 2]).astype(np.int64), info[:, 3].astype(np.int64)
