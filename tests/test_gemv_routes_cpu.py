"""-m "not gpu": which pbl_gemv_kernel configuration a launch gets (pbl_gemv_route, the helper route_of / fused_launch /
pbl_gemv_f16_grouped ask) and whether the case table of test_gpu_gemv_configs.py (gemv_cfg_cases.py) reaches
every configuration in both families.  The library answers; nothing here restates pick_split.
SPLIT = 1 with WPB = 1 no longer exists (it could never be launched): asserted over a sweep below, no case contrived."""
import ctypes as C
import functools

import pytest
import torch

from gemv_cfg_cases import FUSED, SINGLE, WANTED, build_member, seed_of
from pb_llm_amd import _lib
from pb_llm_amd.packing import pack_dense


def route(NRB, P, members):
    s, w = C.c_int(-1), C.c_int(-1)
    assert _lib.lib().pbl_gemv_route(NRB, P, members, C.byref(s), C.byref(w)) == _lib.PBL_OK
    return s.value, w.value


def route_of_case(case, fused):
    return route(case.max_NRB, case.P, len(case.Ns) if fused else 0)


@pytest.mark.parametrize("family", ["single", "fused"])
def test_the_table_reaches_every_configuration_through_both_limits(family):
    fused = family == "fused"
    cases = FUSED if fused else SINGLE
    reached = {}
    for c in cases:
        assert (len(c.Ns) > 1) == fused
        got = route_of_case(c, fused)
        assert got == (c.split, c.wpb), (c.name, "claims", (c.split, c.wpb), "the library launches", got)
        # `via`: which limit sets the split.  "P": a single record of this P splits as far, and these records at a large P would
        # split further; "records": these records split no further at any P.
        m1, mL = (1, len(c.Ns)) if fused else (0, 0)
        if c.via == "P":
            assert route(1, c.P, m1)[0] == c.split and (c.split == 8 or route(c.max_NRB, 64, mL)[0] > c.split), c.name
        else:
            assert route(c.max_NRB, 64, mL)[0] == c.split, c.name
        reached.setdefault(got, set()).add(c.via)
    for cfg, vias in WANTED.items():
        assert cfg in reached, (family, "no case reaches SPLIT, WPB =", cfg)
        assert vias <= reached[cfg], (family, cfg, "reached only via", reached[cfg])
        print(f"{family}: SPLIT = {cfg[0]}, WPB = {cfg[1]} reached via {sorted(reached[cfg])} by "
              f"{[c.name for c in cases if (c.split, c.wpb) == cfg]}")
    for s in (8, 4, 2, 1):
        assert any(c.rich and c.split == s for c in cases), (family, "no rich case (bias, exceptions, N % 16) at SPLIT", s)


def test_split_1_with_one_wave_per_workgroup_is_unreachable():
    """the configuration no longer exists: it is not instantiated, and no route names it.  Fewer than PBL_SPLIT_TARGET_WAVES (8192)
    records always share a record between at least 2 waves, and from there on every launch runs 4 waves per workgroup"""
    seen = set()
    nrbs = sorted(set(list(range(1, 70)) + [2 ** k + d for k in range(6, 21) for d in (-1, 0, 1)] + [1 << 24 >> 4]))
    for members in (0, 1, 2, 3, 4, 7, 64):
        for NRB in nrbs:
            for P in (1, 2, 3, 4, 5, 8, 22, 64):
                s, w = route(NRB, P, members)
                assert s in (1, 2, 4, 8) and (w == s if s > 1 else w in (1, 4)), (NRB, P, members, s, w)
                assert (s, w) != (1, 1), (NRB, P, members)
                seen.add((s, w))
    assert seen == {(8, 8), (4, 4), (2, 2), (1, 4)}
    print("SPLIT = 1, WPB = 1: unreachable over the sweep; configurations seen:", sorted(seen))


def test_route_rejects_bad_arguments():
    L = _lib.lib()
    s, w = C.c_int(7), C.c_int(7)
    assert L.pbl_gemv_route(16, 1, 0, None, C.byref(w)) == _lib.PBL_ERR_INVALID_ARG
    assert L.pbl_gemv_route(16, 1, 0, C.byref(s), None) == _lib.PBL_ERR_INVALID_ARG
    assert L.pbl_gemv_route(16, 1, -1, C.byref(s), C.byref(w)) == _lib.PBL_ERR_INVALID_ARG
    assert L.pbl_gemv_route(0, 1, 0, C.byref(s), C.byref(w)) == _lib.PBL_ERR_INVALID_ARG
    assert L.pbl_gemv_route(16, 0, 0, C.byref(s), C.byref(w)) == _lib.PBL_ERR_INVALID_ARG
    assert (s.value, w.value) == (7, 7)                               # outputs untouched on an error


@functools.lru_cache(maxsize=None)
def packed_of(case, member, sal_f16):
    d = build_member(case.Ns[member], case.K, seed_of(case, member, sal_f16), sal_f16, case.rich)
    return pack_dense(d["W"], d["hi"], d["lo"], d["ss"], d["sz"], d["sal"], sal_f16=sal_f16), d


@pytest.mark.parametrize("case", SINGLE, ids=lambda c: c.name)
def test_no_single_layer_case_declines_any_row_count(case):
    """one GEMV pass takes 4 rows of every single-layer case (the LDS budget): the GPU grid may skip no M.  Both forms share
    the salient positions, so the large cases are packed once."""
    for sal_f16 in ((True,) if case.large else (True, False)):
        p, d = packed_of(case, 0, sal_f16)
        assert (p.N, p.K, p.NRB, p.P, p.G) == (case.Ns[0], case.K, case.max_NRB, case.P, 1)
        assert p.nexc == len(d["exc"]), (case.name, "exceptions", p.nexc)
        assert bool(p.flags & _lib.PBL_FLAG_SAL_F16) == sal_f16
        assert _lib.lib().pbl_linear_push_max_tokens(C.byref(p.layer_struct(None))) == _lib.PBL_MAX_TOKENS_PER_LAUNCH, case.name


@pytest.mark.parametrize("case", [c for c in FUSED if not c.large], ids=lambda c: c.name)
def test_small_fused_members_pack_with_the_exceptions_the_table_promises(case):
    for m in range(len(case.Ns)):
        p, d = packed_of(case, m, True)
        assert p.nexc == len(d["exc"]) and (2 <= p.nexc <= 5 if case.rich else p.nexc == 0)
        if case.rich:
            assert d["exc"][0][0] // 16 == p.NRB - 1                     # one of them in the last record
    assert any(n % 16 for n in case.Ns) == case.rich
    assert torch.is_tensor(p.blob)
