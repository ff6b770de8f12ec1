"""CPU: the launches of gemv_lookahead_cases.py hold the panel and salient-round counts they claim -- read from every record's table
entry of the packed blobs -- reach the routes they claim, and their fixtures name the commit that recorded them."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import gemv_lookahead_cases as LC
from pb_llm_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def rounds(chunks):
    return (chunks + 63) // 64


def test_ring_launch_holds_its_panel_and_round_counts():
    """3, 4, 5, 7 and 8 panels (one K no multiple of 512); every record of a set holds exactly the set's 2, 5, 6, 7 or 4 rounds,
    and the last round of a record is cut short somewhere in every set"""
    launch = LC.RING
    assert [s.K for s in launch.sets] == [1536, 2048, 2304, 3584, 4096] and {s.N for s in launch.sets} == {2048} and launch.members == 64
    assert any(s.K % 512 for s in launch.sets)
    for s, (d, p) in zip(launch.sets, LC.pack_sets(launch)):
        assert p.P == LC.PANELS[s] == (s.K + 511) // 512 and p.NRB == 128 and p.nexc == 0 and p.G == 1, (s, p.P, p.NRB)
        chunks, nexc = LC.record_counts(p.blob.numpy())
        assert not nexc.any()
        r = rounds(chunks)
        assert (r == LC.ROUNDS[s]).all(), (s.K, "rounds per record", sorted(set(r.tolist())), int(chunks.min()), int(chunks.max()))
        assert (chunks % 64 != 0).any()
        assert int(chunks.max()) == p.max_nch
    assert sorted(LC.PANELS.values()) == [3, 4, 5, 7, 8] and sorted(LC.ROUNDS.values()) == [2, 4, 5, 6, 7]
    # a trip of the tile ring is three panels: the walk ends after 0, 1 and 2 panels of a trip; the rounds, in trips of two, after 0 and 1
    assert {v % 3 for v in LC.PANELS.values()} == {0, 1, 2} and {v % 2 for v in LC.ROUNDS.values()} == {0, 1}
    # the ring's first loop runs while p0 + 4 < P: no trip, one, and two (its back edge)
    assert {len(range(0, max(P - 4, 0), 3)) for P in LC.PANELS.values()} == {0, 1, 2}


def test_ring_launch_reaches_the_throughput_route():
    s, w = C.c_int(), C.c_int()
    launch = LC.RING
    assert launch.max_NRB * launch.members >= 8192
    assert _lib.lib().pbl_gemv_route(launch.max_NRB, launch.P, launch.members, C.byref(s), C.byref(w)) == _lib.PBL_OK
    assert (s.value, w.value) == (1, 4)


def test_split_layers_hold_their_counts_and_route():
    """22 and 25 panels at stride 8: wave 0 walks 3 and 4; more than 8 rounds in every record, so wave 0 takes a second one"""
    s, w = C.c_int(), C.c_int()
    walked = []
    for sp in LC.SPLITS:
        d, p = LC.build_split(sp)
        assert (p.N, p.K, p.P, p.NRB) == (64, sp.K, sp.P, 4) and p.nexc == 0
        assert _lib.lib().pbl_gemv_route(p.NRB, p.P, 0, C.byref(s), C.byref(w)) == _lib.PBL_OK
        assert (s.value, w.value) == (LC.SPLIT_WAVES, LC.SPLIT_WAVES)
        walked.append(len(range(0, p.P, LC.SPLIT_WAVES)))
        chunks, _ = LC.record_counts(p.blob.numpy())
        r = rounds(chunks)
        assert (r > LC.SPLIT_WAVES).all() and (r <= 2 * LC.SPLIT_WAVES).all(), (sp.name, r.tolist())
    assert walked == [3, 4]


def test_fixtures_name_their_recording_commit():
    side = json.load(open(os.path.join(GOLDEN, LC.SIDECAR)))
    assert side["recorded_with_commit"] == LC.COMMIT
    names = {LC.fixture_name(launch, M) + ".npy" for launch in LC.LAUNCHES for M in LC.MS}
    names |= {LC.split_fixture_name(sp, M) + ".npy" for sp in LC.SPLITS for M in LC.MS}
    assert set(side["files"]) == names
    for name, meta in side["files"].items():
        flat = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
        assert flat.dtype == np.float16 and flat.size == meta["elements"]
        assert hashlib.sha256(flat.tobytes()).hexdigest() == meta["sha256"], name
