"""-m gpu (the last test: CPU): pbl_gemv_f16_grouped on the throughput route (SPLIT = 1, 4 waves per workgroup) over members that
differ in K, N, bias, exception entries and salient form -- the launches of gemv_persistent_cases.py -- against outputs recorded
from the commit before the kernel's salient rounds were reworked (tools/record_gemv_golden.py; tests/golden/gemv_grouped_*), bit
for bit, and against the float64 product with the weight the oracle's decoder reads out of each blob (check_rows' bound).

The second launch has the fewest work items a throughput launch can have: the route needs max_NRB x members >= 8192 records and a
workgroup owns 4, so no launch has fewer than 2048 items -- which is also the most workgroups a 256-CU chip holds at once
(8 per CU at 4 waves each).  A launch on this route with fewer items than resident workgroups therefore does not exist on this
chip; 2048 items (PLAIN) and 2176 (MIXED) are the two sides of that boundary that do."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import gemv_persistent_cases as GC
from gemv_cfg_cases import FUSED
from oracle import pb_format_ref
from pb_llm_amd import _lib
from test_gpu_decode_prologues import check_rows

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def sets():
    """per launch: [(build_set's dict, host PackedWeight)], packed once"""
    import __graft_entry__ as g
    g.build()
    return {launch.name: GC.pack_sets(launch) for launch in GC.LAUNCHES}


@pytest.fixture(scope="module")
def decoded(sets):
    """per launch and set: float64 [N, K], what the oracle's decoder reads out of the blob -- and it is the matrix that was packed"""
    out = {}
    for launch in GC.LAUNCHES:
        ws = []
        for d, p in sets[launch.name]:
            W = pb_format_ref.decode(p.blob.numpy())
            assert np.array_equal(W, d["W"]), (launch.name, "the blob does not decode to the matrix it was packed from")
            ws.append(W.astype(np.float64))
        out[launch.name] = ws
    return out


def golden_members(launch, M):
    """the fixture's members: `period` arrays [M, N] fp16"""
    flat = np.load(os.path.join(GOLDEN, GC.fixture_name(launch, M) + ".npy"), allow_pickle=False)
    assert flat.dtype == np.float16
    out, cur = [], 0
    for i in range(launch.period):
        n = M * launch.sets[launch.set_of(i)].N
        out.append(flat[cur:cur + n].reshape(M, -1))
        cur += n
    assert cur == flat.size
    return out


def test_fixtures_name_their_recording_commit():
    side = json.load(open(os.path.join(GOLDEN, "gemv_grouped_parent.json")))
    assert side["recorded_with_commit"] == "de42e4d"
    assert set(side["files"]) == {GC.fixture_name(launch, M) + ".npy" for launch in GC.LAUNCHES for M in GC.MS}


@pytest.mark.gpu
@pytest.mark.parametrize("M", GC.MS)
@pytest.mark.parametrize("launch", GC.LAUNCHES, ids=lambda l: l.name)
def test_grouped_launch_equals_the_recorded_outputs(sets, decoded, launch, M):
    """every member's output equals the recorded one bit for bit, stays within the parity bound of the float64 product with the
    decoded weight, and nothing but the members' rows is written"""
    assert torch.cuda.is_available()
    g, buf, keep = GC.build_group(launch, sets[launch.name], M, DEV)
    assert (g.any_groups & 2 != 0) == any(s.sal_f16 for s in launch.sets) and not g.any_groups & 1
    g.launch()
    torch.cuda.synchronize()
    assert bool((buf[keep] == GC.SENTINEL).all()), (launch.name, M, "a store outside the members' rows")
    gold = golden_members(launch, M)
    refs = {}
    for i, y in enumerate(g.y):
        yh = y.cpu().numpy()
        want = gold[i % launch.period]
        same = yh.view(np.uint16) == want.view(np.uint16)
        assert same.all(), (launch.name, M, "member", i, int((~same).sum()), "elements differ from the recording; first at",
                            np.argwhere(~same)[0].tolist())
        key = i % launch.period
        if key not in refs:                                              # (the float64 reference once per distinct member)
            k = launch.set_of(i)
            d = sets[launch.name][k][0]
            x = GC.activations(launch.sets[k].K, M, key).astype(np.float64)
            ref = x @ decoded[launch.name][k].T
            refs[key] = ref if d["bias"] is None else ref + d["bias"].astype(np.float64)
            check_rows(y, refs[key], (launch.name, M, "member", i))


@pytest.mark.gpu
@pytest.mark.parametrize("M", GC.MS)
def test_fewest_items_twice_into_sentinels(sets, M):
    """the launch with the fewest work items the route allows, twice into sentinel-filled outputs: no element outside a member's
    rows changes, and both launches agree bit for bit"""
    launch = GC.PLAIN
    assert launch.items == 2048 < GC.MIXED.items
    g, buf, keep = GC.build_group(launch, sets[launch.name], M, DEV)
    g.launch()
    torch.cuda.synchronize()
    first = buf.clone()
    assert bool((first[keep] == GC.SENTINEL).all()), (M, "first launch: a store outside the members' rows")
    assert not bool((first[~keep] == GC.SENTINEL).any()), (M, "first launch: a row was not written")
    buf.fill_(GC.SENTINEL)
    g.launch()
    torch.cuda.synchronize()
    assert bool((buf[keep] == GC.SENTINEL).all()), (M, "second launch: a store outside the members' rows")
    assert torch.equal(first.view(torch.int16), buf.view(torch.int16)), (M, "two launches of one group differ")


def test_route_answers():
    """pbl_gemv_route still sends these launches to SPLIT = 1 with 4 waves per workgroup, and the small fused cases to a split"""
    s, w = C.c_int(), C.c_int()
    L = _lib.lib()
    for launch in GC.LAUNCHES:
        assert launch.max_NRB * launch.members >= 8192
        assert L.pbl_gemv_route(launch.max_NRB, launch.P, launch.members, C.byref(s), C.byref(w)) == _lib.PBL_OK
        assert (s.value, w.value) == (1, 4), (launch.name, s.value, w.value)
    assert L.pbl_gemv_route(GC.PLAIN.max_NRB, GC.PLAIN.P, GC.PLAIN.members - 1, C.byref(s), C.byref(w)) == _lib.PBL_OK
    assert s.value > 1, "one member fewer no longer fills the throughput route"
    split = [c for c in FUSED if c.split > 1]
    assert split
    for c in split:
        assert L.pbl_gemv_route(c.max_NRB, c.P, len(c.Ns), C.byref(s), C.byref(w)) == _lib.PBL_OK
        assert (s.value, w.value) == (c.split, c.wpb) and s.value > 1, (c.name, s.value, w.value)
