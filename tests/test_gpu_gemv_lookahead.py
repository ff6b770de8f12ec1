"""-m gpu: the decode GEMV at the panel and salient-round counts where its lookahead loops begin, wrap and end -- the launches of
gemv_lookahead_cases.py -- against outputs recorded with the library of the commit before the tile registers became a three-set
ring (tools/record_gemv_golden.py --cases gemv_lookahead_cases; tests/golden/gemv_lookahead_*), bit for bit; against the float64
product with the weight the oracle's decoder reads out of each blob (check_rows' bound); into sentinel-filled buffers, twice."""
import os

import numpy as np
import pytest
import torch

import gemv_lookahead_cases as LC
from oracle import pb_format_ref
from test_gpu_decode_prologues import check_rows

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ring_sets():
    """[(build_set's dict, host PackedWeight, float64 decoded weight)] of the grouped launch, packed and decoded once"""
    import __graft_entry__ as g
    g.build()
    out = []
    for d, p in LC.pack_sets(LC.RING):
        W = pb_format_ref.decode(p.blob.numpy())
        assert np.array_equal(W, d["W"]), "the blob does not decode to the matrix it was packed from"
        out.append((d, p, W.astype(np.float64)))
    return out


@pytest.fixture(scope="module")
def split_layers():
    import __graft_entry__ as g
    g.build()
    out = {}
    for sp in LC.SPLITS:
        d, p = LC.build_split(sp)
        W = pb_format_ref.decode(p.blob.numpy())
        assert np.array_equal(W, d["W"]), "the blob does not decode to the matrix it was packed from"
        out[sp.name] = (p, W.astype(np.float64))
    return out


def golden_members(launch, M):
    flat = np.load(os.path.join(GOLDEN, LC.fixture_name(launch, M) + ".npy"), allow_pickle=False)
    assert flat.dtype == np.float16
    out, cur = [], 0
    for i in range(launch.period):
        n = M * launch.sets[launch.set_of(i)].N
        out.append(flat[cur:cur + n].reshape(M, -1))
        cur += n
    assert cur == flat.size
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("M", LC.MS)
def test_ring_launch_equals_the_recorded_outputs(ring_sets, M):
    """3, 4, 5, 7 and 8 panels and 2 to 7 salient rounds in one grouped launch on the throughput route: nothing outside the
    members' rows is written, a second launch gives the same bits, every member equals the recording bit for bit and stays within
    the parity bound of the float64 product with the decoded weight"""
    assert torch.cuda.is_available()
    launch = LC.RING
    g, buf, keep = LC.build_group(launch, [(d, p) for d, p, _ in ring_sets], M, DEV)
    assert not g.any_groups
    g.launch()
    torch.cuda.synchronize()
    first = buf.clone()
    assert bool((first[keep] == LC.SENTINEL).all()), (M, "first launch: a store outside the members' rows")
    assert not bool((first[~keep] == LC.SENTINEL).any()), (M, "first launch: a row was not written")
    buf.fill_(LC.SENTINEL)
    g.launch()
    torch.cuda.synchronize()
    assert bool((buf[keep] == LC.SENTINEL).all()), (M, "second launch: a store outside the members' rows")
    assert torch.equal(first.view(torch.int16), buf.view(torch.int16)), (M, "two launches of one group differ")
    gold = golden_members(launch, M)
    seen = set()
    for i, y in enumerate(g.y):
        yh = y.cpu().numpy()
        key = i % launch.period
        same = yh.view(np.uint16) == gold[key].view(np.uint16)
        assert same.all(), (M, "member", i, int((~same).sum()), "elements differ from the recording; first at", np.argwhere(~same)[0].tolist())
        if key not in seen:                                              # (the float64 reference once per distinct member)
            seen.add(key)
            k = launch.set_of(i)
            d, _, W = ring_sets[k]
            ref = LC.activations(launch.sets[k].K, M, key).astype(np.float64) @ W.T
            check_rows(y, ref if d["bias"] is None else ref + d["bias"].astype(np.float64), (M, "member", i))


@pytest.mark.gpu
@pytest.mark.parametrize("M", LC.MS)
@pytest.mark.parametrize("sp", LC.SPLITS, ids=lambda s: s.name)
def test_split_layer_equals_the_recorded_output(split_layers, sp, M):
    """one layer whose record eight waves share: a wave walks 3 (4) panels at stride 8 and wave 0 a second salient round"""
    assert torch.cuda.is_available()
    p, W = split_layers[sp.name]
    pd = p.to(DEV)
    xh = LC.activations(sp.K, M, 0)
    x = torch.from_numpy(xh).to(DEV)
    y, buf, keep = LC.run_split(pd, x, M)
    torch.cuda.synchronize()
    first = buf.clone()
    assert bool((first[keep] == LC.SENTINEL).all()), (sp.name, M, "a store outside the layer's rows")
    assert not bool((first[~keep] == LC.SENTINEL).any()), (sp.name, M, "a row was not written")
    y2, buf2, _ = LC.run_split(pd, x, M)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int16), buf2.view(torch.int16)), (sp.name, M, "two launches differ")
    want = np.load(os.path.join(GOLDEN, LC.split_fixture_name(sp, M) + ".npy"), allow_pickle=False).reshape(M, sp.N)
    same = y.cpu().numpy().view(np.uint16) == want.view(np.uint16)
    assert same.all(), (sp.name, M, int((~same).sum()), "elements differ from the recording; first at", np.argwhere(~same)[0].tolist())
    check_rows(y, xh.astype(np.float64) @ W.T, (sp.name, M))
