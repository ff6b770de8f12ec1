"""-m gpu: what the derived artefacts the packed layers keep across calls hold on to, and when they are rebuilt.  The fragment-major
copy of x (quant._XF_CACHE) must not keep the activation alive; the library's own raw-pointer writers bump the version counter of
what they write, so no cache keyed on it serves a stale result; restore_blob_ after a load_state_dict (no forward in between) sizes
the kernels from the NEW blob's header; every trigger _DenseBacked._cache_key documents repacks.  The all-reduce writer is covered
in test_gpu_configs._tp_worker ("p2p")."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import pb_oracle as O
from pb_llm_amd import prep, synth
from pb_llm_amd import quant as Q
from pb_llm_amd.packing import PackedWeight
from test_gpu_gemm import rtn_layer
from test_inference_mode_cpu import header, same_size_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_oracle(y, ref, tol):
    rel, ratio = O.parity_errors(y.detach().float().cpu().numpy(), ref)
    assert rel < tol, (rel, ratio)


def test_fragment_copy_releases_the_activation():
    """three projections of one 300 x 4096 fp16 activation: once x and the outputs are dropped, neither x nor its fragment-major copy
    is alive; drop_gemm_images_ forgets the kept copy as well"""
    from pb_llm_amd import harness as H
    assert Q.GEMM_X_FRAGMENTS
    layers = nn.ModuleList()
    for seed, N in ((11, 512), (12, 256), (13, 384)):
        p, _ = rtn_layer(N, 4096, -1, seed=seed, low_frac=0.9, fp16=True)
        layers.append(Q.PBLinear(p.to(DEV)))
    with torch.no_grad():
        x0 = T(synth.activations((300, 4096), 14, 21))
        ys = [lay(x0) for lay in layers]                           # the images are built here (kept with the layers)
        del x0, ys
        Q.drop_x_fragments_()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        x = T(synth.activations((300, 4096), 15, 21))
        ys = [lay(x) for lay in layers]
        assert len(Q._XF_CACHE) == 1                                # one copy for the three projections
        del x, ys
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == base                # x and its copy are gone
        assert not Q._XF_CACHE
        x = T(synth.activations((300, 4096), 16, 21))
        ys = [lay(x) for lay in layers]
        assert len(Q._XF_CACHE) == 1
        H.drop_gemm_images_(layers)
        assert not Q._XF_CACHE


def test_quant8_rows_bumps_the_version_and_a_dense_backed_layer_repacks():
    W = T(synth.llm_weight(64, 256, seed=17, heavy_tail=True))
    v = W._version
    prep.quant8_rows_(W)
    assert W._version > v
    # a dense-backed layer whose weight the row quantizer rewrites in place (through its pointer) after an eval forward: the next
    # forward packs the written weight.  One large value per row makes the 8-bit step coarse, so the weight really changes.
    N, K = 128, 512
    W0 = synth.llm_weight(N, K, seed=18, heavy_tail=True)
    W0[:, 7] = 40.0
    b = synth.normal((N,), 18, 3, 0.1)
    lay = Q.XnorBinaryLinear(torch.from_numpy(W0), torch.from_numpy(b)).to(DEV).eval()
    xs = {M: T(synth.normal((M, K), 19, M, 1.0)) for M in (1, 40)}
    with torch.no_grad():
        before = {M: lay(x) for M, x in xs.items()}
        for M, x in xs.items():
            assert_oracle(before[M], O.xnor_binary_linear_forward(x.cpu().numpy(), W0, b), 2e-5)
        prep.quant8_rows_(lay.weight)
        W1 = lay.weight.detach().cpu().numpy()
        assert not np.array_equal(W1, W0)
        fresh = Q.XnorBinaryLinear(torch.from_numpy(W1), torch.from_numpy(b)).to(DEV).eval()
        for M, x in xs.items():
            y = lay(x)
            assert_oracle(y, O.xnor_binary_linear_forward(x.cpu().numpy(), W1, b), 2e-5)
            assert torch.equal(y, fresh(x)) and not torch.equal(y, before[M]), M


def test_restore_blob_after_load_state_dict_without_a_forward():
    """release_blob_ -> load_state_dict(other) -> restore_blob_, no forward in between: the kernels must be sized from the NEW blob's
    header (max_nch differs: the loaded layer needs more LDS).  The header is checked on the host BEFORE any launch."""
    a, b_, Wb = same_size_pair()
    ba, bb = synth.normal((256,), 21, 3, 0.1), synth.normal((256,), 22, 3, 0.1)
    lay = Q.PBLinear(a.packed, torch.from_numpy(ba)).to(DEV)
    other = Q.PBLinear(b_.packed, torch.from_numpy(bb))
    assert lay.release_blob_() > 0                                  # (builds the image of the OLD weights: their own header)
    lay.load_state_dict(other.state_dict())
    lay.restore_blob_()
    assert lay.pbl_blob.is_cuda and lay._image_only is None
    assert header(lay.packed) == header(PackedWeight.from_blob(lay.pbl_blob.cpu())) == header(b_.packed)
    ref_lay = other.to(DEV)
    Wbn = Wb.float().numpy()
    with torch.no_grad():
        for M in (1, 3, 40, 300):
            x = T(synth.activations((M, 512), 23, M))
            y = lay(x)
            assert_oracle(y, O.dense_linear(x.cpu().numpy(), Wbn, bb), 1e-3)
            assert torch.equal(y, ref_lay(x)), M


def test_dense_backed_cache_key_triggers_repack():
    """each change _DenseBacked._cache_key documents makes the next eval forward give the NEW weights' result"""
    N, K = 256, 512
    rng = np.random.default_rng(5)

    def new_w():
        return (rng.standard_normal((N, K)) * 0.02).astype(np.float32)

    W, b = new_w(), synth.normal((N,), 25, 3, 0.1)
    lay = Q.XnorBinaryLinear(torch.from_numpy(W), torch.from_numpy(b)).to(DEV).eval()
    xs = {M: T(synth.normal((M, K), 26, M, 1.0)) for M in (1, 40)}
    last = {}

    def check(Wn, what):
        with torch.no_grad():
            for M, x in xs.items():
                y = lay(x)
                assert_oracle(y, O.xnor_binary_linear_forward(x.cpu().numpy(), Wn, b), 2e-5)
                assert M not in last or not torch.equal(y, last[M]), (what, M)
                last[M] = y

    check(W, "initial")
    W = new_w()
    with torch.no_grad():
        lay.weight.copy_(torch.from_numpy(W))
    check(W, "copy_ under no_grad")
    W = new_w()
    lay.weight.data = T(W)
    check(W, ".data = reassignment")
    W = new_w()
    lay.load_state_dict({"weight": torch.from_numpy(W), "bias": torch.from_numpy(b)})
    check(W, "load_state_dict")
    lay.train()
    opt = torch.optim.SGD(lay.parameters(), lr=0.05)
    x = xs[40]
    lay(x).square().sum().backward()
    opt.step()
    lay.eval()
    with torch.no_grad():
        lay.bias.copy_(torch.from_numpy(b))                          # (only the weight step is under test)
    check(lay.weight.detach().cpu().numpy(), "optimizer step")
    W = new_w()
    lay.weight.data.copy_(T(W))                                     # `.data` edits are invisible to the key: invalidate()
    lay.invalidate()
    check(W, ".data.copy_ + invalidate()")
    lay.half()
    with torch.no_grad():
        for M, x in xs.items():
            xh = x.half()
            y = lay(xh)
            assert y.dtype == torch.float16
            assert_oracle(y, O.dense_linear(xh.float().cpu().numpy(), lay.quant_weight().float().cpu().numpy(), b), 1e-3)
            fresh = Q.XnorBinaryLinear(torch.from_numpy(W), torch.from_numpy(b)).to(DEV).half().eval()
            assert torch.equal(y, fresh(xh)), M
