"""-m gpu: the packed layers and harness.fuse_decode_ under torch.inference_mode().  Inference tensors have no version counter, so
nothing computed from an inference-tensor activation may be reused by a later call (the fragment-major copy of x, the fused groups'
hand-over, the deferred norm), and weights that are inference tensors are keyed on their module's reload generation
(quant.tensor_version).  Every case compares the output under inference_mode with the same call under no_grad on a normal tensor,
bit for bit, and with the float64 oracle."""
import copy
import tempfile

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import pb_oracle as O
from pb_llm_amd import io as pio
from pb_llm_amd import synth
from pb_llm_amd import quant as Q
from test_gpu_gemm import rtn_layer
from test_inference_mode_cpu import SAME_SIZE_SEEDS, rtn_fp16, same_size_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {torch.float16: 1e-3, torch.bfloat16: 1e-2, torch.float32: 2e-5}


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def inference_copy(t):
    with torch.inference_mode():
        c = t.clone()
    assert c.is_inference()
    return c


def check_oracle(y, x, Wd, b, what, tol=None):
    """y against the float64 oracle on the values x holds (bf16 / fp32 x: as the kernel sees them)"""
    ref = O.dense_linear(x.float().cpu().numpy().astype(np.float64).reshape(-1, x.shape[-1]), Wd, b)
    rel, ratio = O.parity_errors(y.float().cpu().numpy().reshape(ref.shape), ref)
    tol = tol or TOL[y.dtype]
    assert rel < tol and (ratio < 1.0 or y.dtype != torch.float16), (what, rel, ratio)


@pytest.fixture(scope="module")
def img_layer():
    """an fp16-grid layer with a GEMM image (every routing boundary below: GEMV, matrix-core, small-batch and GEMM kernels)"""
    p, Wd = rtn_layer(512, 1024, -1, seed=31, low_frac=0.9, fp16=True, exceptions=2)
    b = synth.normal((512,), 31, 3, 0.1)
    lay = Q.PBLinear(p.to(DEV), T(b))
    assert Q.fused_gemm_ok(lay.packed)
    return lay, Wd, b


def x_cases():
    for M in (1, 4, 5, 32, 33, 64, 65, 300):
        base = T(synth.activations((M, 1024), 60, M))
        for dt in (torch.float16, torch.bfloat16, torch.float32):
            yield (M, dt), base.to(dt) if dt != torch.float32 else base.float() * 1.0009765625
    yield ("3d", torch.float16), T(synth.activations((2, 150, 1024), 61, 3))


@pytest.mark.parametrize("split_k", [True, False])
@pytest.mark.parametrize("xf", [True, False])
@pytest.mark.parametrize("route", ["native", "ctypes"])
def test_pblinear_image_layer_every_regime(img_layer, monkeypatch, route, xf, split_k):
    lay, Wd, b = img_layer
    monkeypatch.setattr(Q, "GEMM_X_FRAGMENTS", xf)
    monkeypatch.setattr(Q, "GEMM_SPLIT_K", split_k)

    def call(x):
        if route == "native":
            return lay(x)
        return Q._pb_linear_forward(lay.packed, lay.pbl_bias, x, False, torch.float16)

    for what, x in x_cases():
        with torch.no_grad():
            want = call(x)
        xi = inference_copy(x)
        with torch.inference_mode():
            got = call(xi)
            again = call(xi)                                       # a second call with the same inference tensor: nothing reused, same bits
        assert got.dtype == x.dtype and got.shape == (*x.shape[:-1], 512), what
        assert torch.equal(got, want) and torch.equal(again, want), (route, xf, split_k, what)
        check_oracle(got, x, Wd, b, (route, xf, split_k, what))
    Q.drop_x_fragments_()


def test_three_layers_share_an_inference_activation_and_follow_its_writes():
    """q / k / v-like layers called with ONE inference-tensor x at 300 rows, then x.mul_(0.5) inside inference_mode: the outputs follow
    the new contents (an identity-only cache of the fragment copy would serve the old ones)"""
    layers = []
    for seed, N in ((5, 512), (6, 384), (7, 640)):
        p, Wd = rtn_layer(N, 1024, -1, seed=seed, low_frac=0.9, fp16=True, exceptions=1)
        b = synth.normal((N,), seed, 3, 0.1)
        layers.append((Q.PBLinear(p.to(DEV), T(b)), Wd, b))
    x = T(synth.activations((300, 1024), 8, 21))
    with torch.no_grad():
        want = [lay(x) for lay, _, _ in layers]
        want_half = [lay(x * 0.5) for lay, _, _ in layers]
    Q.drop_x_fragments_()
    xi = inference_copy(x)
    with torch.inference_mode():
        got = [lay(xi) for lay, _, _ in layers]
        xi.mul_(0.5)
        got_half = [lay(xi) for lay, _, _ in layers]
    for (lay, Wd, b), g, w, gh, wh in zip(layers, got, want, got_half, want_half):
        assert torch.equal(g, w) and torch.equal(gh, wh)
        assert not torch.equal(gh, g)
        check_oracle(g, x, Wd, b, "x")
        check_oracle(gh, x * 0.5, Wd, b, "x * 0.5")
    assert not Q._XF_CACHE                                           # nothing was kept for an inference tensor


def _fp32_grid_layers():
    N, K = 384, 1024
    W = synth.llm_weight(N, K, seed=43, heavy_tail=True)
    b = synth.normal((N,), 43, 3, 0.1)
    out = [("binary", Q.BinaryLinear(torch.from_numpy(W), torch.from_numpy(b)).to(DEV).eval(), lambda m, x: O.binary_linear_forward(x, W, b)),
           ("xnor", Q.XnorBinaryLinear(torch.from_numpy(W), torch.from_numpy(b)).to(DEV).eval(), lambda m, x: O.xnor_binary_linear_forward(x, W, b))]
    q = Q.BinaryXnorExceptOutliersLinear(torch.from_numpy(W), torch.from_numpy(b), 0.1).to(DEV)
    q.eval()
    q.gen_outlier_mask()

    def qat_ref(m, x):
        return O.pb_qat_forward(x, m.weight.data.float().cpu().numpy(), m.outlier_mask.cpu().numpy(), m.binary_scale.float().cpu().numpy(), b)
    out.append(("qat_f32", q, qat_ref))
    return out


def test_image_only_and_fp32_grid_layers():
    """an image-only layer (release_blob_) and the fp32-grid classes at 1, 40 and 300 rows; the dense-backed layers pack on their first
    call -- under inference_mode for one copy, under no_grad for the other"""
    p, Wd = rtn_layer(512, 1024, -1, seed=33, low_frac=0.9, fp16=True)
    b = synth.normal((512,), 33, 3, 0.1)
    io_lay = Q.PBLinear(p.to(DEV), T(b))
    assert io_lay.release_blob_() > 0
    for M in (1, 40, 300):
        x = T(synth.activations((M, 1024), 62, M))
        with torch.no_grad():
            want = io_lay(x)
        with torch.inference_mode():
            got = io_lay(inference_copy(x))
        assert torch.equal(got, want), M
        check_oracle(got, x, Wd, b, ("image only", M))
    for name, m, ref_fn in _fp32_grid_layers():
        mi = copy.deepcopy(m)
        for M in (1, 40, 300):
            x = T(synth.normal((M, 1024), 44, M, 1.0))
            with torch.no_grad():
                want = m(x)
            with torch.inference_mode():
                got = mi(inference_copy(x))
            assert got.dtype == torch.float32 and torch.equal(got, want), (name, M)
            assert O.parity_errors(got.cpu().numpy(), ref_fn(mi, x.cpu().numpy()))[0] < 2e-5, (name, M)


# ---------------------------------------------------------------- weights that are inference tensors
def _reload_and_check(lay, other_sd, Wd_new, b_new, what):
    with torch.inference_mode():
        lay.load_state_dict(other_sd)
    for M in (1, 300):
        x = T(synth.activations((M, lay.in_features), 63, M))
        with torch.inference_mode():
            check_oracle(lay(inference_copy(x)), x, Wd_new, b_new, (what, "after load_state_dict", M))
        with torch.no_grad():
            check_oracle(lay(x), x, Wd_new, b_new, (what, "after load_state_dict, no_grad", M))


def test_pblinear_weights_built_moved_or_loaded_inside_inference_mode():
    a0, b0, Wb = same_size_pair()
    Wa = rtn_fp16(SAME_SIZE_SEEDS[0])[0].float().numpy()
    Wb = Wb.float().numpy()
    ba = synth.normal((256,), 71, 3, 0.1)
    bb = synth.normal((256,), 72, 3, 0.1)
    other = Q.PBLinear(b0.packed, torch.from_numpy(bb))
    W16, mask, r = rtn_fp16(SAME_SIZE_SEEDS[0])
    cpu_lay = Q.PBLinear(a0.packed, torch.from_numpy(ba))
    with torch.inference_mode():
        built_dev = Q.PBLinear.from_dense(W16.to(DEV), torch.from_numpy(ba).to(DEV), mask.to(DEV), -1, r["hscale"], r["hzero"]).to(DEV)
        moved = copy.deepcopy(cpu_lay).to(DEV)
    with tempfile.TemporaryDirectory() as d:
        pio.save_pb(nn.Sequential(copy.deepcopy(cpu_lay)), d)
        with torch.inference_mode():
            loaded = pio.load_pb(nn.Sequential(nn.Linear(512, 256)), d)[0].to(DEV)
    for what, lay in (("from_dense", built_dev), ("moved", moved), ("load_pb", loaded)):
        assert lay.pbl_blob.is_inference() and lay.pbl_blob.is_cuda, what
        for M in (1, 300):
            x = T(synth.activations((M, 512), 64, M))
            with torch.inference_mode():
                check_oracle(lay(inference_copy(x)), x, Wa, ba, (what, M))
            with torch.no_grad():
                check_oracle(lay(x), x, Wa, ba, (what, "no_grad", M))
        _reload_and_check(lay, other.state_dict(), Wb, bb, what)


def test_dense_backed_layer_moved_inside_inference_mode():
    N, K = 256, 512
    W = synth.llm_weight(N, K, seed=45, heavy_tail=True)
    b = synth.normal((N,), 45, 3, 0.1)
    cpu = Q.BinaryXnorExceptOutliersLinear(torch.from_numpy(W), torch.from_numpy(b), 0.1)
    cpu.eval()
    with torch.inference_mode():
        m = cpu.to(DEV)
        assert m.weight.is_inference()
        xs = {M: T(synth.normal((M, K), 46, M, 1.0)) for M in (1, 300)}
        ys = {M: m(inference_copy(x)) for M, x in xs.items()}          # the outlier mask, the codes and the blob are made here
    Wh, mask, s = m.weight.data.float().cpu().numpy(), m.outlier_mask.cpu().numpy(), m.binary_scale.float().cpu().numpy()
    for M, x in xs.items():
        assert O.parity_errors(ys[M].cpu().numpy(), O.pb_qat_forward(x.cpu().numpy(), Wh, mask, s, b))[0] < 2e-5, M
    # new weights: the binarized part negated (the salient values stay on the layer's code grid), a new bias
    W2 = np.where(mask, Wh, -Wh).astype(np.float32)
    b2 = synth.normal((N,), 47, 3, 0.1)
    with torch.inference_mode():
        m.load_state_dict({"weight": torch.from_numpy(W2), "bias": torch.from_numpy(b2)})
        for M, x in xs.items():
            y = m(inference_copy(x))
            assert O.parity_errors(y.cpu().numpy(), O.pb_qat_forward(x.cpu().numpy(), W2, mask, s, b2))[0] < 2e-5, M
            assert not torch.equal(y, ys[M]), M


# ---------------------------------------------------------------- HF LLaMA, every fuse_decode_ mode
def _groups(model):
    from pb_llm_amd import harness as H
    return {id(m._group[0]): m._group[0] for m in model.modules() if isinstance(m, H._FusedMember)}.values()


def _launches(model):
    return sum(g.launches for g in _groups(model))


@pytest.fixture(scope="module")
def llamas():
    from pb_llm_amd import harness as H
    from test_gpu_decode_prologues import llama
    _, plain = llama()
    out = {"plain": plain}
    for name, kw in (("default", {}), ("merged", {"merge_batched": True}), ("prologues", {"prologues": True}), ("epilogues", {"epilogues": True})):
        m = copy.deepcopy(plain)
        assert H.fuse_decode_(m, **kw) == 4
        out[name] = m
    out["plain_bf16"] = copy.deepcopy(plain).to(torch.bfloat16)
    out["default_bf16"] = copy.deepcopy(out["plain_bf16"])
    H.fuse_decode_(out["default_bf16"])
    return out


def _ids(n, seed, rows=1):
    return torch.from_numpy((synth.uniform01(n, seed, 1) * 1000).astype(np.int64)).view(rows, -1).to(DEV)


def _run(model, steps, ctx):
    """logits of: a 300-token prefill, an 8-token prefill + 6 single-token KV-cache decode steps, batches of 2 / 4 / 5 / 40 rows"""
    out = []
    with ctx():
        out.append(("prefill", 300, model(steps["prefill"], use_cache=False).logits))
        o = model(steps["prompt"], use_cache=True)
        out.append(("prompt", 8, o.logits))
        cache = o.past_key_values
        for t in range(6):
            o = model(steps["decode"][:, t:t + 1], past_key_values=cache, use_cache=True)
            cache = o.past_key_values
            out.append((f"decode {t}", 1, o.logits))
        for B in (2, 4, 5, 40):
            out.append((f"batch {B}", B, model(steps[B], use_cache=False).logits))
    return out


@pytest.mark.parametrize("mode", ["default", "merged", "prologues", "epilogues", "default_bf16"])
def test_llama_fuse_decode_modes_under_inference_mode(llamas, mode):
    steps = {"prefill": _ids(300, 81), "prompt": _ids(8, 82), "decode": _ids(6, 83)}
    steps.update({B: _ids(B, 84 + B, rows=B) for B in (2, 4, 5, 40)})
    model = llamas[mode]
    plain = llamas["plain_bf16" if mode.endswith("bf16") else "plain"]
    want = _run(plain, steps, torch.no_grad)
    want_pro = _run(llamas["prologues"], steps, torch.no_grad) if mode == "epilogues" else None
    before = _launches(model)
    got = _run(model, steps, torch.inference_mode)
    for (name, rows, g), (_, _, w) in zip(got, want):
        if mode == "epilogues" and rows <= 4:
            ref = next(l for n, _, l in want_pro if n == name)       # the folded layer: the prologues=True model's bits, as under no_grad
        else:
            ref = w
        assert g.dtype == ref.dtype and torch.equal(g, ref), (mode, name)
    launched = _launches(model) - before
    if mode == "epilogues":
        # only the folded layers launched (run_folded: 2 groups per layer, 2 layers) -- for the <= 4-row steps: 6 decode steps, the
        # batches of 2 and 4 rows
        assert launched == 2 * 2 * (6 + 2), launched
    else:
        assert launched == 0, (mode, launched)
