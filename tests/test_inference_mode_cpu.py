"""-m "not gpu": the Python state around the kernels under torch.inference_mode() and across weight reloads.  Inference tensors have
no version counter (reading `._version` raises), so every cache key goes through quant.tensor_version, which counts them as version -1
and lets the owning module's load_state_dict generation tell a reload apart.  Here: the host packer path of a PBLinear built, read and
reloaded inside inference_mode, the dense-backed classes' cache key, and a structural check that no other `._version` read is left."""
import ast
import os

import torch

from oracle import pb_oracle as O
from pb_llm_amd import synth
from pb_llm_amd import quant as Q
from pb_llm_amd.packing import PackedWeight

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = ("N", "K", "P", "G", "NRB", "flags", "max_nch", "max_nexc", "nnz", "nexc")


def header(p: PackedWeight) -> tuple:
    return tuple(getattr(p, f) for f in HEADER)


def rtn_fp16(seed, low_frac=0.95, N=256, K=512):
    """(W_fq fp16 tensor, low mask, RTN state) of a synthetic layer on the fp16 grid"""
    W = synth.llm_weight(N, K, seed=seed, heavy_tail=True)
    mask = O.ptq_low_mask(W, low_frac, "magnitude", None, -1)
    r = O.ptq_rtn(W, mask, 8, -1)
    return torch.from_numpy(r["W_fq"]).half(), torch.from_numpy(mask), r


def from_dense(seed):
    W16, mask, r = rtn_fp16(seed)
    return Q.PBLinear.from_dense(W16, None, mask, -1, r["hscale"], r["hzero"])


# seeds whose 256 x 512 blobs have the same byte length (load_state_dict copies in place) but different headers: the second needs
# one more chunk per row (max_nch), so LDS sized from the first's header would be too small for it
SAME_SIZE_SEEDS = (0, 5)


def same_size_pair():
    """(a, b, W16 of b): two host PBLinears whose blobs have equal lengths and different headers"""
    a, b = from_dense(SAME_SIZE_SEEDS[0]), from_dense(SAME_SIZE_SEEDS[1])
    assert a.pbl_blob.numel() == b.pbl_blob.numel()
    assert header(a.packed) != header(b.packed) and a.packed.max_nch < b.packed.max_nch
    return a, b, rtn_fp16(SAME_SIZE_SEEDS[1])[0]


def test_tensor_version_of_inference_tensors():
    t = torch.zeros(4)
    assert Q.tensor_version(t) == (0, t._version)
    t.add_(1)
    assert Q.tensor_version(t) == (0, 1) and Q.tensor_version(t, 3) == (3, 1)
    with torch.inference_mode():
        u = torch.zeros(4)
        assert u.is_inference()
        assert Q.tensor_version(u) == (0, -1)
        u.add_(1)                                                      # undetectable, as documented: only the generation moves
        assert Q.tensor_version(u) == (0, -1) and Q.tensor_version(u, 1) == (1, -1)


def test_pblinear_from_dense_and_reload_inside_inference_mode():
    a0, b0, Wb = same_size_pair()
    with torch.inference_mode():
        W16, mask, r = rtn_fp16(SAME_SIZE_SEEDS[0])
        lay = Q.PBLinear.from_dense(W16, None, mask, -1, r["hscale"], r["hzero"])
        assert lay.pbl_blob.is_inference()
        p = lay.packed
        assert p is lay.packed                                         # nothing changed: the parsed header is reused
        assert header(p) == header(PackedWeight.from_blob(lay.pbl_blob)) == header(a0.packed)
        sd = lay.state_dict()
        assert torch.equal(sd["pbl_blob"], a0.pbl_blob)
        lay.load_state_dict(b0.state_dict())                           # into the inference-tensor buffer, in place
        p2 = lay.packed
        assert p2 is not p and header(p2) == header(b0.packed)         # the reload was seen: the NEW header, validated again
        assert torch.equal(lay.weight.float(), Wb.float())
        assert torch.equal(lay.state_dict()["pbl_blob"], b0.pbl_blob)
    # the same through the normal-tensor path: load_state_dict outside inference_mode
    lay2 = from_dense(SAME_SIZE_SEEDS[0])
    lay2.load_state_dict(b0.state_dict())
    assert header(lay2.packed) == header(b0.packed)


def test_dense_backed_cache_key_triggers():
    """every trigger _DenseBacked._cache_key documents changes the key; a `.data` edit does not (invalidate() is needed)"""
    torch.manual_seed(0)
    lin = Q.XnorBinaryLinear(torch.randn(32, 64), torch.randn(32))
    seen = [lin._cache_key()]

    def changed():
        k = lin._cache_key()
        new = k != seen[-1]
        seen.append(k)
        return new

    with torch.no_grad():
        lin.weight.copy_(torch.randn(32, 64))
    assert changed()
    lin.weight.data = torch.randn(32, 64)
    assert changed()
    lin.load_state_dict({"weight": torch.randn(32, 64), "bias": torch.randn(32)})
    assert changed()
    opt = torch.optim.SGD(lin.parameters(), lr=0.1)
    lin.weight.grad = torch.ones_like(lin.weight)
    opt.step()
    assert changed()
    lin.half()
    assert changed()
    lin.weight.data.copy_(torch.randn(32, 64).half())                 # NOT seen: `.data` has its own version counter
    assert not changed()
    # weights that are inference tensors: the key is readable, and a reload changes it
    with torch.inference_mode():
        inf = Q.XnorBinaryLinear(torch.randn(32, 64), torch.randn(32)).half()
        assert inf.weight.is_inference()
        k0 = inf._cache_key()
        inf.load_state_dict({"weight": torch.randn(32, 64), "bias": torch.randn(32)})
        assert inf._cache_key() != k0
    bx = Q.BinaryXnorExceptOutliersLinear(torch.randn(32, 64), None, 0.1)
    with torch.inference_mode():
        bi = Q.BinaryXnorExceptOutliersLinear(torch.randn(32, 64), None, 0.1)
        bi.outlier_mask, bi.binary_scale = torch.zeros(32, 64, dtype=torch.bool), torch.ones(1, 1)
        assert bi._cache_key()[1][1] == -1
    bx.outlier_mask = torch.zeros(32, 64, dtype=torch.bool)
    k = bx._cache_key()
    bx.outlier_mask[0, 0] = True
    assert bx._cache_key() != k                                        # an in-place mask edit is seen


def _version_reads(tree: ast.AST):
    """(enclosing function name, line) of every `<expr>._version` attribute in a module"""
    out = []

    def walk(node, fn):
        for child in ast.iter_child_nodes(node):
            name = child.name if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) else fn
            if isinstance(child, ast.Attribute) and child.attr == "_version":
                out.append((fn, child.lineno))
            walk(child, name)

    walk(tree, None)
    return out


def test_no_version_counter_read_outside_the_helper():
    pkg = os.path.join(REPO, "pb_llm_amd")
    found = {}
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            with open(os.path.join(pkg, f)) as fh:
                reads = _version_reads(ast.parse(fh.read(), f))
            if reads:
                found[f] = reads
    assert set(found) == {"quant.py"}, found
    assert {fn for fn, _ in found["quant.py"]} == {"tensor_version"}, found
    # the walker finds what it is meant to find
    assert _version_reads(ast.parse("def f(t):\n    return t._version\nx = y._version\n")) == [("f", 2), (None, 3)]
