"""-m gpu: the decode GEMV's prologue / epilogue / bf16 instantiations in EVERY launch configuration -- pbl_gemv_kernel<MB, WPB, SF,
SPLIT, XB, XP> for SPLIT = 8, 4, 2 (latency mode) and SPLIT = 1 with WPB = 4, on fp16-checkpoint (SF) and fp32-grid layers, with a
bias, exception entries and an N that is no multiple of 16, for M = 1 .. 4.  The shapes are gemv_cfg_cases.py's (the smallest that
reach each configuration; test_gemv_routes_cpu.py asks pbl_gemv_route that they do, and that no single-layer case declines an M).

References: float64 restatements of HF's arithmetic (test_decode_prologues_cpu.py) on the dense weight the oracle's decoder
(oracle/pb_format_ref.decode) reads out of the blob, under the project's parity bound (check_rows); the unfused composition on the GPU,
bit for bit where the kernel's fixed fma chain makes that an invariant (residual epilogues, bf16) and under the same bound where
the normaliser may differ by an ulp (RMSNorm; SwiGLU is compared both ways).

The oracle's decoder walks the records in Python (about 1.5 ms each).  Layers of up to 64 records are decoded whole.  Of the
larger ones (up to 8192 records) a sample of records is decoded -- the first and last two, every record holding an exception and 24
spread over the rest -- and must equal, bit for bit, the rows of the matrix the layer was packed from; the reference matrix is
that matrix with the decoded rows written over it."""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gemv_cfg_cases import FUSED, SINGLE, build_member, seed_of
from oracle import pb_format_ref
from oracle import pb_oracle as O
from pb_llm_amd import _lib, synth
from pb_llm_amd import quant as Q
from pb_llm_amd.packing import pack_dense
from pb_llm_amd.runtime import FusedGemv
from test_decode_prologues_cpu import linear_ref, rmsnorm_ref, silu_mul_ref
from test_gpu_decode_epilogues import exact, residual_rows
from test_gpu_decode_prologues import check_rows, norm_input, norm_weight, swiglu_input
from test_gpu_parity import _three_launch_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MS = (1, 2, 3, 4)
SENTINEL = -1536.0                                      # exact in fp16 and bf16; only elements that no member owns are compared with it


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()


# ---------------------------------------------------------------- layers and their reference weights
def decode_records(blob: np.ndarray, recs) -> np.ndarray:
    """the oracle's decoder on a blob holding only the records `recs` of `blob` (header and record table rebuilt around verbatim
    copies of the records): their rows, [16 len(recs), K] fp32"""
    h = pb_format_ref.read_header(blob)
    pos, NRB = h["rb_off_pos"], h["NRB"]
    info = blob[pos: pos + 16 * (NRB + 1)].view(np.uint32).reshape(NRB + 1, 4)
    off = info[:, 0].astype(np.int64) * 16
    n = len(recs)
    rec0 = (pos + 16 * (n + 1) + 127) & ~127
    table = np.zeros((n + 1, 4), np.uint32)
    parts, cur = [], rec0
    for i, b in enumerate(recs):
        table[i] = info[b]
        table[i, 0] = cur // 16
        parts.append(blob[off[b]: off[b + 1]])
        cur += int(off[b + 1] - off[b])
    table[n, 0] = cur // 16
    f = list(pb_format_ref.HDR.unpack(blob[:80].tobytes()))
    f[2], f[6], f[12] = 16 * n, n, cur                                # N, NRB, blob_bytes
    head = np.zeros(rec0, np.uint8)
    head[:80] = np.frombuffer(pb_format_ref.HDR.pack(*f), np.uint8)
    head[pos: pos + 16 * (n + 1)] = table.view(np.uint8).reshape(-1)
    return pb_format_ref.decode(np.concatenate([head] + parts))


def reference_weight(p, d) -> np.ndarray:
    """float64 [N, K]: what the oracle's decoder reads out of the blob (see the module docstring for layers of > 64 records)"""
    blob = p.blob.numpy()
    if p.NRB <= 64:
        W = pb_format_ref.decode(blob)
        assert np.array_equal(W, d["W"]), "the blob does not decode to the matrix it was packed from"
        return W.astype(np.float64)
    recs = sorted({0, 1, p.NRB - 2, p.NRB - 1} | {r // 16 for r, _ in d["exc"]} | set(np.linspace(2, p.NRB - 3, 24).astype(int).tolist()))
    rows = decode_records(blob, recs)
    W = d["W"].astype(np.float64)
    for i, b in enumerate(recs):
        n = min(16, p.N - 16 * b)
        assert np.array_equal(rows[16 * i: 16 * i + n], d["W"][16 * b: 16 * b + n]), ("record", b, "decodes to other rows")
        W[16 * b: 16 * b + n] = rows[16 * i: 16 * i + n]
    return W


@dataclass
class Member:
    lay: Q.PBLinear
    W: np.ndarray                # float64 [N, K], bias excluded
    bias: np.ndarray | None      # float64 [N]

    def ref(self, x):
        """x @ W^T + bias in float64"""
        y = linear_ref(x, self.W)
        return y if self.bias is None else y + self.bias


def build_layers(case, sal_f16):
    out = []
    for m, N in enumerate(case.Ns):
        d = build_member(N, case.K, seed_of(case, m, sal_f16), sal_f16, case.rich)
        p = pack_dense(d["W"], d["hi"], d["lo"], d["ss"], d["sz"], d["sal"], sal_f16=sal_f16)
        assert p.nexc == len(d["exc"]) and (2 <= p.nexc <= 5 if case.rich else p.nexc == 0), (case.name, p.nexc)
        assert bool(p.flags & _lib.PBL_FLAG_SAL_F16) == sal_f16 and p.G == 1
        W = reference_weight(p, d)
        bias = None if d["bias"] is None else torch.from_numpy(d["bias"])
        lay = Q.PBLinear(p, bias, torch.float16 if sal_f16 else torch.float32).to(DEV)
        out.append(Member(lay, W, None if bias is None else d["bias"].astype(np.float64)))
    # the configuration this set runs in, from the library (the CPU test holds the table to it)
    s, w = C.c_int(), C.c_int()
    members = len(case.Ns) if len(case.Ns) > 1 else 0
    assert _lib.lib().pbl_gemv_route(case.max_NRB, case.P, members, C.byref(s), C.byref(w)) == _lib.PBL_OK
    assert (s.value, w.value) == (case.split, case.wpb), (case.name, s.value, w.value)
    return out


def _id(param):
    case, f16 = param
    return f"{case.name}-{'f16' if f16 else 'f32'}"


@pytest.fixture(scope="module", params=[(c, f) for c in SINGLE for f in (True, False)], ids=_id)
def single(request):
    case, f16 = request.param
    return case, build_layers(case, f16)[0]


@pytest.fixture(scope="module", params=[(c, f) for c in FUSED for f in (True, False)], ids=_id)
def fused(request):
    case, f16 = request.param
    ms = build_layers(case, f16)
    return case, ms, FusedGemv([m.lay.packed for m in ms], [m.lay.pbl_bias for m in ms], DEV)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def offset_view(t: torch.Tensor, elems: int = 1) -> torch.Tensor:
    """a contiguous copy of t whose storage starts `elems` elements into a fresh buffer: the values of t at a base address that
    is no multiple of 16 bytes"""
    buf = torch.empty(t.numel() + elems + 8, dtype=t.dtype, device=t.device)
    v = buf[elems: elems + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16
    return v


def same_bits(a, b):
    """equal shape, dtype and values (NaN where NaN), whatever the strides: for views into a wider output"""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    torch.testing.assert_close(a.contiguous(), b.contiguous(), rtol=0, atol=0, equal_nan=True)


def rows_independent(run, x4, what):
    """the M = 4 result equals the four M = 1 results, bit for bit (run: [M, ...] input rows -> [M, N] output or a list of them)"""
    y4 = run(x4)
    y4 = y4 if isinstance(y4, (list, tuple)) else [y4]
    for i in range(x4.shape[0]):
        y1 = run(x4[i:i + 1].contiguous())
        y1 = y1 if isinstance(y1, (list, tuple)) else [y1]
        for a, b in zip(y4, y1):
            torch.testing.assert_close(a[i:i + 1].contiguous(), b.contiguous(), rtol=0, atol=0, equal_nan=True, msg=lambda s: f"{what} row {i}: {s}")
    return y4


def check_residual_rows(y, lin_ref, res, what):
    """y against the float64 statement of HF's two roundings, fp16(fp16(lin) + res), under check_rows' bound; a row holding
    +-inf or NaN is compared on its inf and NaN masks"""
    with np.errstate(over="ignore", invalid="ignore"):
        lin16 = lin_ref.astype(np.float16).astype(np.float64)
        ref = (lin16 + res.double().cpu().numpy()).astype(np.float16).astype(np.float64)
    yn = y.double().cpu().numpy()
    for i in range(ref.shape[0]):
        if np.isfinite(ref[i]).all():
            check_rows(y[i:i + 1], ref[i:i + 1], (what, "row", i))
        else:
            assert np.array_equal(np.isnan(yn[i]), np.isnan(ref[i])), (what, i, "NaN mask")
            assert np.array_equal(np.isposinf(yn[i]), np.isposinf(ref[i])) and np.array_equal(np.isneginf(yn[i]), np.isneginf(ref[i])), (what, i, "inf mask")


# ---------------------------------------------------------------- RMSNorm prologue (fused members)
NORM_ROWS = {1: [[0], [1], [2], [3], [4]], 2: [[0, 4], [1, 2]], 3: [[1, 2, 3], [0, 3, 4]], 4: [[0, 1, 3, 4], [1, 2, 3, 0]]}


def hf_norm(x, w, eps):
    from transformers.models.llama.modeling_llama import LlamaRMSNorm
    norm = LlamaRMSNorm(x.shape[1], eps=eps).half().to(DEV)
    with torch.no_grad():
        norm.weight.copy_(w)
        return norm(x)


def sentinel_call(entry, fg, ms, x, M, dtype, extra=()):
    """the fused launch through the C entry into a sentinel-filled buffer with gaps in front of, between and behind the members'
    columns: returns (the members' columns, True iff every other element of the buffer still holds the sentinel)"""
    Ns = [m.lay.out_features for m in ms]
    offs, cur = [], 3
    for n in Ns:
        offs.append(cur)
        cur += n + 5
    ldy = cur + 7
    buf = torch.full((M * ldy + 64,), SENTINEL, dtype=dtype, device=DEV)
    yoff = (C.c_uint64 * len(Ns))(*offs)
    rc = entry(C.addressof(fg._structs_host), C.addressof(yoff), x.data_ptr(), buf.data_ptr(), len(Ns), M, ldy, fg.max_NRB, fg.K,
               fg.max_nch, fg.flags, 0, *extra, torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.PBL_OK, rc
    grid = buf[:M * ldy].view(M, ldy)
    outs = [grid[:, o:o + n].clone() for o, n in zip(offs, Ns)]
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    km = keep[:M * ldy].view(M, ldy)
    for o, n in zip(offs, Ns):
        km[:, o:o + n] = False
    return outs, bool((buf[keep] == SENTINEL).all())


def test_rmsnorm_prologue(fused):
    """LlamaRMSNorm staged by the fused launch in this configuration, M = 1 .. 4, eps 1e-6 and 1e-5, all five row kinds of
    norm_input, a weight that is not all ones: against float64 and against norm-in-torch + the same launch (check_rows).  Scalar
    staging through a norm weight and an x that start one element off a 16-byte boundary (FusedGemv passes such views through:
    they are contiguous); uneven members into a sentinel-filled buffer; M = 4 equals four M = 1 launches bit for bit."""
    case, ms, fg = fused
    K = case.K
    X = norm_input(K, 300 + K)
    w16 = norm_weight(K, 7 + K)
    w = T(w16)
    for eps in (1e-6, 1e-5):
        for M in MS:
            for sel in NORM_ROWS[M] if eps == 1e-6 else NORM_ROWS[M][:1]:
                x16 = X[sel]
                x = T(x16)
                outs = fg(x, norm=(w, eps))
                assert outs is not None, (case.name, M, "the RMSNorm prologue declined")
                unfused = fg(hf_norm(x, w, eps))
                hn = rmsnorm_ref(x16, w16, eps, np.float16)
                for o, u, m in zip(outs, unfused, ms):
                    assert o.shape == (M, m.lay.out_features) and o.dtype == torch.float16
                    check_rows(o, m.ref(hn), ("float64", case.name, M, sel, eps))
                    check_rows(o, u.double().cpu().numpy(), ("unfused on the GPU", case.name, M, sel, eps))
    eps, sel = 1e-5, NORM_ROWS[4][0]
    x16 = X[sel]
    x = T(x16)
    hn = rmsnorm_ref(x16, w16, eps, np.float16)
    aligned = rows_independent(lambda xx: fg(xx, norm=(w, eps)), x, "RMSNorm prologue")
    for xv, wv, what in ((x, offset_view(w), "norm_w one element off"), (offset_view(x), w, "x one element off"),
                         (offset_view(x), offset_view(w), "both off")):
        outs = fg(xv, norm=(wv, eps))
        for o, a, m in zip(outs, aligned, ms):
            check_rows(o, m.ref(hn), ("float64", what, case.name))
            check_rows(o, a.double().cpu().numpy(), ("the aligned launch", what, case.name))   # (vector and scalar staging sum x^2 in another order)
            if K % 8:                                                # scalar staging either way: the same bits
                same_bits(o, a)
    # uneven members: every member's columns, and not one element beside them
    for M in (1, 4):
        xs = x[:M].contiguous()
        want = fg(xs, norm=(w, eps))
        outs, untouched = sentinel_call(_lib.lib().pbl_gemv_f16_fused_norm_host, fg, ms, xs, M, torch.float16,
                                        extra=(w.data_ptr(), C.c_float(eps)))
        assert untouched, (case.name, M, "a store outside the members' columns")
        for o, a in zip(outs, want):
            same_bits(o, a)


# ---------------------------------------------------------------- SwiGLU prologue (single layers)
def swiglu_case(M, K, seed):
    """swiglu_input's gates (+-30) and up / 16 (exact): the product stays around unit scale, so that in the residual variants the
    linear's fp16 rounding step stays under the parity bound's 1e-3 rms of the sum (see test_residual_epilogues)"""
    gate, up = swiglu_input(M, K, seed)
    return gate, (up.astype(np.float32) / 16).astype(np.float16)


def test_swiglu_prologue(single):
    """silu(gate) * up staged by the GEMV in this configuration, M = 1 .. 4: against float64 and the unfused composition
    (check_rows); the overflow row and the NaN-gate row of test_swiglu_prologue_down_shape; the scalar staging path through a
    gate/up matrix of width 2 K + 4 and through a view starting at column 3, both bit for bit the contiguous call's result."""
    case, m = single
    lay, K = m.lay, case.K
    for M in MS:
        gate, up = swiglu_case(M, K, 400 + M)
        gu = T(np.concatenate([gate, up], 1))
        y = lay.forward_swiglu(gu, K)
        assert y is not None and y.shape == (M, lay.out_features) and y.dtype == torch.float16, (case.name, M, "declined")
        with torch.no_grad():
            yu = lay(F.silu(gu[:, :K]) * gu[:, K:])
        check_rows(y, m.ref(silu_mul_ref(gate, up)), ("float64", case.name, M))
        check_rows(y, yu.double().cpu().numpy(), ("unfused on the GPU", case.name, M))
        # scalar staging: a row stride that is no multiple of 8, then a base address that is no multiple of 16 bytes
        wide = torch.zeros(M, 2 * K + 4, dtype=torch.float16, device=DEV)
        wide[:, :2 * K] = gu
        assert wide.stride(0) % 8 and wide[:, :2 * K].shape[1] == 2 * K
        exact(lay.forward_swiglu(wide, K), y)
        off = torch.zeros(M, 2 * K + 8, dtype=torch.float16, device=DEV)
        view = off[:, 3:3 + 2 * K]
        view.copy_(gu)
        assert view.data_ptr() % 16
        exact(lay.forward_swiglu(view, K), y)
        # non-finite rows: a product that overflows fp16 (silu(20) * 60000), a NaN gate -- as torch gives them
        g2, u2 = gate.copy(), up.copy()
        g2[0, 5], u2[0, 5] = 20.0, 60000.0
        if M > 1:
            g2[1, 9] = np.nan
        gu2 = T(np.concatenate([g2, u2], 1))
        t = F.silu(gu2[:, :K]) * gu2[:, K:]
        assert torch.isinf(t[0, 5])
        y2 = lay.forward_swiglu(gu2, K)
        with torch.no_grad():
            yu2 = lay(t)
        assert torch.equal(torch.isnan(y2), torch.isnan(yu2)) and torch.equal(torch.isinf(y2), torch.isinf(yu2)), (case.name, M)
        assert not torch.isfinite(y2[0]).any()
        if M > 1:
            assert torch.isnan(y2[1]).all()
        if M > 2:
            check_rows(y2[2:], m.ref(silu_mul_ref(g2, u2))[2:], ("float64, finite rows beside the others", case.name, M))
    gate, up = swiglu_case(4, K, 404)
    gate[1, 9] = np.nan
    rows_independent(lambda g: lay.forward_swiglu(g, K), T(np.concatenate([gate, up], 1)), "SwiGLU prologue")


# ---------------------------------------------------------------- residual epilogue, SwiGLU + residual (single layers)
def residual_views(res, N):
    """res, res as rows of a [M, N + 24] tensor (ldr > N), and the same starting at an odd column"""
    M = res.shape[0]
    wide = torch.full((M, N + 24), 77.0, dtype=torch.float16, device=DEV)
    a = wide[:, :N]
    a.copy_(res)
    wide2 = torch.full((M, N + 24), 77.0, dtype=torch.float16, device=DEV)
    b = wide2[:, 1:N + 1]
    b.copy_(res)
    assert b.data_ptr() % 4 == 2 and (M == 1 or (a.stride(0) == N + 24 and b.stride(0) == N + 24))
    return a, b


def test_residual_epilogues(single):
    """residual + layer(x) and residual + layer(silu(gate) * up) in the store of this configuration's GEMV, M = 1 .. 4, with
    residual_rows' three row kinds: bit for bit the unfused composition on the GPU (`res + layer(x)`, `res + forward_swiglu`),
    the same bits for a residual with row stride N + 24 and for one starting at an odd column, and against the float64
    statement of fp16(fp16(lin) + res) under check_rows' bound (rows holding +-inf / NaN: on their masks).

    The inputs keep the linear's output around unit scale (x ~ N(0, 1) on weights of about 0.01 sqrt(K) row norm; up / 16 for
    SwiGLU; row 1, whose residual sits at +-65504, is scaled by 256 so that its sums overflow) against a residual of standard
    deviation 4: where the kernel's fp32 sum and the float64 sum fall on different sides
    of an fp16 rounding boundary of `lin`, the results differ by one fp16 step of lin (at most 2^-8 for |lin| < 4), which
    stays under the bound's 1e-3 rms(ref) ~ 4e-3 however the sum cancels.  With lin and the residual of equal scale that
    double rounding -- not the kernel -- would exceed the bound at a few of the 5e5 outputs of the largest cases."""
    case, m = single
    lay, K, N = m.lay, case.K, lay_n(m)
    for M in MS:
        res = residual_rows(M, N, 500 + M)
        views = residual_views(res, N)
        # the residual epilogue
        x16 = synth.activations((M, K), 510 + M, 1)
        if M > 1:
            x16[1] *= np.float16(256)                               # (row 1 of the residual sits at +-65504: lin must reach 16 to overflow)
        x = T(x16)
        y = lay.forward_residual(x, res)
        assert y is not None and y.shape == (M, N), (case.name, M, "declined")
        with torch.no_grad():
            exact(y, res + lay(x))
        for v in views:
            exact(lay.forward_residual(x, v), y)
        check_residual_rows(y, m.ref(x16), res, ("residual epilogue", case.name, M))
        if M > 1:
            assert torch.isinf(y[1]).any()                          # (+-65504 + lin overflows somewhere)
        # SwiGLU + residual
        gate, up = swiglu_case(M, K, 520 + M)
        if M > 1:
            up[1] *= np.float16(256)
        gu = T(np.concatenate([gate, up], 1))
        ys = lay.forward_swiglu(gu, K, residual=res)
        plain = lay.forward_swiglu(gu, K)
        assert ys is not None and plain is not None, (case.name, M, "declined")
        exact(ys, res + plain)
        with torch.no_grad():
            exact(ys, res + lay(F.silu(gu[:, :K]) * gu[:, K:]))
        for v in views:
            exact(lay.forward_swiglu(gu, K, residual=v), ys)
        check_residual_rows(ys, m.ref(silu_mul_ref(gate, up)), res, ("SwiGLU + residual", case.name, M))
    res = residual_rows(4, N, 504)
    x = T(synth.activations((4, K), 514, 1))
    gate, up = swiglu_case(4, K, 524)
    gu = T(np.concatenate([gate, up], 1))
    pair = torch.cat([x, res], 1)                                      # (rows_independent slices inputs and residual together)
    rows_independent(lambda t: lay.forward_residual(t[:, :K].contiguous(), t[:, K:].contiguous()), pair, "residual epilogue")
    pair = torch.cat([gu, res], 1)
    rows_independent(lambda t: lay.forward_swiglu(t[:, :2 * K].contiguous(), K, residual=t[:, 2 * K:].contiguous()), pair, "SwiGLU + residual")


def lay_n(m):
    return m.lay.out_features


# ---------------------------------------------------------------- bf16 activations converted in the kernel
def bf16_tokens(M, K, seed, nonfinite):
    """unit-scale rows; one token holds a value beyond fp16's range (it is scaled); nonfinite: the last token holds -inf and,
    from two rows on, the first a NaN"""
    x = torch.from_numpy(synth.activations((M, K), seed, 21)).float()
    x[0, 5] = 7.0e4
    if nonfinite:
        x[M - 1, 9] = float("-inf")
        if M > 1:
            x[0, 11] = float("nan")
    return x.bfloat16().to(DEV)


def test_bf16_single_layer(single):
    """layer(x_bf16) -- ONE launch of this configuration's XB instantiation -- equals prepare + fp16 GEMV + finish
    (_three_launch_bf16) bit for bit, M = 1 .. 4, with a token beyond fp16's range and non-finite tokens; and float64 within
    bf16's output rounding (test_gpu_parity's 1e-2 of the largest output)."""
    case, m = single
    lay, K = m.lay, case.K
    for M in MS:
        xb = bf16_tokens(M, K, 600 + M, False)
        y = lay(xb)
        assert y.dtype == torch.bfloat16 and y.shape == (M, lay.out_features)
        exact(y, _three_launch_bf16(lay, xb))
        assert O.parity_errors(y.float().cpu().numpy(), m.ref(xb.double().cpu().numpy()))[0] < 1e-2, (case.name, M)
        xi = bf16_tokens(M, K, 610 + M, True)
        yi = lay(xi)
        exact(yi, _three_launch_bf16(lay, xi))
        assert not torch.isfinite(yi[M - 1]).all()
    rows_independent(lay, bf16_tokens(4, K, 620, True), "bf16 GEMV")


def test_bf16_fused(fused):
    """pbl_gemv_bf16_fused_host through FusedGemv equals the per-member single calls bit for bit, M = 1 .. 4 (finite and
    non-finite tokens); plain fp16 too; uneven members into a sentinel-filled buffer."""
    case, ms, fg = fused
    K = case.K
    for M in MS:
        for nonfinite in (False, True):
            xb = bf16_tokens(M, K, 700 + M, nonfinite)
            outs = fg(xb)
            for o, m in zip(outs, ms):
                assert o.dtype == torch.bfloat16
                same_bits(o, m.lay(xb))
        xh = T(synth.activations((M, K), 710 + M, 1))
        for o, m in zip(fg(xh), ms):
            same_bits(o, m.lay(xh))
            check_rows(o, m.ref(xh.double().cpu().numpy()), ("fp16 fused, float64", case.name, M))
    rows_independent(lambda t: fg(t), bf16_tokens(4, K, 720, True), "bf16 fused GEMV")
    for M in (1, 4):
        xb = bf16_tokens(M, K, 730 + M, False)
        want = fg(xb)
        outs, untouched = sentinel_call(_lib.lib().pbl_gemv_bf16_fused_host, fg, ms, xb, M, torch.bfloat16)
        assert untouched, (case.name, M, "a store outside the members' columns")
        for o, a in zip(outs, want):
            same_bits(o, a)
