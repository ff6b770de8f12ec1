"""Launch helpers above the C ABI: a group of independent PB linears in ONE kernel
launch (fused QKV / gate+up at decode time; the L-layer stream benchmark of
SURVEY.md 8(d)).  Device-resident descriptor tables are built once and reused, so
a launch is a single pbl_gemv_f16_grouped call and is hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .packing import PackedWeight


class GroupedGemv:
    """y_l = x_l @ W_l^T (+ b_l) for l in 0..L-1, all in one launch.  M <= 4 tokens."""

    def __init__(self, packed: list[PackedWeight], biases: list[torch.Tensor | None] | None = None,
                 M: int = 1, device="cuda", shared_x: bool = False, out_f32: bool = False):
        if not packed:
            raise ValueError("empty group")
        if not 1 <= M <= _lib.PBL_MAX_TOKENS_PER_LAUNCH:
            raise ValueError("grouped launch handles 1..4 tokens")
        self.device = torch.device(device)
        self.M = M
        self.packed = [p if p.blob.device == self.device else p.to(self.device) for p in packed]
        biases = biases or [None] * len(packed)
        self.biases = [b.detach().float().to(self.device) if b is not None else None for b in biases]
        if shared_x and len({p.K for p in self.packed}) != 1:
            raise ValueError("shared_x needs equal in_features")
        Kmax = max(p.K for p in self.packed)
        if shared_x:
            xs = torch.zeros(M, Kmax, dtype=torch.float16, device=self.device)
            self.x = [xs] * len(self.packed)
        else:
            self.x = [torch.zeros(M, p.K, dtype=torch.float16, device=self.device) for p in self.packed]
        # one contiguous output buffer (a single all-reduce covers the whole group when sharded)
        self.out_f32 = out_f32
        self.y_all = torch.empty(sum(M * p.N for p in self.packed), dtype=torch.float32 if out_f32 else torch.float16,
                                 device=self.device)
        offs = np.cumsum([0] + [M * p.N for p in self.packed])
        self.y = [self.y_all[offs[i]:offs[i + 1]].view(M, p.N) for i, p in enumerate(self.packed)]
        structs = (_lib.PblLayer * len(self.packed))(*[p.layer_struct(b) for p, b in zip(self.packed, self.biases)])
        raw = np.frombuffer(bytes(structs), dtype=np.uint8).copy()
        self._layers_dev = torch.from_numpy(raw).to(self.device)
        self._x_ptrs = torch.tensor([t.data_ptr() for t in self.x], dtype=torch.int64, device=self.device)
        self._y_ptrs = torch.tensor([t.data_ptr() for t in self.y], dtype=torch.int64, device=self.device)
        self.max_NRB = max(p.NRB for p in self.packed)
        self.max_K = Kmax
        self.max_nch = max(p.max_nch for p in self.packed)
        self.max_nexc = max(p.max_nexc for p in self.packed)
        # bit 0: column-group layers present (the launch then runs the column-group kernel), bit 1: fp16-checkpoint layers present
        self.any_groups = int(any(p.G > 1 for p in self.packed)) | (2 * int(any(p.flags & _lib.PBL_FLAG_SAL_F16 for p in self.packed)))

    def algorithmic_bytes(self) -> int:
        return sum(p.algorithmic_bytes(self.M, b is not None) for p, b in zip(self.packed, self.biases))

    def packed_bytes(self) -> int:
        return sum(p.nbytes for p in self.packed)

    def launch(self, stream: torch.cuda.Stream | None = None) -> list[torch.Tensor]:
        st = (stream or torch.cuda.current_stream(self.device)).cuda_stream
        _lib.check(_lib.lib().pbl_gemv_f16_grouped(
            self._layers_dev.data_ptr(), self._x_ptrs.data_ptr(), self._y_ptrs.data_ptr(), len(self.packed),
            self.M, self.max_NRB, self.max_K, self.max_nch, self.max_nexc, self.any_groups, int(self.out_f32), st),
            "grouped gemv")
        return self.y


class FusedGemv:
    """Decode-time fusion of projections that read the same activation (q/k/v; gate/up): ONE launch, one output tensor.
    __call__(x [M <= 4, K] fp16) -> list of [M, N_l] views of a fresh [M, sum N_l] tensor.  No pointer table refers to x
    or y (pbl_gemv_f16_fused), so every call may use new tensors and the launch can be captured in a hipGraph."""

    def __init__(self, packed: list[PackedWeight], biases: list[torch.Tensor | None] | None = None, device="cuda"):
        if not packed:
            raise ValueError("empty group")
        if len({p.K for p in packed}) != 1:
            raise ValueError("fused projections share their input: equal in_features")
        self.device = torch.device(device)
        self.packed = [p if p.blob.device == self.device else p.to(self.device) for p in packed]
        biases = biases or [None] * len(packed)
        self.biases = [b.detach().float().to(self.device) if b is not None else None for b in biases]
        self.K = self.packed[0].K
        self.Ns = [p.N for p in self.packed]
        self.offs = np.cumsum([0] + self.Ns)
        structs = (_lib.PblLayer * len(self.packed))(*[p.layer_struct(b) for p, b in zip(self.packed, self.biases)])
        self._layers_dev = torch.from_numpy(np.frombuffer(bytes(structs), dtype=np.uint8).copy()).to(self.device)
        self._yoff_dev = torch.tensor(self.offs[:-1].tolist(), dtype=torch.int64, device=self.device)
        # up to PBL_FUSED_INLINE_MAX members: descriptors and offsets go into the kernel arguments (pbl_gemv_f16_fused_host)
        self._inline = len(self.packed) <= _lib.PBL_FUSED_INLINE_MAX
        self._structs_host = structs
        self._yoff_host = (C.c_uint64 * len(self.packed))(*[int(o) for o in self.offs[:-1]])
        self.max_NRB = max(p.NRB for p in self.packed)
        self.max_nch = max(p.max_nch for p in self.packed)
        # bit 0: column-group layers present (the launch then runs the column-group kernel), bit 1: fp16-checkpoint layers present
        self.flags = int(any(p.G > 1 for p in self.packed)) | 2 * int(any(p.flags & _lib.PBL_FLAG_SAL_F16 for p in self.packed))
        self.bf16_ok = self._inline and not (self.flags & 1)

    def __call__(self, x2: torch.Tensor, out_f32: bool = False, norm=None) -> list[torch.Tensor] | None:
        """norm=(weight, eps): x2 is the RAW hidden state and the launch multiplies LlamaRMSNorm(x2) (weight [K] fp16, the norm's
        variance_epsilon) -- the normalisation runs in the kernel's staging phase (pbl_gemv_f16_fused_norm_host).  None when that
        entry declines (column groups, more rows than one pass takes): the caller applies the norm itself and calls again."""
        y = self.run(x2, out_f32, norm)
        if y is None:
            return None
        return [y[:, int(self.offs[i]):int(self.offs[i + 1])] for i in range(len(self.packed))]

    def run(self, x2: torch.Tensor, out_f32: bool = False, norm=None) -> torch.Tensor | None:
        """the launch behind __call__: the whole [M, sum N_l] output (member l at columns offs[l] .. offs[l + 1])"""
        M = x2.shape[0]
        if x2.dtype not in (torch.float16, torch.bfloat16) or not x2.is_contiguous() or x2.shape[1] != self.K or not 1 <= M <= _lib.PBL_MAX_TOKENS_PER_LAUNCH:
            raise _lib.PblError("FusedGemv: x must be a contiguous fp16 / bf16 [M <= 4, K] tensor")
        total = int(self.offs[-1])
        L = _lib.lib()
        if norm is not None:
            w, eps = norm
            if x2.dtype != torch.float16 or w.dtype != torch.float16 or w.device != x2.device or not w.is_contiguous() or w.numel() != self.K:
                raise _lib.PblError("FusedGemv: the RMSNorm prologue takes fp16 x and an fp16 [K] weight on x's device")
            if not self._inline:
                return None
            y = torch.empty(M, total, dtype=torch.float32 if out_f32 else x2.dtype, device=x2.device)
            st = torch.cuda.current_stream(x2.device).cuda_stream
            rc = L.pbl_gemv_f16_fused_norm_host(C.addressof(self._structs_host), C.addressof(self._yoff_host), x2.data_ptr(), y.data_ptr(),
                                                len(self.packed), M, total, self.max_NRB, self.K, self.max_nch, self.flags,
                                                int(out_f32), w.data_ptr(), float(eps), st)
            if rc == _lib.PBL_ERR_UNSUPPORTED:
                return None
            _lib.check(rc, "fused gemv (RMSNorm prologue)")
            return y
        y = torch.empty(M, total, dtype=torch.float32 if out_f32 else x2.dtype, device=x2.device)
        st = torch.cuda.current_stream(x2.device).cuda_stream
        if x2.dtype == torch.bfloat16:
            # bf16 activations converted IN the launch, bf16 result (pbl_gemv_bf16_fused_host; group-free members, at most
            # PBL_FUSED_INLINE_MAX of them: what q/k/v and gate/up are)
            if not self.bf16_ok:
                raise _lib.PblError("FusedGemv: bf16 activations need group-free members and at most 4 of them")
            _lib.check(L.pbl_gemv_bf16_fused_host(C.addressof(self._structs_host), C.addressof(self._yoff_host), x2.data_ptr(), y.data_ptr(),
                                                  len(self.packed), M, total, self.max_NRB, self.K, self.max_nch, self.flags,
                                                  int(out_f32), st), "fused gemv (bf16)")
        elif self._inline:
            _lib.check(L.pbl_gemv_f16_fused_host(C.addressof(self._structs_host), C.addressof(self._yoff_host), x2.data_ptr(), y.data_ptr(),
                                                 len(self.packed), M, total, self.max_NRB, self.K, self.max_nch, self.flags,
                                                 int(out_f32), st), "fused gemv")
        else:
            _lib.check(L.pbl_gemv_f16_fused(self._layers_dev.data_ptr(), self._yoff_dev.data_ptr(), x2.data_ptr(), y.data_ptr(),
                                            len(self.packed), M, total, self.max_NRB, self.K, self.max_nch, self.flags,
                                            int(out_f32), st), "fused gemv")
        return y

    def algorithmic_bytes(self, M: int = 1) -> int:
        # x is read once for the group, not once per layer
        return sum(p.algorithmic_bytes(M, b is not None) for p, b in zip(self.packed, self.biases)) - 2 * M * self.K * (len(self.packed) - 1)


_ROPE_LAYOUTS: dict = {}


def _rope_layout(qkv: torch.Tensor, q_off: int, k_off: int, batch: int, seq: int, n_q: int, n_kv: int, head_dim: int,
                 cos: torch.Tensor, sin: torch.Tensor):
    """(shape, strides) of q_embed and k_embed as HF's apply_rotary_pos_emb returns them for the q / k views of qkv that a fused
    q/k/v launch hands LlamaAttention -- found once per layout by running the same torch ops on meta tensors (TensorIterator's
    stride rules, torch.cat's memory format) and cached"""
    key = (batch, seq, n_q, n_kv, head_dim, qkv.stride(0), q_off, k_off, tuple(cos.shape), cos.stride(), sin.stride())
    got = _ROPE_LAYOUTS.get(key)
    if got is None:
        def meta(t):
            return torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device="meta")

        def view(off, n):
            return meta(qkv[:, off:off + n * head_dim].reshape(batch, seq, n * head_dim).view(batch, seq, -1, head_dim).transpose(1, 2))

        c, s = meta(cos).unsqueeze(1), meta(sin).unsqueeze(1)
        h = head_dim // 2
        outs = [(x * c) + (torch.cat((-x[..., h:], x[..., :h]), dim=-1) * s) for x in (view(q_off, n_q), view(k_off, n_kv))]
        got = _ROPE_LAYOUTS[key] = tuple((tuple(o.shape), tuple(o.stride())) for o in outs)
    return got


def _rope_form(what: str, qkv: torch.Tensor, heads, batch: int, seq: int, head_dim: int, cos: torch.Tensor, sin: torch.Tensor):
    """The argument form rope_f16 and rope_append_f16 (`what`) share.  ValueError unless qkv is an fp16 [batch * seq, n] GPU tensor
    with unit column stride whose rows hold every (column offset, head count) of `heads`.  Returns (ld, the entry's five cos / sin
    arguments) -- or None where cos / sin are not fp16 [1 or batch, 1 or seq, head_dim] tensors of one layout on qkv's device."""
    if qkv.dim() != 2 or qkv.dtype != torch.float16 or not qkv.is_cuda or qkv.stride(1) != 1 or qkv.shape[0] != batch * seq:
        raise ValueError(f"{what}: qkv must be an fp16 [batch * seq, n] GPU tensor with unit column stride")
    if min(off for off, _ in heads) < 0 or max(off + n * head_dim for off, n in heads) > qkv.shape[1]:
        raise ValueError(f"{what}: the {' / '.join('qkv'[:len(heads)])} heads must lie inside a row of qkv")
    if cos.dtype != torch.float16 or sin.dtype != torch.float16 or cos.device != qkv.device or sin.device != qkv.device \
            or cos.dim() != 3 or cos.shape != sin.shape or cos.stride() != sin.stride() or cos.stride(-1) != 1 \
            or cos.shape[0] not in (1, batch) or cos.shape[1] not in (1, seq) or cos.shape[-1] != head_dim:
        return None
    return qkv.stride(0) if qkv.shape[0] > 1 else qkv.shape[1], (
        cos.data_ptr(), sin.data_ptr(), head_dim, cos.stride(0) if cos.shape[0] > 1 else 0, cos.stride(1) if cos.shape[1] > 1 else 0)


def rope_f16(qkv: torch.Tensor, q_off: int, k_off: int, batch: int, seq: int, n_q: int, n_kv: int, head_dim: int,
             cos: torch.Tensor, sin: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor] | None:
    """HF's apply_rotary_pos_emb(q, k, cos, sin) in ONE launch (pbl_rope_f16) for the q and k heads of a fused q/k/v output: qkv
    [batch * seq, >= ...] fp16 with unit column stride holds n_q q heads from column q_off and n_kv k heads from column k_off
    (head_dim each); cos / sin [1 or batch, 1 or seq, head_dim] fp16 (position_embeddings).  Returns (q_embed, k_embed) with
    the values, shapes and strides HF's function gives for the views LlamaAttention makes of a fused launch's output -- or None
    where the entry declines (odd head_dim, head_dim > 256) or cos / sin are not of that form: the caller then runs HF's."""
    form = _rope_form("rope_f16", qkv, ((q_off, n_q), (k_off, n_kv)), batch, seq, head_dim, cos, sin)
    if form is None or head_dim % 2 or head_dim > 256:
        return None
    (qs, qst), (ks, kst) = _rope_layout(qkv, q_off, k_off, batch, seq, n_q, n_kv, head_dim, cos, sin)
    if qst[3] != 1 or kst[3] != 1 or qs != (batch, n_q, seq, head_dim) or ks != (batch, n_kv, seq, head_dim):
        return None
    q = torch.empty_strided(qs, qst, dtype=torch.float16, device=qkv.device)
    k = torch.empty_strided(ks, kst, dtype=torch.float16, device=qkv.device)
    rc = _lib.lib().pbl_rope_f16(qkv.data_ptr(), form[0], q_off, k_off, batch, seq, n_q, n_kv, head_dim, *form[1],
                                 q.data_ptr(), (C.c_int64 * 3)(*qst[:3]), k.data_ptr(), (C.c_int64 * 3)(*kst[:3]),
                                 torch.cuda.current_stream(qkv.device).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "rope")
    return q, k


def _cache_args(k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor, device, what: str):
    """(B, Hkv, max_len, D) of a layer's static KV cache, after checking its form: [B, Hkv, max_len, D] fp16 contiguous k / v on
    `device` and a one-element int64 position there (HF StaticLayer.keys / .values / .cumulative_length)"""
    if k_cache.dtype != torch.float16 or v_cache.dtype != torch.float16 or k_cache.dim() != 4 or k_cache.shape != v_cache.shape \
            or not k_cache.is_contiguous() or not v_cache.is_contiguous() or k_cache.device != device or v_cache.device != device:
        raise ValueError(f"{what}: k_cache / v_cache must be contiguous fp16 [B, Hkv, max_len, D] tensors on the activations' device")
    if pos.dtype != torch.int64 or pos.numel() != 1 or pos.device != device:
        raise ValueError(f"{what}: pos must be a one-element int64 tensor on the activations' device")
    return tuple(int(d) for d in k_cache.shape)


def decode_attention_ok(batch: int, seq: int, n_q: int, n_kv: int, head_dim: int, max_len: int) -> bool:
    """the scope of rope_append_f16 + decode_attention_f16: where both entries run (the caller checks BEFORE the first of them, so
    that a cache row is never appended without the attention that advances the position)"""
    return head_dim in (64, 128) and 1 <= seq <= 4 and 1 <= batch <= 4 and n_kv >= 1 and n_q % n_kv == 0 and 1 <= max_len <= 65536


def rope_append_f16(qkv: torch.Tensor, q_off: int, k_off: int, v_off: int, batch: int, seq: int, n_q: int, n_kv: int, head_dim: int,
                    cos: torch.Tensor, sin: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                    pos: torch.Tensor) -> torch.Tensor | None:
    """rope_f16's q (same values, shape and strides), and in the same launch (pbl_rope_append_f16) the rotated k heads and the raw v
    heads (n_kv heads from column v_off of qkv) written into rows [pos, pos + seq) of the layer's static cache k_cache / v_cache
    [batch, n_kv, max_len, head_dim] fp16; pos (int64, on the device, read there) is not changed.  None where the entry declines
    (head_dim not 64 / 128, seq > 4, batch > 4, n_q % n_kv) or cos / sin are not of rope_f16's form."""
    form = _rope_form("rope_append_f16", qkv, ((q_off, n_q), (k_off, n_kv), (v_off, n_kv)), batch, seq, head_dim, cos, sin)
    B, Hkv, max_len, D = _cache_args(k_cache, v_cache, pos, qkv.device, "rope_append_f16")
    if (B, Hkv, D) != (batch, n_kv, head_dim):
        raise ValueError("rope_append_f16: the cache is not [batch, n_kv, max_len, head_dim]")
    if form is None or not decode_attention_ok(batch, seq, n_q, n_kv, head_dim, max_len):
        return None
    (qs, qst), _ = _rope_layout(qkv, q_off, k_off, batch, seq, n_q, n_kv, head_dim, cos, sin)
    if qst[3] != 1 or qs != (batch, n_q, seq, head_dim):
        return None
    q = torch.empty_strided(qs, qst, dtype=torch.float16, device=qkv.device)
    rc = _lib.lib().pbl_rope_append_f16(qkv.data_ptr(), form[0], q_off, k_off, v_off, batch, seq, n_q, n_kv, head_dim, *form[1],
                                        q.data_ptr(), (C.c_int64 * 3)(*qst[:3]), k_cache.data_ptr(), v_cache.data_ptr(), max_len,
                                        pos.data_ptr(), torch.cuda.current_stream(qkv.device).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "rope + cache append")
    return q


def decode_attention_f16(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor,
                         scaling: float) -> torch.Tensor | None:
    """softmax(scaling q k^T) v of a decode step over a static KV cache (pbl_decode_attn_f16): q [B, Hq, S, D] fp16 (unit d stride:
    rope_append_f16's q), k_cache / v_cache [B, Hkv, max_len, D] fp16, pos the int64 device position -- query row s attends to
    cache rows [0, pos + s].  Returns [B * S, Hq * D] fp16 (what LlamaAttention hands o_proj) and advances pos by S on the device.
    None where the entry declines (decode_attention_ok)."""
    if q.dim() != 4 or q.dtype != torch.float16 or not q.is_cuda or q.stride(3) != 1 or min(q.stride()) < 0:
        raise ValueError("decode_attention_f16: q must be an fp16 [B, Hq, S, D] GPU tensor with unit d stride")
    B, Hq, S, D = (int(d) for d in q.shape)
    Bc, Hkv, max_len, Dc = _cache_args(k_cache, v_cache, pos, q.device, "decode_attention_f16")
    if (Bc, Dc) != (B, D):
        raise ValueError("decode_attention_f16: the cache is not [B, Hkv, max_len, D] for q [B, Hq, S, D]")
    if not decode_attention_ok(B, S, Hq, Hkv, D, max_len):
        return None
    L = _lib.lib()
    out = torch.empty(B * S, Hq * D, dtype=torch.float16, device=q.device)
    ws = torch.empty(int(L.pbl_decode_attn_workspace_bytes(B, S, Hq, D, max_len)), dtype=torch.uint8, device=q.device)
    rc = L.pbl_decode_attn_f16(q.data_ptr(), (C.c_int64 * 3)(*q.stride()[:3]), k_cache.data_ptr(), v_cache.data_ptr(), B, S, Hq, Hkv,
                               D, max_len, float(scaling), pos.data_ptr(), out.data_ptr(), Hq * D, ws.data_ptr(), ws.numel(),
                               torch.cuda.current_stream(q.device).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "decode attention")
    return out


def prefill_attention_ok(batch: int, seq: int, n_q: int, n_kv: int, head_dim: int, max_len: int) -> bool:
    """the scope of prefill_attention_f16 (pbl_prefill_attn_f16): any batch and any seq >= 1 that fits the cache, head_dim 64 or 128,
    n_kv dividing n_q, a grid that fits and a cache of at most 2^40 elements"""
    return head_dim in (64, 128) and 1 <= batch <= 65535 and 1 <= seq <= max_len and n_kv >= 1 and 1 <= n_q <= 65535 \
        and n_q % n_kv == 0 and batch * n_kv * max_len * head_dim <= 1 << 40


def prefill_attention_f16(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                          pos: torch.Tensor, scaling: float) -> torch.Tensor | None:
    """Causal attention of S new rows over a static KV cache (pbl_prefill_attn_f16): q [B, Hq, S, D], k / v [B, Hkv, S, D] fp16 with
    unit d stride (rope_f16's q and k; v a strided view of the q/k/v output), k_cache / v_cache [B, Hkv, max_len, D] fp16, pos the
    int64 device position.  Appends k / v to cache rows [pos, pos + S), lets query row s attend to cache rows [0, pos + s], returns
    [B * S, Hq * D] fp16 (what LlamaAttention hands o_proj) and advances pos by S on the device.  None where the entry declines
    (prefill_attention_ok); the cache and pos are then untouched."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dim() != 4 or t.dtype != torch.float16 or not t.is_cuda or t.device != q.device or t.stride(3) != 1 or min(t.stride()) < 0:
            raise ValueError(f"prefill_attention_f16: {name} must be an fp16 [B, H, S, D] GPU tensor with unit d stride")
    B, Hq, S, D = (int(d) for d in q.shape)
    Bc, Hkv, max_len, Dc = _cache_args(k_cache, v_cache, pos, q.device, "prefill_attention_f16")
    if (Bc, Dc) != (B, D) or tuple(k.shape) != (B, Hkv, S, D) or k.shape != v.shape:
        raise ValueError("prefill_attention_f16: k / v must be [B, Hkv, S, D] and the cache [B, Hkv, max_len, D] for q [B, Hq, S, D]")
    if not prefill_attention_ok(B, S, Hq, Hkv, D, max_len):
        return None
    out = torch.empty(B * S, Hq * D, dtype=torch.float16, device=q.device)
    rc = _lib.lib().pbl_prefill_attn_f16(q.data_ptr(), (C.c_int64 * 3)(*q.stride()[:3]), k.data_ptr(), (C.c_int64 * 3)(*k.stride()[:3]),
                                         v.data_ptr(), (C.c_int64 * 3)(*v.stride()[:3]), k_cache.data_ptr(), v_cache.data_ptr(), B, S,
                                         Hq, Hkv, D, max_len, float(scaling), pos.data_ptr(), out.data_ptr(), Hq * D,
                                         torch.cuda.current_stream(q.device).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "prefill attention")
    return out


def branch_attention_ok(batch: int, seq: int, n_q: int, n_kv: int, head_dim: int, max_len: int) -> bool:
    """the scope of branch_attention_f16 (pbl_branch_attn_f16): prefill_attention_ok's"""
    return prefill_attention_ok(batch, seq, n_q, n_kv, head_dim, max_len)


def branch_attention_f16(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                         pos: torch.Tensor, scaling: float, trunk: torch.Tensor, lo: torch.Tensor) -> torch.Tensor | None:
    """prefill_attention_f16 for S rows packed as [ shared context | branch 0 | branch 1 | ... | padding ] (pbl_branch_attn_f16): the
    same arguments, contract and result, plus trunk (int32 [B], >= 1: the context's rows) and lo (int32 [B, S] contiguous: the packed
    index of the first row of row s's own branch; 0 for a context row, s for a padding row), both on q's device.  Query row s attends
    to cache row k iff k <= pos + s and (k < pos + trunk[b] or k >= pos + lo[b, s]).  None where the entry declines
    (branch_attention_ok); the cache and pos are then untouched."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dim() != 4 or t.dtype != torch.float16 or not t.is_cuda or t.device != q.device or t.stride(3) != 1 or min(t.stride()) < 0:
            raise ValueError(f"branch_attention_f16: {name} must be an fp16 [B, H, S, D] GPU tensor with unit d stride")
    B, Hq, S, D = (int(d) for d in q.shape)
    Bc, Hkv, max_len, Dc = _cache_args(k_cache, v_cache, pos, q.device, "branch_attention_f16")
    if (Bc, Dc) != (B, D) or tuple(k.shape) != (B, Hkv, S, D) or k.shape != v.shape:
        raise ValueError("branch_attention_f16: k / v must be [B, Hkv, S, D] and the cache [B, Hkv, max_len, D] for q [B, Hq, S, D]")
    for name, t, shape in (("trunk", trunk, (B,)), ("lo", lo, (B, S))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or t.device != q.device or not t.is_contiguous():
            raise ValueError(f"branch_attention_f16: {name} must be a contiguous int32 {list(shape)} tensor on the activations' device")
    if not branch_attention_ok(B, S, Hq, Hkv, D, max_len):
        return None
    out = torch.empty(B * S, Hq * D, dtype=torch.float16, device=q.device)
    rc = _lib.lib().pbl_branch_attn_f16(q.data_ptr(), (C.c_int64 * 3)(*q.stride()[:3]), k.data_ptr(), (C.c_int64 * 3)(*k.stride()[:3]),
                                        v.data_ptr(), (C.c_int64 * 3)(*v.stride()[:3]), k_cache.data_ptr(), v_cache.data_ptr(),
                                        trunk.data_ptr(), lo.data_ptr(), B, S, Hq, Hkv, D, max_len, float(scaling), pos.data_ptr(),
                                        out.data_ptr(), Hq * D, torch.cuda.current_stream(q.device).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "branch attention")
    return out


# ---- the FP8 KV cache (csrc/pbl_kv8.hip; the format is stated in include/pbl.h) -------------------------------------------------------
KV8_E_MIN, KV8_E_MAX, KV8_MAX = -15, 7, 448.0


def kv8_quantize(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The torch reference of the FP8 cache's row format (any device, CPU included): x [..., D] (the fp16 values the fp16 cache would
    hold) -> (bytes uint8 [..., D], scale fp32 [...]).  Per row: amax = max |x|; e = the smallest integer with amax <= 448 * 2^e,
    clamped to [-15, 7] (an all-zero row: -15); scale = 2^e; byte j = e4m3fn(x_j / 2^e), round to nearest even.  After the clamp at
    e = 7 a row with amax > 57344 (+-inf included) saturates at +-448; a NaN element becomes a NaN byte and does not enter amax."""
    xf = x.detach().float()
    amax = torch.nan_to_num(xf.abs(), nan=0.0, posinf=float("inf")).amax(-1)
    m, ex = torch.frexp(amax)                               # amax = m * 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9
    e = ex.to(torch.int32) - 9 + (m > 0.875).to(torch.int32)
    e = torch.where(amax == 0, torch.full_like(e, KV8_E_MIN), e)
    e = torch.where(torch.isinf(amax), torch.full_like(e, KV8_E_MAX), e).clamp(KV8_E_MIN, KV8_E_MAX)
    scale = torch.ldexp(torch.ones_like(amax), e)
    y = (xf / scale[..., None]).clamp(-KV8_MAX, KV8_MAX)    # (exact: a power of two; NaN stays NaN)
    return y.to(torch.float8_e4m3fn).view(torch.uint8), scale


def kv8_dequantize(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """kv8_quantize's inverse on what it kept: bytes uint8 [..., D] and scale fp32 [...] -> fp16 [..., D], every value exact (a 4-bit
    significand between 2^-24 and 57344 for scales the format allows)"""
    return (q.view(torch.float8_e4m3fn).float() * scale[..., None].float()).to(torch.float16)


def kv8_ok(batch: int, seq: int, n_q: int, n_kv: int, head_dim: int, max_len: int) -> bool:
    """the scope of the FP8 cache's entries together: rope_append_kv8 + decode_attention_kv8 at seq <= 4 rows, prefill_attention_kv8
    above -- head_dim 64 or 128, batch <= 4, n_kv dividing n_q, 1 <= seq <= max_len <= 65536"""
    return head_dim in (64, 128) and 1 <= batch <= 4 and 1 <= seq <= max_len <= 65536 and n_kv >= 1 and n_q >= 1 and n_q % n_kv == 0


def _cache_args_kv8(k_cache, v_cache, k_scale, v_scale, pos, device, what: str):
    """_cache_args for the FP8 cache: [B, Hkv, max_len, D] uint8 k / v with [B, Hkv, max_len] fp32 scales, all contiguous on `device`"""
    if k_cache.dtype != torch.uint8 or v_cache.dtype != torch.uint8 or k_cache.dim() != 4 or k_cache.shape != v_cache.shape \
            or not k_cache.is_contiguous() or not v_cache.is_contiguous() or k_cache.device != device or v_cache.device != device:
        raise ValueError(f"{what}: k_cache / v_cache must be contiguous uint8 [B, Hkv, max_len, D] tensors on the activations' device")
    for t in (k_scale, v_scale):
        if t.dtype != torch.float32 or t.shape != k_cache.shape[:3] or not t.is_contiguous() or t.device != device:
            raise ValueError(f"{what}: k_scale / v_scale must be contiguous fp32 [B, Hkv, max_len] tensors on the activations' device")
    if pos.dtype != torch.int64 or pos.numel() != 1 or pos.device != device:
        raise ValueError(f"{what}: pos must be a one-element int64 tensor on the activations' device")
    return tuple(int(d) for d in k_cache.shape)


def rope_append_kv8(qkv: torch.Tensor, q_off: int, k_off: int, v_off: int, batch: int, seq: int, n_q: int, n_kv: int, head_dim: int,
                    cos: torch.Tensor, sin: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor,
                    v_scale: torch.Tensor, pos: torch.Tensor) -> torch.Tensor | None:
    """rope_append_f16 over the FP8 cache (pbl_rope_append_kv8): the same q, bit for bit; the rotated k heads and the raw v heads are
    quantised (kv8_quantize's rule) into rows [pos, pos + seq) of k_cache / v_cache [batch, n_kv, max_len, head_dim] uint8 and their
    scales into k_scale / v_scale [batch, n_kv, max_len] fp32; pos is not changed.  None where rope_append_f16 returns None."""
    form = _rope_form("rope_append_kv8", qkv, ((q_off, n_q), (k_off, n_kv), (v_off, n_kv)), batch, seq, head_dim, cos, sin)
    B, Hkv, max_len, D = _cache_args_kv8(k_cache, v_cache, k_scale, v_scale, pos, qkv.device, "rope_append_kv8")
    if (B, Hkv, D) != (batch, n_kv, head_dim):
        raise ValueError("rope_append_kv8: the cache is not [batch, n_kv, max_len, head_dim]")
    if form is None or not decode_attention_ok(batch, seq, n_q, n_kv, head_dim, max_len):
        return None
    (qs, qst), _ = _rope_layout(qkv, q_off, k_off, batch, seq, n_q, n_kv, head_dim, cos, sin)
    if qst[3] != 1 or qs != (batch, n_q, seq, head_dim):
        return None
    q = torch.empty_strided(qs, qst, dtype=torch.float16, device=qkv.device)
    rc = _lib.lib().pbl_rope_append_kv8(qkv.data_ptr(), form[0], q_off, k_off, v_off, batch, seq, n_q, n_kv, head_dim, *form[1],
                                        q.data_ptr(), (C.c_int64 * 3)(*qst[:3]), k_cache.data_ptr(), v_cache.data_ptr(),
                                        k_scale.data_ptr(), v_scale.data_ptr(), max_len, pos.data_ptr(),
                                        torch.cuda.current_stream(qkv.device).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "rope + FP8 cache append")
    return q


def decode_attention_kv8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor, v_scale: torch.Tensor,
                         pos: torch.Tensor, scaling: float) -> torch.Tensor | None:
    """decode_attention_f16 over the FP8 cache (pbl_decode_attn_kv8): bit for bit what decode_attention_f16 returns over
    kv8_dequantize(k_cache, k_scale) / kv8_dequantize(v_cache, v_scale); advances pos by S.  None where that one returns None."""
    if q.dim() != 4 or q.dtype != torch.float16 or not q.is_cuda or q.stride(3) != 1 or min(q.stride()) < 0:
        raise ValueError("decode_attention_kv8: q must be an fp16 [B, Hq, S, D] GPU tensor with unit d stride")
    B, Hq, S, D = (int(d) for d in q.shape)
    Bc, Hkv, max_len, Dc = _cache_args_kv8(k_cache, v_cache, k_scale, v_scale, pos, q.device, "decode_attention_kv8")
    if (Bc, Dc) != (B, D):
        raise ValueError("decode_attention_kv8: the cache is not [B, Hkv, max_len, D] for q [B, Hq, S, D]")
    if not decode_attention_ok(B, S, Hq, Hkv, D, max_len):
        return None
    L = _lib.lib()
    out = torch.empty(B * S, Hq * D, dtype=torch.float16, device=q.device)
    ws = torch.empty(int(L.pbl_decode_attn_workspace_bytes(B, S, Hq, D, max_len)), dtype=torch.uint8, device=q.device)
    rc = L.pbl_decode_attn_kv8(q.data_ptr(), (C.c_int64 * 3)(*q.stride()[:3]), k_cache.data_ptr(), v_cache.data_ptr(), k_scale.data_ptr(),
                               v_scale.data_ptr(), B, S, Hq, Hkv, D, max_len, float(scaling), pos.data_ptr(), out.data_ptr(), Hq * D,
                               ws.data_ptr(), ws.numel(), torch.cuda.current_stream(q.device).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "decode attention (FP8 cache)")
    return out


def prefill_attention_kv8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                          k_scale: torch.Tensor, v_scale: torch.Tensor, pos: torch.Tensor, scaling: float) -> torch.Tensor | None:
    """prefill_attention_f16 over the FP8 cache (pbl_prefill_attn_kv8): k / v are quantised into cache rows [pos, pos + S) and every
    key and value is read back from there, so the result is bit for bit prefill_attention_f16's for k / v replaced by
    kv8_dequantize(*kv8_quantize(.)) over an fp16 cache that holds the dequantised earlier rows; advances pos by S.  None where
    prefill_attention_f16 returns None; the cache and pos are then untouched."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dim() != 4 or t.dtype != torch.float16 or not t.is_cuda or t.device != q.device or t.stride(3) != 1 or min(t.stride()) < 0:
            raise ValueError(f"prefill_attention_kv8: {name} must be an fp16 [B, H, S, D] GPU tensor with unit d stride")
    B, Hq, S, D = (int(d) for d in q.shape)
    Bc, Hkv, max_len, Dc = _cache_args_kv8(k_cache, v_cache, k_scale, v_scale, pos, q.device, "prefill_attention_kv8")
    if (Bc, Dc) != (B, D) or tuple(k.shape) != (B, Hkv, S, D) or k.shape != v.shape:
        raise ValueError("prefill_attention_kv8: k / v must be [B, Hkv, S, D] and the cache [B, Hkv, max_len, D] for q [B, Hq, S, D]")
    if not prefill_attention_ok(B, S, Hq, Hkv, D, max_len):
        return None
    out = torch.empty(B * S, Hq * D, dtype=torch.float16, device=q.device)
    rc = _lib.lib().pbl_prefill_attn_kv8(q.data_ptr(), (C.c_int64 * 3)(*q.stride()[:3]), k.data_ptr(), (C.c_int64 * 3)(*k.stride()[:3]),
                                         v.data_ptr(), (C.c_int64 * 3)(*v.stride()[:3]), k_cache.data_ptr(), v_cache.data_ptr(),
                                         k_scale.data_ptr(), v_scale.data_ptr(), B, S, Hq, Hkv, D, max_len, float(scaling),
                                         pos.data_ptr(), out.data_ptr(), Hq * D, torch.cuda.current_stream(q.device).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "prefill attention (FP8 cache)")
    return out


SELECT_MAX_VOCAB = 1 << 19


def select_token_ok(batch: int, vocab: int) -> bool:
    """the scope of select_token_f16 (pbl_select_token_f16): any batch, a vocabulary of at most 2^19 words"""
    return batch >= 1 and 1 <= vocab <= SELECT_MAX_VOCAB


def select_token_f16(logits: torch.Tensor, step: torch.Tensor, unfinished: torch.Tensor, tokens: torch.Tensor, col0: int,
                     next_ids: torch.Tensor, n_unfinished: torch.Tensor, status: torch.Tensor, temperature: float = 1.0,
                     top_k: int = 0, top_p: float = 1.0, uniforms: torch.Tensor | None = None, eos: torch.Tensor | None = None,
                     pad: int = 0, kept: torch.Tensor | None = None, min_p: float = 0.0) -> bool | None:
    """One token per row of logits [B, V] fp16 (unit column stride; the view out.logits[:, -1] is fine), chosen and booked on the
    device in one call (pbl_select_token_f16; the rules are in include/pbl.h): greedy when `uniforms` is None, else temperature /
    top_k (0 = off) / top_p (1 = off) sampling with the uniform uniforms[step, b] (fp32 [n_steps, B], values in [0, 1)).  All state
    is on the logits' device: step (int64, one element; advanced by one), unfinished (bool or uint8 [B]), tokens (int64 [B, total];
    column col0 + step receives the token), next_ids (int64, B elements: the next step's input), n_unfinished and status (int32,
    one element each; status bit 0: a sampled row held NaN / +inf, bit 1: step out of range), eos (int64 ids or None), kept
    (optional uint8 [B, V]: the mask of tokens that survived the filters).  Nothing is read on the host and nothing allocated:
    capturable in a hipGraph.  True when it ran, None where the entry declines (select_token_ok).  min_p (0 = off, sampling only):
    behind top_k and top_p a token stays only if exp(s - max s) >= min_p (pbl_select_token_minp_f16; with 0 the same result bit for bit)."""
    def dev(t, dtypes, n=None):
        return t.is_cuda and t.device == logits.device and t.dtype in dtypes and t.is_contiguous() and (n is None or t.numel() == n)

    if not logits.is_cuda or logits.dim() != 2 or logits.dtype != torch.float16 or logits.stride(1) != 1 or logits.shape[1] < 1 \
            or logits.shape[0] < 1 or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
        raise ValueError("select_token_f16: logits must be an fp16 [B, V] GPU tensor with unit column stride")
    B, V = (int(d) for d in logits.shape)
    flags = (torch.bool, torch.uint8)
    if not (dev(step, (torch.int64,), 1) and dev(unfinished, flags, B) and dev(next_ids, (torch.int64,), B)
            and dev(n_unfinished, (torch.int32,), 1) and dev(status, (torch.int32,), 1)):
        raise ValueError("select_token_f16: step (int64), unfinished (bool [B]), next_ids (int64 [B]), n_unfinished and status (int32) "
                         "must be contiguous tensors on the logits' device")
    if not dev(tokens, (torch.int64,)) or tokens.dim() != 2 or tokens.shape[0] != B or not 0 <= col0 < tokens.shape[1]:
        raise ValueError("select_token_f16: tokens must be a contiguous int64 [B, total] tensor on the logits' device, 0 <= col0 < total")
    if uniforms is not None and (not dev(uniforms, (torch.float32,)) or uniforms.dim() != 2 or uniforms.shape[1] != B or uniforms.shape[0] < 1):
        raise ValueError("select_token_f16: uniforms must be a contiguous fp32 [n_steps, B] tensor on the logits' device")
    if eos is not None and (not dev(eos, (torch.int64,)) or eos.dim() != 1):
        raise ValueError("select_token_f16: eos must be a 1-D int64 tensor on the logits' device")
    if kept is not None and not dev(kept, flags, B * V):
        raise ValueError("select_token_f16: kept must be a contiguous uint8 [B, V] tensor on the logits' device")
    if not temperature > 0 or top_k < 0 or not 0 < top_p <= 1 or not 0 <= min_p <= 1:
        raise ValueError("select_token_f16: temperature > 0, top_k >= 0, 0 < top_p <= 1 and 0 <= min_p <= 1")
    if not select_token_ok(B, V):
        return None
    n_eos = 0 if eos is None else int(eos.numel())
    rc = _lib.lib().pbl_select_token_minp_f16(
        logits.data_ptr(), logits.stride(0) if B > 1 else V, B, V, float(temperature), int(top_k), float(top_p), float(min_p),
        None if uniforms is None else uniforms.data_ptr(), 0 if uniforms is None else int(uniforms.shape[0]), step.data_ptr(),
        eos.data_ptr() if n_eos else None, n_eos, int(pad), unfinished.data_ptr(), tokens.data_ptr(), int(tokens.shape[1]), int(col0),
        next_ids.data_ptr(), n_unfinished.data_ptr(), status.data_ptr(), None if kept is None else kept.data_ptr(),
        torch.cuda.current_stream(logits.device).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "token selection")
    return True


PROCESS_MAX_NGRAM = 8


def process_logits_ok(batch: int, vocab: int, total: int = 1) -> bool:
    """the scope of process_logits_f16 (pbl_process_logits_f16): select_token_f16's, and a result buffer of fewer than 2^31 columns"""
    return select_token_ok(batch, vocab) and 1 <= total < (1 << 31)


def process_logits_f16(logits: torch.Tensor, tokens: torch.Tensor, col0: int, step: torch.Tensor, repetition_penalty: float = 1.0,
                       no_repeat_ngram_size: int = 0, min_new_tokens: int = 0, min_length: int = 0, eos: torch.Tensor | None = None,
                       scratch: torch.Tensor | None = None) -> bool | None:
    """The logits processors of a decode step, IN PLACE on logits [B, V] fp16 (unit column stride, any row stride and alignment) on
    the device in one launch (pbl_process_logits_f16; the rules are in include/pbl.h), over the history tokens[b, :col0 + step] of
    every row: repetition_penalty (> 0, 1 = off; once per distinct id), no_repeat_ngram_size (0 = off, at most 8: -inf for every token
    that would complete an n-gram the history holds) and, while step < min_new_tokens or col0 + step < min_length, -inf for the eos
    ids.  The result is what HF's processors give on an fp32 copy, rounded to fp16.  tokens (int64 [B, total]), step (int64, one
    element; read, not advanced) and eos (int64 ids or None) are select_token_f16's; scratch: a contiguous fp16 [B, total] tensor,
    needed with a penalty.  Nothing is read on the host and nothing allocated: capturable in a hipGraph.  True when it ran, None where
    the entry declines (process_logits_ok)."""
    def dev(t, dtypes, n=None):
        return t.is_cuda and t.device == logits.device and t.dtype in dtypes and t.is_contiguous() and (n is None or t.numel() == n)

    if not logits.is_cuda or logits.dim() != 2 or logits.dtype != torch.float16 or logits.stride(1) != 1 or logits.shape[1] < 1 \
            or logits.shape[0] < 1 or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
        raise ValueError("process_logits_f16: logits must be an fp16 [B, V] GPU tensor with unit column stride")
    B, V = (int(d) for d in logits.shape)
    if not dev(step, (torch.int64,), 1):
        raise ValueError("process_logits_f16: step must be a contiguous int64 tensor of one element on the logits' device")
    if not dev(tokens, (torch.int64,)) or tokens.dim() != 2 or tokens.shape[0] != B or not 0 <= col0 < tokens.shape[1]:
        raise ValueError("process_logits_f16: tokens must be a contiguous int64 [B, total] tensor on the logits' device, 0 <= col0 < total")
    if eos is not None and (not dev(eos, (torch.int64,)) or eos.dim() != 1):
        raise ValueError("process_logits_f16: eos must be a 1-D int64 tensor on the logits' device")
    if not repetition_penalty > 0 or not 0 <= no_repeat_ngram_size <= PROCESS_MAX_NGRAM:
        raise ValueError(f"process_logits_f16: repetition_penalty > 0 and 0 <= no_repeat_ngram_size <= {PROCESS_MAX_NGRAM}")
    total = int(tokens.shape[1])
    if float(repetition_penalty) != 1.0 and (scratch is None or not dev(scratch, (torch.float16,), B * total)):
        raise ValueError("process_logits_f16: a repetition penalty needs scratch, a contiguous fp16 [B, total] tensor on the logits' device")
    if not process_logits_ok(B, V, total):
        return None
    n_eos = 0 if eos is None else int(eos.numel())
    rc = _lib.lib().pbl_process_logits_f16(
        logits.data_ptr(), logits.stride(0) if B > 1 else V, B, V, tokens.data_ptr(), total, int(col0), step.data_ptr(),
        float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens), int(min_length), eos.data_ptr() if n_eos else None, n_eos,
        None if scratch is None else scratch.data_ptr(), torch.cuda.current_stream(logits.device).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "logits processing")
    return True


SCORE_MAX_VOCAB = 1 << 20


def score_tokens_ok(T: int, V: int) -> bool:
    """the scope of score_tokens_f16 (pbl_score_tokens_f16): any number of rows below 2^31, a vocabulary of at most 2^20 words"""
    return 1 <= T < (1 << 31) and 1 <= V <= SCORE_MAX_VOCAB


def score_tokens_f16(logits: torch.Tensor, targets: torch.Tensor, spans: torch.Tensor | None = None, ignore_index: int = -100):
    """log p(targets[t] | row t) and "targets[t] is the arg-max of row t" for every row of logits [T, V] fp16, in ONE read of the
    logits (pbl_score_tokens_f16; the rules are in include/pbl.h).  logits: any 2-D fp16 GPU view with unit column stride and a row
    stride >= V -- out.logits[0, :-1] and out.logits[0, :-1, :50257] as they are; it is never copied or converted.  targets: int64
    [T] on the logits' device; rows whose target is ignore_index score 0 / False and are not read.  spans: int64 [R, 2] row ranges
    [begin, end) on the device, or None.  Returns (logprob fp32 [T], greedy bool [T], span_sum fp64 [R] | None, span_greedy bool [R]
    | None, span_count int32 [R] | None, status int32 [1]); status bit 0: a target outside [0, V) (its row scores NaN), bit 1: a
    span outside [0, T] (its sum is NaN).  Nothing is read on the host: capturable in a hipGraph.  None where the entry declines
    (score_tokens_ok)."""
    if not logits.is_cuda or logits.dim() != 2 or logits.dtype != torch.float16 or logits.stride(1) != 1 or logits.shape[1] < 1 \
            or logits.shape[0] < 1 or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
        raise ValueError("score_tokens_f16: logits must be an fp16 [T, V] GPU tensor with unit column stride and a row stride >= V")
    T, V = (int(d) for d in logits.shape)
    dev = logits.device
    if targets.device != dev or targets.dtype != torch.int64 or targets.dim() != 1 or targets.numel() != T or not targets.is_contiguous():
        raise ValueError("score_tokens_f16: targets must be a contiguous int64 [T] tensor on the logits' device")
    if spans is not None and (spans.device != dev or spans.dtype != torch.int64 or spans.dim() != 2 or spans.shape[1] != 2
                              or not spans.is_contiguous()):
        raise ValueError("score_tokens_f16: spans must be a contiguous int64 [R, 2] tensor on the logits' device")
    if not score_tokens_ok(T, V):
        return None
    R = 0 if spans is None else int(spans.shape[0])
    logprob = torch.empty(T, dtype=torch.float32, device=dev)
    greedy = torch.empty(T, dtype=torch.bool, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    span_sum = span_greedy = span_count = None
    if spans is not None:
        span_sum = torch.empty(R, dtype=torch.float64, device=dev)
        span_greedy = torch.empty(R, dtype=torch.bool, device=dev)
        span_count = torch.empty(R, dtype=torch.int32, device=dev)
    rc = _lib.lib().pbl_score_tokens_f16(
        logits.data_ptr(), logits.stride(0) if T > 1 else V, T, V, targets.data_ptr(), int(ignore_index), logprob.data_ptr(),
        greedy.data_ptr(), spans.data_ptr() if R else None, R, span_sum.data_ptr() if R else None,
        span_greedy.data_ptr() if R else None, span_count.data_ptr() if R else None, status.data_ptr(),
        torch.cuda.current_stream(dev).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "token scoring")
    return logprob, greedy, span_sum, span_greedy, span_count, status


SPEC_MAX_ROWS = _lib.PBL_MAX_TOKENS_PER_LAUNCH
SPEC_MAX_NGRAM = 4


def spec_verify_ok(batch: int, seq: int, vocab: int) -> bool:
    """the scope of spec_verify_f16 (pbl_spec_verify_f16): the batch * seq <= 4 rows of one decode launch, select_token_f16's vocabulary"""
    return batch >= 1 and seq >= 1 and batch * seq <= SPEC_MAX_ROWS and 1 <= vocab <= SELECT_MAX_VOCAB


def _spec_state(what: str, ids: torch.Tensor, tokens: torch.Tensor, cursor: torch.Tensor, unfinished: torch.Tensor, dev) -> tuple[int, int]:
    """(B, S) of the state spec_verify_f16 and ngram_draft share, after checking its form"""
    def on(t, dtypes, n=None):
        return t.is_cuda and t.device == dev and t.dtype in dtypes and t.is_contiguous() and (n is None or t.numel() == n)

    if not on(ids, (torch.int64,)) or ids.dim() != 2 or ids.shape[0] < 1 or ids.shape[1] < 1:
        raise ValueError(f"{what}: ids must be a contiguous int64 [B, S] GPU tensor")
    B, S = (int(d) for d in ids.shape)
    if not on(tokens, (torch.int64,)) or tokens.dim() != 2 or tokens.shape[0] != B or tokens.shape[1] < 1:
        raise ValueError(f"{what}: tokens must be a contiguous int64 [B, total] tensor on the ids' device")
    if not on(cursor, (torch.int64,), 1) or not on(unfinished, (torch.bool, torch.uint8), B):
        raise ValueError(f"{what}: cursor (int64, one element) and unfinished (bool [B]) must be contiguous tensors on the ids' device")
    return B, S


def spec_verify_f16(logits: torch.Tensor, ids: torch.Tensor, tokens: torch.Tensor, cursor: torch.Tensor, unfinished: torch.Tensor,
                    n_unfinished: torch.Tensor, status: torch.Tensor, positions: torch.Tensor, stats: torch.Tensor,
                    eos: torch.Tensor | None = None, pad: int = 0, max_ngram: int = 0) -> bool | None:
    """The end of a speculative decode step, on the device in one call (pbl_spec_verify_f16; the rules are in include/pbl.h): logits
    [B, S, V] fp16 with unit stride inside a row (the view out.logits[:, -S:, :V] is fine, it is never copied) hold the step's rows
    for ids [B, S] int64 -- column 0 the last emitted token, columns 1 .. S-1 the drafts.  The drafts are compared with the greedy
    tokens of the rows before them; the prefix accepted by every unfinished row plus one bonus token go into tokens [B, total] from
    column `cursor` (int64, one element; advanced), with select_token_f16's eos / pad bookkeeping (unfinished, n_unfinished, status,
    eos, pad); ids[:, 0] becomes the last emitted token; the rejected rows are taken back from every position in `positions` (int64
    [L]: the data_ptr() of each layer's int64 cache position); stats (int64 [PBL_SPEC_STATS_WORDS]) counts steps, accepted drafts
    and tokens.  max_ngram >= 1: ngram_draft follows in the same call.  Nothing is read on the host and nothing allocated: capturable
    in a hipGraph.  True when it ran, None where the entry declines (spec_verify_ok)."""
    if not logits.is_cuda or logits.dim() != 3 or logits.dtype != torch.float16 or logits.stride(2) != 1 or min(logits.shape) < 1:
        raise ValueError("spec_verify_f16: logits must be an fp16 [B, S, V] GPU tensor with unit stride inside a row")
    dev = logits.device
    B, S = _spec_state("spec_verify_f16", ids, tokens, cursor, unfinished, dev)
    V = int(logits.shape[2])
    if tuple(logits.shape[:2]) != (B, S) or (S > 1 and logits.stride(1) < V) or (B > 1 and logits.stride(0) < (S - 1) * logits.stride(1) + V):
        raise ValueError("spec_verify_f16: logits must hold one row per element of ids [B, S], rows that do not overlap")

    def on(t, dtype, n=None):
        return t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous() and t.dim() <= 1 and (n is None or t.numel() == n)

    if not on(n_unfinished, torch.int32, 1) or not on(status, torch.int32, 1) or not on(stats, torch.int64, _lib.PBL_SPEC_STATS_WORDS) \
            or not on(positions, torch.int64):
        raise ValueError("spec_verify_f16: n_unfinished and status (int32, one element), stats (int64 [8]) and positions (int64 [L]) "
                         "must be contiguous tensors on the logits' device")
    if eos is not None and not on(eos, torch.int64):
        raise ValueError("spec_verify_f16: eos must be a 1-D int64 tensor on the logits' device")
    if not 0 <= max_ngram <= SPEC_MAX_NGRAM:
        raise ValueError("spec_verify_f16: max_ngram must be 0 (no drafting) .. 4")
    if not spec_verify_ok(B, S, V) or tokens.shape[1] >= 1 << 31:
        return None
    n_eos, L = 0 if eos is None else int(eos.numel()), int(positions.numel())
    rc = _lib.lib().pbl_spec_verify_f16(
        logits.data_ptr(), logits.stride(0) if B > 1 else S * max(logits.stride(1), V), logits.stride(1) if S > 1 else V, B, S, V,
        ids.data_ptr(), tokens.data_ptr(), int(tokens.shape[1]), cursor.data_ptr(), unfinished.data_ptr(),
        eos.data_ptr() if n_eos else None, n_eos, int(pad), n_unfinished.data_ptr(), status.data_ptr(),
        positions.data_ptr() if L else None, L, stats.data_ptr(), int(max_ngram), torch.cuda.current_stream(dev).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "speculation verify")
    return True


def ngram_draft(tokens: torch.Tensor, cursor: torch.Tensor, unfinished: torch.Tensor, ids: torch.Tensor, max_ngram: int = 2) -> bool | None:
    """Prompt-lookup drafts (pbl_ngram_draft; the rules are in include/pbl.h): ids[b, 1:] of every row from the latest earlier
    occurrence, in the row's history tokens[b, :cursor], of its last max_ngram .. 1 tokens (the longest length that has one); the
    row's last token ids[b, 0] where nothing matches and for rows whose unfinished flag is clear.  All tensors on one GPU (the forms
    of spec_verify_f16); nothing is read on the host.  True when it ran, None where the entry declines (more than 4 elements in ids)."""
    B, S = _spec_state("ngram_draft", ids, tokens, cursor, unfinished, ids.device)
    if not 1 <= max_ngram <= SPEC_MAX_NGRAM:
        raise ValueError("ngram_draft: max_ngram must be 1 .. 4")
    if B * S > SPEC_MAX_ROWS or tokens.shape[1] >= 1 << 31:
        return None
    rc = _lib.lib().pbl_ngram_draft(tokens.data_ptr(), int(tokens.shape[1]), B, cursor.data_ptr(), unfinished.data_ptr(), ids.data_ptr(), S,
                                    int(max_ngram), torch.cuda.current_stream(ids.device).cuda_stream)
    if rc == _lib.PBL_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "n-gram draft")
    return True
