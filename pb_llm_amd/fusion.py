"""Decode-time fusion of HF LLaMA layers over packed linears (fuse_decode_; harness.py re-exports it): q/k/v and gate/up as ONE launch
each, opt-in with norm / SwiGLU prologues and RoPE / residual epilogues.  Each fallback ladder is stated once: _FusedGroup._run, _mlp_tail,
_prefill_layer_forward."""
from __future__ import annotations

import logging
import types
import warnings

import torch
import torch.nn as nn

from . import runtime
from .decoding import _cache_branch, _decode_cache_layer, _kv8_cache_layer, _prefill_cache_layer
from .packing import concat_rows
from .quant import PBLinear, tensor_version

_LOG = logging.getLogger("pb_llm_amd")


class _FusedMember(nn.Module):
    """Stands where q_proj / k_proj / v_proj (or gate_proj / up_proj) stood.  WHICHEVER member is called first with an
    activation launches the whole group once (runtime.FusedGemv) and the others pick their slice up when they are called
    with the SAME tensor object (HF attention / MLP modules pass one hidden_states to all projections).  The group keeps
    a reference to that tensor until the next launch: an identity match can therefore not be a recycled device address
    (the caching allocator hands the next token's activation the address of the previous one), and the call order of the
    members does not matter.  A member called with another tensor -- a view, a copy, the next token -- launches again;
    launches that served no other member are counted (`_FusedGroup.solo_launches`) and reported once, because a model
    that never shares the tensor pays the whole group per projection.  More than 4 rows, or an fp32 activation: each
    member runs its own PBLinear (matrix-core / GEMM regime), bit-identical to the unfused model.  bf16 activations (HF LLaMA
    checkpoints, qat/run_qat.py:120) run the same fused launch with the conversion inside the kernel (round 5)."""

    def __init__(self, group: "_FusedGroup", index: int, own: PBLinear):
        super().__init__()
        self.own = own                      # registered: state_dict / .to() keep working
        self._group, self._index = [group], index          # (list: keep the group out of the module tree)
        self.in_features, self.out_features = own.in_features, own.out_features
        self.global_name = own.global_name

    def forward(self, x):
        g = self._group[0]
        rows = x.numel() // x.shape[-1]
        # normed: folded decode (prologues=True) -- x is the RAW hidden state its norm passed on unchanged, the launch normalises it
        normed, merged_ok = g.norm is not None and g.norm.deferred(x), False
        if not normed:
            if not x.is_cuda or x.is_inference() or (torch.is_grad_enabled() and x.requires_grad):
                return self.own(x)      # (an inference tensor has no version counter: nothing may be reused across calls)
            fused_ok = rows <= 4 and (x.dtype == torch.float16 or (x.dtype == torch.bfloat16 and g.fused.bf16_ok))
            # batched decode (5 .. MERGE_MAX_ROWS rows, any activation dtype): ONE call of the row-wise concatenation of the members
            # (packing.concat_rows: a record is 16 rows with everything it needs inside it) instead of one small-batch launch +
            # reduce per projection
            merged_ok = not fused_ok and g.merge_batched and 4 < rows <= g.MERGE_MAX_ROWS
            if not (fused_ok or merged_ok):
                return self.own(x)
        if g.x_ref is x and g.x_version == tensor_version(x) and g.x_normed == normed and self._index in g.pending:
            g.pending.discard(self._index)          # each launch serves each member once
            g.served += 1
        else:
            g.launch(x, rows, self._index, merged=merged_ok, norm=normed)
        return g.outs[self._index].reshape(*x.shape[:-1], self.out_features)


class _FusedGroup:
    """One fused launch (runtime.FusedGemv) over the member PBLinears.  The launch descriptors snapshot the members' blobs
    (device pointers, LDS sizing): they are rebuilt when a member's blob moved or was rewritten (.to(), load_state_dict)."""
    SOLO_WARN_AFTER = 32
    MERGE_MAX_ROWS = 64            # the small-batch kernel's range: beyond it a merged layer has nothing on its members (same tiles, same rounds)

    def __init__(self, mods: list[PBLinear], merge_batched: bool = False):
        self.mods = mods
        self.x_ref, self.x_version, self.outs, self.pending = None, -1, None, set()
        self.x_normed, self.y_all = False, None     # the last launch normalised x (prologue); its whole [rows, sum N] output
        self.norm = None            # _DeferredNorm whose deferred outputs this group normalises in its launch (prologues=True)
        self.launches = self.served = self.solo_launches = self.merged_launches = 0
        self._warned = False
        self.merged = None          # the members as ONE PBLinear (rows concatenated), built on the first batched call
        self.merge_batched = merge_batched and all(m.out_features % 16 == 0 for m in mods[:-1]) and \
            len({(m.packed.K, m.packed.G, m.packed.flags) for m in mods}) == 1
        self._build()

    def _stamp(self):
        return tuple((m.pbl_blob.data_ptr(), m._blob_version(), None if m.pbl_bias is None else m.pbl_bias.data_ptr()) for m in self.mods)

    def _build(self):
        dev = self.mods[0].pbl_blob.device
        self.fused = runtime.FusedGemv([m.packed for m in self.mods], [m.pbl_bias for m in self.mods], dev)
        self.merged = None
        self.stamp = self._stamp()

    def _refresh(self):
        if self._stamp() != self.stamp:
            self._build()

    def _merged(self) -> PBLinear:
        self._refresh()
        if self.merged is None:
            biases = [m.pbl_bias for m in self.mods]
            bias = None
            if any(b is not None for b in biases):
                dev = self.mods[0].pbl_blob.device
                bias = torch.cat([b if b is not None else torch.zeros(m.out_features, device=dev) for b, m in zip(biases, self.mods)])
            self.merged = PBLinear(concat_rows([m.packed for m in self.mods]), bias, self.mods[0].weight_dtype)
            _LOG.info("fuse_decode_(merge_batched=True): merged layer of %d projections holds %d more packed bytes "
                      "(+ its GEMM image on the first batched call)", len(self.mods), self.merged.packed.nbytes)
        return self.merged

    def _run(self, x, rows, norm: "_DeferredNorm | None" = None) -> torch.Tensor:
        """THE fused-launch ladder: the [rows, sum N] output of ONE launch over x.  norm: x is that norm's raw hidden state -- the
        launch normalises it (the RMSNorm prologue), or, where the entry declines, the kept norm runs in torch first"""
        self._refresh()
        if norm is not None:
            y = self.fused.run(x.reshape(rows, x.shape[-1]).contiguous(), norm=(norm.norm.weight, norm.eps))
            if y is not None:
                return y
            x = norm.norm(x)
        return self.fused.run(x.reshape(rows, x.shape[-1]).contiguous())

    def launch(self, x, rows, index, merged: bool = False, norm: bool = False):
        """_run (norm: with self.norm) or the merged layer, kept for the members to pick their slices up from.  index: the calling
        member (None: a caller that takes the whole output, _FoldedMLP)"""
        if self.pending and self.launches and len(self.pending) == len(self.mods) - 1:
            self.solo_launches += 1          # the previous launch served nobody but its caller
            if self.solo_launches == self.SOLO_WARN_AFTER and not self._warned:
                self._warned = True
                warnings.warn("pb_llm_amd.harness: fused projection group keeps launching for single members -- the model does "
                              "not pass one tensor object to its q/k/v (gate/up) projections; fuse_decode_ gains nothing here")
        if merged:
            y, self.y_all = self._merged()(x.reshape(rows, x.shape[-1])), None
            self.merged_launches += 1
        else:
            y = self.y_all = self._run(x, rows, self.norm if norm else None)
        offs = [int(o) for o in self.fused.offs]        # (the merged layer's rows are the members' rows in order: the same columns)
        self.outs = [y[:, offs[i]:offs[i + 1]] for i in range(len(self.mods))]
        self.x_ref, self.x_version, self.x_normed = x, tensor_version(x), norm
        self.pending = set() if index is None else set(range(len(self.mods))) - {index}
        self.launches += 1

    def run_folded(self, x, rows, norm: "_DeferredNorm") -> torch.Tensor:
        """_run on LlamaRMSNorm(x) for a folded decoder layer (fuse_decode_(epilogues=True)), with no identity or version bookkeeping
        (inference tensors have no version counter): no member picks a slice of it up."""
        y = self._run(x, rows, norm)
        self.x_ref, self.outs, self.y_all, self.pending = None, None, None, set()
        self.launches += 1
        return y


FUSE_SETS = (("q_proj", "k_proj", "v_proj"), ("gate_proj", "up_proj"))     # LLaMA naming (HF)


def _prologue_ok(x: torch.Tensor, weight: torch.Tensor, stateless: bool = False) -> bool:
    """THE predicate of the folded decode path (fuse_decode_(prologues=True)): a deferring norm passes x on unchanged exactly when it
    holds, and the fused group it feeds evaluates it again on the same tensor -- fp16 on the GPU, at most 4 rows, no autograd, and
    not an inference tensor (the hand-over is keyed on the version counter, which those lack).  stateless: the caller keeps nothing
    between calls (the epilogues=True folded layer), so inference tensors qualify."""
    return (x.is_cuda and x.dtype == torch.float16 and x.dim() >= 1 and 1 <= x.numel() // max(x.shape[-1], 1) <= 4
            and weight.dtype == torch.float16 and weight.device == x.device and (stateless or not x.is_inference())
            and not (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)))


class _DeferredNorm(nn.Module):
    """Stands where a decoder layer's LlamaRMSNorm stood (fuse_decode_(prologues=True)).  When the folded path takes the call
    (_prologue_ok) it returns its input UNCHANGED -- the same tensor object -- and the fused launch that reads it (q/k/v, gate/up)
    normalises it in its staging phase; otherwise it calls the kept norm, bit-identical to the unfolded model."""

    def __init__(self, norm: nn.Module):
        super().__init__()
        self.norm = norm                    # registered: state_dict / .to() keep working
        self.eps = float(norm.variance_epsilon)
        self.x_ref, self.x_version = None, -1

    @property
    def weight(self):
        return self.norm.weight

    @property
    def variance_epsilon(self):
        return self.eps

    def forward(self, x):
        if _prologue_ok(x, self.norm.weight):
            self.x_ref, self.x_version = x, tensor_version(x)   # (held until the next call: the identity cannot be a recycled address)
            return x
        self.x_ref = None
        return self.norm(x)

    def deferred(self, x) -> bool:
        """x is what this norm passed on un-normalised (and the predicate still holds for it)"""
        return self.x_ref is x and self.x_version == tensor_version(x) and _prologue_ok(x, self.norm.weight)


class _FoldedMLP(nn.Module):
    """Stands where a LlamaMLP stood (fuse_decode_(prologues=True)); gate_proj / up_proj / down_proj stay its registered children.
    Fed by its deferred post-attention norm: ONE gate/up launch (RMSNorm prologue) and ONE down_proj launch that builds silu(gate) *
    up while it stages its input (PBLinear.forward_swiglu).  Otherwise LlamaMLP's arithmetic, unchanged."""

    def __init__(self, mlp: nn.Module, norm: _DeferredNorm):
        super().__init__()
        self.config = mlp.config
        self.hidden_size, self.intermediate_size = mlp.hidden_size, mlp.intermediate_size
        self.gate_proj, self.up_proj, self.down_proj = mlp.gate_proj, mlp.up_proj, mlp.down_proj
        self.act_fn = mlp.act_fn
        self._norm = [norm]                 # (list: the norm is registered at its own place in the layer)

    def forward(self, x):
        if self._norm[0].deferred(x):
            grp = self.gate_proj._group[0]
            grp.launch(x, x.numel() // x.shape[-1], None, norm=True)
            y = _mlp_tail(self.down_proj, self.act_fn, grp.y_all, self.down_proj.in_features)
            return y.reshape(*x.shape[:-1], y.shape[-1])
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))




def _mlp_tail(down: PBLinear, act_fn, gu: torch.Tensor, inter: int, residual: torch.Tensor | None = None) -> torch.Tensor:
    """THE MLP-tail ladder: down(act_fn(gate) * up) [+ residual] from gu [rows, 2 inter] (gate at column 0, up at column inter) in
    ONE launch (SwiGLU prologue, residual add in the store), else the prologue alone and the add in torch, else the unfused tail"""
    y = None if residual is None else down.forward_swiglu(gu, inter, residual=residual)
    if y is not None:
        return y
    y = down.forward_swiglu(gu, inter)
    if y is None:
        y = down(act_fn(gu[:, :inter]) * gu[:, inter:2 * inter])
    return y if residual is None else residual + y.reshape(residual.shape)


def _prefill_layer_forward(self, hidden_states, past_key_values, position_embeddings, kv8=None, branch=None):
    """THE prefill-attention ladder of a folded layer (decoding.PREFILL_ATTENTION): more than 4 fp16 rows on the GPU without autograd,
    position_embeddings given, the layer not training and a DecodeCache layer that runtime.prefill_attention_ok takes -- else None,
    before anything ran, and the caller runs LlamaDecoderLayer.forward.  The layer as LlamaDecoderLayer / LlamaAttention compute it:
    the input norm, q / k / v through their modules (the GEMM kernels, as without the switch), RoPE in one launch (runtime.rope_f16,
    else HF's apply_rotary_pos_emb), the cache append and the causal attention over the valid rows (runtime.prefill_attention_f16,
    which advances the layer's position on the device as StaticLayer.update would have), o_proj, the residual, the post norm, the
    MLP and the residual.  The attention mask is not used: DecodeCache's unpadded-batch contract.
    kv8: the layer's FP8 cache layer (decoding._kv8_cache_layer) -- the attention is then runtime.prefill_attention_kv8 whatever
    PREFILL_ATTENTION says, and a shape it declines is an error: there is no other path over that cache.
    branch: the cache's branch table (decoding._cache_branch) -- any number of rows then qualifies, PREFILL_ATTENTION is not asked and
    the attention is runtime.branch_attention_f16 (the caller turns None into an error: no other path applies the table)."""
    x = hidden_states
    attn = self.self_attn
    if position_embeddings is None or x.dim() != 3 or (branch is None and x.shape[0] * x.shape[1] <= 4) or not x.is_cuda or x.dtype != torch.float16 \
            or (torch.is_grad_enabled() and x.requires_grad) or self.training or attn.training:
        return None
    B, S, _ = x.shape
    D = attn.head_dim
    n_q, n_kv = attn.q_proj.out_features // D, attn.k_proj.out_features // D
    if kv8 is not None:
        if not runtime.kv8_ok(B, S, n_q, n_kv, D, kv8.max_cache_len):
            raise RuntimeError(f"the FP8 KV cache declines batch {B}, {S} rows, heads {n_q} / {n_kv} x {D} (runtime.kv8_ok)")
        lay = kv8
    else:
        lay = _prefill_cache_layer(past_key_values, attn.layer_idx, B, S, n_q, n_kv, D, branch=branch is not None)
    if lay is None:
        return None
    from transformers.models.llama import modeling_llama as ML
    cos, sin = position_embeddings
    xn = self.input_layernorm(x)
    qk = torch.cat((attn.q_proj(xn).reshape(B * S, n_q * D), attn.k_proj(xn).reshape(B * S, n_kv * D)), dim=1)
    v = attn.v_proj(xn).view(B, S, n_kv, D).transpose(1, 2)
    rot = runtime.rope_f16(qk, 0, n_q * D, B, S, n_q, n_kv, D, cos, sin)
    if rot is None:
        rot = ML.apply_rotary_pos_emb(qk[:, :n_q * D].view(B, S, n_q, D).transpose(1, 2),
                                      qk[:, n_q * D:].view(B, S, n_kv, D).transpose(1, 2), cos, sin)
    if kv8 is not None:
        a = runtime.prefill_attention_kv8(rot[0], rot[1], v, lay.keys, lay.values, lay.key_scales, lay.value_scales,
                                          lay.cumulative_length, attn.scaling)
    elif branch is not None:
        a = runtime.branch_attention_f16(rot[0], rot[1], v, lay.keys, lay.values, lay.cumulative_length, attn.scaling, *branch)
    else:
        a = runtime.prefill_attention_f16(rot[0], rot[1], v, lay.keys, lay.values, lay.cumulative_length, attn.scaling)
    if a is None:                           # (prefill_attention_ok / kv8_ok held for the cache layer)
        raise RuntimeError("the prefill attention entry declined a shape its scope predicate took")
    h1 = x + attn.o_proj(a.view(B, S, -1))
    return h1 + self.mlp(self.post_attention_layernorm(h1))


def _folded_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                          position_embeddings=None, **kwargs):
    """LlamaDecoderLayer.forward of a layer folded by fuse_decode_(epilogues=True), installed on the instance.  At <= 4 fp16 rows
    without autograd, with position_embeddings given: the q/k/v launch (RMSNorm prologue), ONE RoPE launch (runtime.rope_f16),
    HF's cache update and attention interface, o_proj with the residual add in its store, the gate/up launch (RMSNorm prologue) and
    down_proj with the SwiGLU prologue and the residual add -- every step with HF's roundings, so the result equals the
    prologues=True layer's bit for bit.  More than 4 rows with decoding.PREFILL_ATTENTION on: _prefill_layer_forward (the HIP causal prefill attention over
    a DecodeCache).  Every other call runs LlamaDecoderLayer.forward (the prologues=True layer).
    Over an FP8 cache (DecodeSession(..., kv_cache="fp8")) the append and the attention are runtime.rope_append_kv8 +
    decode_attention_kv8 at <= 4 rows and runtime.prefill_attention_kv8 above; a call that cannot take these paths (autograd,
    training, not fp16, no position_embeddings) raises RuntimeError: LlamaDecoderLayer.forward cannot read that cache.
    Over a cache that carries a branch table (DecodeCache.branch, set by scoring.loglikelihood(share_prefix=True)): _prefill_layer_forward
    with runtime.branch_attention_f16 for ANY number of rows; a call that cannot take it raises RuntimeError, because no other path
    applies the table."""
    d_in = self.input_layernorm
    kv8 = _kv8_cache_layer(past_key_values, self.self_attn.layer_idx)
    branch = _cache_branch(past_key_values)
    if branch is not None and kv8 is not None:
        raise RuntimeError("branch attention reads the fp16 KV cache only: there is no FP8 variant")
    if branch is not None or position_embeddings is None or hidden_states.dim() != 3 \
            or not _prologue_ok(hidden_states, d_in.norm.weight, stateless=True):
        out = _prefill_layer_forward(self, hidden_states, past_key_values, position_embeddings, kv8, branch)
        if out is not None:
            return out
        if branch is not None:
            raise RuntimeError("a folded layer over a cache with a branch table runs runtime.branch_attention_f16 only: fp16 activations "
                               "on the GPU, no autograd, eval mode, position_embeddings and heads the entry takes are required")
        if kv8 is not None:
            raise RuntimeError("a folded layer over an FP8 KV cache runs its HIP paths only: fp16 activations on the GPU, no autograd, "
                               "eval mode and position_embeddings are required")
        return type(self).forward(self, hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                  past_key_values=past_key_values, use_cache=use_cache, position_embeddings=position_embeddings, **kwargs)
    from transformers.models.llama import modeling_llama as ML
    attn, mlp = self.self_attn, self.mlp
    B, S, _ = hidden_states.shape
    rows, D = B * S, attn.head_dim
    g_qkv = attn.q_proj._group[0]
    y = g_qkv.run_folded(hidden_states, rows, d_in)
    o_q, o_k, o_v, o_end = (int(o) for o in g_qkv.fused.offs)

    def heads(a, b):                                       # the view LlamaAttention makes of a projection's output
        return y[:, a:b].reshape(B, S, b - a).view(B, S, -1, D).transpose(1, 2)

    cos, sin = position_embeddings
    n_q, n_kv = (o_k - o_q) // D, (o_v - o_k) // D
    a = None
    if kv8 is not None:
        q = None if attn.training else runtime.rope_append_kv8(y, o_q, o_k, o_v, B, S, n_q, n_kv, D, cos, sin, kv8.keys, kv8.values,
                                                               kv8.key_scales, kv8.value_scales, kv8.cumulative_length)
        if q is None:
            raise RuntimeError("a folded layer over an FP8 KV cache runs its HIP paths only: rope_append_kv8 declined this step "
                               "(eval mode, head_dim 64 / 128, batch <= 4 and fp16 cos / sin are required)")
        a = runtime.decode_attention_kv8(q, kv8.keys, kv8.values, kv8.key_scales, kv8.value_scales, kv8.cumulative_length, attn.scaling)
        if a is None:
            raise RuntimeError("decode_attention_kv8 declined a shape rope_append_kv8 took")
        a = a.view(B, S, -1)
    lay = None if kv8 is not None else _decode_cache_layer(past_key_values, attn.layer_idx, B, n_kv, D)
    if lay is not None and not attn.training:
        # DecodeSession's cache: RoPE + the cache append in one launch, then the HIP decode attention over the valid rows only; it
        # advances the layer's position on the device (StaticLayer.cumulative_length), as StaticLayer.update would have
        q = runtime.rope_append_f16(y, o_q, o_k, o_v, B, S, n_q, n_kv, D, cos, sin, lay.keys, lay.values, lay.cumulative_length)
        if q is not None:
            a = runtime.decode_attention_f16(q, lay.keys, lay.values, lay.cumulative_length, attn.scaling)
            if a is None:                   # (decode_attention_ok held for rope_append_f16: the row is appended, the position not)
                raise RuntimeError("decode_attention_f16 declined a shape rope_append_f16 took")
            a = a.view(B, S, -1)
    if a is None:
        qk = runtime.rope_f16(y, o_q, o_k, B, S, n_q, n_kv, D, cos, sin)
        if qk is None:
            qk = ML.apply_rotary_pos_emb(heads(o_q, o_k), heads(o_k, o_v), cos, sin)
        q, k = qk
        v = heads(o_v, o_end)
        if past_key_values is not None:
            k, v = past_key_values.update(k, v, attn.layer_idx)
        interface = ML.ALL_ATTENTION_FUNCTIONS.get_interface(attn.config._attn_implementation, ML.eager_attention_forward)
        a, _ = interface(attn, q, k, v, attention_mask, dropout=0.0 if not attn.training else attn.attention_dropout,
                         scaling=attn.scaling, position_ids=position_ids, use_cache=use_cache, **kwargs)
        a = a.reshape(B, S, -1).contiguous()
    h1 = attn.o_proj.forward_residual(a, hidden_states)
    if h1 is None:
        h1 = hidden_states + attn.o_proj(a)
    gu = mlp.gate_proj._group[0].run_folded(h1, rows, self.post_attention_layernorm)
    return _mlp_tail(mlp.down_proj, mlp.act_fn, gu, mlp.down_proj.in_features, residual=h1).view(h1.shape)


def _gemv_exact(m) -> bool:
    """m is a group-free fp16-exact PBLinear resident on the GPU: what the prologue / epilogue entries of the GEMV take"""
    return isinstance(m, PBLinear) and m.packed.G == 1 and m.weight_dtype == torch.float16 and m.pbl_blob.is_cuda


def _fold_prologues_(model: nn.Module, epilogues: bool = False) -> tuple[int, int]:
    """fuse_decode_(prologues=True): the LLaMA decoder layers whose norms and MLP can be folded into their fused launches.
    epilogues: of those, the layers of type LlamaDecoderLayer with a LlamaAttention and a group-free fp16-exact PBLinear o_proj also
    get the folded forward (_folded_layer_forward).  Returns (layers folded, layers with the folded forward)."""
    try:
        from transformers.models.llama.modeling_llama import LlamaAttention, LlamaDecoderLayer, LlamaMLP, LlamaRMSNorm
    except ImportError:
        return 0, 0

    def group_of(members):
        if not all(isinstance(m_, _FusedMember) for m_ in members):
            return None
        g = members[0]._group[0]
        ok = all(m_._group[0] is g and m_._index == i for i, m_ in enumerate(members)) and len(g.mods) == len(members)
        ok = ok and g.norm is None and g.fused._inline and not g.fused.flags & 1
        return g if ok and all(_gemv_exact(m_.own) for m_ in members) else None

    n = ne = 0
    for layer in list(model.modules()):
        if not isinstance(layer, LlamaDecoderLayer):
            continue
        norms = (getattr(layer, "input_layernorm", None), getattr(layer, "post_attention_layernorm", None))
        if not all(isinstance(nm, LlamaRMSNorm) and nm.weight.dtype == torch.float16 and nm.weight.is_cuda for nm in norms):
            continue
        attn, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
        if not isinstance(mlp, LlamaMLP) or getattr(mlp.config, "hidden_act", None) != "silu" or attn is None:
            continue
        g_qkv = group_of([getattr(attn, nm, None) for nm in ("q_proj", "k_proj", "v_proj")])
        g_gu = group_of([mlp.gate_proj, mlp.up_proj])
        down = mlp.down_proj
        if g_qkv is None or g_gu is None or not _gemv_exact(down) or down.in_features != mlp.gate_proj.out_features:
            continue
        d_in, d_post = _DeferredNorm(norms[0]), _DeferredNorm(norms[1])
        g_qkv.norm, g_gu.norm = d_in, d_post
        layer.input_layernorm, layer.post_attention_layernorm = d_in, d_post
        layer.mlp = _FoldedMLP(mlp, d_post)
        n += 1
        if epilogues and type(layer) is LlamaDecoderLayer and type(attn) is LlamaAttention \
                and _gemv_exact(getattr(attn, "o_proj", None)):
            layer.forward = types.MethodType(_folded_layer_forward, layer)
            ne += 1
    return n, ne


def fuse_decode_(model: nn.Module, sets=FUSE_SETS, merge_batched: bool = False, prologues: bool = False, epilogues: bool = False) -> int:
    """Decode-time fusion: in every module that holds all the projections of a set as PBLinears with one
    in_features (HF LlamaAttention: q/k/v_proj; LlamaMLP: gate/up_proj), replace them by members of one fused launch.
    7 launches per decoder layer become 4.  Returns the number of groups created.  The caller this serves is the token
    loop of gptq_pb/eval_ppl_utils.py:55-64 / qat/eval_after_qat.py:11-33 at batch 1.
    merge_batched (round 5; OPT-IN since round 6, ADVICE r5: the default silently held blob + image + merged blob + merged image): a
    decode BATCH (5 - 64 rows) runs each group as ONE call of the members' row-wise concatenation (packing.concat_rows; built on the
    first such call; costs the members' packed bytes once more plus its GEMM image -- logged once per group at INFO level on the
    "pb_llm_amd" logger) instead of one small-batch launch + reduce per projection (llama-7b decoder layer at 16 rows: 94.0 -> 78.5
    us).  A decode-only phase at batch <= 4 never reads a GEMM image: `drop_gemm_images_` releases them.
    prologues (OPT-IN): in every HF LlamaDecoderLayer whose norms are fp16 LlamaRMSNorms, whose hidden_act is silu and whose q/k/v,
    gate/up and down_proj are group-free fp16-exact PBLinears, fold the two RMSNorms into the q/k/v and gate/up launches and
    silu(gate) * up into the down_proj launch (their staging phases build the row they multiply): at <= 4 fp16 rows 18 small torch
    kernels per layer disappear and the linears stay 4 launches.  Every other call runs what the unfolded model runs.  The folded
    layers are counted once at INFO level on the "pb_llm_amd" logger; the return value is the number of groups, as without it.
    epilogues (OPT-IN; implies the prologue folding): a folded layer of type LlamaDecoderLayer with a LlamaAttention and a group-free
    fp16-exact PBLinear o_proj also runs its decode step as six launches -- q/k/v (RMSNorm prologue), RoPE (one HIP launch instead of
    HF's ~10 elementwise kernels), HF's cache update and attention, o_proj with the residual add in its store, gate/up (RMSNorm
    prologue), down_proj (SwiGLU prologue and residual add) -- bit-identical to the prologues=True layer.  Every other call (more
    rows, other dtypes, autograd, no position_embeddings) runs the prologues=True layer.  Counted at INFO level as well."""
    n = 0
    for mod in list(model.modules()):
        for names in sets:
            subs = [getattr(mod, nm, None) for nm in names]
            if not all(isinstance(m_, PBLinear) for m_ in subs):
                continue
            if len({m_.in_features for m_ in subs}) != 1 or not subs[0].pbl_blob.is_cuda:
                continue
            grp = _FusedGroup(subs, merge_batched)
            for i, (nm, m_) in enumerate(zip(names, subs)):
                setattr(mod, nm, _FusedMember(grp, i, m_))
            n += 1
    if prologues or epilogues:
        folded, with_epilogues = _fold_prologues_(model, epilogues)
        _LOG.info("fuse_decode_(prologues=True): RMSNorm and SwiGLU folded into the decode launches of %d decoder layers", folded)
        if epilogues:
            _LOG.info("fuse_decode_(epilogues=True): RoPE and the residual adds folded into the decode launches of %d decoder layers",
                      with_epilogues)
    return n
