"""Model-level harness: what gptq_pb/run.py:116-178 and
qat/eval_after_qat.py:12-24 do around the hot path, without datasets or checkpoints (none
are available offline): quantize every decoder Linear of a HF causal LM to a dense
fake-quant weight, swap in PBLinear modules, run forward / perplexity-style loops.

`quant_sequential_` is the counterpart of gptq_pb/run.py:quant_sequential on one MI355X: the whole model
stays resident in HBM (288 GB: no layer-by-layer host offload), every decoder Linear is quantised by the fused
GPTQ-PB pipeline (pb_llm_amd/ptq.py) and, optionally, packed on the spot.
`quantize_dense_` takes an external structure producer instead (tests pass the oracle's).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .quant import PBLinear, replace_linear_with_pb, tensor_version


def find_layers(module: nn.Module, name: str = "") -> dict:
    """gptq_pb/modelutils.py:8-16: every nn.Linear below `module`, by dotted name."""
    if isinstance(module, nn.Linear):
        return {name: module}
    res = {}
    for n, child in module.named_children():
        res.update(find_layers(child, name + "." + n if name else n))
    return res


@torch.no_grad()
def quantize_dense_(model: nn.Module, producer, skip=("lm_head",)) -> dict:
    """In place: W <- producer(name, W) -> dict(W_fq, low_mask, hscale, hzero) for every
    Linear (decoder layers only by default, like gptq_pb/run.py which leaves lm_head alone).
    Returns the per-layer side information for `to_pb_`."""
    side = {}
    for name, lin in find_layers(model).items():
        if any(s in name for s in skip):
            continue
        r = producer(name, lin.weight.data)
        lin.weight.data = r["W_fq"].to(lin.weight.dtype).to(lin.weight.device)
        side[name] = r
    return side


def to_pb_(model: nn.Module, side: dict | None = None, skip=("lm_head",)) -> nn.Module:
    """Swap every (fake-quant) Linear for a PBLinear.  With `side` the exact PTQ structure is
    used; without it the structure is re-inferred from the dense weights (flattened checkpoint)."""
    names = {id(m): n for n, m in model.named_modules()}

    def factory(lin: nn.Linear):
        s = (side or {}).get(names[id(lin)])
        if s is None:
            return PBLinear.from_dense(lin.weight.data, lin.bias).to(lin.weight.device)
        return PBLinear.from_dense(lin.weight.data, lin.bias, s.get("low_mask"), s.get("groupsize", -1),
                                   s.get("hscale"), s.get("hzero")).to(lin.weight.device)

    return replace_linear_with_pb(model, factory, skip)


def decoder_layers(model: nn.Module):
    """The list gptq_pb/run.py:49-63 picks per model family."""
    inner = getattr(model, "model", model)
    if hasattr(inner, "decoder") and hasattr(inner.decoder, "layers"):
        return inner.decoder.layers                      # OPT
    if hasattr(inner, "layers"):
        return inner.layers                              # LLaMA
    raise NotImplementedError("unknown decoder layout")


@torch.no_grad()
def quant_sequential_(model: nn.Module, calib_ids, low_frac: float, salient_metric: str = "magnitude", groupsize: int = -1,
                      high_bit: int = 8, disable_gptq: bool = False, percdamp: float = 0.01, pack: bool = False,
                      quant_only: str = "", log=None) -> dict:
    """gptq_pb/run.py:36-178 on the GPU.  calib_ids: iterable of token-id tensors [1, seqlen] (the dataloader's
    batch[0]).  Layer by layer: capture the layer's inputs, accumulate every Linear's Hessian through forward hooks
    (:148-156), quantise each Linear (:158-169), re-run the layer with the quantised weights to feed the next one
    (:171-172).  pack=True swaps each quantised Linear for a PBLinear right away.  Returns {name: error}."""
    from .ptq import LowHighGPTQ
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("quant_sequential_ needs the model on the GPU: there is no host path")
    layers = decoder_layers(model)
    use_cache = getattr(model.config, "use_cache", False)
    model.config.use_cache = False
    captured = []

    def catch(module, args, kwargs):                     # the reference's Catcher (:72-83)
        captured.append((args, kwargs))
        raise ValueError

    handle = layers[0].register_forward_pre_hook(catch, with_kwargs=True)
    for ids in calib_ids:
        try:
            model(ids.to(dev))
        except ValueError:
            pass
    handle.remove()
    inps = [a[0] if a else k["hidden_states"] for a, k in captured]
    errors = {}
    for i, layer in enumerate(layers):
        subset = {n: m for n, m in find_layers(layer).items() if quant_only in n}
        gpts = {n: LowHighGPTQ(m, salient_metric, groupsize, high_bit, disable_gptq) for n, m in subset.items()}
        handles = [subset[n].register_forward_hook(lambda _, inp, out, n=n: gpts[n].add_batch(inp[0].data, out.data))
                   for n in gpts]

        def run(j, hidden):
            args, kwargs = captured[j]
            if args:
                out = layer(hidden, *args[1:], **kwargs)
            else:
                out = layer(**{**kwargs, "hidden_states": hidden})
            return out[0] if isinstance(out, tuple) else out

        for j, h in enumerate(inps):
            run(j, h)
        for h in handles:
            h.remove()
        for n, g in gpts.items():
            info = g.fasterquant(low_frac, percdamp=percdamp)
            errors[f"{i}.{n}"] = info["error"]
            if log:
                log(f"{i} {n} error {info['error']:.4f}")
            if pack:
                parent = layer
                *path, leaf = n.split(".")
                for p_ in path:
                    parent = getattr(parent, p_)
                setattr(parent, leaf, g.to_pb().to(dev))
            g.free()
        inps = [run(j, h) for j, h in enumerate(inps)]
    model.config.use_cache = use_cache
    return errors


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
        if g.norm is not None and g.norm.deferred(x):
            # folded decode (fuse_decode_(prologues=True)): x is the RAW hidden state its norm passed on unchanged; the launch
            # normalises it while it stages it
            if g.x_ref is x and g.x_version == tensor_version(x) and g.x_normed and self._index in g.pending:
                g.pending.discard(self._index)
                g.served += 1
            else:
                g.launch(x, rows, self._index, norm=True)
            return g.outs[self._index].reshape(*x.shape[:-1], self.out_features)
        if not x.is_cuda or x.is_inference() or (torch.is_grad_enabled() and x.requires_grad):
            return self.own(x)          # (an inference tensor has no version counter: nothing may be reused across calls)
        fused_ok = rows <= 4 and (x.dtype == torch.float16 or (x.dtype == torch.bfloat16 and g.fused.bf16_ok))
        # batched decode (5 .. MERGE_MAX_ROWS rows, any activation dtype): ONE call of the row-wise concatenation of the members
        # (packing.concat_rows: a record is 16 rows with everything it needs inside it) instead of one small-batch launch + reduce
        # per projection
        merged_ok = not fused_ok and g.merge_batched and 4 < rows <= g.MERGE_MAX_ROWS
        if not (fused_ok or merged_ok):
            return self.own(x)
        if g.x_ref is x and g.x_version == tensor_version(x) and not g.x_normed and self._index in g.pending:   # each launch serves each member once
            g.pending.discard(self._index)
            g.served += 1
            return g.outs[self._index].reshape(*x.shape[:-1], self.out_features)
        g.launch(x, rows, self._index, merged=merged_ok)
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
        return tuple((m.pbl_blob.data_ptr(), m._blob_version(), None if m.pbl_bias is None else m.pbl_bias.data_ptr())
                     for m in self.mods)

    def _build(self):
        from .runtime import FusedGemv
        dev = self.mods[0].pbl_blob.device
        self.fused = FusedGemv([m.packed for m in self.mods], [m.pbl_bias for m in self.mods], dev)
        self.merged = None
        self.stamp = self._stamp()

    def _merged(self) -> PBLinear:
        if self.merged is None:
            from .packing import concat_rows
            biases = [m.pbl_bias for m in self.mods]
            bias = None
            if any(b is not None for b in biases):
                dev = self.mods[0].pbl_blob.device
                bias = torch.cat([b if b is not None else torch.zeros(m.out_features, device=dev) for b, m in zip(biases, self.mods)])
            self.merged = PBLinear(concat_rows([m.packed for m in self.mods]), bias, self.mods[0].weight_dtype)
            import logging
            logging.getLogger("pb_llm_amd").info("fuse_decode_(merge_batched=True): merged layer of %d projections holds %d more packed bytes "
                                                 "(+ its GEMM image on the first batched call)", len(self.mods), self.merged.packed.nbytes)
            self.offs = [0]
            for m in self.mods:
                self.offs.append(self.offs[-1] + m.out_features)
        return self.merged

    def launch(self, x, rows, index, merged: bool = False, norm: bool = False):
        """index: the calling member (None: a caller that takes the whole output, _FoldedMLP).  norm: x is the raw hidden state of
        self.norm -- the launch normalises it (the RMSNorm prologue), or, where the entry declines, the kept norm runs in torch first"""
        if self.pending and self.launches and len(self.pending) == len(self.mods) - 1:
            self.solo_launches += 1          # the previous launch served nobody but its caller
            if self.solo_launches == self.SOLO_WARN_AFTER and not self._warned:
                import warnings
                self._warned = True
                warnings.warn("pb_llm_amd.harness: fused projection group keeps launching for single members -- the model does "
                              "not pass one tensor object to its q/k/v (gate/up) projections; fuse_decode_ gains nothing here")
        if self._stamp() != self.stamp:
            self._build()
        self.y_all = None
        if merged:
            y = self._merged()(x.reshape(rows, x.shape[-1]))
            self.outs = [y[:, self.offs[i]:self.offs[i + 1]] for i in range(len(self.mods))]
            self.merged_launches += 1
        else:
            x2 = x.reshape(rows, x.shape[-1]).contiguous()
            y = None
            if norm:
                y = self.fused.run(x2, norm=(self.norm.norm.weight, self.norm.eps))
                if y is None:
                    x2 = self.norm.norm(x).reshape(rows, x.shape[-1]).contiguous()
            if y is None:
                y = self.fused.run(x2)
            self.y_all = y
            self.outs = [y[:, int(self.fused.offs[i]):int(self.fused.offs[i + 1])] for i in range(len(self.mods))]
        self.x_ref, self.x_version, self.x_normed = x, tensor_version(x), norm
        self.pending = set() if index is None else set(range(len(self.mods))) - {index}
        self.launches += 1

    def run_folded(self, x, rows, norm: "_DeferredNorm") -> torch.Tensor:
        """The whole [rows, sum N] output of ONE launch on LlamaRMSNorm(x), for a folded decoder layer (fuse_decode_(epilogues=True)):
        the RMSNorm prologue, or, where it declines, the kept norm in torch and the plain launch -- what launch(norm=True) runs.  No
        identity or version bookkeeping (inference tensors have no version counter): no member picks a slice of it up."""
        if self._stamp() != self.stamp:
            self._build()
        x2 = x.reshape(rows, x.shape[-1]).contiguous()
        y = self.fused.run(x2, norm=(norm.norm.weight, norm.eps))
        if y is None:
            y = self.fused.run(norm.norm(x).reshape(rows, x.shape[-1]).contiguous())
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
            rows = x.numel() // x.shape[-1]
            grp.launch(x, rows, None, norm=True)
            gu = grp.y_all                                          # [rows, 2 I]: gate at column 0, up at column I
            inter = self.down_proj.in_features
            y = self.down_proj.forward_swiglu(gu, inter)
            if y is None:                                           # declined (rows / LDS budget): the unfused tail
                y = self.down_proj(self.act_fn(gu[:, :inter]) * gu[:, inter:2 * inter])
            return y.reshape(*x.shape[:-1], y.shape[-1])
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


# The HIP decode attention in folded layers (_folded_layer_forward) over a DecodeCache.  False: those layers append to the cache and
# attend through HF's StaticLayer.update and attention interface instead (tools/bench_generate.py compares the two).
DECODE_ATTENTION = True
_DECODE_CACHE = None                     # the DecodeCache class, made on first use (transformers is imported lazily)


def _decode_cache_layer(cache, layer_idx: int, batch: int, n_kv: int, head_dim: int):
    """the StaticLayer of `cache` that the decode-attention branch may append to and attend over: cache is a DecodeCache, its layer
    is a plain, initialised StaticLayer of fp16 [batch, n_kv, max_len, head_dim] tensors -- else None (HF's path)"""
    if not DECODE_ATTENTION or _DECODE_CACHE is None or not isinstance(cache, _DECODE_CACHE) or layer_idx is None \
            or layer_idx >= len(cache.layers):
        return None
    from transformers.cache_utils import StaticLayer
    from .runtime import decode_attention_ok
    lay = cache.layers[layer_idx]
    if type(lay) is not StaticLayer or not lay.is_initialized or lay.keys.dtype != torch.float16:
        return None
    B, H, L, D = lay.keys.shape
    if (B, H, D) != (batch, n_kv, head_dim) or not decode_attention_ok(batch, 1, n_kv, n_kv, head_dim, L):
        return None
    return lay


def _folded_layer_forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_values=None, use_cache=False,
                          position_embeddings=None, **kwargs):
    """LlamaDecoderLayer.forward of a layer folded by fuse_decode_(epilogues=True), installed on the instance.  At <= 4 fp16 rows
    without autograd, with position_embeddings given: the q/k/v launch (RMSNorm prologue), ONE RoPE launch (runtime.rope_f16),
    HF's cache update and attention interface, o_proj with the residual add in its store, the gate/up launch (RMSNorm prologue) and
    down_proj with the SwiGLU prologue and the residual add -- every step with HF's roundings, so the result equals the
    prologues=True layer's bit for bit.  Every other call runs LlamaDecoderLayer.forward (the prologues=True layer)."""
    d_in = self.input_layernorm
    if position_embeddings is None or hidden_states.dim() != 3 or not _prologue_ok(hidden_states, d_in.norm.weight, stateless=True):
        return type(self).forward(self, hidden_states, attention_mask=attention_mask, position_ids=position_ids,
                                  past_key_values=past_key_values, use_cache=use_cache, position_embeddings=position_embeddings, **kwargs)
    from transformers.models.llama import modeling_llama as ML
    from .runtime import rope_f16
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
    lay = _decode_cache_layer(past_key_values, attn.layer_idx, B, n_kv, D)
    if lay is not None and not attn.training:
        # DecodeSession's cache: RoPE + the cache append in one launch, then the HIP decode attention over the valid rows only; it
        # advances the layer's position on the device (StaticLayer.cumulative_length), as StaticLayer.update would have
        from .runtime import decode_attention_f16, rope_append_f16
        q = rope_append_f16(y, o_q, o_k, o_v, B, S, n_q, n_kv, D, cos, sin, lay.keys, lay.values, lay.cumulative_length)
        if q is not None:
            a = decode_attention_f16(q, lay.keys, lay.values, lay.cumulative_length, attn.scaling)
            if a is None:                   # (decode_attention_ok held for rope_append_f16: the row is appended, the position not)
                raise RuntimeError("decode_attention_f16 declined a shape rope_append_f16 took")
            a = a.view(B, S, -1)
    if a is None:
        qk = rope_f16(y, o_q, o_k, B, S, n_q, n_kv, D, cos, sin)
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
    inter = mlp.down_proj.in_features
    out = mlp.down_proj.forward_swiglu(gu, inter, residual=h1)
    if out is None:
        t = mlp.down_proj.forward_swiglu(gu, inter)
        if t is None:
            t = mlp.down_proj(mlp.act_fn(gu[:, :inter]) * gu[:, inter:2 * inter])
        out = h1 + t.reshape(h1.shape)
    return out.view(h1.shape)


def _fold_prologues_(model: nn.Module, epilogues: bool = False) -> tuple[int, int]:
    """fuse_decode_(prologues=True): the LLaMA decoder layers whose norms and MLP can be folded into their fused launches.
    epilogues: of those, the layers of type LlamaDecoderLayer with a LlamaAttention and a group-free fp16-exact PBLinear o_proj also
    get the folded forward (_folded_layer_forward).  Returns (layers folded, layers with the folded forward)."""
    try:
        from transformers.models.llama.modeling_llama import LlamaAttention, LlamaDecoderLayer, LlamaMLP, LlamaRMSNorm
    except ImportError:
        return 0, 0
    import types

    def group_of(members):
        if not all(isinstance(m_, _FusedMember) for m_ in members):
            return None
        g = members[0]._group[0]
        ok = all(m_._group[0] is g and m_._index == i for i, m_ in enumerate(members)) and len(g.mods) == len(members)
        ok = ok and g.norm is None and g.fused._inline and not g.fused.flags & 1
        return g if ok and all(m_.own.packed.G == 1 and m_.own.weight_dtype == torch.float16 for m_ in members) else None

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
        if g_qkv is None or g_gu is None or not isinstance(down, PBLinear) or down.packed.G != 1 \
                or down.weight_dtype != torch.float16 or not down.pbl_blob.is_cuda or down.in_features != mlp.gate_proj.out_features:
            continue
        d_in, d_post = _DeferredNorm(norms[0]), _DeferredNorm(norms[1])
        g_qkv.norm, g_gu.norm = d_in, d_post
        layer.input_layernorm, layer.post_attention_layernorm = d_in, d_post
        layer.mlp = _FoldedMLP(mlp, d_post)
        n += 1
        o = getattr(attn, "o_proj", None)
        if epilogues and type(layer) is LlamaDecoderLayer and type(attn) is LlamaAttention and isinstance(o, PBLinear) \
                and o.packed.G == 1 and o.weight_dtype == torch.float16 and o.pbl_blob.is_cuda:
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
        import logging
        logging.getLogger("pb_llm_amd").info("fuse_decode_(prologues=True): RMSNorm and SwiGLU folded into the decode launches of %d "
                                             "decoder layers", folded)
        if epilogues:
            logging.getLogger("pb_llm_amd").info("fuse_decode_(epilogues=True): RoPE and the residual adds folded into the decode "
                                                 "launches of %d decoder layers", with_epilogues)
    return n


def build_gemm_images_(model: nn.Module, release_blobs: bool = False) -> tuple[int, int]:
    """Build and keep the GEMM image of every packed fp16-checkpoint linear of `model` NOW (quant._kept_image), instead of on its
    first prefill call: afterwards calls with 5 - 64 rows run the small-batch kernel over the image under the default
    quant.SMALL_BATCH_IMAGE = "auto" -- also inside a hipGraph capture, where an image cannot be built (the build reads two words
    back).  Costs the images' memory on top of the blobs (1.7 - 2.4 x the blob's bytes) -- unless release_blobs (round 6): then the
    image becomes each layer's ONLY device copy (PBLinear.release_blob_: the blob moves to host memory, state_dict() still holds it;
    every row count multiplies from the image) -- what an evaluation run wants (qat/eval_after_qat.py:11-33, gptq_pb/eval_ppl_utils.py:
    55-64 call the layers with whole 2048-token windows only): a llama-7b-shaped model at 5 % hessian salients holds 4.2 GB instead
    of 6.3.  Returns (layers with an image, image bytes); `release_blobs_` / `restore_blobs_` do the second step on their own."""
    from . import quant as Q
    n = nbytes = 0
    for m in model.modules():
        if isinstance(m, Q.PBLinear) and m._image_only is not None:
            n += 1
            nbytes += m._image_only[0].data.numel()
        elif isinstance(m, Q.PBLinear) and m.weight_dtype == torch.float16 and m.pbl_blob.is_cuda and Q.fused_gemm_ok(m.packed):
            img = Q._kept_image(m.packed)
            if img is not None:
                n += 1
                nbytes += img.data.numel()
    if release_blobs:
        release_blobs_(model)
    return n, nbytes


def release_blobs_(model: nn.Module, pin: bool = False) -> int:
    """PBLinear.release_blob_ on every packed linear of `model` that has a GEMM image (fp16-checkpoint layers; others keep their
    blob); returns the device bytes released.  Not on a model whose projections were fused for decode (fuse_decode_: the fused
    launches read the blobs) -- un-fused layers released here are simply skipped by a later fuse_decode_."""
    from . import quant as Q
    if any(isinstance(m, _FusedMember) for m in model.modules()):
        raise RuntimeError("release_blobs_: the model's projections are fused for decode (fuse_decode_), whose launches read the blobs")
    n = 0
    for m in model.modules():
        if isinstance(m, Q.PBLinear) and m._image_only is None and m.pbl_blob.is_cuda and m.weight_dtype == torch.float16 \
                and Q.fused_gemm_ok(m.packed) and Q._kept_image(m.packed) is not None:
            n += m.release_blob_(pin)
    torch.cuda.empty_cache()
    return n


def restore_blobs_(model: nn.Module) -> int:
    """the blobs of every image-only linear back on the device (decode through the GEMV again); returns the layers restored"""
    from . import quant as Q
    n = 0
    for m in model.modules():
        if isinstance(m, Q.PBLinear) and m._image_only is not None:
            m.restore_blob_()
            n += 1
    return n


def drop_gemm_images_(model: nn.Module) -> int:
    """Release every kept GEMM image (and kept salient list) of `model`'s packed linears -- the memory knob next to
    build_gemm_images_: with the round-5 defaults every fp16-exact linear gets an image on its first call with 5 rows or more
    (1.7 - 2.4 x the blob's bytes; 4.2 GB for a 7B model at 5 % hessian salients), which a decode-only phase at batch <= 4 never
    reads.  The next call that wants an image rebuilds it.  Not while a captured graph that uses the images may still be replayed.
    Also forgets the kept fragment-major copy of the last activation (quant.drop_x_fragments_).  Returns the bytes released."""
    from . import quant as Q
    Q.drop_x_fragments_()
    n = 0
    for m in model.modules():
        if isinstance(m, Q.PBLinear):
            p = m.packed
            kept = p.__dict__.pop("_gemm_image", None)
            if kept is not None and kept[1] is not None:
                n += kept[1].data.numel()
            lst = p.__dict__.pop("_gemm_list", None)
            if lst is not None and lst[1] is not None:
                n += lst[1].numel()
    return n


class GraphedForward:
    """One forward of `model` on a fixed input shape captured in a hipGraph (the C ABI launches are asynchronous and
    allocation free; torch's caching allocator serves the temporaries from the graph's private pool).  replay(ids) copies
    the new token ids into the static input and replays: per-token host cost is one graph launch instead of hundreds of
    Python-side kernel launches."""

    def __init__(self, model: nn.Module, example_ids: torch.Tensor, warmup: int = 2):
        self.model = model
        self.static_ids = example_ids.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(warmup):
                model(self.static_ids, use_cache=False)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.static_logits = model(self.static_ids, use_cache=False).logits

    def replay(self, ids: torch.Tensor) -> torch.Tensor:
        self.static_ids.copy_(ids)
        self.graph.replay()
        return self.static_logits


def _decode_cache_class():
    global _DECODE_CACHE
    if _DECODE_CACHE is None:
        from transformers.cache_utils import StaticCache

        class DecodeCache(StaticCache):
            """transformers' StaticCache for an UNPADDED batch whose rows all share one position, allocated up front (so that a
            decode step can be captured before any row is written).  Made by DecodeSession / generate, not by the user.  HF code
            that receives it treats it as a StaticCache: StaticLayer.update, prefill of more than 4 rows, unfolded layers and bf16
            models keep working.  A folded layer (fuse_decode_(epilogues=True)) whose cache layer is a plain fp16 StaticLayer
            appends to it and attends over its valid rows with the HIP decode attention (runtime.rope_append_f16 /
            decode_attention_f16) instead; that path ignores the attention mask, hence the unpadded-batch contract."""

            def __init__(self, config, batch: int, max_cache_len: int, device, dtype):
                super().__init__(config=config, max_cache_len=max_cache_len)
                text = config.get_text_config(decoder=True)
                head_dim = getattr(text, "head_dim", None) or text.hidden_size // text.num_attention_heads
                self.early_initialization(batch, text.num_key_value_heads, head_dim, dtype, torch.device(device))
                self.batch = batch

        DecodeCache.__qualname__ = "DecodeCache"
        _DECODE_CACHE = DecodeCache
    return _DECODE_CACHE


def __getattr__(name):
    if name == "DecodeCache":
        return _decode_cache_class()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


class DecodeSession:
    """Decoding state of `model` (a HF causal LM) for `batch` unpadded rows and at most `max_length` positions: a DecodeCache
    on the device and, with graph=True, ONE decode step captured in a hipGraph on its first call and replayed for every later
    token.  Every forward gets a ready 4D causal mask built on the device from the cache's position (create_causal_mask passes a
    4D mask through), so nothing in a step reads the position on the host.  The host keeps its own count (`pos`) to enforce
    max_length.

    prefill / step hand the logits back and leave the choice of the token to the caller.  begin_selection / select / step_select
    keep the choice on the device as well (runtime.select_token_f16: greedy or temperature / top-k / top-p sampling, eos / pad
    bookkeeping): the captured unit is then "forward over static_ids, select into static_ids", and a generation is one replay per
    token with nothing read on the host (run_selection reads the unfinished count every poll_every tokens)."""

    def __init__(self, model: nn.Module, batch: int, max_length: int, graph: bool = True):
        if batch < 1 or max_length < 1:
            raise ValueError("DecodeSession: batch and max_length must be >= 1")
        emb = model.get_input_embeddings().weight
        self.model, self.batch, self.max_length, self.use_graph = model, int(batch), int(max_length), graph
        self.device, self.dtype = emb.device, emb.dtype
        self.cache = _decode_cache_class()(model.config, self.batch, self.max_length, self.device, self.dtype)
        self._cols = torch.arange(self.max_length, device=self.device)
        self._bool_mask = model.config._attn_implementation == "sdpa"
        self.static_ids = torch.zeros(self.batch, 1, dtype=torch.long, device=self.device)
        self.graph, self.static_logits, self.pos = None, None, 0
        self.sel, self.sel_graph = None, None

    def _mask(self, seq: int) -> torch.Tensor:
        """[batch, 1, seq, max_length]: query row s sees cache rows [0, position + s] (bool for SDPA, additive otherwise)"""
        rows = self.cache.layers[0].cumulative_length + torch.arange(seq, device=self.device)
        m = (self._cols[None, :] <= rows[:, None])[None, None].expand(self.batch, 1, seq, self.max_length)
        if self._bool_mask:
            return m
        return torch.zeros((), dtype=self.dtype, device=self.device).masked_fill(~m, torch.finfo(self.dtype).min)

    def _forward(self, ids: torch.Tensor) -> torch.Tensor:
        out = self.model(ids, attention_mask=self._mask(ids.shape[1]), past_key_values=self.cache, use_cache=True, logits_to_keep=1)
        return out.logits[:, -1]

    def _advance(self, seq: int):
        if self.pos + seq > self.max_length:
            raise ValueError(f"DecodeSession: {self.pos} + {seq} positions exceed max_length = {self.max_length}")
        self.pos += seq

    @torch.no_grad()
    def prefill(self, ids: torch.Tensor) -> torch.Tensor:
        """ids [batch, S] at the current position, eagerly (<= 4 rows in folded layers: the HIP kernels; more: HF's StaticLayer.update
        and attention).  Returns the last position's logits [batch, vocab]."""
        if ids.dim() != 2 or ids.shape[0] != self.batch or ids.shape[1] < 1:
            raise ValueError(f"DecodeSession.prefill: ids must be [{self.batch}, S >= 1]")
        self._advance(ids.shape[1])
        return self._forward(ids.to(self.device))

    @torch.no_grad()
    def step(self, tok: torch.Tensor) -> torch.Tensor:
        """one token per row (tok [batch] or [batch, 1]) at the current position; returns the logits [batch, vocab] -- with
        graph=True a view of the graph's static output, overwritten by the next step"""
        if tok.numel() != self.batch:
            raise ValueError(f"DecodeSession.step: one token per row ({self.batch})")
        self._advance(1)
        if not self.use_graph:
            return self._forward(tok.reshape(self.batch, 1).to(self.device))
        self.static_ids.copy_(tok.reshape(self.batch, 1))
        if self.graph is None:
            self.graph, self.static_logits = self._capture(lambda: self._forward(self.static_ids))
        self.graph.replay()
        return self.static_logits

    def _capture(self, unit, state=()):
        """GraphedForward's pattern: warm-up of `unit` on a side stream (it writes this position's rows, which the replay rewrites;
        its position advance and what it did to the tensors in `state` are undone), then the capture, which runs nothing.
        Returns (graph, what unit returned under capture)"""
        keep = [lay.cumulative_length for lay in self.cache.layers] + list(state)
        saved = [t.clone() for t in keep]
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(2):
                unit()
                for t, v in zip(keep, saved):
                    t.copy_(v)
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = unit()
        return graph, out

    # ---- token selection on the device
    def begin_selection(self, prompt: torch.Tensor, total: int, eos=(), pad: int | None = None, uniforms: torch.Tensor | None = None,
                        temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
        """Start a generation whose tokens are chosen on the device: allocates the result `tokens` [batch, total] (int64, the
        prompt [batch, P] in front, returned), the step counter, the rows' unfinished flags, their count and the status word.
        uniforms None: greedy; else fp32 [>= total - P, batch] uniforms in [0, 1), row t for the t-th new token, with temperature /
        top_k (0 = off) / top_p (1 = off).  eos: ids that finish a row (finished rows receive `pad`)."""
        if prompt.dim() != 2 or prompt.shape[0] != self.batch or not prompt.shape[1] < total:
            raise ValueError(f"DecodeSession.begin_selection: prompt must be [{self.batch}, P < total]")
        dev, P = self.device, int(prompt.shape[1])
        if uniforms is not None:
            if uniforms.dim() != 2 or uniforms.shape[0] < total - P or uniforms.shape[1] != self.batch:
                raise ValueError(f"DecodeSession.begin_selection: uniforms must be [>= {total - P}, {self.batch}]")
            uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
        tokens = torch.zeros(self.batch, total, dtype=torch.long, device=dev)
        tokens[:, :P] = prompt
        eos = [int(e) for e in eos]
        self.sel = dict(tokens=tokens, col0=P, n=int(total) - P, done=0, uniforms=uniforms, pad=0 if pad is None else int(pad),
                        eos=torch.tensor(eos, dtype=torch.long, device=dev) if eos else None,
                        step=torch.zeros(1, dtype=torch.long, device=dev), unfinished=torch.ones(self.batch, dtype=torch.bool, device=dev),
                        count=torch.full((1,), self.batch, dtype=torch.int32, device=dev),
                        status=torch.zeros(1, dtype=torch.int32, device=dev), params=(float(temperature), int(top_k), float(top_p)))
        self.sel_graph = None                                  # a captured unit holds the previous selection's tensors and parameters
        return tokens

    @torch.no_grad()
    def select(self, logits: torch.Tensor) -> None:
        """choose the next token of every row from `logits` [batch, vocab] fp16 on the device: it lands in the result, in static_ids
        (the next step's input) and in the bookkeeping of begin_selection.  A missing kernel is an error, not a fallback."""
        from .runtime import select_token_f16
        c = self.sel
        T, k, p = c["params"]
        if select_token_f16(logits, c["step"], c["unfinished"], c["tokens"], c["col0"], self.static_ids, c["count"], c["status"],
                            temperature=T, top_k=k, top_p=p, uniforms=c["uniforms"], eos=c["eos"], pad=c["pad"]) is None:
            raise ValueError("DecodeSession.select: pbl_select_token_f16 declines these logits (runtime.select_token_ok)")

    def _unit(self):
        self.select(self._forward(self.static_ids))

    @torch.no_grad()
    def step_select(self) -> None:
        """one decode step over the tokens the last selection left in static_ids, and the selection of the next ones: with
        graph=True ONE replay of a unit captured on the first call"""
        self._advance(1)
        if not self.use_graph:
            return self._unit()
        if self.sel_graph is None:
            c = self.sel
            self.sel_graph, _ = self._capture(self._unit, [self.static_ids, c["step"], c["unfinished"], c["count"], c["status"], c["tokens"]])
        self.sel_graph.replay()

    @torch.no_grad()
    def run_selection(self, n: int, poll_every: int = 8) -> int:
        """up to n more step_select calls; with eos ids, the device's count of unfinished rows is read after every poll_every-th new
        token of the generation and the loop ends once it is zero (rows that had finished receive pad meanwhile).  Returns the
        number of new tokens generated so far (the first one comes from select on the prefill's logits)."""
        c = self.sel
        for _ in range(n):
            if c["eos"] is not None and c["done"] % poll_every == 0 and int(c["count"]) == 0:
                break
            self.step_select()
            c["done"] += 1
        return c["done"]

    def selection_result(self) -> torch.Tensor:
        """the prompt and the new tokens so far, cut after the column at which the last row finished (what a check after every
        token would have returned); RuntimeError if a sampled row held NaN or +inf (torch.multinomial raises for such a row)"""
        c = self.sel
        status = int(c["status"])
        if status & 1:
            raise RuntimeError("generate: a row of logits held NaN or +inf (or nothing finite) while sampling")
        if status & 2:
            raise RuntimeError("generate: the selection step ran outside the result buffer or the table of uniforms")
        P, done = c["col0"], c["done"]
        if c["eos"] is not None and done:
            hit = torch.isin(c["tokens"][:, P:P + done], c["eos"])
            first = torch.where(hit.any(1), hit.int().argmax(1) + 1, done)
            done = int(first.max())
        return c["tokens"][:, :P + done]

    def reset(self):
        """zero the cache rows and positions (the captured step stays valid: same tensors)"""
        self.cache.reset()
        self.pos = 0


def _generation_limits(model: nn.Module, prompt_len: int, max_length=None, max_new_tokens=None, eos_token_id=None,
                       pad_token_id=None) -> tuple[int, list, int | None]:
    """(total length, eos ids, pad id) as model.generate resolves them for greedy decoding: max_new_tokens wins over max_length;
    without either, the generation config's max_new_tokens, else its max_length NEW tokens (capped at max_position_embeddings);
    ValueError where nothing is left to generate.  eos defaults to the generation config's, pad to its pad_token_id, else the
    first eos id"""
    gc = getattr(model, "generation_config", None)
    if max_new_tokens is None and max_length is None:
        max_new_tokens = getattr(gc, "max_new_tokens", None)
    if max_new_tokens is not None:
        if int(max_new_tokens) < 1:
            raise ValueError("generate: max_new_tokens must be >= 1")
        total = prompt_len + int(max_new_tokens)
    elif max_length is not None:
        total = int(max_length)
    else:                                          # the config's max_length counts NEW tokens then, within max_position_embeddings
        total = prompt_len + int(getattr(gc, "max_length", None) or 20)
        cap = getattr(getattr(model, "config", None), "max_position_embeddings", None)
        total = min(total, cap) if cap is not None else total
    if total <= prompt_len:
        raise ValueError(f"Input length of input_ids is {prompt_len}, but `max_length` is set to {total}: set max_new_tokens")
    if eos_token_id is None:
        eos_token_id = getattr(gc, "eos_token_id", None)
    eos = [] if eos_token_id is None else [int(e) for e in (eos_token_id if isinstance(eos_token_id, (list, tuple)) else [eos_token_id])]
    if pad_token_id is None:
        pad_token_id = getattr(gc, "pad_token_id", None)
    if pad_token_id is None and eos:
        pad_token_id = eos[0]
    return total, eos, None if pad_token_id is None else int(pad_token_id)


_GREEDY_DEFAULTS = {"do_sample": False, "num_beams": 1, "use_cache": True}
_SAMPLING_ARGS = ("temperature", "top_k", "top_p")


def _sampling_params(model: nn.Module, temperature=None, top_k=None, top_p=None) -> tuple[float, int, float]:
    """(temperature, top_k, top_p) as model.generate resolves them for do_sample=True: the argument, else the value in
    model.generation_config, else -- for fields still None -- transformers' GenerationConfig._get_default_generation_params().
    temperature 1.0, top_k 0 and top_p 1.0 mean "off" (HF builds no warper for them)."""
    from transformers import GenerationConfig
    gc = getattr(model, "generation_config", None)
    defaults = GenerationConfig._get_default_generation_params()
    vals = []
    for name, v in (("temperature", temperature), ("top_k", top_k), ("top_p", top_p)):
        if v is None:
            v = getattr(gc, name, None)
        if v is None:
            v = defaults[name]
        vals.append(v)
    return float(vals[0]), int(vals[1]), float(vals[2])


@torch.no_grad()
def generate(model: nn.Module, input_ids: torch.Tensor, max_length: int | None = None, max_new_tokens: int | None = None,
             eos_token_id=None, pad_token_id: int | None = None, attention_mask: torch.Tensor | None = None, graph: bool = True,
             generator: torch.Generator | None = None, uniforms: torch.Tensor | None = None, poll_every: int = 8,
             **kwargs) -> torch.Tensor:
    """Decoding of an unpadded batch input_ids [B, P] on the GPU: greedy -- what model.generate(input_ids, do_sample=False, ...)
    returns -- or, with do_sample=True, sampling with temperature / top_k / top_p (values not passed are resolved as model.generate
    resolves them: _sampling_params).  The result is the prompt followed by the new tokens, rows that met eos padded with
    pad_token_id, ending where every row has finished or at the length limit.  One DecodeSession: the prompt is prefilled eagerly,
    then each token replays ONE captured unit -- the decode step and the HIP token selection (pbl_select_token_f16), which writes
    the token into the result and into the next step's input and keeps the eos / pad bookkeeping on the device.  The host reads
    the count of unfinished rows every `poll_every` tokens (never without an eos id); tokens generated after every row finished
    are pad and are cut off, so the result does not depend on poll_every.

    Sampling draws its uniforms ONCE per call, before the loop: torch.rand([new tokens, B]) from `generator` (default: the default
    generator of the model's device, so torch.manual_seed(n) reproduces a run), or the caller's table `uniforms` [>= new tokens, B]
    (values in [0, 1)).  graph=True and graph=False consume the same numbers and give the same tokens.  The token stream for a
    given seed differs from model.generate's (torch.multinomial consumes the generator differently); the distribution is the same,
    up to HF's arbitrary choice inside a block of tied values at the top-p boundary.

    Handed to model.generate unchanged: an attention_mask with zeros (a padded batch), a model off the GPU, beams, any other
    generation argument (repetition_penalty, min_p, ...), do_sample=False together with sampling arguments, and sampling on a model
    whose logits are not fp16.  model.generate cannot honour `generator` or `uniforms`, so a call that passes one of them and must
    be handed over raises ValueError.  Greedy decoding of logits that are not fp16 keeps the selection in torch."""
    sample = kwargs.get("do_sample", False) is True
    fixed = {k: v for k, v in _GREEDY_DEFAULTS.items() if not (sample and k == "do_sample")}
    known = set(_GREEDY_DEFAULTS) | (set(_SAMPLING_ARGS) if sample else set())
    native = all(kwargs[k] == v for k, v in fixed.items() if k in kwargs) and not set(kwargs) - known
    padded = attention_mask is not None and not bool(attention_mask.all())
    if native and sample:
        T, top_k, top_p = _sampling_params(model, *(kwargs.get(k) for k in _SAMPLING_ARGS))
        native = T > 0 and top_k >= 0 and 0 < top_p <= 1 and model.get_input_embeddings().weight.dtype == torch.float16

    def hand_over():
        if generator is not None or uniforms is not None:
            raise ValueError("generate: generator= and uniforms= belong to the sampling loop on the GPU (an unpadded batch on a GPU model "
                             "with fp16 logits, do_sample=True with temperature / top_k / top_p only); model.generate cannot honour them")
        hf = dict(kwargs)
        for k, v in (("max_length", max_length), ("max_new_tokens", max_new_tokens), ("eos_token_id", eos_token_id),
                     ("pad_token_id", pad_token_id), ("attention_mask", attention_mask)):
            if v is not None:
                hf[k] = v
        return model.generate(input_ids, **hf)

    if not native or padded or not input_ids.is_cuda or input_ids.dim() != 2:
        return hand_over()
    if poll_every < 1:
        raise ValueError("generate: poll_every must be >= 1")
    B, P = input_ids.shape
    total, eos, pad = _generation_limits(model, P, max_length, max_new_tokens, eos_token_id, pad_token_id)
    from .runtime import select_token_ok
    sess = DecodeSession(model, B, total - 1, graph=graph)
    logits = sess.prefill(input_ids)
    if logits.dtype == torch.float16 and select_token_ok(B, logits.shape[1]):
        table = None
        if sample:
            if uniforms is not None:
                table = uniforms
            else:                                          # one draw for the whole call; a host generator draws on the host
                gdev = generator.device if generator is not None else input_ids.device
                table = torch.rand(total - P, B, generator=generator, device=gdev, dtype=torch.float32)
        else:
            T, top_k, top_p = 1.0, 0, 1.0
        sess.begin_selection(input_ids, total, eos=eos, pad=pad, uniforms=table, temperature=T, top_k=top_k, top_p=top_p)
        sess.select(logits)
        sess.sel["done"] = 1
        sess.run_selection(total - P - 1, poll_every)
        return sess.selection_result()
    if sample:
        return hand_over()
    out = [input_ids]
    eos_t = torch.tensor(eos, dtype=input_ids.dtype, device=input_ids.device) if eos else None
    unfinished = torch.ones(B, dtype=torch.bool, device=input_ids.device)
    cur = P
    while True:
        nxt = logits.float().argmax(-1).to(input_ids.dtype)
        if eos_t is not None:
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
            unfinished &= ~torch.isin(nxt, eos_t)
        out.append(nxt[:, None])
        cur += 1
        if cur >= total or (eos_t is not None and not bool(unfinished.any())):
            break
        logits = sess.step(nxt)
    return torch.cat(out, 1)


@torch.no_grad()
def perplexity(model: nn.Module, input_ids: torch.Tensor, seqlen: int) -> float:
    """The loop of gptq_pb/eval_ppl_utils.py:55-86 / evaluate.py:126-156 on pre-tokenised ids
    [1, n*seqlen]: mean NLL over non-overlapping windows -> exp."""
    n = input_ids.numel() // seqlen
    nll = 0.0
    for i in range(n):
        batch = input_ids[:, i * seqlen:(i + 1) * seqlen]
        logits = model(batch).logits.float()
        loss = nn.functional.cross_entropy(logits[0, :-1], batch[0, 1:], reduction="sum")
        nll += float(loss)
    return float(torch.exp(torch.tensor(nll / (n * (seqlen - 1)))))
