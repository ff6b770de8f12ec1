"""Model-level harness: what gptq_pb/run.py:116-178 and
qat/eval_after_qat.py:12-24 do around the hot path, without datasets or checkpoints (none
are available offline): quantize every decoder Linear of a HF causal LM to a dense
fake-quant weight, swap in PBLinear modules, run forward / perplexity-style loops.

`quant_sequential_` is the counterpart of gptq_pb/run.py:quant_sequential on one MI355X: the whole model
stays resident in HBM (288 GB: no layer-by-layer host offload), every decoder Linear is quantised by the fused
GPTQ-PB pipeline (pb_llm_amd/ptq.py) and, optionally, packed on the spot.
`quantize_dense_` takes an external structure producer instead (tests pass the oracle's).
Decode fusion (`fuse_decode_`) lives in fusion.py, generation (`DecodeSession`, `generate`) in decoding.py and continuation scoring
(`token_logprobs`, `loglikelihood`) in scoring.py; re-exported here.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import decoding, quant as Q, scoring
from .decoding import DecodeSession, _generation_limits, _sampling_params, generate  # noqa: F401
from .fusion import FUSE_SETS, _DeferredNorm, _FoldedMLP, _FusedGroup, _FusedMember, fuse_decode_  # noqa: F401
from .quant import PBLinear, replace_linear_with_pb
from .scoring import _batches, loglikelihood, token_logprobs  # noqa: F401


def __getattr__(name):                   # harness.DecodeCache: the class decoding.py builds on first use (transformers stays lazy)
    if name == "DecodeCache":
        return decoding._decode_cache_class()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


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


def _image_of(m: PBLinear):
    """the GEMM image (quant._kept_image: built on first use) of an fp16-checkpoint layer that holds its blob on the GPU, else None"""
    ok = m.weight_dtype == torch.float16 and m.pbl_blob.is_cuda and Q.fused_gemm_ok(m.packed)
    return Q._kept_image(m.packed) if ok else None


def build_gemm_images_(model: nn.Module, release_blobs: bool = False) -> tuple[int, int]:
    """Build and keep the GEMM image of every packed fp16-checkpoint linear of `model` NOW (quant._kept_image), instead of on its
    first prefill call: afterwards calls with 5 - 64 rows run the small-batch kernel over the image under the default
    quant.SMALL_BATCH_IMAGE = "auto" -- also inside a hipGraph capture, where an image cannot be built (the build reads two words
    back).  Costs the images' memory on top of the blobs (1.7 - 2.4 x the blob's bytes) -- unless release_blobs (round 6): then the
    image becomes each layer's ONLY device copy (PBLinear.release_blob_: the blob moves to host memory, state_dict() still holds it;
    every row count multiplies from the image) -- what an evaluation run wants (qat/eval_after_qat.py:11-33, gptq_pb/eval_ppl_utils.py:
    55-64 call the layers with whole 2048-token windows only): a llama-7b-shaped model at 5 % hessian salients holds 4.2 GB instead
    of 6.3.  Returns (layers with an image, image bytes); `release_blobs_` / `restore_blobs_` do the second step on their own."""
    n = nbytes = 0
    for m in model.modules():
        if isinstance(m, PBLinear):
            img = m._image_only[0] if m._image_only is not None else _image_of(m)
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
    if any(isinstance(m, _FusedMember) for m in model.modules()):
        raise RuntimeError("release_blobs_: the model's projections are fused for decode (fuse_decode_), whose launches read the blobs")
    n = 0
    for m in model.modules():
        if isinstance(m, PBLinear) and m._image_only is None and _image_of(m) is not None:
            n += m.release_blob_(pin)
    torch.cuda.empty_cache()
    return n


def restore_blobs_(model: nn.Module) -> int:
    """the blobs of every image-only linear back on the device (decode through the GEMV again); returns the layers restored"""
    n = 0
    for m in model.modules():
        if isinstance(m, PBLinear) and m._image_only is not None:
            m.restore_blob_()
            n += 1
    return n


def drop_gemm_images_(model: nn.Module) -> int:
    """Release every kept GEMM image (and kept salient list) of `model`'s packed linears -- the memory knob next to
    build_gemm_images_: with the round-5 defaults every fp16-exact linear gets an image on its first call with 5 rows or more
    (1.7 - 2.4 x the blob's bytes; 4.2 GB for a 7B model at 5 % hessian salients), which a decode-only phase at batch <= 4 never
    reads.  The next call that wants an image rebuilds it.  Not while a captured graph that uses the images may still be replayed.
    Also forgets the kept fragment-major copy of the last activation (quant.drop_x_fragments_).  Returns the bytes released."""
    Q.drop_x_fragments_()
    n = 0
    for m in model.modules():
        if isinstance(m, PBLinear):
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
        self.graph, self.static_logits = decoding._capture_graph(lambda: model(self.static_ids, use_cache=False).logits,
                                                                 self.static_ids.device, warmup=warmup)

    def replay(self, ids: torch.Tensor) -> torch.Tensor:
        self.static_ids.copy_(ids)
        self.graph.replay()
        return self.static_logits



@torch.no_grad()
def perplexity(model: nn.Module, input_ids: torch.Tensor, seqlen: int, fused: bool = False) -> float:
    """The loop of gptq_pb/eval_ppl_utils.py:55-86 / evaluate.py:126-156 on pre-tokenised ids
    [1, n*seqlen]: mean NLL over non-overlapping windows -> exp.  fused=True: every window's fp16 logits are scored by one HIP
    call over the view logits[0, :-1] (no fp32 copy, no cross_entropy) and the host reads once, after the last window
    (scoring.perplexity_fused)."""
    if fused:
        return scoring.perplexity_fused(model, input_ids, seqlen)
    n = input_ids.numel() // seqlen
    nll = 0.0
    for i in range(n):
        batch = input_ids[:, i * seqlen:(i + 1) * seqlen]
        logits = model(batch).logits.float()
        loss = nn.functional.cross_entropy(logits[0, :-1], batch[0, 1:], reduction="sum")
        nll += float(loss)
    return float(torch.exp(torch.tensor(nll / (n * (seqlen - 1)))))
