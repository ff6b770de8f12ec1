"""Continuation scoring (harness.py re-exports it): token_logprobs and loglikelihood, the counterpart of lm-eval's `_model_call` +
`_loglikelihood_tokens` for the accuracy tasks, and the fused tail of harness.perplexity.  fp16 logits on the GPU are scored by ONE
read of the logits (runtime.score_tokens_f16); any other logits (a bf16 or fp32 model, a model on the CPU) by torch.
loglikelihood(share_prefix=True) computes a context that several requests share ONCE: shared_prefix_plan packs their continuations
behind it, and one forward with branch attention (runtime.branch_attention_f16 in folded fp16 layers, a 4-D mask everywhere else)
scores them all."""
from __future__ import annotations

import logging
from typing import NamedTuple

import torch
import torch.nn as nn

from . import runtime

_LOG = logging.getLogger("pb_llm_amd")
IGNORE_INDEX = -100
_fallback_logged = False
# loglikelihood(share_prefix=True) on an fp16 model on the GPU whose decoder layers are all fuse_decode_(epilogues=True) folded layers:
# the packed forward runs over a DecodeCache with the HIP branch attention (runtime.branch_attention_f16).  False: that model takes
# the route of every other model -- no cache, a 4-D branch mask handed to HF's attention.  Read HERE when a call starts.
BRANCH_ATTENTION = True


def _score_torch(logits: torch.Tensor, targets: torch.Tensor, spans: torch.Tensor | None, ignore_index: int):
    """score_tokens_f16's results from torch: log_softmax in fp32, gather, argmax; spans in fp64"""
    T, V = logits.shape
    lsm = torch.log_softmax(logits.float(), -1)
    ignored = targets == ignore_index
    bad = ~ignored & ((targets < 0) | (targets >= V))
    safe = targets.clamp(0, V - 1)
    logprob = lsm.gather(1, safe[:, None])[:, 0]
    greedy = lsm.argmax(-1) == safe
    logprob = torch.where(ignored, torch.zeros_like(logprob), torch.where(bad, torch.full_like(logprob, float("nan")), logprob))
    greedy = greedy & ~ignored & ~bad
    status = torch.zeros(1, dtype=torch.int32, device=logits.device)
    status |= bad.any().to(torch.int32)
    if spans is None:
        return logprob, greedy, None, None, None, status
    R = spans.shape[0]
    span_sum = torch.zeros(R, dtype=torch.float64, device=logits.device)
    span_greedy = torch.ones(R, dtype=torch.bool, device=logits.device)
    span_count = torch.zeros(R, dtype=torch.int32, device=logits.device)
    for r, (b, e) in enumerate(spans.tolist()):
        if b < 0 or e > T or b > e:
            span_sum[r], span_greedy[r] = float("nan"), False
            status |= 2
            continue
        keep = ~ignored[b:e]
        span_sum[r] = logprob[b:e][keep].double().sum()
        span_greedy[r] = bool(greedy[b:e][keep].all())
        span_count[r] = int(keep.sum())
    return logprob, greedy, span_sum, span_greedy, span_count, status


def _score(logits: torch.Tensor, targets: torch.Tensor, spans: torch.Tensor | None = None, ignore_index: int = IGNORE_INDEX):
    """rows [T, V] -> (logprob, greedy, span_sum, span_greedy, span_count, status): the HIP kernel for fp16 logits on the GPU (a
    shape it declines is an error, not a fallback), torch for everything else -- said once per process"""
    global _fallback_logged
    if logits.dtype == torch.float16 and logits.is_cuda:
        out = runtime.score_tokens_f16(logits, targets, spans, ignore_index)
        if out is None:
            raise ValueError(f"scoring: pbl_score_tokens_f16 declines logits of shape {tuple(logits.shape)} (runtime.score_tokens_ok)")
        return out
    if not _fallback_logged:
        _fallback_logged = True
        _LOG.info("scoring: %s logits on %s are scored by torch (log_softmax in fp32, gather, argmax); the HIP kernel "
                  "(pbl_score_tokens_f16) takes fp16 logits on the GPU", str(logits.dtype).replace("torch.", ""), logits.device.type)
    return _score_torch(logits, targets, spans, ignore_index)


def _rows(logits: torch.Tensor, vocab_limit: int | None) -> torch.Tensor:
    """logits [B, T, V] as the 2-D view [B * T, V'] of evenly strided rows (V' = vocab_limit columns): no copy"""
    B, T, V = logits.shape
    if logits.stride(2) != 1 or (B > 1 and logits.stride(0) != T * logits.stride(1)):
        raise ValueError("scoring: the model's logits are not [B, T, V] with evenly strided rows")
    rows = logits[0] if B == 1 else logits.flatten(0, 1)
    return rows if vocab_limit is None else rows[:, :vocab_limit]


def _device(model: nn.Module) -> torch.device:
    return next(model.parameters()).device


@torch.no_grad()
def token_logprobs(model: nn.Module, input_ids: torch.Tensor, vocab_limit: int | None = None):
    """log p(ids[:, t+1] | ids[:, :t+1]) and "ids[:, t+1] is the arg-max" for t in [0, T-1): (fp32 [B, T-1], bool [B, T-1]).  One
    forward, one scoring call over the view logits[:, :-1, :vocab_limit]: the rows are handed over as [B * T, V'] with the last
    row of every sequence marked ignore_index, which the kernel does not read."""
    if input_ids.dim() != 2 or input_ids.shape[1] < 2:
        raise ValueError("token_logprobs: input_ids must be [B, T >= 2]")
    B, T = input_ids.shape
    ids = input_ids.to(_device(model))
    rows = _rows(model(ids).logits, vocab_limit)
    targets = torch.full((B, T), IGNORE_INDEX, dtype=torch.int64, device=rows.device)
    targets[:, :-1] = ids[:, 1:]
    logprob, greedy, _, _, _, status = _score(rows, targets.view(-1))
    if int(status):
        raise RuntimeError(f"token_logprobs: a token id lies outside the {rows.shape[1]} scored columns of the vocabulary")
    return logprob.view(B, T)[:, :-1], greedy.view(B, T)[:, :-1]


def _checked(requests, batch_size: int, max_length: int) -> list:
    """[(ctx + cont as ints, len(cont))] per request, after the checks every loglikelihood call makes before it computes anything"""
    if batch_size < 1 or max_length < 1:
        raise ValueError("loglikelihood: batch_size and max_length must be at least 1")
    toks = []
    for i, (ctx, cont) in enumerate(requests):
        ctx, cont = [int(t) for t in ctx], [int(t) for t in cont]
        if not ctx:
            raise ValueError(f"loglikelihood: request {i} has an empty context")
        if not cont:
            raise ValueError(f"loglikelihood: request {i} has an empty continuation")
        if len(cont) > max_length:
            raise ValueError(f"loglikelihood: the continuation of request {i} ({len(cont)} tokens) is longer than max_length = {max_length}")
        toks.append((ctx + cont, len(cont)))
    return toks


def _batches(requests, batch_size: int, max_length: int, pad_token_id: int = 0):
    """lm-eval 0.3's BaseLM._loglikelihood_tokens batching: requests longest first (key: -len(ctx + cont), then the tokens), each
    input (ctx + cont)[-(max_length + 1):][:-1], right-padded to the batch's longest.  Yields (input_ids int64 [b, L], targets int64
    [b * L] -- the continuation's tokens at its rows, ignore_index elsewhere --, spans int64 [b, 2] -- the continuation's rows of
    request j in the flattened [b * L, V] logits --, request_indices), all on the CPU."""
    toks = _checked(requests, batch_size, max_length)
    order = sorted(range(len(toks)), key=lambda i: (-len(toks[i][0]), tuple(toks[i][0])))
    for s in range(0, len(order), batch_size):
        idx = order[s:s + batch_size]
        inps = [toks[i][0][-(max_length + 1):][:-1] for i in idx]
        L = max(len(x) for x in inps)
        input_ids = torch.full((len(idx), L), int(pad_token_id), dtype=torch.int64)
        targets = torch.full((len(idx), L), IGNORE_INDEX, dtype=torch.int64)
        spans = torch.empty(len(idx), 2, dtype=torch.int64)
        for j, (i, inp) in enumerate(zip(idx, inps)):
            n = toks[i][1]
            input_ids[j, :len(inp)] = torch.tensor(inp, dtype=torch.int64)
            targets[j, len(inp) - n:len(inp)] = torch.tensor(toks[i][0][-n:], dtype=torch.int64)
            spans[j, 0], spans[j, 1] = j * L + len(inp) - n, j * L + len(inp)
        yield input_ids, targets.view(-1), spans, idx


class PackedBatch(NamedTuple):
    """One forward of shared_prefix_plan: b packed sequences right-padded to L rows.  tokens / position_ids / lo: b lists of L ints;
    trunk: b ints; requests: [(request index, sequence j, score rows)] -- the packed rows of sequence j whose logits score the
    request's continuation tokens, in order (the last trunk row first, then the request's own branch rows)"""
    tokens: list
    position_ids: list
    trunk: list
    lo: list
    requests: list


class SharedPrefixPlan(NamedTuple):
    """batches: the PackedBatches, longest first; unshared: the indices of the requests that go the unshared way, ascending"""
    batches: list
    unshared: list


def shared_prefix_plan(requests, batch_size: int, max_length: int, pad_token_id: int = 0) -> SharedPrefixPlan:
    """Group the requests whose context token lists are EQUAL; a group of two or more becomes one packed sequence

        [ trunk: the T context tokens | branch 0: cont_0[:-1] | branch 1: cont_1[:-1] | ... | right padding ]

    with position_ids i for trunk row i and T + i for row i of any branch, trunk = T and lo[s] = the packed index of the first row
    of row s's own branch (0 for trunk rows, s for padding rows): runtime.branch_attention_f16's tables.  The last trunk row scores
    cont_j[0] for every j, branch j's rows score cont_j[1:]; a one-token continuation has no branch rows.
    Unshared (scoring._batches, unchanged): a group of one; a request that lm-eval's left truncation would touch (len(ctx + cont) >
    max_length + 1); what is left of a group whose packed length exceeds max_length after it was split, in request order, into
    sub-groups that fit.  A batch holds whole groups whose request counts sum to at most batch_size (at least one group); batches
    run longest packed length first.  Empty contexts / continuations raise what loglikelihood raises without the plan."""
    toks = _checked(requests, batch_size, max_length)
    by_ctx, unshared = {}, []
    for i, (full, n) in enumerate(toks):
        if len(full) > max_length + 1:
            unshared.append(i)
        else:
            by_ctx.setdefault(tuple(full[:-n]), []).append(i)
    groups = []                                                   # [(packed length, [request indices])]
    for ctx, members in by_ctx.items():
        sub, rows = [], len(ctx)
        for i in members + [None]:
            extra = 0 if i is None else toks[i][1] - 1
            if i is None or (sub and rows + extra > max_length):
                if len(sub) > 1:
                    groups.append((rows, sub))
                else:
                    unshared += sub
                sub, rows = [], len(ctx)
            if i is not None:
                sub.append(i)
                rows += extra
    groups.sort(key=lambda g: (-g[0], g[1][0]))
    batches, cur, count = [], [], 0
    for g in groups + [None]:
        if cur and (g is None or count + len(g[1]) > batch_size):
            L = cur[0][0]
            b = PackedBatch([], [], [], [], [])
            for j, (rows, members) in enumerate(cur):
                full, n = toks[members[0]]
                T = len(full) - n
                tokens, position_ids, lo = list(full[:T]), list(range(T)), [0] * T
                for i in members:
                    full, n = toks[i]
                    start = len(tokens)
                    b.requests.append((i, j, [T - 1] + list(range(start, start + n - 1))))
                    tokens += full[T:-1]
                    position_ids += range(T, T + n - 1)
                    lo += [start] * (n - 1)
                pad = L - len(tokens)
                b.tokens.append(tokens + [int(pad_token_id)] * pad)
                b.position_ids.append(position_ids + [0] * pad)
                b.lo.append(lo + list(range(L - pad, L)))
                b.trunk.append(T)
            batches.append(b)
            cur, count = [], 0
        if g is not None:
            cur.append(g)
            count += len(g[1])
    return SharedPrefixPlan(batches, sorted(unshared))


def _branch_mask(trunk: torch.Tensor, lo: torch.Tensor, cols: int, dtype: torch.dtype, as_bool: bool) -> torch.Tensor:
    """[b, 1, L, cols]: query row s sees column k iff k <= s and (k < trunk or k >= lo[s]) -- bool for SDPA, additive otherwise
    (DecodeSession._mask's two forms)"""
    L = lo.shape[1]
    k = torch.arange(cols, device=lo.device)[None, None, :]
    rows = torch.arange(L, device=lo.device)[None, :, None]
    m = ((k <= rows) & ((k < trunk[:, None, None]) | (k >= lo[:, :, None])))[:, None]
    if as_bool:
        return m
    return torch.zeros((), dtype=dtype, device=lo.device).masked_fill(~m, torch.finfo(dtype).min)


def _branch_route(model: nn.Module, plan: SharedPrefixPlan) -> bool:
    """the packed forwards of `plan` take the HIP route: BRANCH_ATTENTION is on, the model is fp16 on the GPU, every decoder layer is a
    fuse_decode_(epilogues=True) folded layer and runtime.branch_attention_ok takes every batch"""
    from . import fusion
    emb = model.get_input_embeddings().weight
    if not BRANCH_ATTENTION or not plan.batches or emb.dtype != torch.float16 or not emb.is_cuda:
        return False
    try:
        from transformers.models.llama.modeling_llama import LlamaDecoderLayer
    except ImportError:
        return False
    layers = [m for m in model.modules() if isinstance(m, LlamaDecoderLayer)]
    cfg = model.config.get_text_config(decoder=True)
    if not layers or len(layers) != cfg.num_hidden_layers \
            or not all(getattr(lay.forward, "__func__", None) is fusion._folded_layer_forward for lay in layers):
        return False
    head_dim = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
    return all(runtime.branch_attention_ok(len(b.trunk), len(b.tokens[0]), cfg.num_attention_heads, cfg.num_key_value_heads, head_dim,
                                           len(b.tokens[0])) for b in plan.batches)


def _loglikelihood_shared(model: nn.Module, requests, batch_size: int, max_length: int, vocab_limit: int | None,
                          pad_token_id: int) -> list:
    """loglikelihood(share_prefix=True).  Per PackedBatch: ONE forward of the decoder over the packed rows, a gather of the score
    rows into request-major order (the shared trunk row once per request), the output embedding over those rows only, one scoring
    call with one span per request, one device-to-host read.  The forward: over a DecodeCache that carries the batch's branch table
    (_branch_route: runtime.branch_attention_f16 in every layer), else without a cache under a 4-D branch mask."""
    plan = shared_prefix_plan(requests, batch_size, max_length, pad_token_id)
    results = [None] * len(requests)
    if plan.unshared:
        rest = _loglikelihood_unshared(model, [requests[i] for i in plan.unshared], batch_size, max_length, vocab_limit, pad_token_id)
        for i, r in zip(plan.unshared, rest):
            results[i] = r
    dev = _device(model)
    decoder, head = model.get_decoder(), model.get_output_embeddings()
    dtype = model.get_input_embeddings().weight.dtype
    as_bool = model.config._attn_implementation == "sdpa"
    caches = {}                                                   # batch rows -> DecodeCache (the HIP route)
    if _branch_route(model, plan):
        from .decoding import _decode_cache_class
        for b in sorted({len(b.trunk) for b in plan.batches}):
            longest = max(len(pb.tokens[0]) for pb in plan.batches if len(pb.trunk) == b)
            caches[b] = _decode_cache_class()(model.config, b, longest, dev, dtype)
    for pb in plan.batches:
        b, L = len(pb.trunk), len(pb.tokens[0])
        ids = torch.tensor(pb.tokens, dtype=torch.int64).to(dev)
        position_ids = torch.tensor(pb.position_ids, dtype=torch.int64).to(dev)
        trunk = torch.tensor(pb.trunk, dtype=torch.int32).to(dev)
        lo = torch.tensor(pb.lo, dtype=torch.int32).to(dev)
        cache = caches.get(b)
        if cache is None:
            hidden = decoder(input_ids=ids, attention_mask=_branch_mask(trunk, lo, L, dtype, as_bool), position_ids=position_ids,
                             use_cache=False).last_hidden_state
        else:
            cache.reset()
            cache.branch = (trunk, lo)
            try:                                                  # (the folded layers do not read the mask; it is the right one all the same)
                hidden = decoder(input_ids=ids, attention_mask=_branch_mask(trunk, lo, cache.max_cache_len, dtype, as_bool),
                                 position_ids=position_ids, past_key_values=cache, use_cache=True).last_hidden_state
            finally:
                cache.branch = None
        gather, targets, spans = [], [], []
        for i, j, rows in pb.requests:
            spans.append((len(gather), len(gather) + len(rows)))
            gather += [j * L + r for r in rows]
            targets += requests[i][1]
        logits = head(hidden.flatten(0, 1)[torch.tensor(gather, dtype=torch.int64).to(dev)])
        rows = logits if vocab_limit is None else logits[:, :vocab_limit]
        _, _, span_sum, span_greedy, _, status = _score(rows, torch.tensor([int(t) for t in targets], dtype=torch.int64).to(rows.device),
                                                        torch.tensor(spans, dtype=torch.int64).to(rows.device))
        host = torch.cat([span_sum, span_greedy.double(), status.double()]).cpu()          # the one read of the batch
        if int(host[-1]):
            raise RuntimeError(f"loglikelihood: scoring status {int(host[-1])}: a continuation token lies outside the "
                               f"{rows.shape[1]} scored columns of the vocabulary")
        n = len(pb.requests)
        for r, (i, _, _) in enumerate(pb.requests):
            results[i] = (float(host[r]), bool(host[n + r]))
    return results


@torch.no_grad()
def loglikelihood(model: nn.Module, requests, batch_size: int = 1, max_length: int | None = None, vocab_limit: int | None = None,
                  pad_token_id: int = 0, share_prefix: bool = False) -> list:
    """[(log p(continuation | context), the continuation is the greedy decoding)] for requests = [(context_ids, continuation_ids)],
    in request order, with the semantics of lm-eval 0.3's BaseLM._loglikelihood_tokens (see _batches; no attention mask is passed:
    the padding sits after every real token of a causal model).  Per batch: one forward, one scoring call with one span per request,
    one device-to-host read.
    share_prefix=True: requests with EQUAL contexts (the choices of a multiple-choice document) are packed behind one copy of the
    context and scored by one forward with branch attention (shared_prefix_plan, _loglikelihood_shared); every other request goes
    the way it goes with False.  The results agree with False up to the rounding of the attention and of the linears at another row
    count."""
    if max_length is None:
        max_length = int(model.config.max_position_embeddings)
    if share_prefix:
        return _loglikelihood_shared(model, requests, batch_size, max_length, vocab_limit, pad_token_id)
    return _loglikelihood_unshared(model, requests, batch_size, max_length, vocab_limit, pad_token_id)


def _loglikelihood_unshared(model: nn.Module, requests, batch_size: int, max_length: int, vocab_limit: int | None,
                            pad_token_id: int) -> list:
    dev = _device(model)
    results = [None] * len(requests)
    for input_ids, targets, spans, idx in _batches(requests, batch_size, max_length, pad_token_id):
        rows = _rows(model(input_ids.to(dev)).logits, vocab_limit)
        _, _, span_sum, span_greedy, _, status = _score(rows, targets.to(rows.device), spans.to(rows.device))
        host = torch.cat([span_sum, span_greedy.double(), status.double()]).cpu()          # the one read of the batch
        if int(host[-1]):
            raise RuntimeError(f"loglikelihood: scoring status {int(host[-1])}: a continuation token lies outside the "
                               f"{rows.shape[1]} scored columns of the vocabulary")
        n = len(idx)
        for j, i in enumerate(idx):
            results[i] = (float(host[j]), bool(host[n + j]))
    return results


@torch.no_grad()
def perplexity_fused(model: nn.Module, input_ids: torch.Tensor, seqlen: int) -> float:
    """harness.perplexity(fused=True): per window one scoring call over the view logits[0, :-1] with one span; the fp64 span sums
    stay on the device and the host reads once, after the last window"""
    n = input_ids.numel() // seqlen
    dev = _device(model)
    ids = input_ids.to(dev)
    span = torch.tensor([[0, seqlen - 1]], dtype=torch.int64, device=dev)
    sums, flags = [], []
    for i in range(n):
        batch = ids[:, i * seqlen:(i + 1) * seqlen]
        logits = model(batch).logits
        _, _, span_sum, _, _, status = _score(logits[0, :-1], batch[0, 1:].contiguous(), span.to(logits.device))
        sums.append(span_sum)
        flags.append(status)
    host = torch.cat([torch.cat(sums).sum()[None], torch.cat(flags).max()[None].double()]).cpu()
    if int(host[1]):
        raise RuntimeError("perplexity: a token id lies outside the model's vocabulary")
    return float(torch.exp(torch.tensor(-float(host[0]) / (n * (seqlen - 1)))))
