"""Continuation scoring (harness.py re-exports it): token_logprobs and loglikelihood, the counterpart of lm-eval's `_model_call` +
`_loglikelihood_tokens` for the accuracy tasks, and the fused tail of harness.perplexity.  fp16 logits on the GPU are scored by ONE
read of the logits (runtime.score_tokens_f16); any other logits (a bf16 or fp32 model, a model on the CPU) by torch."""
from __future__ import annotations

import logging

import torch
import torch.nn as nn

from . import runtime

_LOG = logging.getLogger("pb_llm_amd")
IGNORE_INDEX = -100
_fallback_logged = False


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


def _batches(requests, batch_size: int, max_length: int, pad_token_id: int = 0):
    """lm-eval 0.3's BaseLM._loglikelihood_tokens batching: requests longest first (key: -len(ctx + cont), then the tokens), each
    input (ctx + cont)[-(max_length + 1):][:-1], right-padded to the batch's longest.  Yields (input_ids int64 [b, L], targets int64
    [b * L] -- the continuation's tokens at its rows, ignore_index elsewhere --, spans int64 [b, 2] -- the continuation's rows of
    request j in the flattened [b * L, V] logits --, request_indices), all on the CPU."""
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


@torch.no_grad()
def loglikelihood(model: nn.Module, requests, batch_size: int = 1, max_length: int | None = None, vocab_limit: int | None = None,
                  pad_token_id: int = 0) -> list:
    """[(log p(continuation | context), the continuation is the greedy decoding)] for requests = [(context_ids, continuation_ids)],
    in request order, with the semantics of lm-eval 0.3's BaseLM._loglikelihood_tokens (see _batches; no attention mask is passed:
    the padding sits after every real token of a causal model).  Per batch: one forward, one scoring call with one span per request,
    one device-to-host read."""
    if max_length is None:
        max_length = int(model.config.max_position_embeddings)
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
