#!/usr/bin/env python3
"""Prefill over a static KV cache at prompt length 128 / 1024 / 4096 on the llama-7b-shaped HF model of bench_generate.py (4096 /
11008 / 32 heads, 6 layers, distinct packed weights, fuse_decode_(epilogues=True)), batch 1, max_length = P + 256, one process:
  off        DecodeSession.prefill with decoding.PREFILL_ATTENTION = False: StaticLayer.update and HF's attention interface over all
             max_length rows behind the [1, 1, P, max_length] mask (the path without the switch: the baseline)
  on         the same with decoding.PREFILL_ATTENTION = True: runtime.prefill_attention_f16 in the folded layers
  attention  the attention call alone (append + attention + position advance, 32 heads, D = 128) against
             F.scaled_dot_product_attention(is_causal=True) on a contiguous prefix of exactly P keys -- the library's best case, which
             the static-cache path does not get
Per case and length: us (median over reps; the two prefill cases alternate, the session reset before each call).  The prefill logits
of on and off are compared, and at P = 128 the logits of the prefill and 8 forced decode steps: max |on - off| and d_ref, the max
difference between HF's sdpa and eager attention on the off path.
  python tools/bench_prefill_attention.py [--layers 6] [--prompts 128,1024,4096] [--reps 7] [--out profiles/r13_prefill_attention.json]"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from transformers import LlamaConfig, LlamaForCausalLM  # noqa: E402

from pb_llm_amd import decoding, harness as H, ptq, runtime  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--prompts", default="128,1024,4096")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r13_prefill_attention.json"))
args = ap.parse_args()
prompts = [int(c) for c in args.prompts.split(",")]
SLACK = 256

t_setup = time.time()
cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=args.layers, num_attention_heads=32,
                  num_key_value_heads=32, vocab_size=1024, max_position_embeddings=max(prompts) + SLACK)
torch.manual_seed(0)
with torch.device("cuda"):
    model = LlamaForCausalLM(cfg).half().eval()
with torch.no_grad():
    for n, p in model.named_parameters():
        if "norm" in n:
            p.copy_(1 + 0.1 * torch.randn_like(p.float()))
for layer in model.model.layers:                      # distinct packed weights per layer (RTN + magnitude, 5 % salients)
    for name, lin in H.find_layers(layer).items():
        q = ptq.LowHighGPTQ(lin, "magnitude", -1, 8, disable_gptq=True)
        q.add_batch(torch.zeros(1, 8, lin.in_features, device="cuda"))
        q.H += torch.eye(lin.in_features, device="cuda")
        q.fasterquant(0.95)
        pb = q.to_pb().to("cuda")
        q.free()
        parent = layer
        *path, leaf = name.split(".")
        for p_ in path:
            parent = getattr(parent, p_)
        setattr(parent, leaf, pb)
torch.cuda.empty_cache()
H.fuse_decode_(model, epilogues=True)
nepi = sum("forward" in vars(m) for m in model.model.layers)
ids = torch.randint(0, cfg.vocab_size, (1, max(prompts) + 16), device="cuda")
setup_s = time.time() - t_setup


def timed(fn, before=None):
    if before is not None:
        before()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def median(v):
    v = sorted(v)
    return round(v[len(v) // 2], 1), round(100 * (v[-1] - v[0]) / v[len(v) // 2], 2)


def prefill_kernels(sess, P):
    from torch.profiler import ProfilerActivity, profile
    sess.reset()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        sess.prefill(ids[:, :P])
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(ev), sum("pbl_prefill_attn_kernel" in e.name for e in ev)


def forced_logits(switch, P, steps=8, impl=None):
    """logits of the prefill of ids[:, :P] and of `steps` decode steps fed ids[:, P:P + steps]: [1, 1 + steps, V]"""
    was = model.config._attn_implementation
    decoding.PREFILL_ATTENTION = switch
    if impl is not None:
        model.config._attn_implementation = impl
    try:
        sess = H.DecodeSession(model, 1, P + SLACK, graph=False)
        lg = [sess.prefill(ids[:, :P]).float().clone()]
        for t in range(P, P + steps):
            lg.append(sess.step(ids[:, t]).float().clone())
    finally:
        decoding.PREFILL_ATTENTION = False
        model.config._attn_implementation = was
    return torch.stack(lg, 1)


out = dict(model=f"llama-7b shape (4096 / 11008 / 32 heads), {args.layers} decoder layers, distinct packed weights, "
                 f"fuse_decode_(epilogues=True), batch 1, DecodeSession.prefill, max_length = P + {SLACK}", layers_epilogues=nepi,
           reps=args.reps)
with torch.no_grad():
    for P in prompts:
        sess = H.DecodeSession(model, 1, P + SLACK, graph=False)
        cases = {"off": False, "on": True}
        logits, times = {}, {k: [] for k in cases}

        def run(k):
            decoding.PREFILL_ATTENTION = cases[k]
            try:
                return sess.prefill(ids[:, :P])
            finally:
                decoding.PREFILL_ATTENTION = False

        for k in cases:                                        # warm-up (GEMM images, workspaces), kernel counts, logits
            for _ in range(2):
                sess.reset()
                logits[k] = run(k).float().clone()
            decoding.PREFILL_ATTENTION = cases[k]
            try:
                out[f"{k}_P{P}_kernels"], out[f"{k}_P{P}_prefill_attn_launches"] = prefill_kernels(sess, P)
            finally:
                decoding.PREFILL_ATTENTION = False
        for rep in range(args.reps):                           # off / on / off / ...
            for k in cases:
                times[k].append(timed(lambda: run(k), before=sess.reset))
        for k in cases:
            out[f"{k}_P{P}_us"], out[f"{k}_P{P}_spread_pct"] = median(times[k])
        out[f"P{P}_on_over_off"] = round(out[f"on_P{P}_us"] / out[f"off_P{P}_us"], 3)
        out[f"P{P}_prefill_logits_max_abs_diff_on_vs_off"] = float((logits["on"] - logits["off"]).abs().max())
        out[f"P{P}_prefill_logits_max_abs"] = float(logits["off"].abs().max())
        del sess
        torch.cuda.empty_cache()

        # the attention call alone: one layer's shapes, the cache sized as the session's
        Hq, D, L = 32, 128, P + SLACK
        g = torch.Generator(device="cuda").manual_seed(P)
        q = torch.randn(1, Hq, P, D, generator=g, device="cuda").half()
        k_new = torch.randn(1, Hq, P, D, generator=g, device="cuda").half()
        v_new = torch.randn(1, Hq, P, D, generator=g, device="cuda").half()
        kc, vc = torch.zeros(1, Hq, L, D, dtype=torch.float16, device="cuda"), torch.zeros(1, Hq, L, D, dtype=torch.float16, device="cuda")
        pos = torch.zeros((), dtype=torch.int64, device="cuda")
        calls = {"kernel": lambda: runtime.prefill_attention_f16(q, k_new, v_new, kc, vc, pos, D ** -0.5),
                 "sdpa": lambda: F.scaled_dot_product_attention(q, k_new, v_new, is_causal=True, scale=D ** -0.5)}
        at = {k: [] for k in calls}
        for k, fn in calls.items():
            for _ in range(3):
                pos.zero_()
                fn()
        for rep in range(args.reps):
            for k, fn in calls.items():
                at[k].append(timed(fn, before=pos.zero_))
        for k in calls:
            out[f"attention_{k}_P{P}_us"], out[f"attention_{k}_P{P}_spread_pct"] = median(at[k])
        pos.zero_()
        a = calls["kernel"]().view(1, P, Hq, D).transpose(1, 2).float()
        out[f"attention_P{P}_max_abs_diff_vs_sdpa"] = float((a - calls["sdpa"]().float()).abs().max())
        out[f"attention_P{P}_causal_tflops_kernel"] = round(2 * 2 * Hq * D * (P * (P + 1) / 2) / out[f"attention_kernel_P{P}_us"] / 1e6, 1)
        del q, k_new, v_new, kc, vc
        torch.cuda.empty_cache()

    # the yardstick of tests/test_gpu_prefill_attention.py on this model: on vs off against HF's sdpa vs eager (off path), P = 128
    P = min(prompts)
    on, off = forced_logits(True, P), forced_logits(False, P)
    sdpa, eager = forced_logits(False, P, impl="sdpa"), forced_logits(False, P, impl="eager")
    out[f"P{P}_forced_logits_max_abs_diff_on_vs_off"] = float((on - off).abs().max())
    out[f"P{P}_forced_logits_d_ref_sdpa_vs_eager"] = float((sdpa - eager).abs().max())
out["setup_s"] = round(setup_s, 1)
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(line + "\n")
