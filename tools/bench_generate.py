#!/usr/bin/env python3
"""Greedy decode over a KV cache at context 128 / 1024 / 4096 on a llama-7b-shaped HF model (4096 / 11008 / 32 heads, distinct
packed weights per layer as in bench_decode_prologues.py, fuse_decode_(epilogues=True)), three cases alternated in one process:
  hf       HF's DynamicCache, eager (what model.generate runs per token)
  static   harness.DecodeSession with decoding.DECODE_ATTENTION = False: HF's StaticLayer.update and SDPA over all max_len rows
           behind the mask, the step replayed from a hipGraph
  kernels  harness.DecodeSession: rope_append_f16 + decode_attention_f16 in the folded layers, the same graph replay
Per case and context: us per token (median over reps of `iters` tokens from the same context: the session's positions / the
DynamicCache are cut back to it before each rep), kernels per token (torch.profiler, one eager step outside the timed window) and
the K / V bytes the attention must read per token.  The logits of the first step are compared with the hf case.
  python tools/bench_generate.py [--layers 6] [--contexts 128,1024,4096] [--reps 5] [--iters 32] [--only kernels]
(--only: one case, e.g. for a rocprofv3 --kernel-trace --stats run)"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from transformers import DynamicCache, LlamaConfig, LlamaForCausalLM  # noqa: E402

from pb_llm_amd import decoding, harness as H, ptq  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--contexts", default="128,1024,4096")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--iters", type=int, default=32)
ap.add_argument("--only", choices=["hf", "static", "kernels"], default=None)
args = ap.parse_args()
contexts = [int(c) for c in args.contexts.split(",")]
cases = [args.only] if args.only else ["hf", "static", "kernels"]

t_setup = time.time()
cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=args.layers, num_attention_heads=32,
                  num_key_value_heads=32, vocab_size=1024, max_position_embeddings=max(contexts) + 256)
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
ids = torch.randint(0, cfg.vocab_size, (1, max(contexts) + args.iters + 8), device="cuda")
setup_s = time.time() - t_setup


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


class HFCase:
    def __init__(self, C):
        self.C, self.cache = C, DynamicCache(config=cfg)
        model(ids[:, :C], past_key_values=self.cache, use_cache=True, logits_to_keep=1)
        self.first = self.step(C).float().clone()             # the logits of the first decode step, as the sessions' `first`
        self.rewind()

    def rewind(self):
        extra = self.cache.get_seq_length() - self.C
        if extra > 0:
            self.cache.crop(-extra)                          # back to the context: drop the newest `extra` rows

    def step(self, t):
        return model(ids[:, t:t + 1], past_key_values=self.cache, use_cache=True, logits_to_keep=1).logits[:, -1]


class SessionCase:
    def __init__(self, C, kernels, graph=True):
        decoding.DECODE_ATTENTION = kernels
        try:
            self.C, self.sess = C, H.DecodeSession(model, 1, C + args.iters + 4, graph=graph)
            self.sess.prefill(ids[:, :C])
            self.step(C)                                   # the capture (with DECODE_ATTENTION as this case wants it)
            self.rewind()
            self.first = self.step(C).float().clone()
            self.rewind()
        finally:
            decoding.DECODE_ATTENTION = True

    def rewind(self):
        for lay in self.sess.cache.layers:
            lay.cumulative_length.fill_(self.C)
        self.sess.pos = self.C

    def step(self, t):
        return self.sess.step(ids[:, t])


def make(case, C):
    return HFCase(C) if case == "hf" else SessionCase(C, case == "kernels")


out = dict(model=f"llama-7b shape (4096 / 11008 / 32 heads), {args.layers} decoder layers, distinct packed weights, "
                 f"fuse_decode_(epilogues=True), batch 1, greedy decode", layers_epilogues=nepi, reps=args.reps, iters=args.iters)
with torch.no_grad():
    for C in contexts:
        runs = {k: make(k, C) for k in cases}
        for k, r in runs.items():                          # kernels per token: one eager step (the graph replays the same launches)
            if k == "hf":
                r.rewind()
                out[f"{k}_kernels_per_token"] = count_kernels(lambda: r.step(C))
            elif f"{k}_kernels_per_token" not in out:
                e = SessionCase(min(contexts), k == "kernels", graph=False)
                e.rewind()
                decoding.DECODE_ATTENTION = k == "kernels"            # (an eager step reads the switch when it runs)
                try:
                    out[f"{k}_kernels_per_token"] = count_kernels(lambda: e.step(min(contexts)))
                finally:
                    decoding.DECODE_ATTENTION = True
                del e
        times = {k: [] for k in runs}
        for k, r in runs.items():                          # warm-up
            r.rewind()
            for t in range(4):
                r.step(C + t)
        torch.cuda.synchronize()
        for rep in range(args.reps):                       # hf / static / kernels / hf / ...
            for k, r in runs.items():
                r.rewind()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for t in range(args.iters):
                    r.step(C + t)
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        for k in runs:
            v = sorted(times[k])
            out[f"{k}_ctx{C}_us_per_token"] = round(v[len(v) // 2], 1)
            out[f"{k}_ctx{C}_spread_pct"] = round(100 * (v[-1] - v[0]) / v[len(v) // 2], 2)
            if "hf" in runs and k != "hf":
                out[f"{k}_ctx{C}_first_logits_max_abs_diff_vs_hf"] = float((runs[k].first - runs["hf"].first).abs().max())
        # what the decode attention must read per token: K and V rows [0, C] of every layer (2 * Hkv * D * 2 B * (C + 1) * layers)
        out[f"ctx{C}_kv_bytes_per_token"] = 2 * 32 * 128 * 2 * (C + 1) * args.layers
        del runs
        torch.cuda.empty_cache()
out["setup_s"] = round(setup_s, 1)
print(json.dumps(out))
