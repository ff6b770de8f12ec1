#!/usr/bin/env python3
"""Decode prologues (harness.fuse_decode_(prologues=True), mode "folded") and epilogues (fuse_decode_(epilogues=True), mode
"epilogues") against fuse_decode_ alone (mode "plain") on a llama-7b-shaped HF model (4096 / 11008 / 32 heads), one token per
forward, each mode captured in a hipGraph (GraphedForward) and replayed A/B/C/A/B/C in one process.
Every decoder layer holds its OWN packed weights (~65 MB at 5 % salients): with 6 layers the weights exceed the 256 MiB Infinity Cache
and a replay streams them from HBM.  The vocabulary is small (the head is a dense linear outside the comparison), so us per decoder
layer = us per token / layers.  Kernels per token are counted with torch.profiler in a pass of their own, outside the timed window.
  python tools/bench_decode_prologues.py [--layers 6] [--reps 7] [--iters 200] [--only folded]   (--only: rocprofv3 runs)
The epilogues mode's logits are compared with the folded mode's (they must be equal: epilogues_logits_max_abs_diff)."""
import argparse
import copy
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from transformers import LlamaConfig, LlamaForCausalLM  # noqa: E402

from pb_llm_amd import harness as H, ptq  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--only", choices=["plain", "folded", "epilogues"], default=None)
args = ap.parse_args()

t_setup = time.time()
cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=args.layers, num_attention_heads=32,
                  num_key_value_heads=32, vocab_size=1024, max_position_embeddings=256)
torch.manual_seed(0)
with torch.device("cuda"):
    model = LlamaForCausalLM(cfg).half().eval()
with torch.no_grad():
    for n, p in model.named_parameters():
        if "norm" in n:
            p.copy_(1 + 0.1 * torch.randn_like(p.float()))
packed_bytes = 0
for layer in model.model.layers:                      # distinct packed weights per layer (RTN + magnitude, 5 % salients)
    for name, lin in H.find_layers(layer).items():
        q = ptq.LowHighGPTQ(lin, "magnitude", -1, 8, disable_gptq=True)
        q.add_batch(torch.zeros(1, 8, lin.in_features, device="cuda"))
        q.H += torch.eye(lin.in_features, device="cuda")
        q.fasterquant(0.95)
        pb = q.to_pb().to("cuda")
        q.free()
        packed_bytes += pb.packed.nbytes
        parent = layer
        *path, leaf = name.split(".")
        for p_ in path:
            parent = getattr(parent, p_)
        setattr(parent, leaf, pb)
torch.cuda.empty_cache()
plain = model
folded = copy.deepcopy(model)
epilogues = copy.deepcopy(model)
H.fuse_decode_(plain)
H.fuse_decode_(folded, prologues=True)
H.fuse_decode_(epilogues, epilogues=True)
nfold = sum(isinstance(m, H._FoldedMLP) for m in folded.modules())
nepi = sum("forward" in vars(m) for m in epilogues.model.layers)
ids = torch.randint(0, cfg.vocab_size, (1, 64), device="cuda")
modes = {"plain": plain, "folded": folded, "epilogues": epilogues}
if args.only:
    modes = {args.only: modes[args.only]}


def kernels_per_token(m):
    from torch.profiler import ProfilerActivity, profile
    with torch.no_grad():
        m(ids[:, :1], use_cache=False)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            m(ids[:, :1], use_cache=False)
            torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


counts = {k: kernels_per_token(m) for k, m in modes.items()}
graphs = {k: H.GraphedForward(m, ids[:, :1]) for k, m in modes.items()}
setup_s = time.time() - t_setup

logits = {k: g.replay(ids[:, 5:6]).float().clone() for k, g in graphs.items()}
for g in graphs.values():                              # warm-up
    for i in range(20):
        g.replay(ids[:, i:i + 1])
torch.cuda.synchronize()
times = {k: [] for k in graphs}
for r in range(args.reps):                             # A / B / A / B ...
    for k, g in graphs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.iters):
            g.replay(ids[:, i % 64:i % 64 + 1])
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)   # us per token


def med(v):
    return sorted(v)[len(v) // 2]


L = args.layers
out = dict(model=f"llama-7b shape (4096 / 11008 / 32 heads), {L} decoder layers, distinct packed weights, 1 token, hipGraph replay",
           packed_MB_per_decoder_layer=round(packed_bytes / L / 1e6, 1), layers_folded=nfold, layers_epilogues=nepi, reps=args.reps, iters=args.iters,
           setup_s=round(setup_s, 1))
for k in graphs:
    out[f"{k}_us_per_layer"] = round(med(times[k]) / L, 2)
    out[f"{k}_us_per_token"] = round(med(times[k]), 1)
    out[f"{k}_spread_pct"] = round(100 * (max(times[k]) - min(times[k])) / med(times[k]), 2)
    out[f"{k}_kernels_per_token"] = counts[k]
if "folded" in graphs and "plain" in graphs:
    a, b = logits["folded"], logits["plain"]
    out["logits_rel_max_diff"] = float((a - b).abs().max() / b.abs().max())
    out["folded_speedup"] = round(med(times["plain"]) / med(times["folded"]), 3)
if "folded" in graphs and "epilogues" in graphs:
    out["epilogues_logits_max_abs_diff"] = float((logits["epilogues"] - logits["folded"]).abs().max())
    out["epilogues_logits_equal"] = bool(torch.equal(logits["epilogues"], logits["folded"]))
    out["epilogues_saving_us_per_layer"] = round((med(times["folded"]) - med(times["epilogues"])) / L, 2)
print(json.dumps(out))
