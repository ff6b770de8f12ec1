#!/usr/bin/env python3
"""Multiple-choice scoring with and without sharing the context, on the llama-7b-shaped HF model of bench_generate.py (4096 / 11008 /
32 heads, 6 layers, distinct packed weights, fuse_decode_(epilogues=True)), one process:
  unshared   harness.loglikelihood(share_prefix=False): every (context, continuation) request is its own sequence
  shared     harness.loglikelihood(share_prefix=True) at the SAME batch_size: one packed sequence per document, the HIP branch
             attention (runtime.branch_attention_f16) over a DecodeCache
on DOCS documents per shape:
  mmlu_512 / mmlu_1536   context 512 / 1536, four one-token continuations
  hellaswag              context 64, four continuations of 24 tokens
  boolq                  context 256, two one-token continuations
Per shape: ms per call of each (median over reps, the two alternate), shared / unshared, the rows each forwards, and the largest
per-request |shared - unshared|.
  attention  the attention call alone on one document's packed rows (32 heads, D = 128, append + attention + position advance):
             runtime.branch_attention_f16 against runtime.prefill_attention_f16 over the same rows (which computes the plain causal
             mask: the cost of the mask policy)
The keys "test_gpu_branch_attention" (the model-level figures tests/test_gpu_branch_attention.py prints) and "tile_skip_ab" (the A/B
run behind DESIGN.md's tile-skip decision) of an existing --out file are kept.
  python tools/bench_shared_prefix.py [--layers 6] [--docs 8] [--batch-size 16] [--reps 5] [--out profiles/r16_shared_prefix.json]"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from transformers import LlamaConfig, LlamaForCausalLM  # noqa: E402

from pb_llm_amd import harness as H, ptq, runtime, scoring  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--docs", type=int, default=8)
ap.add_argument("--batch-size", type=int, default=16)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r16_shared_prefix.json"))
args = ap.parse_args()
SHAPES = {"mmlu_512": (512, (1, 1, 1, 1)), "mmlu_1536": (1536, (1, 1, 1, 1)), "hellaswag": (64, (24, 24, 24, 24)), "boolq": (256, (1, 1))}
VOCAB, MAX_POS = 1024, 2048


def median(v):
    v = sorted(v)
    return v[len(v) // 2], round(100 * (v[-1] - v[0]) / v[len(v) // 2], 2)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def event_us(fn, before):
    before()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def attention_alone():
    """{shape: branch / prefill us over one document's packed rows}"""
    res = {}
    Hq, D = 32, 128
    for name, (T, conts) in SHAPES.items():
        plan = scoring.shared_prefix_plan([(list(range(T)), [0] * n) for n in conts], len(conts), MAX_POS)
        (pb,) = plan.batches
        S = len(pb.tokens[0])
        g = torch.Generator(device="cuda").manual_seed(S)
        q, k_new, v_new = (torch.randn(1, Hq, S, D, generator=g, device="cuda").half() for _ in range(3))
        kc, vc = (torch.zeros(1, Hq, S, D, dtype=torch.float16, device="cuda") for _ in range(2))
        pos = torch.zeros((), dtype=torch.int64, device="cuda")
        trunk = torch.tensor(pb.trunk, dtype=torch.int32, device="cuda")
        lo = torch.tensor(pb.lo, dtype=torch.int32, device="cuda")
        calls = {"branch": lambda: runtime.branch_attention_f16(q, k_new, v_new, kc, vc, pos, D ** -0.5, trunk, lo),
                 "prefill": lambda: runtime.prefill_attention_f16(q, k_new, v_new, kc, vc, pos, D ** -0.5)}
        times = {k: [] for k in calls}
        for fn in calls.values():
            for _ in range(3):
                pos.zero_()
                fn()
        for _ in range(max(args.reps, 9)):
            for k, fn in calls.items():
                times[k].append(event_us(fn, pos.zero_))
        res[name] = dict(rows=S)
        for k in calls:
            res[name][f"{k}_us"], res[name][f"{k}_spread_pct"] = (round(x, 2) for x in median(times[k]))
        res[name]["branch_over_prefill"] = round(res[name]["branch_us"] / res[name]["prefill_us"], 3)
    return res


t_setup = time.time()
cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=args.layers, num_attention_heads=32,
                  num_key_value_heads=32, vocab_size=VOCAB, max_position_embeddings=MAX_POS)
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
setup_s = time.time() - t_setup

out = dict(model=f"llama-7b shape (4096 / 11008 / 32 heads), {args.layers} decoder layers, distinct packed weights, "
                 f"fuse_decode_(epilogues=True), vocab {VOCAB}", docs=args.docs, batch_size=args.batch_size, reps=args.reps)
if os.path.exists(args.out):                           # figures other runs put here stay
    with open(args.out) as f:
        out = {**{k: v for k, v in json.load(f).items() if k in ("test_gpu_branch_attention", "tile_skip_ab")}, **out}
gen = torch.Generator().manual_seed(1)
for name, (T, conts) in SHAPES.items():
    reqs = []
    for _ in range(args.docs):
        ctx = torch.randint(0, VOCAB, (T,), generator=gen).tolist()
        reqs += [(ctx, torch.randint(0, VOCAB, (n,), generator=gen).tolist()) for n in conts]
    cases = {"unshared": False, "shared": True}
    calls = []
    real = runtime.branch_attention_f16
    runtime.branch_attention_f16 = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        got = {k: H.loglikelihood(model, reqs, batch_size=args.batch_size, max_length=MAX_POS, share_prefix=sw) for k, sw in cases.items()}
    finally:
        runtime.branch_attention_f16 = real
    times = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, sw in cases.items():
            times[k].append(wall_ms(lambda: H.loglikelihood(model, reqs, batch_size=args.batch_size, max_length=MAX_POS, share_prefix=sw))[0])
    plan = scoring.shared_prefix_plan(reqs, args.batch_size, MAX_POS)
    r = dict(context=T, continuations=list(conts), requests=len(reqs), branch_attention_calls=len(calls),
             rows_unshared=sum(i.numel() for i, _, _, _ in scoring._batches(reqs, args.batch_size, MAX_POS)),
             rows_shared=sum(len(b.trunk) * len(b.tokens[0]) for b in plan.batches))
    for k in cases:
        r[f"{k}_ms"], r[f"{k}_spread_pct"] = (round(x, 2) for x in median(times[k]))
    r["shared_over_unshared"] = round(r["shared_ms"] / r["unshared_ms"], 3)
    r["max_abs_diff_shared_vs_unshared"] = max(abs(a[0] - b[0]) for a, b in zip(got["shared"], got["unshared"]))
    r["greedy_flags_differ"] = sum(a[1] != b[1] for a, b in zip(got["shared"], got["unshared"]))
    out[name] = r
    print(name, json.dumps(r), flush=True)
    torch.cuda.empty_cache()
with torch.no_grad():
    out["attention"] = attention_alone()
out["setup_s"] = round(setup_s, 1)
print(json.dumps(out["attention"]))
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
