#!/usr/bin/env python3
"""Token scoring (runtime.score_tokens_f16 = pbl_score_tokens_f16) against the two torch compositions it replaces, alternated in one
process on random fp16 logits:
  kernel   one scoring call with one span over all rows (per-row log-prob + is-greedy, fp64 span sum)
  parent   the tail of harness.perplexity: logits.float() + F.cross_entropy(reduction="sum")
  lmeval   lm-eval's composition on the device: log_softmax over the fp16 logits, gather, argmax
Shapes: 2047 x 32000 and 2047 x 128256 (one 2048-token perplexity window) and 2048 x 32000 (a loglikelihood batch of 16 x 128 rows).
Every call reads the next of a ring of logits buffers that together exceed the 256 MiB last-level cache several times, so a number
is a memory number, not a cache number.  Each timing is device events around at least --min-seconds of back-to-back calls; the
median over --reps alternated rounds is reported.
  python tools/bench_scoring.py [--reps 5] [--min-seconds 0.5] [--out profiles/r11_scoring.json]
  python tools/bench_scoring.py --only kernel --shape 0 --calls 200        # under `rocprofv3 --kernel-trace --stats --output-format csv`
  python tools/bench_scoring.py --merge profiles/r11_scoring.json --stats 0=DIR0 1=DIR1 2=DIR2
(--merge needs no GPU: it reads the *kernel_stats.csv below each DIR and adds the kernel's own time per call, T * V * 2 bytes over
that time, and that figure as a fraction of 8 TB/s.)"""
import argparse
import csv
import glob
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(2047, 32000, "perplexity window, V = 32000"), (2047, 128256, "perplexity window, V = 128256"),
          (16 * 128, 32000, "loglikelihood batch of 16 x 128 rows, V = 32000")]
RING_BYTES = 1 << 30                     # logits buffers per shape: at least this many bytes, and at least 3 buffers
PEAK_BYTES_PER_S = 8e12

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=0.5)
ap.add_argument("--only", choices=["kernel", "parent", "lmeval"], default=None)
ap.add_argument("--shape", type=int, default=None)
ap.add_argument("--calls", type=int, default=0, help="with --only: this many calls, untimed (a profiler times them)")
ap.add_argument("--out", default=None)
ap.add_argument("--merge", default=None)
ap.add_argument("--stats", nargs="*", default=[])
args = ap.parse_args()


def kernel_stats(root):
    """{kernel name: average ns} of the *kernel_stats.csv files below root"""
    found = {}
    for path in glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or row.get("Kernel_Name") or ""
                calls = float(row.get("Calls") or 0)
                total = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
                if calls:
                    found[name] = (total / calls, int(calls))
    return found


if args.merge:
    with open(args.merge) as f:
        out = json.load(f)
    for item in args.stats:
        idx, root = item.split("=", 1)
        T, V, _ = SHAPES[int(idx)]
        entry = out["shapes"][int(idx)]
        for name, (ns, calls) in kernel_stats(root).items():
            if "pbl_score_tokens_kernel" in name:
                entry["rocprof_score_kernel_us"] = round(ns / 1e3, 2)
                entry["rocprof_score_kernel_calls"] = calls
                entry["logits_bytes_per_s_over_kernel_time"] = round(T * V * 2 / (ns * 1e-9), -9)
                entry["fraction_of_8TBps"] = round(T * V * 2 / (ns * 1e-9) / PEAK_BYTES_PER_S, 3)
            elif "pbl_score_spans_kernel" in name:
                entry["rocprof_spans_kernel_us"] = round(ns / 1e3, 2)
    with open(args.merge, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    sys.exit(0)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pb_llm_amd.runtime import score_tokens_f16  # noqa: E402

DEV = torch.device("cuda:0")


class Shape:
    def __init__(self, T, V):
        self.T, self.V = T, V
        n = max(3, -(-RING_BYTES // (T * V * 2)))
        g = torch.Generator(device=DEV).manual_seed(T + V)
        self.ring = []
        for _ in range(n):                                   # N(0, 3^2) logits, made in slices to keep the fp32 temporary small
            buf = torch.empty(T, V, dtype=torch.float16, device=DEV)
            for r in range(0, T, 256):
                buf[r:r + 256] = torch.randn(min(256, T - r), V, generator=g, device=DEV).mul_(3).half()
            self.ring.append(buf)
        self.targets = torch.randint(0, V, (T,), generator=g, device=DEV)
        self.span = torch.tensor([[0, T]], dtype=torch.int64, device=DEV)
        self.i = 0

    def next(self):
        self.i = (self.i + 1) % len(self.ring)
        return self.ring[self.i]

    def kernel(self):
        return score_tokens_f16(self.next(), self.targets, self.span)[2]

    def parent(self):
        return F.cross_entropy(self.next().float(), self.targets, reduction="sum")

    def lmeval(self):
        lsm = F.log_softmax(self.next(), dim=-1)
        return lsm.gather(1, self.targets[:, None]).sum(), (lsm.argmax(-1) == self.targets).all()

    def timed(self, case, calls):
        fn = getattr(self, case)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / calls             # seconds per call


cases = [args.only] if args.only else ["kernel", "parent", "lmeval"]
picked = range(len(SHAPES)) if args.shape is None else [args.shape]
out = dict(what="token scoring: pbl_score_tokens_f16 (one span over all rows) against logits.float() + F.cross_entropy (parent) and "
                "log_softmax + gather + argmax on the fp16 logits (lmeval); us per call, device events around >= min_seconds of calls, "
                "median of reps alternated rounds, logits from a ring of buffers larger than the last-level cache",
           reps=args.reps, min_seconds=args.min_seconds, shapes=[None] * len(SHAPES))
with torch.no_grad():
    for si in picked:
        T, V, what = SHAPES[si]
        s = Shape(T, V)
        if args.calls:
            for c in cases:
                for _ in range(args.calls):
                    getattr(s, c)()
            torch.cuda.synchronize()
            continue
        a, b = s.kernel(), s.parent()
        entry = dict(T=T, V=V, what=what, ring_buffers=len(s.ring), ring_bytes=len(s.ring) * T * V * 2, logits_bytes=T * V * 2,
                     kernel_vs_parent_rel_diff_of_the_sum=abs(float(a[0]) + float(b)) / abs(float(b)))
        calls = {}
        for c in cases:                                      # warm-up, and the number of calls that fills min_seconds
            s.timed(c, 3)
            calls[c] = max(5, int(args.min_seconds / s.timed(c, 5)) + 1)
        times = {c: [] for c in cases}
        for _ in range(args.reps):                           # kernel / parent / lmeval / kernel / ...
            for c in cases:
                times[c].append(s.timed(c, calls[c]))
        for c in cases:
            v = sorted(times[c])
            entry[f"{c}_us_per_call"] = round(v[len(v) // 2] * 1e6, 1)
            entry[f"{c}_spread_pct"] = round(100 * (v[-1] - v[0]) / v[len(v) // 2], 2)
            entry[f"{c}_calls_per_timing"] = calls[c]
        if "kernel" in times:
            for c in cases:
                if c != "kernel":
                    entry[f"{c}_over_kernel"] = round(entry[f"{c}_us_per_call"] / entry["kernel_us_per_call"], 2)
            entry["logits_bytes_per_s_over_call_time"] = round(T * V * 2 / (entry["kernel_us_per_call"] * 1e-6), -9)
        out["shapes"][si] = entry
        del s
        torch.cuda.empty_cache()
if not args.calls:
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))
