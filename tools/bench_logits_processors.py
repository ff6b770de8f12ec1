#!/usr/bin/env python3
"""The logits processors on the device (pbl_process_logits_f16, min_p in pbl_select_token_minp_f16) against what they replace, and
harness.generate end to end.  One JSON line; --out writes it to a file as well (profiles/r15_logits_processors.json).

(a) processing alone: V in {32000, 128256} x history in {128, 1024, 4096}, batch 1, repetition_penalty 1.1, no_repeat_ngram_size 3 and
    a min_new_tokens that blocks two eos ids.  us per call of the kernel (runtime.process_logits_f16, in place on the fp16 logits) and
    of HF's RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor on an fp32 device
    copy of the same logits (the copy included: model.generate makes it every step).  HF's chain runs EAGERLY, as model.generate runs
    it: `--calls` calls in a host loop between two events, so its figure holds the host's launch cost of about a dozen torch ops per
    call -- that is part of what HF pays.  The kernel is timed the same way (kernel_eager) and as `--calls` calls inside ONE graph
    replay (kernel_replay: what a replayed decode unit pays).  The three are alternated over `--reps` repetitions in this process:
    median and spread ((max - min) / median) per cell; kernel_at_most_hf compares the two eager figures.
(b) end to end: the model of tools/bench_sampling.py (llama-7b-shaped layers, distinct packed weights, fuse_decode_(epilogues=True),
    vocabulary 32000), batch 1, a 128-token prompt, 256 new tokens, eos_token_id set to an id the run does not produce.  us per token
    (host clock around the call, synchronised) of harness.generate greedy and sampled (T 0.7 / k 50 / p 0.9) with every processor
    off, of the sampled call with repetition_penalty 1.1 / no_repeat_ngram_size 3 / min_p 0.05, of model.generate with those
    arguments -- HF's path, where such a call went before -- and, with --tree PATH (an export of the parent commit, built), of the
    two calls without processors on that tree.  Every figure comes from fresh child processes, the trees alternated (new, parent,
    new, parent, ...), `--reps` children per tree; a child runs each case once to warm up and takes the median of three timed calls.
  python tools/bench_logits_processors.py [--tree PATH] [--reps 5] [--calls 200] [--layers 6] [--skip-kernel] [--skip-e2e] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=None, help="a built export of the parent commit: its generate without processors is timed beside this tree's")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--prompt", type=int, default=128)
ap.add_argument("--new", type=int, default=256)
ap.add_argument("--skip-kernel", action="store_true")
ap.add_argument("--skip-e2e", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help="(internal) comma-separated cases to time in this process")
ap.add_argument("--repo", default=os.path.dirname(HERE), help="(internal) the tree a child imports pb_llm_amd from")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.repo))
SAMPLING = dict(temperature=0.7, top_k=50, top_p=0.9)
PROCESSORS = dict(repetition_penalty=1.1, no_repeat_ngram_size=3, min_p=0.05)


def stats(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return round(med, 2), round((v[-1] - v[0]) / med, 4)


# ---------------------------------------------------------------- (b) one child: build the model, time the cases
def child():
    import torch
    from transformers import LlamaConfig, LlamaForCausalLM
    from pb_llm_amd import harness as H, ptq
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=args.layers, num_attention_heads=32,
                      num_key_value_heads=32, vocab_size=32000, max_position_embeddings=args.prompt + args.new + 8)
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
    model.generation_config.eos_token_id = None
    model.generation_config.pad_token_id = 0
    ids = torch.randint(0, cfg.vocab_size, (1, args.prompt), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    total = args.prompt + args.new
    handed = []
    hf_generate = model.generate
    model.generate = lambda *a, **k: (handed.append(1), hf_generate(*a, **k))[1]
    runs = {"greedy": lambda **kw: H.generate(model, ids, max_new_tokens=args.new, **kw),
            "sample": lambda **kw: H.generate(model, ids, max_new_tokens=args.new, do_sample=True, **SAMPLING, **kw),
            "sample_proc": lambda **kw: H.generate(model, ids, max_new_tokens=args.new, do_sample=True, **SAMPLING, **PROCESSORS, **kw),
            "hf_sample_proc": lambda **kw: hf_generate(ids, max_new_tokens=args.new, do_sample=True, **SAMPLING, **PROCESSORS, **kw)}
    out = {}
    for case in args.child.split(","):
        torch.manual_seed(7)
        first = runs[case]()                                # warm-up, and the tokens this seed produces
        assert first.shape == (1, total), first.shape
        eos = next(t for t in range(cfg.vocab_size) if t not in set(first[0, args.prompt:].tolist()))
        times = []
        for _ in range(3):
            torch.manual_seed(7)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = runs[case](eos_token_id=eos)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e6 / args.new)
            assert got.shape == (1, total), f"{case}: a row stopped early ({tuple(got.shape)})"
            assert case.startswith("hf_") or bool((got == first).all()), f"{case}: the tokens changed between two runs of one seed"
        out[case] = sorted(times)[1]
    assert not handed, "a harness.generate case was handed to model.generate"
    print("CHILD " + json.dumps(out), flush=True)


def run_child(repo, cases):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", cases, "--repo", repo, "--layers", str(args.layers),
           "--prompt", str(args.prompt), "--new", str(args.new)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("CHILD ")]
    if res.returncode != 0 or not lines:
        raise RuntimeError(f"child {cases} on {repo} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    print(f"[bench_logits_processors] {os.path.relpath(repo)} {cases}: {lines[-1][6:]}", file=sys.stderr, flush=True)
    return json.loads(lines[-1][6:])


def end_to_end(out):
    new_tree = os.path.abspath(args.repo)
    series = {"greedy": [], "sample": [], "sample_proc": [], "hf_sample_proc": [], "parent_greedy": [], "parent_sample": []}
    for _ in range(args.reps):                             # new, parent, new, parent, ...
        for k, v in run_child(new_tree, "greedy,sample,sample_proc,hf_sample_proc").items():
            series[k].append(v)
        if args.tree:
            for k, v in run_child(os.path.abspath(args.tree), "greedy,sample").items():
                series["parent_" + k].append(v)
    tag = "T0.7_k50_p0.9"
    proc = "penalty1.1_ngram3_minp0.05"
    e2e = dict(model=f"llama-7b shape (4096 / 11008 / 32 heads), {args.layers} decoder layers, distinct packed weights, "
                     f"fuse_decode_(epilogues=True), vocabulary 32000, batch 1", prompt=args.prompt, new_tokens=args.new,
               children_per_tree=args.reps, timed_calls_per_child=3)
    names = {"greedy": "generate_greedy_processors_off", "sample": f"generate_sample_{tag}_processors_off",
             "sample_proc": f"generate_sample_{tag}_{proc}", "hf_sample_proc": f"hf_model_generate_sample_{tag}_{proc}",
             "parent_greedy": "parent_commit_generate_greedy", "parent_sample": f"parent_commit_generate_sample_{tag}"}
    for k, v in series.items():
        if v:
            e2e[names[k] + "_us_per_token"], e2e[names[k] + "_spread"] = stats(v)
    e2e["processors_cost_us_per_token"] = round(e2e[names["sample_proc"] + "_us_per_token"] - e2e[names["sample"] + "_us_per_token"], 2)
    for k in ("greedy", "sample"):
        if series["parent_" + k]:
            spread = max(e2e[names[k] + "_spread"], e2e[names["parent_" + k] + "_spread"])
            bound = round(e2e[names["parent_" + k] + "_us_per_token"] * (1 + spread), 2)
            e2e[f"{k}_off_bound_us_per_token"], e2e[f"{k}_off_within_bound"] = bound, e2e[names[k] + "_us_per_token"] <= bound
    out["end_to_end"] = e2e


# ---------------------------------------------------------------- (a) processing alone
def processing(out):
    import torch
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)
    from pb_llm_amd import runtime as R
    dev = "cuda"
    theta, ngram = 1.1, 3
    cells = []
    for V in (32000, 128256):
        for hist in (128, 1024, 4096):
            g = torch.Generator(dev).manual_seed(V + hist)
            logits = (torch.randn(1, V, device=dev, generator=g) * 3).half()
            tokens = torch.randint(0, V, (1, hist + 8), device=dev, generator=g)
            tokens[0, hist - 2:hist] = tokens[0, 10:12]        # one banned 3-gram
            history = tokens[:, :hist].clone()
            step = torch.tensor([hist - 16], dtype=torch.long, device=dev)
            eos = torch.tensor([1, 2], dtype=torch.long, device=dev)
            scratch = torch.empty(1, hist + 8, dtype=torch.float16, device=dev)
            hf = [RepetitionPenaltyLogitsProcessor(theta), NoRepeatNGramLogitsProcessor(ngram),
                  MinNewTokensLengthLogitsProcessor(16, hist, eos, device=dev)]
            sink = torch.zeros(1, V, dtype=torch.float32, device=dev)

            def kernel_calls():                                # in place, call after call: the values drift, the work does not
                for _ in range(args.calls):
                    R.process_logits_f16(logits, tokens, 16, step, repetition_penalty=theta, no_repeat_ngram_size=ngram,
                                         min_new_tokens=hist, eos=eos, scratch=scratch)

            def hf_calls():
                for _ in range(args.calls):
                    scores = logits.float()
                    for proc in hf:
                        scores = proc(history, scores)
                    sink.copy_(scores)

            s_ = torch.cuda.Stream()                       # the kernel's calls captured once: what a replayed decode unit pays
            s_.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s_), torch.no_grad():
                kernel_calls()
            torch.cuda.current_stream().wait_stream(s_)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr), torch.no_grad():
                kernel_calls()
            gr.replay()
            with torch.no_grad():
                hf_calls()                                     # warm-up of the eager chain
            torch.cuda.synchronize()
            runs = {"kernel_replay": gr.replay, "kernel_eager": kernel_calls, "hf_eager": hf_calls}
            times = {k: [] for k in runs}
            for _ in range(args.reps):                     # replay, kernel eager, hf eager, replay, ...
                for label, fn in runs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    with torch.no_grad():
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[label].append(e0.elapsed_time(e1) * 1e3 / args.calls)
            cell = dict(V=V, history=hist)
            for label in runs:
                cell[label + "_us"], cell[label + "_spread"] = stats(times[label])
            cell["kernel_at_most_hf"] = cell["kernel_eager_us"] <= cell["hf_eager_us"]
            cells.append(cell)
            print(f"[bench_logits_processors] {cells[-1]}", file=sys.stderr, flush=True)
            del gr
    out["processing"] = dict(calls_per_replay=args.calls, reps=args.reps, repetition_penalty=theta, no_repeat_ngram_size=ngram,
                             eos_ids_blocked=2, cells=cells, every_cell_kernel_at_most_hf=all(c["kernel_at_most_hf"] for c in cells))


if __name__ == "__main__":
    if args.child:
        child()
    else:
        result = {}
        if not args.skip_kernel:
            processing(result)
        if not args.skip_e2e:
            end_to_end(result)
        line = json.dumps(result)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        print(line)
