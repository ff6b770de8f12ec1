#!/usr/bin/env python3
"""Token selection on the device (pbl_select_token_f16) against what it replaces, and harness.generate end to end.  One JSON line.

(a) selection alone: V in {32000, 128256} x B in {1, 4} x {greedy; T 0.7, k 50, p 0.9; k 0, p 0.9}.  us per call of the kernel
    (runtime.select_token_f16) and of the torch composition it replaces (argmax for greedy; HF's TemperatureLogitsWarper,
    TopKLogitsWarper, TopPLogitsWarper, softmax and multinomial on fp32 scores otherwise), each as `--calls` calls inside ONE graph
    replay, the two alternated over `--reps` repetitions in this process: median and spread ((max - min) / median) per cell.
(b) end to end: the model of tools/bench_generate.py (llama-7b-shaped layers, distinct packed weights, fuse_decode_(epilogues=True))
    with a 32000-word vocabulary, batch 1, a 128-token prompt, 256 new tokens, eos_token_id set to an id the run does not produce
    (checked: the result has full length), so the finished-count poll is timed but no row stops early.  us per token (host clock
    around the call, synchronised) of harness.generate greedy and with T 0.7 / k 50 / p 0.9, of model.generate(do_sample=True, same
    arguments) -- HF's path -- and, with --tree PATH (an export of the parent commit, built), of the same greedy call on that tree.
    Every figure comes from fresh child processes, the trees alternated (new, parent, new, parent, ...), `--reps` children per tree;
    a child runs each case once to warm up and takes the median of three timed calls.
  python tools/bench_sampling.py [--tree PATH] [--reps 5] [--calls 200] [--layers 6] [--skip-select] [--skip-e2e]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=None, help="a built export of the parent commit: its greedy generate is timed beside this tree's")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--prompt", type=int, default=128)
ap.add_argument("--new", type=int, default=256)
ap.add_argument("--skip-select", action="store_true")
ap.add_argument("--skip-e2e", action="store_true")
ap.add_argument("--child", default=None, help="(internal) comma-separated cases to time in this process: greedy,sample,hf_sample")
ap.add_argument("--repo", default=os.path.dirname(HERE), help="(internal) the tree a child imports pb_llm_amd from")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.repo))
SAMPLING = dict(temperature=0.7, top_k=50, top_p=0.9)


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
    runs = {"greedy": lambda **kw: H.generate(model, ids, max_new_tokens=args.new, **kw),
            "sample": lambda **kw: H.generate(model, ids, max_new_tokens=args.new, do_sample=True, **SAMPLING, **kw),
            "hf_sample": lambda **kw: model.generate(ids, max_new_tokens=args.new, do_sample=True, **SAMPLING, **kw)}
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
            assert case == "hf_sample" or bool((got == first).all()), f"{case}: the tokens changed between two runs of one seed"
        out[case] = sorted(times)[1]
    print("CHILD " + json.dumps(out), flush=True)


def run_child(repo, cases):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", cases, "--repo", repo, "--layers", str(args.layers),
           "--prompt", str(args.prompt), "--new", str(args.new)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("CHILD ")]
    if res.returncode != 0 or not lines:
        raise RuntimeError(f"child {cases} on {repo} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    print(f"[bench_sampling] {os.path.relpath(repo)} {cases}: {lines[-1][6:]}", file=sys.stderr, flush=True)
    return json.loads(lines[-1][6:])


def end_to_end(out):
    new_tree = os.path.abspath(args.repo)
    series = {"greedy": [], "sample": [], "hf_sample": [], "parent_greedy": []}
    for _ in range(args.reps):                             # new, parent, new, parent, ...
        r = run_child(new_tree, "greedy,sample,hf_sample")
        for k, v in r.items():
            series[k].append(v)
        if args.tree:
            series["parent_greedy"].append(run_child(os.path.abspath(args.tree), "greedy")["greedy"])
    e2e = dict(model=f"llama-7b shape (4096 / 11008 / 32 heads), {args.layers} decoder layers, distinct packed weights, "
                     f"fuse_decode_(epilogues=True), vocabulary 32000, batch 1", prompt=args.prompt, new_tokens=args.new,
               children_per_tree=args.reps, timed_calls_per_child=3)
    names = {"greedy": "generate_greedy", "sample": "generate_sample_T0.7_k50_p0.9", "hf_sample": "hf_model_generate_sample_T0.7_k50_p0.9",
             "parent_greedy": "parent_commit_generate_greedy"}
    for k, v in series.items():
        if v:
            e2e[names[k] + "_us_per_token"], e2e[names[k] + "_spread"] = stats(v)
    if series["parent_greedy"]:
        spread = max(e2e["generate_greedy_spread"], e2e["parent_commit_generate_greedy_spread"])
        e2e["greedy_bound_us_per_token"] = round(e2e["parent_commit_generate_greedy_us_per_token"] * (1 + spread), 2)
        e2e["greedy_within_bound"] = e2e["generate_greedy_us_per_token"] <= e2e["greedy_bound_us_per_token"]
    out["end_to_end"] = e2e


# ---------------------------------------------------------------- (a) selection alone
def selection(out):
    import torch
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    from pb_llm_amd import runtime as R
    dev = "cuda"
    cells = []
    for V in (32000, 128256):
        for B in (1, 4):
            for name, T, k, p in (("greedy", 1.0, 0, 1.0), ("T0.7_k50_p0.9", 0.7, 50, 0.9), ("k0_p0.9", 1.0, 0, 0.9)):
                g = torch.Generator(dev).manual_seed(V + B)
                logits = (torch.randn(B, V, device=dev, generator=g) * 3).half()
                u = None if name == "greedy" else torch.rand(args.calls, B, device=dev, generator=g)
                st = dict(step=torch.zeros(1, dtype=torch.long, device=dev), unfinished=torch.ones(B, dtype=torch.bool, device=dev),
                          tokens=torch.zeros(B, args.calls, dtype=torch.long, device=dev), next_ids=torch.zeros(B, 1, dtype=torch.long, device=dev),
                          count=torch.zeros(1, dtype=torch.int32, device=dev), status=torch.zeros(1, dtype=torch.int32, device=dev))
                warpers = ([TemperatureLogitsWarper(T)] if T != 1.0 else []) + ([TopKLogitsWarper(k)] if k else []) \
                    + ([TopPLogitsWarper(p)] if p < 1.0 else [])
                sink = torch.zeros(B, dtype=torch.long, device=dev)

                def kernel_calls():
                    st["step"].zero_()
                    for _ in range(args.calls):
                        R.select_token_f16(logits, st["step"], st["unfinished"], st["tokens"], 0, st["next_ids"], st["count"], st["status"],
                                           temperature=T, top_k=k, top_p=p, uniforms=u)

                def torch_calls():
                    for _ in range(args.calls):
                        if u is None:
                            sink.copy_(torch.argmax(logits, -1))
                            continue
                        scores = logits.float()
                        for w in warpers:
                            scores = w(None, scores)
                        sink.copy_(torch.multinomial(torch.softmax(scores, -1), 1).squeeze(1))

                graphs = {}
                for label, fn in (("kernel", kernel_calls), ("torch", torch_calls)):
                    s = torch.cuda.Stream()
                    s.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(s), torch.no_grad():
                        fn()
                    torch.cuda.current_stream().wait_stream(s)
                    torch.cuda.synchronize()
                    gr = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gr), torch.no_grad():
                        fn()
                    gr.replay()
                    torch.cuda.synchronize()
                    graphs[label] = gr
                assert int(st["status"]) == 0
                times = {"kernel": [], "torch": []}
                for _ in range(args.reps):                 # kernel, torch, kernel, torch, ...
                    for label, gr in graphs.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        gr.replay()
                        e1.record()
                        torch.cuda.synchronize()
                        times[label].append(e0.elapsed_time(e1) * 1e3 / args.calls)
                km, ks = stats(times["kernel"])
                tm, ts = stats(times["torch"])
                cells.append(dict(V=V, B=B, mode=name, kernel_us=km, kernel_spread=ks, torch_us=tm, torch_spread=ts,
                                  kernel_at_most_torch=km <= tm))
                print(f"[bench_sampling] {cells[-1]}", file=sys.stderr, flush=True)
                del graphs
    out["selection"] = dict(calls_per_replay=args.calls, reps=args.reps, cells=cells,
                            every_cell_kernel_at_most_torch=all(c["kernel_at_most_torch"] for c in cells))


if __name__ == "__main__":
    if args.child:
        child()
    else:
        result = {}
        if not args.skip_select:
            selection(result)
        if not args.skip_e2e:
            end_to_end(result)
        print(json.dumps(result))
