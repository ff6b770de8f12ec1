#!/usr/bin/env python3
"""Prompt-lookup speculative decoding (pbl_spec_verify_f16 / pbl_ngram_draft; DecodeSession.begin_speculation): what a step of
1 + K rows costs against the one-row step, what the control plane costs alone, and tokens/s at the two ends of acceptance.
Writes profiles/r12_speculation.json and prints it as one JSON line.  One process, one model per vocabulary: the model of
tools/bench_generate.py (llama-7b-shaped layers, distinct packed weights, fuse_decode_(epilogues=True)), batch 1.

(a) unit: per vocabulary {32000, 128256} and context {128, 1024, 4096} the replay time of the captured units -- "one-row step +
    pbl_select_token_f16" (DecodeSession.step_select, the unit of the commit before this feature, unchanged here) and "(1 + K)-row
    step + verify + draft" at K = 0, 1, 3 -- alternated over `--reps` repetitions of `--steps` replays each, median and spread
    ((max - min) / median).  ratio - 1 is the break-even acceptance: the accepted drafts per step that pay for the wider step.
(b) control plane alone: us per call, `--calls` calls per graph replay, of verify (S = 4, no drafting), verify + draft and the
    draft alone at history 128 / 4096 / 65536, for both vocabularies.
(c) tokens/s over `--new` tokens at context 128 with forced drafts (step_speculate(drafts=)) taken from the one-row run: all right
    (100 % acceptance) and all wrong (0 %), beside the one-row loop's; the accepted drafts per step are reported as counted.
  python tools/bench_speculation.py [--layers 6] [--reps 5] [--steps 32] [--calls 50] [--new 128] [--vocabs 32000,128256]
                                    [--contexts 128,1024,4096] [--out profiles/r12_speculation.json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--new", type=int, default=128)
ap.add_argument("--vocabs", default="32000,128256")
ap.add_argument("--contexts", default="128,1024,4096")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r12_speculation.json"))
args = ap.parse_args()

import torch  # noqa: E402

DEV = "cuda"


def stats(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return round(med, 2), round((v[-1] - v[0]) / med, 4)


def build_model(vocab, max_positions):
    from transformers import LlamaConfig, LlamaForCausalLM
    from pb_llm_amd import harness as H, ptq
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=args.layers, num_attention_heads=32,
                      num_key_value_heads=32, vocab_size=vocab, max_position_embeddings=max_positions)
    torch.manual_seed(0)
    with torch.device(DEV):
        model = LlamaForCausalLM(cfg).half().eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_(1 + 0.1 * torch.randn_like(p.float()))
    for layer in model.model.layers:                      # distinct packed weights per layer (RTN + magnitude, 5 % salients)
        for name, lin in H.find_layers(layer).items():
            q = ptq.LowHighGPTQ(lin, "magnitude", -1, 8, disable_gptq=True)
            q.add_batch(torch.zeros(1, 8, lin.in_features, device=DEV))
            q.H += torch.eye(lin.in_features, device=DEV)
            q.fasterquant(0.95)
            pb = q.to_pb().to(DEV)
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
    return model


def timed(graph, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


# ---------------------------------------------------------------- (a) the captured units
@torch.no_grad()
def units(model, vocab, ctx):
    from pb_llm_amd import harness as H
    ids = torch.randint(0, vocab, (1, ctx), device=DEV, generator=torch.Generator(DEV).manual_seed(ctx))
    room = (args.reps + 2) * args.steps                    # replays per unit; a speculative one advances by at most 1 + K
    graphs = {}
    sess = H.DecodeSession(model, 1, ctx + room + 2, graph=True)
    sess.begin_selection(ids, ctx + room + 2)
    sess.select(sess.prefill(ids))
    sess.step_select()
    graphs["step_select"] = (sess, sess.sel_graph)
    for K in (0, 1, 3):
        total = ctx + room * (1 + K) + 2
        s = H.DecodeSession(model, 1, total - 1 + K, graph=True)
        s.begin_speculation(ids, total, draft_tokens=K, max_ngram=2)
        s.step_speculate()
        graphs[f"K{K}"] = (s, s.spec_graph)
    for _, g in graphs.values():                           # one untimed pass each
        timed(g, args.steps)
    times = {k: [] for k in graphs}
    for _ in range(args.reps):                             # step_select, K0, K1, K3, step_select, ...
        for k, (_, g) in graphs.items():
            times[k].append(timed(g, args.steps))
    cell = dict(V=vocab, context=ctx)
    base = None
    for k, v in times.items():
        med, spread = stats(v)
        cell[k + "_us"], cell[k + "_spread"] = med, spread
        base = med if base is None else base
        if k != "step_select":
            cell[k + "_ratio"] = round(med / base, 4)
    for k in ("K1", "K3"):
        cell[k + "_break_even_accepted_per_step"] = round(cell[k + "_ratio"] - 1, 4)
    for k in ("K0", "K1", "K3"):                           # what the replays did: nothing ran into the no-op
        st = graphs[k][0].speculation_stats()
        assert st["steps"] == 1 + (args.reps + 1) * args.steps, (k, st)
        cell[k + "_accepted_per_step"] = round(st["accepted"] / st["steps"], 3)
    print(f"[bench_speculation] {cell}", file=sys.stderr, flush=True)
    return cell


# ---------------------------------------------------------------- (b) the control plane alone
def control_plane(vocab, hist):
    from pb_llm_amd import runtime as R
    S, calls = 4, args.calls
    g = torch.Generator(DEV).manual_seed(vocab + hist)
    logits = (torch.randn(1, S, vocab, device=DEV, generator=g) * 3).half()
    total = hist + (S + 1) * calls + 8
    tokens = torch.randint(0, vocab, (1, total), device=DEV, generator=g)
    tokens[0, hist - 2:hist] = tokens[0, hist // 2:hist // 2 + 2]          # one 2-gram match half way
    ids = torch.zeros(1, S, dtype=torch.long, device=DEV)
    state = torch.tensor([hist, 1], dtype=torch.long, device=DEV)
    cursor, count = state[:1], state[1:].view(torch.int32)[:1]
    unfinished = torch.ones(1, dtype=torch.bool, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = torch.zeros(8, dtype=torch.long, device=DEV)
    pos = [torch.tensor(hist, dtype=torch.long, device=DEV) for _ in range(32)]
    table = torch.tensor([p.data_ptr() for p in pos], dtype=torch.long, device=DEV)

    def verify(ngram):
        for _ in range(calls):
            R.spec_verify_f16(logits, ids, tokens, cursor, unfinished, count, status, table, st, max_ngram=ngram)

    def draft():
        for _ in range(calls):
            R.ngram_draft(tokens, cursor, unfinished, ids, 2)

    out = dict(V=vocab, history=hist)
    for name, fn in (("verify", lambda: verify(0)), ("verify_draft", lambda: verify(2)), ("draft", draft)):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fn()
        t = []
        for _ in range(args.reps + 1):
            state.copy_(torch.tensor([hist, 1], device=DEV))
            for p in pos:
                p.fill_(hist + S * calls)
            t.append(timed(gr, 1) / calls)
        out[name + "_us"], out[name + "_spread"] = stats(t[1:])
    assert int(status) == 0
    print(f"[bench_speculation] {out}", file=sys.stderr, flush=True)
    return out


# ---------------------------------------------------------------- (c) tokens/s at 0 % and 100 % acceptance
@torch.no_grad()
def end_to_end(model, vocab, ctx=128):
    from pb_llm_amd import harness as H
    n = args.new
    ids = torch.randint(0, vocab, (1, ctx), device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    total = ctx + n

    def clock(fn):
        fn()                                               # warm-up (captures the graph of a fresh session)
        t = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return res, n / sorted(t)[1]

    G, plain = clock(lambda: H.generate(model, ids, max_new_tokens=n))
    out = dict(V=vocab, context=ctx, new_tokens=n, one_row_loop_tokens_per_s=round(plain, 1))
    for K in (1, 3):
        for name, shift in (("all_right", 0), ("all_wrong", 1)):
            def run():
                sess = H.DecodeSession(model, 1, total - 1 + K, graph=True)
                sess.begin_speculation(ids, total, draft_tokens=K)
                ext = torch.cat([G, torch.zeros(1, K, dtype=torch.long, device=DEV)], 1)
                c = ctx + 1
                while c < total:                           # the host knows the cursor: every draft right (or wrong) by construction
                    sess.step_speculate((ext[:, c:c + K] + shift) % vocab)
                    c += 1 if shift else K + 1
                sess.run_speculation()                     # (whatever a rejected "right" draft left over)
                return sess
            sess, tps = clock(run)
            st = sess.speculation_stats()
            out[f"K{K}_{name}_tokens_per_s"] = round(tps, 1)
            out[f"K{K}_{name}_accepted_per_step"] = round(st["accepted"] / st["steps"], 3)
            out[f"K{K}_{name}_tokens_equal_one_row_loop"] = bool(torch.equal(sess.speculation_result(), G))
        res, tps = clock(lambda: H.generate(model, ids, max_new_tokens=n, prompt_lookup_num_tokens=K))
        out[f"K{K}_prompt_lookup_tokens_per_s"] = round(tps, 1)
        out[f"K{K}_prompt_lookup_tokens_equal_one_row_loop"] = bool(torch.equal(res, G))
    print(f"[bench_speculation] {out}", file=sys.stderr, flush=True)
    return out


if __name__ == "__main__":
    import __graft_entry__ as g
    g.build()
    vocabs = [int(v) for v in args.vocabs.split(",")]
    contexts = [int(c) for c in args.contexts.split(",")]
    result = dict(what="tools/bench_speculation.py on one MI355X, one process: (a) replay time of the captured decode units, one-row step + "
                       "select against (1 + K)-row step + verify + draft; (b) verify / draft alone; (c) tokens/s with forced drafts",
                  model=f"llama-7b shape (4096 / 11008 / 32 heads), {args.layers} decoder layers, distinct packed weights, "
                        "fuse_decode_(epilogues=True), batch 1",
                  reps=args.reps, replays_per_rep=args.steps, calls_per_replay=args.calls, unit=[], control_plane=[], end_to_end=[])
    for V in vocabs:
        for hist in (128, 4096, 65536):
            result["control_plane"].append(control_plane(V, hist))
    for V in vocabs:
        model = build_model(V, max(contexts) + (args.reps + 2) * args.steps * 4 + 16)
        for ctx in contexts:
            result["unit"].append(units(model, V, ctx))
        result["end_to_end"].append(end_to_end(model, V))
        del model
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
