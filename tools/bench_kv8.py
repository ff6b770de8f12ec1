#!/usr/bin/env python3
"""The FP8 KV cache against the fp16 cache, one process, every step under its own time limit (a step that runs over ends the run
with what was measured so far):
  (a) decode   the decode attention call alone (pbl_decode_attn_kv8 against pbl_decode_attn_f16; 32 heads, D = 128, B = 1, one query
               row) at context 128 / 1024 / 4096 / 16384, over a RING of caches larger than the 256 MB last-level cache so that every
               call streams its rows from HBM; the calls over the ring are captured in one hipGraph per format (no host time inside
               the window) and the two graphs alternate
  (b) prefill  append + attention of a 1024- and a 4096-row prefill (pbl_prefill_attn_kv8 against pbl_prefill_attn_f16)
  (c) generate us per token of DecodeSession.step on the 6 llama-7b-shaped layers of tools/bench_generate.py at context 128 / 1024 /
               4096 with both caches (the captured step replayed, the sessions alternating)
  (d) bytes    what each session's cache holds
  (e) logits   max |logits fp8 - logits fp16| over a 128-token prefill and 8 forced steps on that model, beside the same figure
               between HF's sdpa and eager attention on the fp16 path
Per timing: the median over reps and the spread (max - min over the median, in percent).
  python tools/bench_kv8.py [--layers 6] [--reps 9] [--iters 32] [--out profiles/r14_kv_cache_fp8.json]"""
import argparse
import contextlib
import json
import os
import signal
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from transformers import LlamaConfig, LlamaForCausalLM  # noqa: E402

from pb_llm_amd import harness as H, ptq, runtime  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--decode-contexts", default="128,1024,4096,16384")
ap.add_argument("--prefills", default="1024,4096")
ap.add_argument("--contexts", default="128,1024,4096")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--iters", type=int, default=32)
ap.add_argument("--ring-mb", type=int, default=640, help="bytes of FP8 cache the ring of (a) holds at least (the fp16 ring: twice)")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r14_kv_cache_fp8.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_kv8.py measures on the GPU only"
HQ, D = 32, 128
out = dict(reps=args.reps, iters=args.iters)


class StepTimeout(Exception):
    pass


@contextlib.contextmanager
def limit(seconds, what):
    def expired(*_):
        raise StepTimeout(what)

    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def finish(code=0):
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    sys.exit(code)


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


def stats(v, digits=2):
    v = sorted(v)
    return round(v[len(v) // 2], digits), round(100 * (v[-1] - v[0]) / v[len(v) // 2], 2)


def alternate(cases, key, scale=1.0, before=None):
    """reps rounds of every case in turn; out[<case>_<key>_us / _spread_pct]"""
    t = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, fn in cases.items():
            t[k].append(timed(fn, before) * scale)
    for k in cases:
        out[f"{k}_{key}_us"], out[f"{k}_{key}_spread_pct"] = stats(t[k])
    return t


def graph_of(unit, before):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        before()
        unit()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    before()
    with torch.cuda.graph(g):
        unit()
    return g


def quantized_random(shape, gen):
    """random FP8 rows: bytes of finite e4m3fn values and power-of-two scales in [2^-6, 2^4] (what the attention reads; made on the
    device, no reference quantiser in the way)"""
    b = torch.randint(0, 256, shape, generator=gen, device="cuda", dtype=torch.uint8)
    b = torch.where((b & 0x7f) == 0x7f, b & 0xf0, b)
    s = torch.exp2(torch.randint(-6, 5, shape[:-1], generator=gen, device="cuda").float())
    return b, s


try:
    # ---------------------------------------------------------------- (a) the decode attention call alone
    for C in [int(c) for c in args.decode_contexts.split(",")]:
        with limit(120, f"decode attention at context {C}"), torch.no_grad():
            L = C + 64
            per_set = 2 * HQ * L * D                                    # FP8 bytes of one K + V set
            n = max(2, min(512, -(-args.ring_mb * (1 << 20) // per_set)))
            gen = torch.Generator(device="cuda").manual_seed(C)
            ring8, ring16 = [], []
            for _ in range(n):
                kq, ks = quantized_random((1, HQ, L, D), gen)
                vq, vs = quantized_random((1, HQ, L, D), gen)
                ring8.append((kq, vq, ks, vs))
                ring16.append((runtime.kv8_dequantize(kq, ks), runtime.kv8_dequantize(vq, vs)))
            q = torch.randn(1, HQ, 1, D, generator=gen, device="cuda").half()
            pos_all = torch.empty(n, dtype=torch.int64, device="cuda")
            pos = [pos_all[i:i + 1] for i in range(n)]
            outs8, outs16 = [], []

            def run8():
                outs8[:] = [runtime.decode_attention_kv8(q, kq, vq, ks, vs, pos[i], D ** -0.5) for i, (kq, vq, ks, vs) in enumerate(ring8)]

            def run16():
                outs16[:] = [runtime.decode_attention_f16(q, k, v, pos[i], D ** -0.5) for i, (k, v) in enumerate(ring16)]

            def rewind():
                pos_all.fill_(C - 1)                                    # the query row attends to rows [0, C - 1]: C keys

            g8, g16 = graph_of(run8, rewind), graph_of(run16, rewind)
            rewind(), g8.replay(), rewind(), g16.replay()
            torch.cuda.synchronize()
            same = all(torch.equal(a, b) for a, b in zip(outs8, outs16))
            alternate({"decode_attn_fp8": g8.replay, "decode_attn_fp16": g16.replay}, f"ctx{C}", 1.0 / n, rewind)
            out[f"decode_attn_ctx{C}_ring_sets"] = n
            out[f"decode_attn_ctx{C}_ring_mb_fp8"], out[f"decode_attn_ctx{C}_ring_mb_fp16"] = per_set * n >> 20, 2 * per_set * n >> 20
            out[f"decode_attn_ctx{C}_bits_equal"] = same
            out[f"decode_attn_ctx{C}_fp8_over_fp16"] = round(out[f"decode_attn_fp8_ctx{C}_us"] / out[f"decode_attn_fp16_ctx{C}_us"], 3)
            out[f"decode_attn_ctx{C}_gbs_fp8"] = round(2 * HQ * C * (D + 4) / out[f"decode_attn_fp8_ctx{C}_us"] / 1e3, 1)
            out[f"decode_attn_ctx{C}_gbs_fp16"] = round(2 * HQ * C * D * 2 / out[f"decode_attn_fp16_ctx{C}_us"] / 1e3, 1)
            del ring8, ring16, g8, g16, outs8, outs16
            torch.cuda.empty_cache()

    # ---------------------------------------------------------------- (b) append + attention of a prefill
    for P in [int(c) for c in args.prefills.split(",")]:
        with limit(120, f"prefill attention of {P} rows"), torch.no_grad():
            L = P + 256
            gen = torch.Generator(device="cuda").manual_seed(P)
            q, k_new, v_new = (torch.randn(1, HQ, P, D, generator=gen, device="cuda").half() for _ in range(3))
            kc, vc = (torch.zeros(1, HQ, L, D, dtype=torch.float16, device="cuda") for _ in range(2))
            kq, vq = (torch.zeros(1, HQ, L, D, dtype=torch.uint8, device="cuda") for _ in range(2))
            ks, vs = (torch.zeros(1, HQ, L, device="cuda") for _ in range(2))
            p = torch.zeros((), dtype=torch.int64, device="cuda")
            calls = {"prefill_attn_fp8": lambda: runtime.prefill_attention_kv8(q, k_new, v_new, kq, vq, ks, vs, p, D ** -0.5),
                     "prefill_attn_fp16": lambda: runtime.prefill_attention_f16(q, k_new, v_new, kc, vc, p, D ** -0.5)}
            for fn in calls.values():
                for _ in range(3):
                    p.zero_()
                    fn()
            alternate(calls, f"P{P}", before=p.zero_)
            out[f"prefill_attn_P{P}_fp8_over_fp16"] = round(out[f"prefill_attn_fp8_P{P}_us"] / out[f"prefill_attn_fp16_P{P}_us"], 3)
            p.zero_()
            a8 = calls["prefill_attn_fp8"]().float()
            p.zero_()
            out[f"prefill_attn_P{P}_max_abs_diff_fp8_vs_fp16"] = float((a8 - calls["prefill_attn_fp16"]().float()).abs().max())
            del q, k_new, v_new, kc, vc, kq, vq, ks, vs
            torch.cuda.empty_cache()

    # ---------------------------------------------------------------- (c) - (e) the 6-layer model of tools/bench_generate.py
    contexts = [int(c) for c in args.contexts.split(",")]
    with limit(300, "model set-up"):
        t_setup = time.time()
        cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=args.layers, num_attention_heads=HQ,
                          num_key_value_heads=HQ, vocab_size=1024, max_position_embeddings=max(contexts) + 256)
        torch.manual_seed(0)
        with torch.device("cuda"):
            model = LlamaForCausalLM(cfg).half().eval()
        with torch.no_grad():
            for nm, prm in model.named_parameters():
                if "norm" in nm:
                    prm.copy_(1 + 0.1 * torch.randn_like(prm.float()))
        for layer in model.model.layers:                      # distinct packed weights per layer (RTN + magnitude, 5 % salients)
            for name, lin in H.find_layers(layer).items():
                qz = ptq.LowHighGPTQ(lin, "magnitude", -1, 8, disable_gptq=True)
                qz.add_batch(torch.zeros(1, 8, lin.in_features, device="cuda"))
                qz.H += torch.eye(lin.in_features, device="cuda")
                qz.fasterquant(0.95)
                pb = qz.to_pb().to("cuda")
                qz.free()
                parent = layer
                *path, leaf = name.split(".")
                for p_ in path:
                    parent = getattr(parent, p_)
                setattr(parent, leaf, pb)
        torch.cuda.empty_cache()
        H.fuse_decode_(model, epilogues=True)
        ids = torch.randint(0, cfg.vocab_size, (1, max(contexts) + args.iters + 8), device="cuda")
        out["model"] = (f"llama-7b shape (4096 / 11008 / 32 heads), {args.layers} decoder layers, distinct packed weights, "
                        "fuse_decode_(epilogues=True), batch 1, DecodeSession.step replayed from a hipGraph")
        out["setup_s"] = round(time.time() - t_setup, 1)

    class Case:
        def __init__(self, C, kv_cache):
            self.C, self.sess = C, H.DecodeSession(model, 1, C + args.iters + 4, graph=True, kv_cache=kv_cache)
            self.prefill = self.sess.prefill(ids[:, :C]).float().clone()
            self.sess.step(ids[:, C])                          # the capture
            self.rewind()
            self.first = self.sess.step(ids[:, C]).float().clone()
            self.rewind()

        def rewind(self):
            for lay in self.sess.cache.layers:
                lay.cumulative_length.fill_(self.C)
            self.sess.pos = self.C

        def run(self):
            for t in range(args.iters):
                self.sess.step(ids[:, self.C + t])

        def cache_bytes(self):
            return sum(sum(t.numel() * t.element_size() for t in vars(lay).values()
                           if isinstance(t, torch.Tensor) and t.dim() >= 3) for lay in self.sess.cache.layers)

    for C in contexts:
        with limit(180, f"generate at context {C}"), torch.no_grad():
            runs = {"generate_fp8": Case(C, "fp8"), "generate_fp16": Case(C, "fp16")}
            for r in runs.values():
                r.rewind()
                r.run()
            t = {k: [] for k in runs}
            for _ in range(args.reps):
                for k, r in runs.items():
                    t[k].append(timed(r.run, r.rewind) / args.iters)
            for k, r in runs.items():
                out[f"{k}_ctx{C}_us_per_token"], out[f"{k}_ctx{C}_spread_pct"] = stats(t[k], 1)
                out[f"{k}_ctx{C}_cache_bytes"] = r.cache_bytes()
            out[f"generate_ctx{C}_fp8_over_fp16"] = round(out[f"generate_fp8_ctx{C}_us_per_token"] / out[f"generate_fp16_ctx{C}_us_per_token"], 3)
            a, b = runs["generate_fp8"], runs["generate_fp16"]
            out[f"ctx{C}_first_step_logits_max_abs_diff_fp8_vs_fp16"] = float((a.first - b.first).abs().max())
            out[f"ctx{C}_prefill_logits_max_abs_diff_fp8_vs_fp16"] = float((a.prefill - b.prefill).abs().max())
            out[f"ctx{C}_logits_max_abs"] = float(b.first.abs().max())
            del runs, a, b
            torch.cuda.empty_cache()

    def forced_logits(P, steps=8, impl=None, **session):
        was = model.config._attn_implementation
        if impl is not None:
            model.config._attn_implementation = impl
        try:
            sess = H.DecodeSession(model, 1, P + 64, graph=False, **session)
            lg = [sess.prefill(ids[:, :P]).float().clone()]
            for t in range(P, P + steps):
                lg.append(sess.step(ids[:, t]).float().clone())
        finally:
            model.config._attn_implementation = was
        return torch.stack(lg, 1)

    with limit(120, "forced logits"), torch.no_grad():
        P = min(contexts)
        l8, l16 = forced_logits(P, kv_cache="fp8"), forced_logits(P)
        sdpa, eager = forced_logits(P, impl="sdpa"), forced_logits(P, impl="eager")
        out[f"P{P}_forced_logits_max_abs_diff_fp8_vs_fp16"] = float((l8 - l16).abs().max())
        out[f"P{P}_forced_logits_d_ref_sdpa_vs_eager"] = float((sdpa - eager).abs().max())
        out[f"P{P}_forced_logits_max_abs"] = float(l16.abs().max())
except StepTimeout as e:
    out["timed_out"] = str(e)
    finish(1)
finish()
