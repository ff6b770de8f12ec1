#!/usr/bin/env python3
"""bench.py -- PB-linear GEMV stream benchmark (BASELINE.json metric).

A "step" is one pass of the hot path over one batch of synthetic input: L
(default 224 = the number of linears in llama-7b) llama-7b q_proj-shaped
partially-binarized linears (4096x4096, xnor low_frac=0.9 + 10 % int8 salient,
groupsize -1, RTN structure from the oracle's restatement of gptq_pb) each applied to
its own bs=1 fp16 activation vector.  All inputs are resident in HBM before the timed
region; the L layer blobs live at distinct HBM addresses (> 1.2 GB, beyond the 256 MiB
Infinity Cache), so the stream is served by HBM, not by cache.

value = layer-tokens/s = L * M * steps / t  (whole job).
roofline.achieved = ALGORITHMIC bytes per launch / average launch duration (HIP events on the
launch stream), where B_alg(N,K,nnz,M) is SURVEY.md 8(d)'s formula (1 bit/weight sign plane +
uint8 code and 8-bit index per salient + row params + row pointers + fp16 x and y).

--gpus 1: ONE grouped HIP launch per step (BASELINE configs[1]).
--gpus N > 1 (BASELINE configs[4]): the SAME L layers are sharded over N ranks with the
LLaMA tensor-parallel mapping -- layer i plays role i % 7 of a decoder layer: q, k, v, gate, up are
N-split (each rank owns a slice of the output rows, no exchange), o and down are K-split (each rank
owns a slice of the input columns; the fp32 partial outputs of the K-split layers are summed over the
ranks -- 64 dependent exchanges per step, as a decoder runs them).  Round 5 defaults (`--collective auto
--tp-collectives fused --tp-graph 1`): every K-split layer is ONE GEMV whose epilogue pushes the partial
straight into every peer's buffer over xGMI + a reduce kernel (libpbl's peer-to-peer path), the whole step
(N-split launch + 64 x [push GEMV + reduce]) captured in one hipGraph; validated against an RCCL all-reduce
of the same partials before anything is timed, with an automatic, group-wide fallback -- fused -> p2p
all-reduce per layer -> RCCL per layer -- if the peer mapping, the validation or the capture fails.  The
RCCL per-layer path `north_star` names is ALSO timed (outside the K steps the line reports) and printed in
the same JSON line as `rccl_per_layer_baseline`.  Total work is fixed: strong scaling.  `--parallel dp`
keeps round 1's independent streams per rank.  Run directly, `bench.py --gpus N` starts the N ranks itself
(torch.distributed.run); started by torch.distributed.run it checks WORLD_SIZE == N.

Clock pre-heat: a cold MI355X needs ~1 s of load before its clocks settle (20 timed steps are 6 ms);
the SAME launch is therefore repeated for --preheat-s seconds (default 2.0, reported as `preheat_s`)
before the W warm-up and K timed steps.  steps / warmup are exactly what the command line says.

A plain run measures the headline only.  `--full` adds everything else the line used to carry: the CPU baseline
(`cpu_baseline`), the cfg3 / cfg4 side entries (`side`) and, with --gpus N > 1, the RCCL per-layer baseline and the
per-phase timings of the step (`rccl_per_layer_baseline`, `tp_phases`).

`--dump-outputs DIR`: after the timed steps, what the timed path computed in its last step is written as DIR/<name>.npy
(float32; at most 64 MB in all, beyond that a fixed, seeded sample of every array).  The inputs depend on the arguments
only, so two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
TRAFFIC_PROFILE = os.path.join("profiles", "traffic_r06.json")
DUMP_MAX_BYTES = 60_000_000      # --dump-outputs payload: under 64 MB in all, .npy headers included


def dump_outputs(dirname, arrays, suffix=""):
    """--dump-outputs: every tensor of `arrays` (name -> tensor) as <dirname>/<name><suffix>.npy in float32.  Above DUMP_MAX_BYTES
    in all, every array is cut to a fixed, seeded sample of its flattened elements (the same positions in every run with the same
    arguments), in proportion to its size."""
    os.makedirs(dirname, exist_ok=True)
    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(v.nbytes for v in host.values())
    for name, v in host.items():
        if total > DUMP_MAX_BYTES:
            k = max(1, v.size * DUMP_MAX_BYTES // total)
            v = v.reshape(-1)[np.sort(np.random.default_rng(0).choice(v.size, k, replace=False))]
        np.save(os.path.join(dirname, name + suffix + ".npy"), np.ascontiguousarray(v, dtype=np.float32))


def build_base_layers(n_distinct, N, K, low_frac, seed0):
    """Synthetic PB layers via the oracle's restatement of the reference PTQ RTN path
    (structure only -- the oracle is not timed here and not on the product path)."""
    from oracle import pb_oracle as O
    from pb_llm_amd import synth
    out = []
    for i in range(n_distinct):
        W = synth.llm_weight(N, K, seed=seed0 + i)
        mask = O.ptq_low_mask(W, low_frac, "magnitude", None, -1)
        r = O.ptq_rtn(W, mask, 8, -1)
        out.append(dict(W=r["W_fq"], hi=(r["scale"][0] + r["mean"][0]).reshape(-1), lo=(-r["scale"][0] + r["mean"][0]).reshape(-1),
                        ss=np.asarray(r["hscale"], np.float32).reshape(-1), sz=np.asarray(r["hzero"], np.float32).reshape(-1),
                        sal=(~mask).astype(np.uint8)))
    return out


def pack_slice(b, rows=None, cols=None):
    """PBL1 blob of rows [r0, r1) x columns [c0, c1) of a base layer (levels / code grid are per ROW,
    so every slice reproduces the full layer's values exactly)."""
    from pb_llm_amd.packing import pack_dense
    r0, r1 = rows if rows else (0, b["W"].shape[0])
    c0, c1 = cols if cols else (0, b["W"].shape[1])
    return pack_dense(b["W"][r0:r1, c0:c1], b["hi"][r0:r1], b["lo"][r0:r1], b["ss"][r0:r1], b["sz"][r0:r1],
                      np.ascontiguousarray(b["sal"][r0:r1, c0:c1]))


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(dense_layers, K, M, budget_s=8.0):
    """The reference's CPU path on this box's host cores, via the oracle's statement of it
    (oracle/pb_oracle.py: torch_dense_linear = F.linear over the dense fake-quant weight, what
    gptq_pb/run.py / eval_after_qat.py execute per layer; SURVEY 8(d) last row), on a bounded sample:
    fp32 with every host thread (the headline `value`), fp16 with every thread, fp32 on one thread, and
    the QAT layer as written (weight re-simulated on every call)."""
    from oracle import pb_oracle as O
    from pb_llm_amd import synth
    Ws = [torch.from_numpy(w) for w in dense_layers]
    xs = [torch.from_numpy(synth.activations((M, K), 900 + i, 21)).float() for i in range(len(Ws))]

    def timed(ws, xv, budget):
        for w, x in zip(ws, xv):
            O.torch_dense_linear(x, w)
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < budget:
            for w, x in zip(ws, xv):
                O.torch_dense_linear(x, w)
            n += len(ws)
        return n, time.perf_counter() - t0

    threads = torch.get_num_threads()
    n, dt = timed(Ws, xs, budget_s)
    out = dict(value=n * M / dt, unit="layer-tokens/s", cores=threads, kind="port", cpu_model=cpu_model(),
               sample=f"{n} fp32 F.linear calls (oracle.torch_dense_linear) over {len(Ws)} distinct dense "
                      f"{Ws[0].shape[0]}x{K} fake-quant weights (cache-cold rotation), {dt:.1f} s",
               ms_per_layer=1e3 * dt / n)
    try:  # fp16 operands, as the reference's fp16 checkpoints would run on a CPU
        W16, x16 = [w.half() for w in Ws], [x.half() for x in xs]
        n16, dt16 = timed(W16, x16, budget_s / 2)
        out["fp16_ms_per_layer"] = 1e3 * dt16 / n16
        out["fp16_layer_tokens_per_s"] = n16 * M / dt16
    except RuntimeError as e:  # no fp16 CPU kernel in this torch build
        out["fp16_ms_per_layer"] = None
        out["fp16_note"] = str(e)[:120]
    # as-written QAT forward: a few calls are enough (tens of ms each)
    w = Ws[0]
    mask = w.abs() > w.abs().flatten().kthvalue(int(0.9 * w.numel()))[0]
    scale = w[~mask].abs().mean().view(1, 1)
    O.torch_qat_forward_as_written(xs[0], w, mask, scale)
    t1 = time.perf_counter()
    nq = 5
    for _ in range(nq):
        O.torch_qat_forward_as_written(xs[0], w, mask, scale)
    out["qat_forward_as_written_ms_per_layer"] = 1e3 * (time.perf_counter() - t1) / nq
    torch.set_num_threads(1)
    try:
        n1, dt1 = timed(Ws, xs, budget_s / 2)
        out["one_thread_fp32_ms_per_layer"] = 1e3 * dt1 / n1
        out["one_thread_fp32_layer_tokens_per_s"] = n1 * M / dt1
    finally:
        torch.set_num_threads(threads)
    return out


def side_layers(workload, dev, synth_mode):
    """The linears of a side workload as PBLinear modules on `dev` (own device copy per linear) + M.
    synth_mode "oracle": the structure comes from the oracle's restatement of the reference's RTN path on the host (what
    `--workload cfg3 | cfg4` measured in rounds 3 - 5; tens of seconds of numpy per layer); "device": the product's own producer
    (pb_llm_amd/ptq.py LowHighGPTQ, disable_gptq = RTN values, then to_pb: salient selection, quantizers and packer all on the
    GPU -- row f2 of SURVEY 8) on random-init fp16 weights N(0, 0.02^2) with a 1 % heavy tail and, for the hessian metric,
    calibration activations whose hot channels (1 %, 20 x) concentrate the salients in columns: the same kind of layer in a
    fraction of a second, which is what lets the driver's own command carry these lines."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import pb_llm_amd.quant as Q
    from pb_llm_amd import synth
    shapes = ([("q", 4096, 4096)] * 4 + [("gate", 11008, 4096)] * 2 + [("down", 4096, 11008)]) if workload == "cfg3" else \
             ([("ffn_in", 13824, 5120)] * 6 + [("ffn_out", 5120, 13824)] * 6)       # cfg4: 6 device copies each, beyond the Infinity Cache
    M = 2048 if workload == "cfg3" else 32
    low_frac, metric = (0.95, "hessian") if workload == "cfg3" else (0.8, "magnitude")
    built = {}
    if synth_mode == "oracle":
        from cfg_shapes import hessian_layer
        from oracle import pb_oracle as O
        for _, N, K in shapes:
            if (N, K) in built:
                continue
            if workload == "cfg3":
                W, mask, r = hessian_layer(N, K, low_frac, seed=300 + len(built))
            else:
                W = synth.llm_weight(N, K, seed=N % 97)
                mask = O.ptq_low_mask(W, low_frac, "magnitude", None, -1)
                r = O.ptq_rtn(W, mask, 8, -1)
            built[(N, K)] = Q.PBLinear.from_dense(torch.from_numpy(r["W_fq"]).half(), None, torch.from_numpy(mask), -1, r["hscale"], r["hzero"])
    else:
        from pb_llm_amd.ptq import LowHighGPTQ
        gen = torch.Generator(device=dev)
        for _, N, K in shapes:
            if (N, K) in built:
                continue
            gen.manual_seed(300 + len(built))
            W = torch.randn(N, K, device=dev, generator=gen) * 0.02
            tail = torch.rand(N, K, device=dev, generator=gen) < 0.01
            W = torch.where(tail, W * 4.0, W)
            lin = torch.nn.Linear(K, N, bias=False, device=dev, dtype=torch.float16)
            lin.weight.data = W.half()
            del W, tail
            g = LowHighGPTQ(lin, metric, -1, 8, disable_gptq=True)
            X = torch.randn(1024, K, device=dev, generator=gen)
            if metric == "hessian":
                hot = torch.randperm(K, device=dev, generator=gen)[:max(1, K // 100)]
                X[:, hot] *= 20.0
            g.add_batch(X)
            g.fasterquant(low_frac)
            built[(N, K)] = g.to_pb()
            g.free()
            del g, lin, X
        torch.cuda.empty_cache()
    def own_copy(pk):                                   # every linear multiplies from its own bytes in HBM
        return type(pk)(pk.blob.to(dev).clone() if pk.blob.device == dev else pk.blob.to(dev), pk.N, pk.K, pk.P, pk.G, pk.NRB, pk.flags,
                        pk.max_nch, pk.max_nexc, pk.nnz, pk.nexc)
    layers = [Q.PBLinear(own_copy(built[(N, K)].packed), None) for _, N, K in shapes]
    return layers, M


def measure_side(workload, steps, warmup, preheat_s, gemm_backend="default", small_batch_image="default", synth_mode="oracle",
                 dump_dir=None):
    """--workload cfg3 | cfg4: the other single-GPU configurations of BASELINE.json, as bench lines of their own (`--workload`)
    and, compact, under "side" in the driver's default line (round 6).  One step = one pass over the
    configuration's linears through the modules' forward with the LIBRARY'S DEFAULTS, timed with HIP events on torch's current
    stream (the stream the modules launch on) after its own pre-heat.
      cfg3  configs[2]: the seven linears of a llama-7b decoder layer, low_frac 0.95 HESSIAN salients, M = 2048 (prefill);
            bound: fp16 MFMA (2.5 PFLOP/s dense).  value = tokens/s of the 32-layer stack's linears = M / (32 t_layer).
      cfg4  configs[3]: llama-13b FFN 13824x5120 and 5120x13824, low_frac 0.8, M = 32; bound: HBM."""
    import pb_llm_amd.quant as Q
    from pb_llm_amd import synth
    import __graft_entry__ as ge
    ge.build()
    dev = torch.device("cuda:0")
    t_build = time.perf_counter()
    layers, M = side_layers(workload, dev, synth_mode)
    t_build = time.perf_counter() - t_build
    flops = sum(2.0 * M * l.out_features * l.in_features for l in layers)
    old = (Q.GEMM_BACKEND, Q.SMALL_BATCH_IMAGE)
    if gemm_backend != "default":
        Q.GEMM_BACKEND = gemm_backend
    gemm_backend = Q.GEMM_BACKEND                      # (what ran: reported in the line)
    if workload == "cfg4" and small_batch_image != "default":
        Q.SMALL_BATCH_IMAGE = small_batch_image
    small_batch_image = Q.SMALL_BATCH_IMAGE
    xs = {K: torch.from_numpy(synth.activations((M, K), 3, 21)).to(dev) for K in {l.in_features for l in layers}}
    if workload == "cfg3":
        # a decoder layer's call pattern (gptq_pb/eval_ppl_utils.py:55-64 through the HF model): q / k / v share one activation tensor,
        # o has its own, gate / up share one, down has its own -- FOUR distinct tensors per layer, so the fragment-major copy the
        # GEMM kernel reads x from (quant.GEMM_X_FRAGMENTS) is made four times per step, as in the model, not once
        x_of = [xs[4096]] * 3 + [xs[4096].clone()] + [xs[4096].clone()] * 2 + [xs[11008]]
    else:
        x_of = [xs[l.in_features] for l in layers]
    alg = sum(l.packed.algorithmic_bytes(M) for l in layers)

    def run():
        return [l(x) for l, x in zip(layers, x_of)]

    try:
        with torch.no_grad():
            t_pre = time.perf_counter()
            run(); torch.cuda.synchronize()
            while time.perf_counter() - t_pre < preheat_s:
                run(); torch.cuda.synchronize()
            for _ in range(warmup):
                run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(steps):
                last = run()
            e1.record()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
    finally:
        Q.GEMM_BACKEND, Q.SMALL_BATCH_IMAGE = old
    if dump_dir:
        dump_outputs(dump_dir, {f"y{i:02d}": y for i, y in enumerate(last)})
        del last
    dev_s = e0.elapsed_time(e1) * 1e-3 / steps
    same_box = {}
    if workload == "cfg3" and gemm_backend in ("auto", "fused"):
        # the same step on the same box in the same process, so that the line can be read without knowing the box: (i) what the
        # reference itself executes -- the dense fp16 library GEMM on the fake-quant weight (gptq_pb/gptq.py:180-184 writes it back,
        # gptq_pb/eval_ppl_utils.py:55-64 calls F.linear on it) --, (ii) the LDS-staged kernel of round 5 (no fragment-major copy of x)
        def timed(fn, pre=0.5, n=10):
            t = time.perf_counter()
            fn(); torch.cuda.synchronize()
            while time.perf_counter() - t < pre:
                fn(); torch.cuda.synchronize()
            a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record()
            for _ in range(n):
                fn()
            a1.record(); torch.cuda.synchronize()
            return a0.elapsed_time(a1) * 1e3 / n
        try:
            with torch.no_grad():
                dense = [l.weight.to(torch.float16) for l in layers]
                same_box["dense_library_us_per_step"] = timed(lambda: [torch.nn.functional.linear(x, w) for w, x in zip(dense, x_of)])
                del dense
                xf_old = Q.GEMM_X_FRAGMENTS
                try:
                    Q.GEMM_X_FRAGMENTS = False
                    same_box["lds_staged_kernel_us_per_step"] = timed(run)
                finally:
                    Q.GEMM_X_FRAGMENTS = xf_old
                # ... and what the four fragment-major copies of a step cost alone (they are inside us_per_step)
                same_box["x_copies_us_per_step"] = timed(lambda: [Q.x_fragments(x) for x in (x_of[0], x_of[3], x_of[4], x_of[6])])
            same_box["vs_dense_library"] = 1e6 * dev_s / same_box["dense_library_us_per_step"]
        except Exception as e:       # noqa: BLE001 -- the comparison figures are extras: the step's own number is never lost to them
            same_box["same_box_error"] = f"{type(e).__name__}: {str(e)[:200]}"
    imgs = [getattr(l.packed, "_gemm_image", (None, None))[1] for l in layers]
    n_img = sum(1 for i in imgs if i is not None)
    if workload == "cfg3":
        roof = {"bound": "mfma", "achieved": flops / dev_s / 1e12, "peak": 2500.0, "unit": "TFLOP/s", "traffic": None,
                "kernel": ("pbl_unpack_kernel + library GEMM" if gemm_backend == "library" else
                           f"pbl_gemm_img_kernel ({n_img} of {len(layers)} layers have a GEMM image; the rest: " +
                           ("pbl_gemm_kernel)" if gemm_backend in ("fused", "auto") else "pbl_unpack_kernel + library GEMM)")),
                "us_per_step": 1e6 * dev_s, **same_box}
        value, unit = M / (32 * wall / steps), "tokens/s (linears of a 32-layer stack)"
        work = "llama-7b decoder-layer linears (q,k,v,o 4096x4096; gate,up 11008x4096; down 4096x11008), low_frac 0.95 hessian, M=2048"
    else:
        roof = {"bound": "hbm", "achieved": alg / dev_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "traffic": None,
                "kernel": (f"small-batch kernel over the layers' GEMM images ({n_img} of {len(layers)} layers)" if n_img
                           else "pbl_mfma_kernel + pbl_mfma_reduce over the packed records"),
                "us_per_step": 1e6 * dev_s, "us_per_layer": 1e6 * dev_s / len(layers),
                "algorithmic_bytes_per_step": alg,
                "blob_bytes": sum(l.packed.blob.numel() for l in layers),
                "image_bytes": sum(i.data.numel() for i in imgs if i is not None)}
        value, unit = len(layers) * M / (wall / steps), "layer-tokens/s"
        work = "llama-13b FFN 13824x5120 + 5120x13824 (6 device copies each), low_frac 0.8, M=32"
    roof["frac"] = roof["achieved"] / roof["peak"]
    if workload == "cfg4" and roof.get("image_bytes"):
        # `achieved` counts the ALGORITHMIC bytes (the packed blob: what the layer needs); the image kernel reads the image instead
        roof["bytes_read_GBps"] = roof["image_bytes"] / dev_s / 1e9
        roof["bytes_read_frac"] = roof["bytes_read_GBps"] / roof["peak"]
    nnz = sum(int(l.packed.nnz) for l in layers)
    tot = sum(l.out_features * l.in_features for l in layers)
    line = {"metric": f"PB-linear side workload {workload}", "value": value, "unit": unit, "n_gpus": 1,
            "steps": steps, "warmup": warmup, "preheat_s": preheat_s, "ms_per_step": 1e3 * wall / steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16 in/out, f32 accumulate",
            "data": "synthetic", "config": {"workload": work, "gemm_backend": gemm_backend, "synth": synth_mode, "salient_frac": nnz / tot,
                                            "build_s": round(t_build, 2), **({"small_batch_image": small_batch_image} if workload == "cfg4" else {})},
            "roofline": roof}
    del layers, xs, x_of
    torch.cuda.empty_cache()
    return line


def run_side_workload(a):
    print(json.dumps(measure_side(a.workload, a.steps, a.warmup, a.preheat_s, a.gemm_backend, a.small_batch_image, a.synth,
                                  a.dump_outputs)), flush=True)


def side_summary(budget_note="library defaults, device-synthesised layers (the product's GPU producer), own pre-heat + HIP events"):
    """configs[2] and configs[3] inside the driver's default line: {"cfg3": {...}, "cfg4": {...}}.  A side line
    that fails is reported as {"error": ...}: the headline is never lost to it."""
    out = {"note": budget_note}
    for wl, steps, warmup, pre in (("cfg3", 10, 3, 1.0), ("cfg4", 20, 5, 1.0)):
        t0 = time.perf_counter()
        try:
            l = measure_side(wl, steps, warmup, pre, synth_mode="device")
            r = l["roofline"]
            d = {"us_per_step": r["us_per_step"], "frac": r["frac"], "bound": r["bound"], "achieved": r["achieved"], "unit": r["unit"],
                 "kernel": r["kernel"], "steps": steps, "warmup": warmup, "preheat_s": pre, "workload": l["config"]["workload"],
                 "salient_frac": l["config"]["salient_frac"]}
            if wl == "cfg4":
                d.update(us_per_layer=r["us_per_layer"], bytes_read_frac=r.get("bytes_read_frac"), image_bytes=r.get("image_bytes"),
                         blob_bytes=r.get("blob_bytes"), algorithmic_bytes_per_step=r.get("algorithmic_bytes_per_step"))
            else:
                d.update(gemm_backend=l["config"]["gemm_backend"],
                         **{k: r[k] for k in ("dense_library_us_per_step", "lds_staged_kernel_us_per_step", "x_copies_us_per_step", "vs_dense_library", "same_box_error") if k in r})
            d["wall_s"] = round(time.perf_counter() - t0, 2)
            out[wl] = d
        except Exception as e:       # noqa: BLE001 -- reported in the line
            out[wl] = {"error": f"{type(e).__name__}: {str(e)[:300]}", "wall_s": round(time.perf_counter() - t0, 2)}
    return out


# role of layer i in a llama decoder layer (SURVEY 8(e) "LLaMA layer mapping"): True = K-split (+ all-reduce)
TP_KSPLIT_ROLE = (False, False, False, True, False, False, True)   # q k v o gate up down


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--preheat-s", type=float, default=2.0,
                    help="seconds of the same launch before warm-up, so that clocks have settled (reported)")
    ap.add_argument("--layers", type=int, default=224)
    ap.add_argument("--distinct", type=int, default=4, help="distinct synthetic weight sets (replicated to L blobs)")
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--K", type=int, default=4096)
    ap.add_argument("--M", type=int, default=1)
    ap.add_argument("--low-frac", type=float, default=0.9)
    ap.add_argument("--mode", choices=["grouped", "graph", "eager"], default="grouped")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: the CPU baseline, the cfg3 / cfg4 side entries and, with "
                         "--gpus N > 1, the RCCL per-layer baseline and the per-phase timings of the step")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--parallel", choices=["auto", "dp", "tp"], default="auto",
                    help="auto: tp when --gpus > 1; tp: LLaMA tensor-parallel mapping of the layer stream + one "
                         "all-reduce of the K-split partial outputs per step (strong scaling); dp: independent "
                         "layer streams per rank (weak scaling, no collective)")
    ap.add_argument("--collective", choices=["auto", "rccl", "p2p"], default="auto",
                    help="tp exchange: auto (default) = libpbl's peer-to-peer path over IPC-mapped buffers, RCCL if the mapping or its "
                         "validation fails on any rank; p2p = the same without the fallback; rccl = torch.distributed all_reduce")
    ap.add_argument("--tp-collectives", choices=["per-layer", "stacked", "fused"], default="fused",
                    help="tp: fused (default) = every K-split layer is ONE GEMV whose epilogue pushes the partial to every rank + a reduce "
                         "kernel (p2p only; falls back to per-layer); per-layer = GEMV launch + one all-reduce of [M, N] fp32 per K-split "
                         "layer (64 per step, 16 KB each at M = 1); stacked = ONE all-reduce of all K-split partials per step (the easy case)")
    ap.add_argument("--tp-graph", type=int, choices=[0, 1], default=1,
                    help="tp fused: capture the whole step (N-split launch + 64 x [push GEMV + reduce]) in one hipGraph and replay it")
    ap.add_argument("--small-batch-image", choices=["default", "auto", "0", "1"], default="default",
                    help="cfg4: default = the library's own setting (quant.SMALL_BATCH_IMAGE, \"1\" since round 5: the small-batch kernel over the "
                         "layers' GEMM images, built on the first call; 1.7 x the blob's bytes at 20 %% salients); 0 = the kernel over the packed "
                         "records; auto = an image only if a prefill call built one")
    ap.add_argument("--workload", choices=["cfg2", "cfg3", "cfg4"], default="cfg2",
                    help="cfg2 = BASELINE configs[1], the headline GEMV stream (default, what the driver runs); cfg3 / cfg4: "
                         "configs[2] / configs[3] as side lines (see run_side_workload)")
    ap.add_argument("--synth", choices=["oracle", "device"], default="oracle",
                    help="cfg3 / cfg4: where the layers' structure comes from (see side_layers); the driver line's \"side\" entries use device")
    ap.add_argument("--no-side", action="store_true", help="default workload with --full: skip the cfg3 / cfg4 side entries of the line")
    ap.add_argument("--gemm-backend", choices=["default", "auto", "tuned", "library", "fused"], default="default",
                    help="cfg3: quant.GEMM_BACKEND -- default = the library's own setting (\"auto\": always the hand-written kernel over each "
                         "layer's GEMM image, round 5); tuned = round 4's routing (library GEMM where the 128 x 256 tiles leave a thin last "
                         "round); library: pbl_unpack_dev + library GEMM")
    a = ap.parse_args()
    if a.workload != "cfg2":
        assert a.gpus == 1, "side workloads are single-GPU lines"
        return run_side_workload(a)

    if a.gpus > 1 and "RANK" not in os.environ:
        # started directly: become the launcher of N ranks, one per GPU (RCCL over xGMI)
        if torch.cuda.device_count() < a.gpus and os.environ.get("PBL_BENCH_BACKEND", "nccl") == "nccl":
            sys.exit(f"bench.py --gpus {a.gpus}: only {torch.cuda.device_count()} GPU(s) visible")
        port = os.environ.get("MASTER_PORT", "29511")
        os.execvp(sys.executable, [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                                   f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1", "--master-port", port,
                                   os.path.abspath(__file__), *sys.argv[1:]])

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    use_dist = "RANK" in os.environ  # launched by torch.distributed.run (any world size, incl. 1)
    if world != a.gpus:
        sys.exit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}; launch one rank per GPU "
                 f"(python -m torch.distributed.run --nproc-per-node {a.gpus} bench.py --gpus {a.gpus} ...)")
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback for the product path)"
    # PBL_BENCH_BACKEND=gloo: plumbing test of the multi-rank path on a box with fewer GPUs than ranks (ranks share devices,
    # control tensors travel over gloo, --collective p2p does the data-path sum); never a measurement.
    backend = os.environ.get("PBL_BENCH_BACKEND", "nccl")
    dev = torch.device(f"cuda:{local % torch.cuda.device_count() if backend != 'nccl' else local}")
    torch.cuda.set_device(dev)
    ctl = dev if backend == "nccl" else torch.device("cpu")
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        assert dist.get_world_size() == a.gpus

    import __graft_entry__ as ge
    ge.build()
    from pb_llm_amd import synth
    from pb_llm_amd.quant import PBLinear
    from pb_llm_amd.runtime import GroupedGemv

    parallel = a.parallel if a.parallel != "auto" else ("tp" if world > 1 else "dp")
    tp = parallel == "tp" and world > 1
    base = build_base_layers(a.distinct, a.N, a.K, a.low_frac, seed0=1000 + (0 if tp else 17 * rank))
    xs_host = [synth.activations((a.M, a.K), 5000 + i + (0 if tp else 1000 * rank), 21) for i in range(a.layers)]

    groups = []          # (GroupedGemv, needs_allreduce)
    if tp:
        from pb_llm_amd.parallel import split_points, COL_ALIGN, ROW_ALIGN
        r0, r1 = split_points(a.N, world, ROW_ALIGN)[rank:rank + 2]
        c0, c1 = split_points(a.K, world, COL_ALIGN)[rank:rank + 2]
        nsh = [pack_slice(b, rows=(r0, r1)) for b in base]
        ksh = [pack_slice(b, cols=(c0, c1)) for b in base]
        n_ids = [i for i in range(a.layers) if not TP_KSPLIT_ROLE[i % 7]]
        k_ids = [i for i in range(a.layers) if TP_KSPLIT_ROLE[i % 7]]
        gn = GroupedGemv([nsh[i % a.distinct].to(dev) for i in n_ids], None, M=a.M, device=dev)
        gk = GroupedGemv([ksh[i % a.distinct].to(dev) for i in k_ids], None, M=a.M, device=dev, out_f32=True)
        for t, i in zip(gn.x, n_ids):
            t.copy_(torch.from_numpy(xs_host[i]))
        for t, i in zip(gk.x, k_ids):
            t.copy_(torch.from_numpy(np.ascontiguousarray(xs_host[i][:, c0:c1])))
        groups = [(gn, False), (gk, True)]
    else:
        full = [pack_slice(b) for b in base]
        packed = [full[i % a.distinct].to(dev) for i in range(a.layers)]
        # .to(dev) of a host blob allocates a fresh device buffer per call: L distinct HBM regions
        assert len({p.blob.data_ptr() for p in packed}) == a.layers
        g = GroupedGemv(packed, None, M=a.M, device=dev)
        for t, xh in zip(g.x, xs_host):
            t.copy_(torch.from_numpy(xh))
        groups = [(g, False)]
    torch.cuda.synchronize()

    singles = None
    if a.mode != "grouped":
        singles = [(PBLinear(p, None), x) for g, _ in groups for p, x in zip(g.packed, g.x)]
    kev = []            # (start, end) events around the GEMV launches of a step (tp, eager: the timed region also holds the collective)

    # ---- tensor parallel: which exchange runs.  Decided ONCE, group-wide (every rank must take the same path: the fused pair, the
    # p2p all-reduce and RCCL wait on different things), validated against the baseline collective before anything is timed.
    comm, tp_path, tp_notes = None, None, []

    def base_all_reduce(t):
        """the baseline collective north_star names: RCCL on a node; in plumbing mode (ranks share a device, gloo) through the host"""
        if backend == "nccl":
            dist.all_reduce(t)
        else:
            c = t.cpu()
            dist.all_reduce(c)
            t.copy_(c)

    if tp:
        import ctypes as C
        from pb_llm_amd import _lib
        from pb_llm_amd.parallel import P2PAllReduce, agree_min
        gn, gk = groups[0][0], groups[1][0]
        yk16 = [torch.empty(a.M, a.N, dtype=torch.float16, device=dev) for _ in gk.packed]
        if a.collective in ("auto", "p2p"):
            try:
                comm = P2PAllReduce(gk.y_all.numel(), dev)       # collective: raises on EVERY rank if any rank cannot map its peers
            except _lib.PblError as e:
                if a.collective == "p2p":
                    raise
                tp_notes.append(f"p2p unavailable ({e}); RCCL")
        want = a.tp_collectives
        if comm is None and want == "fused":
            want = "per-layer"
        if want == "fused":
            lim = min(_lib.lib().pbl_linear_push_max_tokens(C.byref(p.layer_struct(None))) for p in gk.packed)
            if agree_min(lim, None, dev) < a.M:                  # one GEMV pass on every rank, or not fused at all
                tp_notes.append(f"fused push takes {lim} tokens per pass here, M = {a.M}: per-layer")
                want = "per-layer"

        def step_tp(path, record=False):
            """one step on `path`: 'fused' | 'p2p-per-layer' | 'p2p-stacked' | 'rccl-per-layer' | 'rccl-stacked'; returns this rank's
            outputs (its rows of the N-split layers, the summed K-split layers)"""
            if record:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            gn.launch()
            if path == "fused":
                if record:
                    e1.record()
                    kev.append((e0, e1))
                for pk, xk, yk in zip(gk.packed, gk.x, yk16):
                    if not comm.fused_linear_(pk, None, xk, yk):
                        raise SystemExit("--tp-collectives fused: the K-split shard is not one GEMV pass")
                return {"y_nsplit": gn.y, "y_ksplit": yk16}
            gk.launch()
            if record:
                e1.record()
                kev.append((e0, e1))
            parts = gk.y if path.endswith("per-layer") else [gk.y_all]
            for t in parts:
                if path.startswith("p2p"):
                    comm.all_reduce_(t)
                else:
                    base_all_reduce(t)
            return {"y_nsplit": gn.y, "y_ksplit": gk.y}

        # reference sums through the baseline collective, once
        gk.launch()
        ref = gk.y_all.clone()
        base_all_reduce(ref)
        torch.cuda.synchronize()

        def valid(path):
            """does `path` reproduce the baseline collective's sums on every rank?  (collective; never raises on one rank only)"""
            ok = 1
            try:
                for _ in range(3):                               # more calls than slot sets
                    step_tp(path)
                torch.cuda.synchronize()
                if path == "fused":
                    got = torch.cat([y.reshape(-1).float() for y in yk16])
                    tol = 2e-3 * float(ref.abs().max())          # fp16 outputs
                else:
                    got, tol = gk.y_all.float(), 1e-5 * float(ref.abs().max())
                err = float((got - ref).abs().max())
                ok = int(err == err and err <= tol)
                if comm is not None:
                    comm.check()
            except (_lib.PblError, RuntimeError) as e:
                tp_notes.append(f"{path}: {str(e)[:120]}")
                ok = 0
            return bool(agree_min(ok, None, dev))

        chain = (["fused"] if want == "fused" else []) + ([f"p2p-{want if want != 'fused' else 'per-layer'}"] if comm is not None else []) \
            + [f"rccl-{want if want != 'fused' else 'per-layer'}"]
        for cand in chain:
            if cand.startswith("rccl") or valid(cand):
                tp_path = cand
                break
            tp_notes.append(f"{cand} failed its validation against the baseline collective: falling back")

    fused_tp = tp_path == "fused"

    def step(record=False):
        """one step; returns its outputs, name -> list of per-layer tensors"""
        if tp:
            return step_tp(tp_path, record)
        if a.mode == "grouped":
            return {"y": groups[0][0].launch()}          # one group unless tp
        return {"y": [m(x) for m, x in singles]}

    def capture(fn):
        """(graph, the outputs the captured step writes on every replay)"""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            outs = fn()
        return gr, outs

    graph, graph_outs = None, None
    tp_graphed = False
    if a.mode == "graph" and not tp:
        graph, graph_outs = capture(step)
        run = graph.replay
    elif fused_tp and a.tp_graph:
        # the whole step in ONE hipGraph: the call number of the push / reduce pair lives in the peers' buffers, so a replay advances
        # it like an eager call.  A failed capture is agreed over the group (all ranks replay, or all ranks launch eagerly).
        ok = 1
        try:
            graph, graph_outs = capture(step)
        except (RuntimeError, _lib.PblError) as e:
            tp_notes.append(f"hipGraph capture of the fused step failed ({str(e)[:100]}): eager launches")
            ok, graph = 0, None
        if agree_min(ok, None, dev) and graph is not None:
            run, tp_graphed = graph.replay, True
        else:
            run = step
    else:
        run = step

    # clock pre-heat: the same launch, for a fixed time (disclosed in the JSON line)
    t_pre = time.perf_counter()
    n_pre = 0
    pre_batches = []    # (seconds since the start of the pre-heat, device ms of one batch of 32 steps): the SUSTAINED rate
    while a.preheat_s > 0:
        pe0, pe1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        pe0.record()
        for _ in range(32):
            run()
        pe1.record()
        n_pre += 32
        torch.cuda.synchronize()
        pre_batches.append((time.perf_counter() - t_pre, pe0.elapsed_time(pe1)))
        done = time.perf_counter() - t_pre >= a.preheat_s
        if use_dist:   # every rank must leave the loop after the same number of collectives
            flag = torch.tensor([int(done)], device=ctl)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            done = bool(flag.item())
        if done:
            break
    preheat_s = time.perf_counter() - t_pre if a.preheat_s > 0 else 0.0

    def timed(run_fn, record):
        """W warm-up steps, then EXACTLY K steps between barrier + synchronize on both sides; max over the ranks.  Also returns the
        last step's outputs (a graph replay returns none: the captured step's buffers hold them)"""
        kev.clear()
        last = None
        for _ in range(a.warmup):
            run_fn()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(a.steps):
            if record:
                last = step(True)
            else:
                last = run_fn()
        e1.record()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize()
        wall_ = time.perf_counter() - t0
        dev_ = e0.elapsed_time(e1) * 1e-3
        kern_ = sum(s_.elapsed_time(e_) for s_, e_ in kev) * 1e-3 if kev else dev_
        if use_dist:
            tt = torch.tensor([wall_, dev_, kern_], device=ctl, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            wall_, dev_, kern_ = tt.tolist()
        return wall_, dev_, kern_, (last if last is not None else graph_outs)

    def dump(outs):
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, {k: torch.stack(v) for k, v in outs.items()}, f"_rank{rank}" if world > 1 else "")

    rec = tp and not tp_graphed
    wall, dev_s, kern_s, outs = timed(run, rec)
    dump(outs)
    tp_valid_after = None
    if tp and comm is not None and tp_path != "rccl-per-layer" and not tp_path.startswith("rccl"):
        # a peer wait that timed out poisons the sums with NaN and sets the buffer's status word: the number above would describe a
        # broken exchange.  Agreed over the group; the line then carries the RCCL measurement instead and says so.
        ok = 1
        try:
            comm.check()
        except _lib.PblError as e:
            tp_notes.append(str(e)[:120])
            ok = 0
        tp_valid_after = bool(agree_min(ok, None, dev))
    rccl_base = None
    if tp and (tp_path != "rccl-per-layer") and (backend == "nccl" or os.environ.get("PBL_BENCH_BASELINE") == "1") and \
            (a.full or tp_valid_after is False):
        # the baseline north_star names, timed the same way OUTSIDE the K steps reported above: GEMV launches + one RCCL all-reduce per
        # K-split layer (64 eager 16 KB collectives per step).  A plain run times it only to replace a broken exchange's number.
        main_path, tp_path = tp_path, "rccl-per-layer"
        bw, bd, bk, bouts = timed(step, True)
        tp_path = main_path
        rccl_base = {"value": a.layers * a.M * a.steps / bw, "unit": "layer-tokens/s", "ms_per_step": 1e3 * bw / a.steps,
                     "us_per_step_device": 1e6 * bd / a.steps, "collective_us_per_step": 1e6 * (bd - bk) / a.steps,
                     "what": f"grouped GEMV launches + {len(groups[1][0].packed)} torch.distributed all_reduce calls of [{a.M},{a.N}] fp32 per step "
                             f"({'RCCL' if backend == 'nccl' else 'gloo through the host: plumbing only'}), eager"}
        if tp_valid_after is False:
            tp_notes.append(f"{main_path} reported a timed-out peer wait: the line carries the RCCL per-layer measurement")
            wall, dev_s, kern_s, tp_path, tp_graphed = bw, bd, bk, "rccl-per-layer", False
            dump(bouts)

    tp_phases = None
    if tp and a.full:
        # where a step's time goes, per phase, from a few EAGER steps of the path that was timed (outside the K steps above; round 6,
        # VERDICT r5 item 9): the N-split launch, and per K-split layer the push GEMV + reduce kernel (fused), or the GEMV launch + the
        # all-reduce calls (per-layer / stacked paths); HIP events on the launch stream, max over ranks
        ph = {}
        try:
            if comm is not None:
                comm.phase_events = []
            n_ev = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step_tp(tp_path)
                e1.record()
                n_ev.append((e0, e1))
            torch.cuda.synchronize()
            ph["eager_step_us"] = 1e3 * sum(s_.elapsed_time(e_) for s_, e_ in n_ev) / len(n_ev)
            if comm is not None and comm.phase_events:
                for kind in sorted({k for k, _, _ in comm.phase_events}):
                    v = [s_.elapsed_time(e_) for k, s_, e_ in comm.phase_events if k == kind]
                    ph[f"{kind}_us_per_call"] = 1e3 * sum(v) / len(v)
                    ph[f"{kind}_calls_per_step"] = len(v) // 3
            g0e, g1e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g0e.record(); gn.launch(); g1e.record()
            torch.cuda.synchronize()
            ph["nsplit_gemv_us"] = 1e3 * g0e.elapsed_time(g1e)
            if use_dist:
                keys = sorted(ph)
                tt = torch.tensor([ph[k] for k in keys], device=ctl, dtype=torch.float64)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                ph = dict(zip(keys, tt.tolist()))
        except Exception as e:      # noqa: BLE001 -- diagnostics never cost the line
            ph["error"] = f"{type(e).__name__}: {str(e)[:160]}"
        finally:
            if comm is not None:
                comm.phase_events = None
        if comm is not None and os.environ.get("PBL_BENCH_P2P_SELFTEST", "1") == "1":
            try:
                ph["p2p_pair_allreduce_16KB_us"] = P2PAllReduce.selftest_pairs(dev)
            except Exception as e:  # noqa: BLE001
                ph["p2p_pair_allreduce_16KB_us"] = f"{type(e).__name__}: {str(e)[:160]}"
        tp_phases = ph

    traffic, traffic_source = None, None
    key = f"N{a.N}_K{a.K}_L{a.layers}_M{a.M}_lf{a.low_frac}_{a.mode}"
    try:  # HBM bytes per launch: PMC passes cannot run inside this process; the value is read from the committed
        # rocprofv3 profile of this exact workload and labelled with its source
        tj = json.load(open(os.path.join(REPO, TRAFFIC_PROFILE)))
        if tj.get("workload_key") == key and world == 1:
            traffic, traffic_source = tj["hbm_bytes_per_launch"], TRAFFIC_PROFILE
    except (OSError, ValueError, KeyError):
        pass
    if rank == 0:
        b_alg = sum(g.algorithmic_bytes() for g, _ in groups)          # this rank's shards (the whole stream at N=1)
        packed_b = sum(g.packed_bytes() for g, _ in groups)
        nl = 1 if a.mode == "grouped" else a.layers
        per_launch_s = kern_s / (a.steps * nl)
        achieved = b_alg / nl / per_launch_s / 1e9
        # sustained figure: the pre-heat loop runs the same launch back to back for preheat_s seconds; its second half (clocks
        # settled at the package power cap) is timed batch by batch with HIP events.  The K timed steps above follow a
        # synchronize and are a burst of a few ms -- both are reported ("the bench times a burst").
        sus_us, sus_n = None, 0
        if not tp and pre_batches:
            late = [ms for t, ms in pre_batches if t >= 0.5 * preheat_s] or [pre_batches[-1][1]]
            sus_n = 32 * len(late) * nl
            sus_us = 1e3 * sum(late) / sus_n
        if tp:
            nk = len(groups[1][0].packed)
            coll = 'libpbl one-shot p2p' if tp_path.startswith('p2p') else ('RCCL' if backend == 'nccl' else 'gloo (plumbing run: ranks share a device)')
            par = (f"tp{world}: llama mapping, q/k/v/gate/up N-split (no exchange), o/down K-split + " +
                   (f"{nk} fused K-split layers per step (GEMV epilogue pushes the partial to every rank over peer-mapped buffers + reduce kernel)"
                    + (", the whole step replayed as ONE hipGraph" if tp_graphed else ", eager launches") if tp_path == "fused" else
                    f"{nk} {coll} all-reduces of [{a.M},{a.N}] fp32 per step (one per K-split layer)" if tp_path.endswith("per-layer")
                    else f"one {coll} all-reduce of [{nk},{a.M},{a.N}] fp32 per step"))
        else:
            par = f"dp{world} (independent layer streams, no collective)"
        out = {
            "metric": "PB-linear GEMV tokens/sec + achieved HBM GB/s, llama-7b 4096x4096 low_frac=0.9",
            "value": (1 if tp else world) * a.layers * a.M * a.steps / wall,
            "unit": "layer-tokens/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "preheat_s": round(preheat_s, 3),
            "ms_per_step": 1e3 * wall / a.steps,
            "higher_is_better": True, "scaling": "strong" if tp else "weak", "vs_baseline": None,
            "dtype": "f16 (x, y) / 1-bit + u8 weights, f32 accumulate", "data": "synthetic",
            "config": {"workload": f"llama-7b q_proj {a.N}x{a.K} xnor low_frac={a.low_frac} + int8 salient, "
                                   f"bs={a.M} GEMV, stream of {a.layers} layer blobs at distinct HBM addresses "
                                   f"({a.distinct} distinct weight sets), mode={a.mode}",
                       "layers_per_step": a.layers, "tokens": a.M, "parallelism": par},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                         "kernel": "pbl_gemv_kernel<1,4>" if a.mode == "grouped" else "pbl_gemv_kernel<1,1>",
                         "algorithmic_bytes_per_launch": b_alg / nl,
                         "packed_bytes_per_launch": packed_b / nl,
                         "us_per_launch": 1e6 * per_launch_s,
                         "sustained_us_per_launch": sus_us,
                         "sustained_frac": (b_alg / nl / (sus_us * 1e-6) / 1e9 / HBM_PEAK_GBS) if sus_us else None,
                         "sustained_launches": sus_n,
                         "us_per_layer": 1e6 * kern_s / (a.steps * a.layers),
                         "us_per_step": 1e6 * dev_s / a.steps,
                         "collective_us_per_step": (1e6 * (dev_s - kern_s) / a.steps) if tp else 0.0,
                         "note": (("per rank: bytes of rank 0's shards / the WHOLE graph-replayed step (GEMVs + exchange: a lower bound on the "
                                   "kernels' rate)" if tp_graphed else
                                   "per rank: bytes of rank 0's shards / the GEMV launches of a step; us_per_step is the whole step "
                                   "on the device, collectives included (max over ranks)") if tp else
                                  "one grouped launch = the whole stream")},
        }
        if tp:
            out["config"]["tp_path"] = tp_path + ("+graph" if tp_graphed else "")
            out["config"]["tp_requested"] = f"--collective {a.collective} --tp-collectives {a.tp_collectives} --tp-graph {a.tp_graph}"
            out["config"]["tp_validated_against_baseline_collective"] = True if not tp_path.startswith("rccl") else None
            if tp_notes:
                out["config"]["tp_notes"] = tp_notes
            if rccl_base is not None:
                out["rccl_per_layer_baseline"] = rccl_base
            if tp_phases is not None:
                out["tp_phases"] = tp_phases
        if a.full and not a.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline([b["W"] for b in base], a.K, a.M)
        if a.full and world == 1 and not a.no_side and a.mode == "grouped":
            # BASELINE configs[2] / configs[3] measured by the SAME process the driver times (after the headline: its numbers are
            # final above; the stream's blobs are released first)
            groups.clear()
            run = None
            torch.cuda.empty_cache()
            out["side"] = side_summary()
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
