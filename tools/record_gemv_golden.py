#!/usr/bin/env python3
"""Record the fixtures of tests/test_gpu_gemv_persistent.py: the outputs of its two grouped launches (tests/gemv_persistent_cases.py),
M = 1 and M = 4, as the library in use computes them on the GPU.

    PBL_LIB=/path/to/libpbl.so-of-the-recording-commit  tools/record_gemv_golden.py [--out tests/golden] [--commit de42e4d]

--cases MODULE records another case module of tests/ instead (gemv_lookahead_cases: tests/test_gpu_gemv_lookahead.py).  A case
module has LAUNCHES, MS, pack_sets, build_group, fixture_name and SENTINEL as gemv_persistent_cases does; it may name its sidecar
(SIDECAR) and its recording commit (COMMIT, the default of --commit), and may add single-layer launches (SPLITS with build_split,
run_split, split_fixture_name and activations), recorded one [M, N] block per file.

The committed fixtures were recorded with the library built from commit de42e4d (the parent of the change that reworked the
kernel's salient rounds); PBL_LIB selects that build, the in-tree library is used when it is unset.  Per (launch, M) one
tests/golden/<fixture_name>.npy holds the first `period` members' outputs back to back (fp16), and gemv_grouped_parent.json the
recording commit, the library's sha256 and every file's sha256.  Before anything is written the launch is checked: nothing outside
the members' rows was written, a second launch gives the same bits, and every member equals the fixture member it repeats."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    ap.add_argument("--commit", default=None, help="the commit the library in use was built from (goes into the sidecar); "
                    "default: the case module's COMMIT, de42e4d for gemv_persistent_cases")
    ap.add_argument("--cases", default="gemv_persistent_cases", help="the case module of tests/ to record")
    a = ap.parse_args()
    import importlib
    GC = importlib.import_module(a.cases)
    a.commit = a.commit or getattr(GC, "COMMIT", "de42e4d")
    from pb_llm_amd import _lib
    _lib.lib()
    os.makedirs(a.out, exist_ok=True)
    side = {"recorded_with_commit": a.commit, "library": os.path.basename(_lib.LIB_PATH),
            "library_sha256": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(), "files": {}}
    for launch in GC.LAUNCHES:
        sets = GC.pack_sets(launch)
        for M in GC.MS:
            g, buf, keep = GC.build_group(launch, sets, M, "cuda:0")
            g.launch()
            torch.cuda.synchronize()
            first = buf.clone()
            assert bool((buf[keep] == GC.SENTINEL).all()), (launch.name, M, "a store outside the members' rows")
            g.launch()
            torch.cuda.synchronize()
            assert torch.equal(first.view(torch.int16), buf.view(torch.int16)), (launch.name, M, "two launches differ")
            ys = [y.cpu().numpy() for y in g.y]
            for i, y in enumerate(ys):
                assert np.array_equal(y.view(np.uint16), ys[i % launch.period].view(np.uint16)), (launch.name, M, i)
            flat = np.concatenate([y.reshape(-1) for y in ys[:launch.period]])
            name = GC.fixture_name(launch, M) + ".npy"
            np.save(os.path.join(a.out, name), flat)
            side["files"][name] = {"sha256": hashlib.sha256(flat.tobytes()).hexdigest(), "elements": int(flat.size)}
            print(name, flat.size, "fp16 values")
    for sp in getattr(GC, "SPLITS", ()):
        _, p = GC.build_split(sp)
        pd = p.to("cuda:0")
        for M in GC.MS:
            x = torch.from_numpy(GC.activations(sp.K, M, 0)).to("cuda:0")
            y, buf, keep = GC.run_split(pd, x, M)
            torch.cuda.synchronize()
            assert bool((buf[keep] == GC.SENTINEL).all()), (sp.name, M, "a store outside the layer's rows")
            _, again, _ = GC.run_split(pd, x, M)
            torch.cuda.synchronize()
            assert torch.equal(buf.view(torch.int16), again.view(torch.int16)), (sp.name, M, "two launches differ")
            flat = y.cpu().numpy().reshape(-1)
            name = GC.split_fixture_name(sp, M) + ".npy"
            np.save(os.path.join(a.out, name), flat)
            side["files"][name] = {"sha256": hashlib.sha256(flat.tobytes()).hexdigest(), "elements": int(flat.size)}
            print(name, flat.size, "fp16 values")
    with open(os.path.join(a.out, getattr(GC, "SIDECAR", "gemv_grouped_parent.json")), "w") as f:
        json.dump(side, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
