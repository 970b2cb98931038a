"""ms per call of orbgpu_sim3_solve_batch_device: N = 100, 300, 1500 correspondences x 1, 16 candidates x H = 300
hypotheses.  HIP events around the call (its one host round trip for max_its included), 5 warm-up calls, median of 50;
writes profiles/sim3_bench.json.

usage: python tools/bench_sim3.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fuzz_sim3 as F  # noqa: E402
import sim3_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402


def main():
    import torch
    rows = []
    stream = torch.cuda.current_stream().cuda_stream
    for n in (100, 300, 1500):
        for cands in (1, 16):
            scenes = [M.make_scene(n, 100 * n + c) for c in range(cands)]
            ups = [F.upload(torch, sc) for sc in scenes]
            probs = [u[0] for u in ups]
            ms = []
            for it in range(55):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                G.sim3_solve_batch_device(probs, stream=stream)
                b.record()
                torch.cuda.synchronize()
                if it >= 5:
                    ms.append(a.elapsed_time(b))
            r = F.download(ups[0][1], scenes[0])
            rows.append({"n": n, "candidates": cands, "hypotheses": 300, "max_its": r["max_its"], "median_ms": float(np.median(ms)),
                         "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))})
            print(rows[-1])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sim3_bench.json"), "w") as f:
        json.dump({"what": "orbgpu_sim3_solve_batch_device, HIP events, 5 warm-up calls, median of 50", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
