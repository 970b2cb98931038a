"""ms per call of orbgpu_pnp_solve_batch_device: one candidate, and a batch of 8, at N = 300 and 1200 kept rows, 300 sets
of 4 offered (the reference's parameters use max_its = 35 of them).  HIP events around the call (its one host round trip
for the RANSAC parameters included), 5 warm-up calls, median of 50; writes profiles/pnp_times.json.  No time target is set
for these entry points: the figures are a record, not a bound.

usage: python tools/bench_pnp.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fuzz_pnp as F  # noqa: E402
import pnp_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402


def main():
    import torch
    rows = []
    stream = torch.cuda.current_stream().cuda_stream
    for n in (300, 1200):
        for cands in (1, 8):
            scenes = [M.make_scene(n, 100 * n + c) for c in range(cands)]
            ups = [F.upload(torch, sc) for sc in scenes]
            probs = [u[0] for u in ups]
            ms = []
            for it in range(55):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                G.pnp_solve_batch_device(probs, stream=stream)
                b.record()
                torch.cuda.synchronize()
                if it >= 5:
                    ms.append(a.elapsed_time(b))
            r = F.download(ups[0][1], scenes[0])
            rows.append({"n": n, "candidates": cands, "sets_offered": 300, "min_set": 4, "max_its": r["max_its"],
                         "accepted": r["accepted"], "median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)),
                         "max_ms": float(np.max(ms))})
            print(rows[-1])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pnp_times.json"), "w") as f:
        json.dump({"what": "orbgpu_pnp_solve_batch_device, HIP events, 5 warm-up calls, median of 50", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
