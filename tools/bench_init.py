"""ms per orbgpu_initializer_batch_device call: HIP events around the call, 5 warm-up calls, the median of 50.
N in {300, 1200} x 1 / 8 problems, n_hyp = 200 (the reference's iterations).  Writes profiles/init_times.json.

usage: python tools/bench_init.py

There is no time target: a new entry point has no earlier figure, and the CPU model is no baseline."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import init_model as M  # noqa: E402
import fuzz_init as F  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402

WARMUP, CALLS = 5, 50


def measure(torch, scenes):
    ups = [F.upload(torch, sc) for sc in scenes]
    problems = [u[0] for u in ups]
    stream = torch.cuda.current_stream().cuda_stream
    times = []
    for k in range(WARMUP + CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        G.initializer_batch_device(problems, stream=stream)
        b.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            times.append(a.elapsed_time(b))
    got = [F.download(u[1], sc) for u, sc in zip(ups, scenes)]
    return float(np.median(times)), float(np.min(times)), float(np.max(times)), got


def main():
    import torch
    rows = []
    for n in (300, 1200):
        for problems in (1, 8):
            scenes = [M.make_scene(n, 31000 + n + k, "general" if k % 2 == 0 else "planar", n_hyp=200) for k in range(problems)]
            med, lo, hi, got = measure(torch, scenes)
            rows.append({"N": n, "problems": problems, "n_hyp": 200, "ms_median": med, "ms_min": lo, "ms_max": hi,
                         "success": [int(g["success"]) for g in got], "used_homography": [int(g["used_homography"]) for g in got]})
            print("N %4d x %d problems, 200 hypotheses: median %.3f ms (min %.3f, max %.3f) per call" % (n, problems, med, lo, hi))
    out = {"what": "ms per orbgpu_initializer_batch_device call, HIP events around the call (the entry point's wait for the "
                   "stream and its upload of the problem records included), %d warm-up calls, median of %d" % (WARMUP, CALLS),
           "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "init_times.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
