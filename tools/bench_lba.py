"""Milliseconds per call of Optimizer::LocalBundleAdjustment on the device (orbgpu_local_ba_device), host preparation
apart from the device.

usage: python tools/bench_lba.py [--reps R] [--out profiles/lba_times.json]

A call first builds, on the host, the index structure the fixed summation order needs (edges sorted by point, per-pose edge
lists, per-block pair lists of the reduced system), converts the state to double and uploads it; then one workgroup runs
both rounds.  The entry point returns once everything is enqueued, so per call this reports
    host_ms    from the call to its return (preparation, upload, launch), and
    device_ms  from the return to the end of the stream (what the kernel still had to do),
their medians over R calls after one warm-up call, for a few seeded local maps up to the size of the reference's typical
one (about 20 free key frames and as many fixed cameras, 3000 points, 25000 observations).  The LM iterations and trials of
each map are listed, since the time follows them.  No CPU figure is given: the float64 model of tests/lba_model.py is a
definition, not an implementation, and g2o is not available here; neither would be a fair baseline."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = [(3, 2, 100, 0.7), (8, 6, 600, 0.5), (14, 12, 1500, 0.4), (20, 20, 3000, 0.2)]  # free, fixed, points, share seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lba_times.json"))
    a = ap.parse_args()
    import torch
    import fuzz_lba as F
    import lba_model as M
    from orb_slam2_map_amd import lib as G
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for nf, nx, npts, obs in SIZES:
        sc = M.make_scene(nf, nx, npts, 900 + nf, mode="mixed", obs_frac=obs)
        p, d = F.upload(torch, sc)
        host, dev = [], []
        for rep in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            G.local_ba_device(p, stream=stream)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rep:
                host.append(1e3 * (t1 - t0))
                dev.append(1e3 * (t2 - t1))
        _, r, _ = F.download(d, sc)
        rows.append({"free_poses": nf, "fixed_cameras": nx, "points": npts, "edges": r["n_edges"], "erased": r["n_erased"],
                     "iterations": r["iterations"], "trials": r["trials"], "reduced_in_lds": r["reduced_in_lds"],
                     "host_ms": statistics.median(host), "device_ms": statistics.median(dev),
                     "host_ms_all": host, "device_ms_all": dev})
        print("%2d free + %2d fixed poses, %5d points, %6d edges: host %.2f ms, device %.2f ms per call (iterations %r, trials %r)"
              % (nf, nx, npts, r["n_edges"], rows[-1]["host_ms"], rows[-1]["device_ms"], r["iterations"], r["trials"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"note": "orbgpu_local_ba_device, one problem per call; medians of %d calls after one warm-up; host_ms includes "
                           "the ctypes marshalling of the problem; no CPU baseline (see tools/bench_lba.py)" % a.reps,
                   "sizes": rows}, f, indent=1)


if __name__ == "__main__":
    main()
