"""Milliseconds per call of Optimizer::BundleAdjustment on the device (orbgpu_bundle_adjustment_device), host preparation
apart from the device.

usage: python tools/bench_ba.py [--reps R] [--out profiles/ba_times.json]

As tools/bench_lba.py: a call first builds, on the host, the index structure the fixed summation order needs, converts the
state to double and uploads it; then ONE workgroup runs optimize(20).  Per call this reports
    host_ms    from the call to its return (preparation, upload, launch), and
    device_ms  from the return to the end of the stream (what the kernel still had to do),
their medians over R calls after one warm-up call, with the robust kernel on (Tracking.cc:963) and off (LoopClosing.cc:647),
for seeded maps from the monocular bootstrap (KF 0 and one more key frame, 150 points) to 200 key frames and 16384 points.
The LM iterations and trials of each map are listed, since the time follows them.

These are the first numbers for whole-map sizes and the figure a later multi-workgroup solver has to beat; they are a
record, not a claim: one workgroup per map is a correctness-first shape, and no CPU figure is given -- the float64 model of
tests/ba_model.py is a definition, not an implementation, and the times are not compared with g2o."""
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

# free poses (KF 0, fixed, comes on top), points, share of the key frames that see a point, mode
SIZES = [(1, 150, 1.0, "mono"), (30, 3000, 0.25, "mixed"), (96, 10000, 0.08, "mixed"), (200, 16384, 0.03, "mixed")]
ITERATIONS = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_times.json"))
    a = ap.parse_args()
    import torch
    import fuzz_ba as F
    from orb_slam2_map_amd import lib as G
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for nf, npts, obs, mode in SIZES:
        for robust in (True, False):
            sc = F.make_scene(nf, 0, npts, 900 + nf, n_iterations=ITERATIONS, robust=robust, mode=mode, kf0_fixed=True, obs_frac=obs)
            p, d = F.upload(torch, sc)
            host, dev = [], []
            for rep in range(a.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                G.bundle_adjustment_device(p, stream=stream)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if rep:
                    host.append(1e3 * (t1 - t0))
                    dev.append(1e3 * (t2 - t1))
            _, r, _ = F.download(d, sc)
            rows.append({"poses": nf + 1, "free_poses": nf, "points": npts, "edges": r["n_edges"], "robust": robust,
                         "n_iterations": ITERATIONS, "iterations": r["iterations"], "trials": r["trials"],
                         "chi2_start": r["chi2_start"], "chi2_end": r["chi2_end"], "reduced_in_lds": r["reduced_in_lds"],
                         "host_ms": statistics.median(host), "device_ms": statistics.median(dev),
                         "host_ms_all": host, "device_ms_all": dev})
            print("%3d poses, %5d points, %6d edges, robust %d: host %.2f ms, device %.2f ms per call (iterations %d, trials %d, "
                  "S in %s)" % (nf + 1, npts, r["n_edges"], robust, rows[-1]["host_ms"], rows[-1]["device_ms"], r["iterations"],
                                r["trials"], "LDS" if r["reduced_in_lds"] else "global memory"), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"note": "orbgpu_bundle_adjustment_device, one problem per call, optimize(%d); medians of %d calls after one "
                           "warm-up; host_ms includes the ctypes marshalling of the problem; a first, unrepeated record for "
                           "whole-map sizes, one workgroup per map; no CPU baseline and no comparison with g2o (see "
                           "tools/bench_ba.py)" % (ITERATIONS, a.reps), "sizes": rows}, f, indent=1)


if __name__ == "__main__":
    main()
