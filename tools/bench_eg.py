"""Milliseconds per call of Optimizer::OptimizeEssentialGraph on the device (orbgpu_essential_graph_device and
orbgpu_essential_graph_correct_points_device), host preparation apart from the device.

usage: python tools/bench_eg.py [--reps R] [--sizes 50,500,2000] [--out profiles/eg_times.json]

A call first builds, on the host, the index structure (the taken edges, the reverse Cuthill-McKee order, the envelope, the
per-block edge lists) and uploads it with the states; then ONE workgroup runs optimize(20).  Per call this reports
    host_ms    from the call to its return (preparation, upload, launch),
    device_ms  from the return to the end of the stream (what the kernel still had to do), and
    points_ms  the correction of 100 points per key frame, launch to end of stream,
their medians over R calls after one warm-up call (rings of 2000: one call, no warm-up), for seeded closed rings of 50, 500
and 2000 key frames with 4 and 12 neighbours per key frame (reach 2 and 6), the scale free (monocular) and fixed.  The
envelope and the bandwidth of each ring and its LM iterations and trials are listed, since the time follows them.

No split into linearise / factor / rest is given: the kernel carries no time stamps.  These are the first numbers for this
optimiser and the figure a multi-workgroup solve has to beat; they are a record, not a claim, and they are not compared with
g2o, which is not on the machine."""
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

ITERATIONS = 20
POINTS_PER_KF = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="50,500,2000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eg_times.json"))
    a = ap.parse_args()
    import torch
    import eg_model as M
    import fuzz_eg as F
    from orb_slam2_map_amd import lib as G
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for V in [int(v) for v in a.sizes.split(",")]:
        for reach in (2, 6):
            for fix_scale in (False, True):
                sc = M.make_scene(V, 700 + V + reach, reach=reach, fix_scale=fix_scale, rot_drift=0.1, trans_drift=0.5,
                                  scale_drift=0.1, n_corrected=2 * reach, n_iterations=ITERATIONS, compose=True,
                                  n_points=POINTS_PER_KF * V)
                p, d = F.upload(torch, sc)
                reps, warm = (1, 0) if V >= 2000 else (a.reps, 1)
                host, dev, pts = [], [], []
                for rep in range(reps + warm):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    G.essential_graph_device(p, stream=stream)
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    F.correct_points(torch, sc, d)
                    torch.cuda.synchronize()
                    t3 = time.perf_counter()
                    if rep >= warm:
                        host.append(1e3 * (t1 - t0))
                        dev.append(1e3 * (t2 - t1))
                        pts.append(1e3 * (t3 - t2))
                _, r, _ = F.download(d, sc)
                rows.append({"key_frames": V, "neighbours": 2 * reach, "edges": r["n_edges"], "fix_scale": fix_scale,
                             "points": POINTS_PER_KF * V, "free_active": r["n_free_active"], "envelope": r["envelope"],
                             "bandwidth": r["bandwidth"], "n_iterations": ITERATIONS, "iterations": r["iterations"],
                             "trials": r["trials"], "chi2_start": r["chi2_start"], "chi2_end": r["chi2_end"],
                             "host_ms": statistics.median(host), "device_ms": statistics.median(dev),
                             "device_ms_per_trial": statistics.median(dev) / max(r["trials"], 1),
                             "points_ms": statistics.median(pts), "host_ms_all": host, "device_ms_all": dev, "points_ms_all": pts})
                print("%4d key frames, %2d neighbours, fix_scale %d: %6d edges, envelope %8d doubles, bandwidth %3d; host %.2f ms, "
                      "device %.2f ms per call (iterations %d, trials %d: %.2f ms per trial), %d points %.3f ms" % (
                          V, 2 * reach, fix_scale, r["n_edges"], r["envelope"], r["bandwidth"], rows[-1]["host_ms"],
                          rows[-1]["device_ms"], r["iterations"], r["trials"], rows[-1]["device_ms_per_trial"], POINTS_PER_KF * V,
                          rows[-1]["points_ms"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"note": "orbgpu_essential_graph_device, one ring per call, optimize(%d); medians of %d calls after one warm-up "
                           "(2000 key frames: one call); host_ms includes the ctypes marshalling of the problem; points_ms "
                           "includes the launch; a first, unrepeated record, one workgroup per graph, no in-kernel split; no CPU "
                           "baseline and no comparison with g2o (see tools/bench_eg.py)" % (ITERATIONS, a.reps),
                   "sizes": rows}, f, indent=1)


if __name__ == "__main__":
    main()
