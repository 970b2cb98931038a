"""Times orbgpu_covis_keyframe_culling and orbgpu_covis_observations on one stated map and reports the share of the
sequential kernel.

usage: python tools/bench_cull.py [--out profiles/cull_bench.json] [--reps 30] [--key-frames 500] [--slots 2000]
                                  [--candidates 30] [--no-trace]

The map: --key-frames key frames of --slots slots each; a key frame holds points on 40 % of its slots, drawn from a
window of 4 x slots point ids that slides by slots / 20 per key frame (neighbours share points, far key frames do not: a
point is held by about eight key frames, so that some candidates are redundant and their going changes the test for the
later ones), octaves uniform in 0-2, three slots in four stereo, one stereo slot in ten far.  The candidates
are --candidates consecutive key frames from the middle of the map, newest first (the newest key frames of such a map
are never redundant: the points ahead of them are held by nobody else yet).  The call is timed with HIP
events on the current stream (it returns synchronised) and with the host clock, after a warm-up, median of --reps.  The
kernels' share comes from a second run of the same calls in a child process under `rocprofv3 --kernel-trace --stats`
(--trace-child); --no-trace leaves it out and says so.  One JSON document; nothing here is a pass criterion."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from orb_slam2_map_amd import lib as G  # noqa: E402
from bench_covis import timed  # noqa: E402

SLIDE = 20  # the window of point ids moves by slots / SLIDE per key frame: a point is in reach of 80 key frames, held by 8
KERNELS = ("k_covis_cull_count", "k_covis_cull_resolve", "k_covis_cull_emit")


def plant(g, n_kf, n_slots, rng):
    window = 4 * n_slots
    filled = int(0.4 * n_slots)
    for k in range(n_kf):
        slots = np.full(n_slots, -1, np.int64)
        pts = (k * (n_slots // SLIDE) + rng.choice(window, size=filled, replace=False)).astype(np.int64)
        slots[rng.choice(n_slots, size=filled, replace=False)] = pts
        g.add_keyframe(k, n_slots, slots)
        stereo = rng.random(n_slots) < 0.75
        far = stereo & (rng.random(n_slots) < 0.1)
        g.set_keypoints(k, rng.integers(0, 3, n_slots) | np.where(stereo, g.KP_STEREO, 0) | np.where(far, g.KP_FAR, 0))


def scene(a):
    rng = np.random.default_rng(a.key_frames + a.slots)
    g = G.CovisibilityGraph(initial_rows=a.key_frames, initial_slots=a.key_frames * a.slots)
    plant(g, a.key_frames, a.slots, rng)
    top = a.key_frames // 2 + a.candidates // 2
    cand = np.arange(top, top - a.candidates, -1, dtype=np.int64)
    cand = cand[(cand > 0) & (cand < a.key_frames)]
    return g, cand


def kernel_shares(a):
    """the same calls in a fresh child under rocprofv3; total nanoseconds per culling kernel"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--reps", str(a.reps), "--key-frames", str(a.key_frames),
               "--slots", str(a.slots), "--candidates", str(a.candidates)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return dict(error="rocprofv3 run failed (exit %d): %s" % (r.returncode, r.stdout[-400:]))
        ns = {k: 0.0 for k in KERNELS}
        calls = {k: 0 for k in KERNELS}
        for row in csv.DictReader(open(files[0])):
            for k in KERNELS:
                if k in row["Name"]:
                    ns[k] += float(row["TotalDurationNs"])
                    calls[k] += int(row["Calls"])
        return dict(total_ns=ns, calls=calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cull_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--key-frames", type=int, default=500)
    ap.add_argument("--slots", type=int, default=2000)
    ap.add_argument("--candidates", type=int, default=30)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    g, cand = scene(a)
    try:
        if a.trace_child:  # culling calls only, so that the kernel totals divide by the calls
            for _ in range(a.reps):
                g.keyframe_culling(cand, None, 3, 0)
            return
        first = g.keyframe_culling(cand)
        cap = first["n_points_bad"]
        cull = timed(lambda: g.keyframe_culling(cand, None, 3, cap), a.reps)
        held = np.arange(min((a.key_frames - 1) * (a.slots // SLIDE) + 4 * a.slots, 1 << 20), dtype=np.int64)  # every id planted
        obs = timed(lambda: g.observations(held), a.reps)
    finally:
        g.close()
    doc = dict(what="orbgpu_covis_keyframe_culling and orbgpu_covis_observations: median of %d calls after a warm-up, HIP events "
                    "around the call (*_ms) and host clock (*_host_ms), one session, one MI355X" % a.reps,
               map=dict(key_frames=a.key_frames, slots_per_key_frame=a.slots, filled=0.4, candidates=int(len(cand)),
                        pool_bytes=9 * a.key_frames * a.slots, point_window=4 * a.slots, window_slide=a.slots // SLIDE, octaves="uniform 0-2", stereo=0.75, far_of_stereo=0.1, th_obs=3),
               culling_ms=cull[0], culling_host_ms=cull[1], query_points=int(first["n_query_points"]),
               culled=int(first["n_culled"]), skipped=int(first["n_skipped"]), bad_points=int(first["n_points_bad"]),
               verdicts=first["verdict"].tolist(), observations_ids=int(len(held)), observations_ms=obs[0], observations_host_ms=obs[1],
               not_measured="the reference's own KeyFrameCulling (it cannot be built here): its host cost is unmeasured and not "
                            "estimated; the Python model is no baseline")
    if a.no_trace:
        doc["kernel_share"] = "not measured (--no-trace)"
    else:
        ks = kernel_shares(a)
        if "error" in ks:
            doc["kernel_share"] = "not measured: " + ks["error"]
        else:
            total = sum(ks["total_ns"].values())
            doc["kernel_share"] = dict(
                how="rocprofv3 --kernel-trace --stats over %d culling calls in a child process of their own" % a.reps,
                per_call_us={k: ks["total_ns"][k] / max(ks["calls"][k], 1) / 1e3 for k in KERNELS},
                share_of_the_three_kernels={k: ks["total_ns"][k] / total if total else 0.0 for k in KERNELS})
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
