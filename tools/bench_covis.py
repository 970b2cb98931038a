"""Times orbgpu_covis_local_map and orbgpu_covis_connections and sets them beside the stream bound.

usage: python tools/bench_covis.py [--out profiles/covis_bench.json] [--reps 50] [--sizes 100,1000,5000] [--slots 1000,2000]

For every (key frames, slots per key frame) a map is planted: each key frame holds points on 40 % of its slots, drawn
from a window of the point ids that slides with the key frame (neighbours share points, far key frames do not), parents
form a chain, covisibles are the ten nearest earlier key frames.  The frame holds about 300 points of the newest key
frames.  Each call is timed with HIP events on the current stream (the calls return synchronised) and with the host clock,
after a warm-up, median of --reps; a batched set_slots of one key frame is timed the same way.  The bound is the pool's
bytes over the read rate orbgpu_measure_copy_bandwidth reaches in the same run (its figure counts bytes read + written, so
the read rate is half of it).  One JSON document; nothing here is a pass criterion."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam2_map_amd import lib as G  # noqa: E402


def plant(g, n_kf, n_slots, rng):
    window = 4 * n_slots
    filled = int(0.4 * n_slots)
    last = None
    for k in range(n_kf):
        slots = np.full(n_slots, -1, np.int64)
        pts = (k * (n_slots // 8) + rng.choice(window, size=filled, replace=False)).astype(np.int64)
        slots[rng.choice(n_slots, size=filled, replace=False)] = pts
        g.add_keyframe(k, n_slots, slots)
        g.set_parent(k, k - 1)
        g.set_covisibles(k, [j for j in range(k - 1, max(k - 11, -1), -1)])
        last = slots
    return last


def timed(fn, reps, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    dev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    return float(np.median(dev)), float(np.median(host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covis_bench.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", default="100,1000,5000")
    ap.add_argument("--slots", default="1000,2000")
    a = ap.parse_args()
    gbs = G.measure_copy_bandwidth(1 << 30, 10)
    read_gbs = gbs / 2.0
    rows = []
    for n_slots in [int(x) for x in a.slots.split(",")]:
        for n_kf in [int(x) for x in a.sizes.split(",")]:
            rng = np.random.default_rng(n_kf + n_slots)
            g = G.CovisibilityGraph(initial_rows=n_kf, initial_slots=n_kf * n_slots)
            try:
                t0 = time.perf_counter()
                last = plant(g, n_kf, n_slots, rng)
                t_plant = time.perf_counter() - t0
                held = last[last >= 0]
                kp = np.full(1000, -1, np.int64)
                kp[rng.choice(1000, size=300, replace=False)] = rng.choice(held, size=300)
                first = g.local_map(kp, [])
                caps = (first["n_kfs"], first["n_points"])
                prev = first["kf_ids"]
                lm = timed(lambda: g.local_map(kp, prev, *caps), a.reps)
                con = g.connections(n_kf - 1, 15)
                cn = timed(lambda: g.connections(n_kf - 1, 15, n_kf, n_kf), a.reps)
                idx = np.flatnonzero(last >= 0).astype(np.int32)
                ss = timed(lambda: g.set_slots(np.full(len(idx), n_kf - 1, np.int64), idx, last[idx]), a.reps)
                pool_bytes = 8 * n_kf * n_slots
                rows.append(dict(key_frames=n_kf, slots_per_key_frame=n_slots, pool_bytes=pool_bytes,
                                 stream_bound_ms=pool_bytes / (read_gbs * 1e9) * 1e3,
                                 local_map_ms=lm[0], local_map_host_ms=lm[1], local_kfs=int(first["n_kfs"]),
                                 local_points=int(first["n_points"]), voted=int(first["n_voted"]),
                                 connections_ms=cn[0], connections_host_ms=cn[1], connected=int(con["n"]),
                                 set_slots_entries=int(len(idx)), set_slots_ms=ss[0], set_slots_host_ms=ss[1],
                                 plant_s=t_plant))
                print(json.dumps(rows[-1]), flush=True)
            finally:
                g.close()
    doc = dict(what="orbgpu_covis_local_map / orbgpu_covis_connections / batched set_slots of one key frame: median of %d "
                    "calls after a warm-up, HIP events around the call (*_ms) and host clock (*_host_ms), one session, one "
                    "MI355X" % a.reps,
               copy_bandwidth_gbs=gbs, read_rate_gbs=read_gbs,
               not_measured="the reference's own UpdateLocalMap / UpdateConnections (they cannot be built here): their host "
                            "cost is unmeasured and not estimated; the Python model is no baseline",
               rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
