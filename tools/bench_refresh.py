"""Times orbgpu_covis_refresh_points and orbgpu_mappoint_table_refresh on tools/bench_cull.py's map, and the route the
library offered before them for the same work.

usage: python tools/bench_refresh.py [--out profiles/refresh_bench.json] [--reps 30] [--key-frames 500] [--slots 2000]
                                     [--points 3000] [--no-trace]

The map is bench_cull.plant's (a point is held by about eight key frames) with random descriptors on every slot, centres in
a unit cube, three scale levels and points 2 to 6 units away.  Two call sizes: --points consecutive held points from the
middle of the map (a local bundle adjustment's write-back) and every held point (a global one's).  Two forms: the host form
with every output, and the table form with none (the results stay in the MapPoint table).  The comparison route is what a
caller could do before: per point the observation list from a host mirror (CSR arrays in R1's order, built outside the
timing, standing for MapPoint::mObservations), a numpy gather of the descriptor rows, orbgpu_distinctive_descriptors, the
normals and distances in vectorised numpy (FP64 sums: the same work, not the same bits) and orbgpu_mappoint_table_upsert.
Calls are timed with HIP events around the call and with the host clock, 5 warm-ups, median of --reps.  Per-kernel times
come from a child process of its own under `rocprofv3 --kernel-trace --stats` (--trace-child).  ORBGPU_DEBUG_REFRESH_SELECT=
rows in the environment selects the stored distance row in the one-wave kernel; the document records which ran.  One JSON
document; nothing here is a pass criterion."""
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
from bench_cull import SLIDE  # noqa: E402

KERNELS = ("k_covis_cull_count", "k_covis_refresh_scan", "k_covis_refresh_fill", "k_covis_refresh<64", "k_covis_refresh<256",
           "k_table_refresh_gather")


def scene(a):
    """bench_cull.plant with the slots kept on the host, plus the three columns; returns the graph and the host mirror"""
    rng = np.random.default_rng(a.key_frames + a.slots)
    n_kf, n_slots = a.key_frames, a.slots
    g = G.CovisibilityGraph(initial_rows=n_kf, initial_slots=n_kf * n_slots)
    window, filled = 4 * n_slots, int(0.4 * n_slots)
    slots = np.full((n_kf, n_slots), -1, np.int64)
    desc = rng.integers(0, 256, (n_kf, n_slots, 32), dtype=np.uint8)
    octave = rng.integers(0, 3, (n_kf, n_slots)).astype(np.uint8)
    centres = rng.random((n_kf, 3)).astype(np.float32)
    for k in range(n_kf):
        pts = (k * (n_slots // SLIDE) + rng.choice(window, size=filled, replace=False)).astype(np.int64)
        slots[k, rng.choice(n_slots, size=filled, replace=False)] = pts
        g.add_keyframe(k, n_slots, slots[k])
        g.set_keypoints(k, octave[k])
        g.set_descriptors(k, desc[k])
    g.set_centres(np.arange(n_kf), centres)
    sf = (np.float32(1.2) ** np.arange(3, dtype=np.float32)).astype(np.float32)
    g.set_scale_factors(sf)
    # the mirror: observations in R1's order (ascending point, key frame, index) as CSR
    kf_of, idx_of = np.nonzero(slots >= 0)
    pid = slots[kf_of, idx_of]
    order = np.lexsort((idx_of, kf_of, pid))
    kf_of, idx_of, pid = kf_of[order], idx_of[order], pid[order]
    held, start = np.unique(pid, return_index=True)
    n_pts = int(held.max()) + 1
    first = np.full(n_pts + 1, 0, np.int64)
    count = np.zeros(n_pts, np.int64)
    count[held] = np.diff(np.append(start, len(pid)))
    first[1:] = np.cumsum(count)
    v = rng.normal(size=(n_pts, 3))
    pos = (0.5 + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(2.0, 6.0, (n_pts, 1))).astype(np.float32)
    ref = np.zeros(n_pts, np.int64)
    ref[held] = kf_of[start]  # mpRefKF: the first observer
    mirror = dict(kf=kf_of, idx=idx_of, first=first, count=count, desc=desc.reshape(-1, 32), octave=octave.reshape(-1), centres=centres,
                  sf=sf, n_slots=n_slots, pos=pos, ref=ref, held=held)
    return g, mirror


def previous_route(table, m, ids):
    """host gather + orbgpu_distinctive_descriptors + numpy normals + upsert"""
    cnt = m["count"][ids]
    off = np.zeros(len(ids) + 1, np.int32)
    off[1:] = np.cumsum(cnt)
    take = np.repeat(m["first"][ids] - off[:-1], cnt) + np.arange(off[-1])
    kf, idx = m["kf"][take], m["idx"][take]
    flat = np.ascontiguousarray(m["desc"][kf * m["n_slots"] + idx])
    best = np.zeros(len(ids), np.int32)
    G.check(G.lib().orbgpu_distinctive_descriptors(len(ids), G._p(off), G._p(flat), G._p(best), 0))
    chosen = flat[off[:-1] + best]
    d = np.repeat(m["pos"][ids], cnt, axis=0) - m["centres"][kf]
    nrm = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
    normal = (np.add.reduceat(d / nrm[:, None], off[:-1], axis=0) / cnt[:, None]).astype(np.float32)
    is_ref = kf == np.repeat(m["ref"][ids], cnt)
    at = np.minimum.reduceat(np.where(is_ref, np.arange(len(kf)), len(kf)), off[:-1])
    level = m["octave"][kf[at] * m["n_slots"] + idx[at]]
    mx = (nrm[at].astype(np.float32) * m["sf"][level]).astype(np.float32)
    table.upsert(ids, None, normal, (mx / m["sf"][-1]).astype(np.float32), mx, chosen)


def kernel_times(a):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--reps", str(a.reps), "--key-frames", str(a.key_frames),
               "--slots", str(a.slots), "--points", str(a.points)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return dict(error="rocprofv3 run failed (exit %d): %s" % (r.returncode, r.stdout[-400:]))
        ns, calls = {k: 0.0 for k in KERNELS}, {k: 0 for k in KERNELS}
        for row in csv.DictReader(open(files[0])):
            for k in KERNELS:
                if k in row["Name"]:
                    ns[k] += float(row["TotalDurationNs"])
                    calls[k] += int(row["Calls"])
        return dict(per_call_us={k: ns[k] / max(calls[k], 1) / 1e3 for k in KERNELS}, calls=calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refresh_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--key-frames", type=int, default=500)
    ap.add_argument("--slots", type=int, default=2000)
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    g, m = scene(a)
    table = G.MapPointTable(initial_rows=len(m["held"]))
    try:
        held = m["held"]
        mid = len(held) // 2
        local = np.ascontiguousarray(held[max(mid - a.points // 2, 0):mid + (a.points + 1) // 2])
        if a.trace_child:  # the host form of the local size only, so that the kernel totals divide by the calls
            for _ in range(a.reps):
                g.refresh_points(local, m["ref"][local], m["pos"][local])
            return
        table.upsert(held, m["pos"][held], np.zeros((len(held), 3), np.float32), np.zeros(len(held), np.float32),
                     np.zeros(len(held), np.float32), np.zeros((len(held), 32), np.uint8))
        rows = []
        for name, ids in (("local", local), ("all", held)):
            first = g.refresh_points(ids, m["ref"][ids], m["pos"][ids])
            host = timed(lambda: g.refresh_points(ids, m["ref"][ids], m["pos"][ids]), a.reps)
            tab = timed(lambda: table.refresh(g, ids, m["ref"][ids]), a.reps)
            prev = timed(lambda: previous_route(table, m, ids), a.reps)
            rows.append(dict(call=name, points=int(len(ids)), entries=int(first["n_entries"]), max_obs=int(first["max_obs"]),
                             n_descriptors=int(first["n_descriptors"]), n_normals=int(first["n_normals"]),
                             host_form_ms=host[0], host_form_host_ms=host[1], table_form_ms=tab[0], table_form_host_ms=tab[1],
                             previous_route_ms=prev[0], previous_route_host_ms=prev[1]))
    finally:
        table.close()
        g.close()
    doc = dict(what="orbgpu_covis_refresh_points (host form, every output) and orbgpu_mappoint_table_refresh (table form, no host "
                    "output): median of %d calls after 5 warm-ups, HIP events around the call (*_ms) and host clock (*_host_ms), one "
                    "session, one MI355X" % a.reps,
               selection="stored distance row" if os.environ.get("ORBGPU_DEBUG_REFRESH_SELECT") == "rows" else "bisection, distances recomputed",
               map=dict(key_frames=a.key_frames, slots_per_key_frame=a.slots, filled=0.4, held_points=int(len(m["held"])),
                        window_slide=a.slots // SLIDE, levels=3, descriptors="random bytes"),
               calls=rows,
               previous_route="observation lists from a host CSR mirror built outside the timing, numpy gather of the descriptor rows, "
                              "orbgpu_distinctive_descriptors, numpy normals (FP64 sums: the same work, not the same bits), "
                              "orbgpu_mappoint_table_upsert",
               not_measured="the reference's own per-object loop (ComputeDistinctiveDescriptors + UpdateNormalAndDepth per MapPoint: a "
                            "std::map copy under a mutex and one cv::Mat clone per observer) cannot be built here; it is unmeasured "
                            "and not estimated")
    if a.no_trace:
        doc["kernels"] = "not measured (--no-trace)"
    else:
        kt = kernel_times(a)
        doc["kernels"] = "not measured: " + kt["error"] if "error" in kt else dict(
            how="rocprofv3 --kernel-trace --stats over %d host-form calls of the local size in a child process of their own" % a.reps, **kt)
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
