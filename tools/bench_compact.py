"""Times orbgpu_covis_graph_compact and orbgpu_keyframe_db_compact, and the queries before and after them.

usage: python tools/bench_compact.py [--out profiles/compact_bench.json] [--reps 30] [--runs 3] [--key-frames 5000]
                                     [--slots 2000] [--keep 5] [--points 3000] [--compact-reps 3] [--no-trace]

The map is tools/bench_cull.py's shape (a point is held by about eight key frames) scaled to a long run, with random
descriptors on every slot, centres and three scale levels; every key frame whose index is no multiple of --keep is then
set bad through the hooks of KeyFrame::SetBadFlag (the children to the next surviving parent, the flag) and erased from a
key-frame database of the same history (--words words per vector).  Three handles of each kind are queried: (1) bad rows
in place, (2) compacted, (3) a fresh handle that holds only the survivors -- the yardstick for (2).  The queries -- local_map,
connections, keyframe_culling, refresh_points over --points points, detect_reloc -- are timed with HIP events around the
call, 5 warm-ups, median of --reps, in --runs passes that alternate the three states.  The compaction itself is one-shot:
it is timed on --compact-reps graphs built for it, with hipMemGetInfo before and after; its kernel times come from a child
process of its own under `rocprofv3 --kernel-trace --stats` (--trace-child).  One JSON document; nothing here is a pass
criterion."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from orb_slam2_map_amd import lib as G  # noqa: E402
from bench_covis import timed  # noqa: E402
from bench_cull import SLIDE  # noqa: E402
from bench_kfdb import N_WORDS, draw, similar  # noqa: E402

KERNELS = ("k_compact_pool", "k_compact_rows", "k_compact_gather")
HBM_COPY_TBS = 6.29  # bytes read + written per second of a float4 copy on this part, as measured for the micro-architecture notes


def key_frame(a, k):
    """the content of key frame k, the same whenever it is asked for"""
    rng = np.random.default_rng([a.key_frames, a.slots, k])
    n = a.slots
    window, filled = 4 * n, int(0.4 * n)
    slots = np.full(n, -1, np.int64)
    slots[rng.choice(n, size=filled, replace=False)] = (k * (n // SLIDE) + rng.choice(window, size=filled, replace=False)).astype(np.int64)
    return slots, rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.random(3).astype(np.float32)


def add(g, a, k, parent, covisibles):
    slots, kp, desc, centre = key_frame(a, k)
    g.add_keyframe(k, a.slots, slots)
    g.set_keypoints(k, kp)
    g.set_descriptors(k, desc)
    g.set_centres([k], [centre])
    g.set_parent(k, parent)
    g.set_covisibles(k, covisibles)


def build_graph(a, culled):
    """every key frame, then -- if `culled` -- the hooks of SetBadFlag on those that do not survive"""
    g = G.CovisibilityGraph()  # default first sizes: the handle grows as on a long run, and C5 returns to those sizes
    g.set_scale_factors(np.float32(1.2) ** np.arange(3, dtype=np.float32))
    for k in range(a.key_frames):
        add(g, a, k, k - 1, [j for j in range(k - 1, max(k - 11, -1), -1)])
    if culled:
        for k in range(a.key_frames):
            if k % a.keep == 0:  # ChangeParent and UpdateBestCovisibles of a survivor
                g.set_parent(k, k - a.keep if k else -1)
                g.set_covisibles(k, [j for j in range(k - a.keep, max(k - 10 * a.keep - 1, -1), -a.keep)])
        g.set_bad([k for k in range(a.key_frames) if k % a.keep])
    return g


def build_survivors(a):
    g = G.CovisibilityGraph()
    g.set_scale_factors(np.float32(1.2) ** np.arange(3, dtype=np.float32))
    for k in range(0, a.key_frames, a.keep):
        add(g, a, k, k - a.keep if k else -1, [j for j in range(k - a.keep, max(k - 10 * a.keep - 1, -1), -a.keep)])
    return g


def vector(a, q, k):
    rng = np.random.default_rng([a.key_frames, a.words, k])
    return similar(rng, q, a.words, 0.33) if k % 10 == 0 else draw(rng, a.words)


def build_db(a, q, ids, erase):
    db = G.KeyFrameDatabase(N_WORDS)
    for k in ids:
        db.set_covisibles(k, [j for j in range(k - 5 * a.keep, k + 5 * a.keep + 1, a.keep) if j != k and 0 <= j < a.key_frames][:10])
        db.add(k, *vector(a, q, k))
    if erase:
        db.erase([k for k in ids if k % a.keep])
    return db


def timed_once(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def free_bytes():
    import torch
    return int(torch.cuda.mem_get_info()[0])


def kernel_times(a):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--key-frames", str(a.key_frames), "--slots", str(a.slots), "--keep", str(a.keep),
               "--words", str(a.words)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1100)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return dict(error="rocprofv3 run failed (exit %d): %s" % (r.returncode, r.stdout[-400:]))
        out = {}
        for row in csv.DictReader(open(files[0])):
            if any(k in row["Name"] for k in KERNELS):
                out[row["Name"].split("(")[0][-80:]] = dict(calls=int(row["Calls"]), total_us=float(row["TotalDurationNs"]) / 1e3)
        return dict(kernels=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--key-frames", type=int, default=5000)
    ap.add_argument("--slots", type=int, default=2000)
    ap.add_argument("--keep", type=int, default=5, help="every keep-th key frame survives")
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--compact-reps", type=int, default=3)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    q = draw(np.random.default_rng(20261021), a.words)
    every = list(range(a.key_frames))
    if a.trace_child:  # one compaction of each handle, so that the kernel totals are one call's
        g, db = build_graph(a, True), build_db(a, q, every, True)
        g.compact()
        db.compact()
        g.close()
        db.close()
        return
    # the compaction, one-shot: a graph and a database per repetition; the last ones are state (2)
    compactions = []
    for rep in range(a.compact_reps):
        if rep:
            g2.close()  # noqa: F821
            db2.close()  # noqa: F821
        g2, db2 = build_graph(a, True), build_db(a, q, every, True)
        torch.cuda.synchronize()
        f0 = free_bytes()
        res, ms, host_ms = timed_once(g2.compact)
        f1 = free_bytes()
        dres, dms, dhost_ms = timed_once(db2.compact)
        f2 = free_bytes()
        compactions.append(dict(graph=res, graph_ms=ms, graph_host_ms=host_ms, graph_freed_bytes=f1 - f0, database=dres,
                                database_ms=dms, database_host_ms=dhost_ms, database_freed_bytes=f2 - f1))
    g1, db1 = build_graph(a, True), build_db(a, q, every, True)
    g3, db3 = build_survivors(a), build_db(a, q, every[::a.keep], False)
    states = (("bad rows in place", g1, db1), ("compacted", g2, db2), ("fresh handle of the survivors", g3, db3))
    # the queries, the same for every state: they name survivors only
    last = (a.key_frames - 1) // a.keep * a.keep
    mid = a.key_frames // 2 // a.keep * a.keep
    rng = np.random.default_rng(7)
    held = key_frame(a, last)[0]
    held = held[held >= 0]
    kp = np.full(1000, -1, np.int64)
    kp[rng.choice(1000, size=300, replace=False)] = rng.choice(held, size=300)
    cand = np.arange(mid + 15 * a.keep, mid - 15 * a.keep, -a.keep, dtype=np.int64)
    cand = cand[(cand > 0) & (cand < a.key_frames)]
    pts, ref = [], []
    for k in range(mid, a.key_frames, a.keep):  # --points distinct points held by survivors, each with an observer as reference
        s = key_frame(a, k)[0]
        for p in s[s >= 0]:
            pts.append(int(p))
            ref.append(k)
        if len(set(pts)) >= a.points:
            break
    pts, first = np.unique(np.array(pts, np.int64), return_index=True)
    pts, ref = pts[:a.points], np.array(ref, np.int64)[first][:a.points]
    pos = (0.5 + 4.0 * np.random.default_rng(8).normal(size=(len(pts), 3))).astype(np.float32)
    answers, rows = [], []
    try:
        for name, g, db in states:
            lm = g.local_map(kp, [])
            cn = g.connections(last, 15)
            cu = g.keyframe_culling(cand)
            rf = g.refresh_points(pts, ref, pos)
            rl = db.DetectRelocalizationCandidates(*q)
            answers.append(dict(state=name, size=list(g.size()), database_size=db.size(), local_map_kfs=int(lm["n_kfs"]),
                                local_map_points=int(lm["n_points"]), connections=int(cn["n"]), culled=int(cu["n_culled"]),
                                refresh_entries=int(rf["n_entries"]), refresh_descriptors=int(rf["n_descriptors"]),
                                reloc_candidates=int(len(rl))))
        for run in range(a.runs):
            for name, g, db in states:
                caps = (answers[0]["local_map_kfs"], answers[0]["local_map_points"])
                row = dict(run=run, state=name)
                row["local_map_ms"] = timed(lambda: g.local_map(kp, [], *caps), a.reps)[0]
                row["connections_ms"] = timed(lambda: g.connections(last, 15), a.reps)[0]
                row["keyframe_culling_ms"] = timed(lambda: g.keyframe_culling(cand, None, 3, 0), a.reps)[0]
                row["refresh_points_ms"] = timed(lambda: g.refresh_points(pts, ref, pos), a.reps)[0]
                row["detect_reloc_ms"] = timed(lambda: db.DetectRelocalizationCandidates(*q), a.reps)[0]
                rows.append(row)
    finally:
        for _, g, db in states:
            g.close()
            db.close()
    same = all({k: v for k, v in x.items() if k not in ("state", "size")} == {k: v for k, v in answers[0].items() if k not in ("state", "size")}
               for x in answers)
    res = compactions[-1]["graph"]
    moved = 41 * res["slots_after"]
    doc = dict(what="orbgpu_covis_graph_compact / orbgpu_keyframe_db_compact and the queries in three states: median of %d calls after 5 "
                    "warm-ups, HIP events around the call, %d passes alternating the states, one session, one MI355X" % (a.reps, a.runs),
               map=dict(key_frames=a.key_frames, slots_per_key_frame=a.slots, filled=0.4, window_slide=a.slots // SLIDE,
                        survivors="every %d-th key frame" % a.keep, descriptors="random bytes", words_per_vector=a.words,
                        refresh_points=int(len(pts)), culling_candidates=int(len(cand))),
               rows_dropped_share=1.0 - res["rows_after"] / max(res["rows_before"], 1),
               slots_dropped_share=1.0 - res["slots_after"] / max(res["slots_before"], 1),
               the_three_states_answer_alike=bool(same), answers=answers, queries=rows, compactions=compactions,
               graph_pool_bytes_moved=dict(read=moved, written=moved))
    if a.no_trace:
        doc["kernels"] = "not measured (--no-trace)"
    else:
        kt = kernel_times(a)
        if "error" in kt:
            doc["kernels"] = "not measured: " + kt["error"]
        else:
            pool_us = sum(v["total_us"] for k, v in kt["kernels"].items() if "k_compact_pool" in k and "32" in k)  # <8, 1, 32>: the graph's
            doc["kernels"] = dict(how="rocprofv3 --kernel-trace --stats over one compaction of each handle in a child process of its own",
                                  graph_pool_copy_share_of_hbm_copy_rate=(2 * moved / (pool_us * 1e-6) / (HBM_COPY_TBS * 1e12)) if pool_us else None,
                                  hbm_copy_rate_tbs=HBM_COPY_TBS, **kt)
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
