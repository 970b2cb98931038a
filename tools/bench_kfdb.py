"""Milliseconds per query of the device KeyFrameDatabase (orbgpu_keyframe_db_detect_loop / _detect_reloc).

usage: python tools/bench_kfdb.py [--out profiles/kfdb_bench.json] [--sizes 100,1000,5000] [--words 1000]

Databases of 100 / 1000 / 5000 key frames of about 1000 words each (vocabulary of 10^6 words, like ORBvoc), a query of
about 1000 words; one key frame in ten is a "similar place" sharing about a third of the query's words, the others share
what chance gives.  Every key frame names its ten nearest ids as covisible.  Each figure: HIP events around the call (the
call returns synchronised, so this is the caller's latency), 5 warm-up calls, median of 50.  Beside it the bound the
design implies: the pool streamed once at 12 bytes per entry, at the copy bandwidth measured on the same device."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam2_map_amd import lib as G  # noqa: E402

N_WORDS = 1000000
WARMUP, REPS = 5, 50


def draw(rng, n):
    ids = np.unique(rng.integers(0, N_WORDS, n + n // 16))[:n].astype(np.int32)
    vals = rng.uniform(0.05, 1.0, len(ids))
    return ids, vals / vals.sum()


def similar(rng, q, n, share):
    keep = rng.choice(len(q[0]), size=int(share * len(q[0])), replace=False)
    own = draw(rng, n - len(keep))
    ids, first = np.unique(np.concatenate([q[0][keep], own[0]]), return_index=True)
    vals = np.concatenate([q[1][keep] * rng.uniform(0.5, 1.5, len(keep)), own[1]])[first]
    return ids.astype(np.int32), vals / vals.sum()


def build(rng, n_kf, words, q):
    db = G.KeyFrameDatabase(N_WORDS, initial_rows=n_kf)
    entries = 0
    for i in range(n_kf):
        v = similar(rng, q, words, 0.33) if i % 10 == 0 else draw(rng, words)
        db.set_covisibles(i, [j for j in range(i - 5, i + 6) if j != i and 0 <= j < n_kf][:10])
        db.add(i, *v)
        entries += len(v[0])
    return db, entries


def time_call(torch, call):
    for _ in range(WARMUP):
        call()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfdb_bench.json"))
    ap.add_argument("--sizes", default="100,1000,5000")
    ap.add_argument("--words", type=int, default=1000)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    rng = np.random.default_rng(20261018)
    copy_gbs = G.measure_copy_bandwidth(1 << 30, 5)  # bytes read + written per second
    read_gbs = copy_gbs / 2.0
    rows = []
    for n_kf in (int(x) for x in a.sizes.split(",")):
        q = draw(rng, a.words)
        db, entries = build(rng, n_kf, a.words, q)
        conn = list(range(0, n_kf, 97))[:20]
        n_loop = len(db.DetectLoopCandidates(q[0], q[1], conn, 0.01))
        n_reloc = len(db.DetectRelocalizationCandidates(*q))
        sharing = len(db.last_query()["id"])
        loop_ms = time_call(torch, lambda: db.DetectLoopCandidates(q[0], q[1], conn, 0.01))
        reloc_ms = time_call(torch, lambda: db.DetectRelocalizationCandidates(*q))
        score_ms = time_call(torch, lambda: db.score(q[0], q[1], conn))
        pool_bytes = 12 * entries
        bound_ms = pool_bytes / (read_gbs * 1e9) * 1e3
        rows.append(dict(key_frames=n_kf, words_per_key_frame=a.words, query_words=len(q[0]), pool_bytes=pool_bytes,
                         sharing_rows=sharing, loop_candidates=n_loop, reloc_candidates=n_reloc,
                         detect_loop_ms_median=loop_ms[0], detect_loop_ms_min=loop_ms[1], detect_reloc_ms_median=reloc_ms[0],
                         detect_reloc_ms_min=reloc_ms[1], score_20_ids_ms_median=score_ms[0], stream_bound_ms=bound_ms,
                         reloc_over_bound=reloc_ms[0] / bound_ms))
        print(json.dumps(rows[-1]))
        db.close()
    out = dict(tool="tools/bench_kfdb.py", timing="HIP events around the call; %d warm-up calls, median of %d" % (WARMUP, REPS),
               copy_bandwidth_gbs=copy_gbs, read_bandwidth_gbs_assumed=read_gbs,
               bound="pool streamed once: 12 bytes per entry / read bandwidth", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
