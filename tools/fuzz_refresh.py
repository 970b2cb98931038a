"""Randomised comparison of the device refresh of MapPoint descriptor, normal and depth (orbgpu_covis_refresh_points,
orbgpu_mappoint_table_refresh and the three columns orbgpu_covis_graph_set_scale_factors / _set_descriptors / _set_centres
fill) with the CPU model (tests/refresh_model.py).

usage: python tools/fuzz_refresh.py SECONDS SEED

Each round creates a graph (initial rows and slots drawn, sometimes with the queries forced through global memory), plants
key frames of the edge sizes over shared points -- some without descriptors, some without a centre, sometimes no scale table
-- and a MapPoint table that holds most of the points, some flagged bad.  Then refreshes in both forms (random subsets in
random order, each half alone and both, unknown and bad references, in/out arrays that start from random bytes) alternate
with edits (set_slots, set_bad, moved centres, new key frames, a new scale table), refused calls and local_map queries
(the graph must be what it was).  Every output, and every row of the table, must equal the model's bit for bit.  Exit
status 1 on any mismatch."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import covis_model as M  # noqa: E402
import refresh_model as RM  # noqa: E402
import fuzz_cull  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402


class RefreshPair(fuzz_cull.CullPair):
    """fuzz_cull.CullPair whose table model is refresh_model.RefreshGraph, with the new calls"""

    def __init__(self, initial_rows=0, initial_slots=0):
        super().__init__(initial_rows, initial_slots)
        self.model = RM.RefreshGraph()

    def set_scale_factors(self, scale_factors):
        return self._raise(self._edit("set_scale_factors", scale_factors))

    def set_descriptors(self, kf_id, desc):
        return self._raise(self._edit("set_descriptors", kf_id, desc))

    def set_centres(self, kf_ids, centres):
        return self._raise(self._edit("set_centres", kf_ids, centres))

    def refresh(self, mp_ids, ref_kf_ids, world_pos, what=3, initial=None):
        err, got, want = self._both("refresh_points", lambda: self.dev.refresh_points(mp_ids, ref_kf_ids, world_pos, what, initial=initial),
                                    lambda: self.model.refresh(mp_ids, ref_kf_ids, world_pos, what, initial))
        return err if err or want is None else RM.compare(got, want)

    def refresh_table(self, table, mirror, mp_ids, ref_kf_ids, what=3, initial=None, outputs=G.REFRESH_OUTPUTS):
        """the table form; `mirror` (id -> dict of world_pos, normal, min_dist, max_dist, desc, bad) is what the table's rows
        hold and is updated with the model's results; every listed row is read back and compared"""
        ids = [int(p) for p in mp_ids]
        pre = [RM.UNKNOWN if p not in mirror else RM.BAD if mirror[p]["bad"] else 0 for p in ids]
        pos = np.array([mirror[p]["world_pos"] if p in mirror else np.zeros(3, np.float32) for p in ids], np.float32).reshape(-1, 3)
        err, got, want = self._both("table refresh", lambda: table.refresh(self.dev, ids, ref_kf_ids, what, outputs, initial),
                                    lambda: self.model.refresh(ids, ref_kf_ids, pos, what, initial, pre))
        if err or want is None:
            return err
        err = RM.compare(got, want)
        # what the rows must hold now: the model's values where it wrote, the mirror's otherwise
        rows =self.model.refresh(ids, ref_kf_ids, pos, what, dict(
            normal=[mirror.get(p, ZERO)["normal"] for p in ids], min_dist=[mirror.get(p, ZERO)["min_dist"] for p in ids],
            max_dist=[mirror.get(p, ZERO)["max_dist"] for p in ids], desc=[mirror.get(p, ZERO)["desc"] for p in ids]), pre)
        for i, p in enumerate(ids):
            if err or p not in mirror:
                continue
            for name in ("normal", "min_dist", "max_dist", "desc"):
                mirror[p][name] = np.array(rows[name][i])
            r = table.read(p)
            for name in ("world_pos", "normal", "min_dist", "max_dist", "desc"):
                a = np.atleast_1d(np.asarray(r[name], mirror[p][name].dtype)).view(np.uint8)
                if not np.array_equal(a, np.atleast_1d(mirror[p][name]).view(np.uint8)):
                    err = "table row of point %d, %s: %s, model %s (status 0x%x)" % (p, name, r[name], mirror[p][name], want["status"][i])
            if r["bad"] != mirror[p]["bad"]:
                err = "table row of point %d: bad flag %d" % (p, r["bad"])
        return err


ZERO = dict(normal=np.zeros(3, np.float32), min_dist=np.float32(0), max_dist=np.float32(0), desc=np.zeros(32, np.uint8))


def fill_table(rng, table, ids, pos, n_bad=0):
    """upserts the points with random attributes and flags the first n_bad of a random order; returns the mirror"""
    ids = [int(p) for p in ids]
    j = RM.junk(rng, len(ids))
    table.upsert(ids, pos, j["normal"], j["min_dist"], j["max_dist"], j["desc"], np.ones(len(ids), np.int32))
    mirror = {p: dict(world_pos=np.array(pos[i], np.float32), normal=j["normal"][i], min_dist=j["min_dist"][i],
                      max_dist=j["max_dist"][i], desc=j["desc"][i], bad=0) for i, p in enumerate(ids)}
    bad = [ids[int(i)] for i in rng.permutation(len(ids))[:n_bad]]
    if bad:
        table.set_bad(bad)
        for p in bad:
            mirror[p]["bad"] = 1
    return mirror


def refused_call(rng, pair, kf_ids):
    k = kf_ids[int(rng.integers(len(kf_ids)))]
    n = len(pair.model.row_of[k].slots)
    kind = int(rng.integers(7))
    if kind == 0:
        return pair._edit("set_descriptors", 10 ** 12 + 1, np.zeros((1, 32), np.uint8))
    if kind == 1:
        return pair._edit("set_descriptors", k, np.zeros((n + 1, 32), np.uint8))
    if kind == 2:
        return pair._edit("set_scale_factors", [1.0, float(rng.choice([0.0, -1.0, np.nan, np.inf]))])
    if kind == 3:
        return pair._edit("set_scale_factors", np.ones(int(rng.choice([0, 17]))))
    if kind == 4:
        return pair.refresh([3, 3], [k, k], np.zeros((2, 3)))
    if kind == 5:
        return pair.refresh([3, -1], [k, k], np.zeros((2, 3)))
    return pair.refresh([3], [k], np.zeros((1, 3)), int(rng.choice([0, 4, 8])))


def one_round(rng, counts):
    if rng.random() < 0.3:
        os.environ["ORBGPU_DEBUG_COVIS_LDS_IDS"] = str(int(rng.choice([0, 1, 8])))
    else:
        os.environ.pop("ORBGPU_DEBUG_COVIS_LDS_IDS", None)
    pair = RefreshPair(initial_rows=int(rng.choice([0, 2, 2, 16])), initial_slots=int(rng.choice([0, 8, 64])))
    table = G.MapPointTable(initial_rows=int(rng.choice([0, 8])))
    errs = []

    def count(op):
        counts[op] = counts.get(op, 0) + 1
    try:
        n_levels = int(rng.integers(1, 9))
        n_kf, n_slots, n_pts = int(rng.integers(2, 20)), int(rng.choice(M.SLOT_SIZES[1:])), int(rng.integers(5, 80))
        try:
            kf_ids, pts, pos, ref = RM.base_scene(rng, pair, n_kf, n_slots, n_pts, max_obs=min(n_kf, 12), first_kf=int(rng.integers(0, 2 ** 40)),
                                                  n_levels=n_levels, descriptors=rng.random() < 0.9, centres=rng.random() < 0.9,
                                                  scale=rng.random() < 0.9)
        except AssertionError as e:
            return ["planting: %s" % e]
        known =[p for p in pts if rng.random() < 0.9] or pts[:1]
        mirror = fill_table(rng, table, known, pos[known], n_bad=int(rng.integers(0, 3)))
        next_kf = max(kf_ids) + 1
        for step in range(int(rng.integers(6, 30))):
            u = rng.random()
            try:
                sel = [pts[int(i)] for i in rng.permutation(len(pts))[:int(rng.integers(0, len(pts) + 1))]]
                refs = [ref[p] if rng.random() < 0.9 else int(rng.choice([kf_ids[0], 10 ** 13])) for p in sel]
                what = int(rng.choice([1, 2, 3, 3]))
                if u < 0.35:
                    extra = [10 ** 9 + step] if rng.random() < 0.3 else []  # a point held nowhere
                    op, err = "refresh", pair.refresh(sel + extra, refs + kf_ids[:len(extra)], np.concatenate([pos[sel], np.ones((len(extra), 3), np.float32)]),
                                                      what, RM.junk(rng, len(sel) + len(extra)))
                elif u < 0.60:
                    extra = [10 ** 9 + step] if rng.random() < 0.3 else []  # a point the table does not know
                    outputs = G.REFRESH_OUTPUTS if rng.random() < 0.5 else ()
                    op, err = "table_refresh", pair.refresh_table(table, mirror, sel + extra, refs + kf_ids[:len(extra)], what,
                                                                  RM.junk(rng, len(sel) + len(extra)) if outputs else None, outputs)
                elif u < 0.68:
                    op, err = "refused", refused_call(rng, pair, kf_ids)
                elif u < 0.76:
                    some = [kf_ids[int(i)] for i in rng.integers(0, len(kf_ids), int(rng.integers(1, 6)))] + [10 ** 13]
                    op, err = "set_centres", pair.set_centres(some, rng.random((len(some), 3)).astype(np.float32))
                elif u < 0.84:
                    k = kf_ids[int(rng.integers(len(kf_ids)))]
                    m = int(rng.integers(1, 5))
                    op, err = "set_slots", pair.set_slots([k] * m, rng.integers(0, n_slots, m), [int(rng.choice(pts + [-1])) for _ in range(m)])
                elif u < 0.88:
                    op, err = "set_bad", pair.set_bad([kf_ids[int(rng.integers(len(kf_ids)))]])
                elif u < 0.92:
                    op, err = "set_scale_factors", pair.set_scale_factors(np.float32(rng.uniform(1.05, 1.5)) ** np.arange(int(rng.integers(1, 17)), dtype=np.float32))
                elif u < 0.96:
                    op = "add_keyframe"
                    err = pair.add_keyframe(next_kf, n_slots, [int(rng.choice(pts + [-1])) for _ in range(n_slots)])
                    pair.set_keypoints(next_kf, rng.integers(0, n_levels, n_slots).astype(np.uint8))
                    if rng.random() < 0.8:
                        pair.set_descriptors(next_kf, RM.PATTERNS[rng.integers(0, len(RM.PATTERNS), n_slots)])
                    if rng.random() < 0.8:
                        pair.set_centres([next_kf], rng.random((1, 3)).astype(np.float32))
                    kf_ids.append(next_kf)
                    next_kf += int(rng.integers(1, 5))
                else:
                    op, err = "local_map", pair.local_map(sel[:40], [])
            except AssertionError as e:
                op, err = "hook", str(e)
            count(op)
            if err:
                errs.append("step %d (%s): %s" % (step, op, err))
                break
        if not errs and pair.size():
            errs.append(pair.size())
    finally:
        table.close()
        pair.close()
        os.environ.pop("ORBGPU_DEBUG_COVIS_LDS_IDS", None)
    return errs


def run(seconds, seed):
    rng = np.random.default_rng(seed)
    counts, errs, rounds = {}, [], 0
    t_end = time.time() + seconds
    while True:
        errs += one_round(rng, counts)
        rounds += 1
        if errs or time.time() >= t_end:
            return rounds, counts, errs


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    t0 = time.time()
    rounds, counts, errs = run(seconds, seed)
    for e in errs[:20]:
        print("MISMATCH " + e)
    print("%s %d rounds, %d refreshes, %d table refreshes, %d refused calls, %d other calls in %.1f s (seed %d; vs "
          "tests/refresh_model.py, bit for bit)" % (
              "fuzz FAILED" if errs else "fuzz ok", rounds, counts.get("refresh", 0), counts.get("table_refresh", 0), counts.get("refused", 0),
              sum(v for k, v in counts.items() if k not in ("refresh", "table_refresh", "refused")), time.time() - t0, seed))
    sys.exit(1 if errs else 0)


if __name__ == "__main__":
    main()
