"""Randomised comparison of the device key-frame culling (orbgpu_covis_keyframe_culling, orbgpu_covis_observations,
orbgpu_covis_graph_set_keypoints) with the CPU model (tests/cull_model.py).

usage: python tools/fuzz_cull.py SECONDS SEED

Each round creates a graph (initial rows and slots drawn, sometimes with the counting query forced through global memory)
and plants a random map through the model's pointer map, whose hooks go to the device and to the table model alike: key
frames of the edge sizes with random octaves, stereo and far flags.  Then culling calls with random candidate lists (id 0,
unknown ids, bad rows, duplicates, not_erase flags, thresholds, capacities) alternate with observation queries, refused
calls, local_map / connections queries (the graph must be what it was) and the reference's own KeyFrameCulling on the
pointer map, whose SetBadFlag hooks edit both graphs.  Every output must equal the model's.  Exit status 1 on any mismatch."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import covis_model as M  # noqa: E402
import cull_model as CM  # noqa: E402
import fuzz_covis  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402

RESULT_FIELDS = ("n_culled", "n_to_be_erased", "n_skipped", "n_points_bad", "n_query_points")


class CullPair(fuzz_covis.Pair):
    """fuzz_covis.Pair whose table model is cull_model.CullGraph, with the three new calls"""

    def __init__(self, initial_rows=0, initial_slots=0):
        super().__init__(initial_rows, initial_slots)
        self.model = CM.CullGraph()

    def set_keypoints(self, kf_id, kp):
        return self._raise(self._edit("set_keypoints", kf_id, kp))

    def observations(self, mp_ids):
        err, got, want = self._both("observations", lambda: self.dev.observations(mp_ids), lambda: self.model.observations(mp_ids))
        if err or want is None:
            return err
        for name, g, w in zip(("n_obs", "n_slots"), got, want):
            if not np.array_equal(g, w):
                return "observations %s: %s, model %s" % (name, g[:12], w[:12])
        return ""

    def keyframe_culling(self, kf_ids, not_erase=None, th_obs=3, point_capacity=None):
        err, got, want = self._both("keyframe_culling", lambda: self.dev.keyframe_culling(kf_ids, not_erase, th_obs, point_capacity),
                                    lambda: self.model.keyframe_culling(kf_ids, not_erase, th_obs))
        if err or want is None:
            return err
        for k in RESULT_FIELDS:
            if got[k] != want[k]:
                return "keyframe_culling %s: %s, model %s" % (k, got[k], want[k])
        for k in ("verdict", "n_mps", "n_redundant"):
            if not np.array_equal(got[k], want[k]):
                return "keyframe_culling %s: %s, model %s" % (k, got[k][:16], want[k][:16])
        w = want["bad_point_ids"] if point_capacity is None else want["bad_point_ids"][:point_capacity]
        if not np.array_equal(got["bad_point_ids"], w):
            return "keyframe_culling bad_point_ids: %s, model %s" % (got["bad_point_ids"][:12], w[:12])
        return ""


def refused_call(rng, pair, pm):
    """a call both sides must refuse, or ignore -- and that changes nothing"""
    kfs = list(pm.kfs.values())
    kf = kfs[int(rng.integers(len(kfs)))]
    kind = int(rng.integers(8))
    if kind == 0:
        return pair._edit("set_keypoints", 10 ** 12 + 1, [0])
    if kind == 1:
        return pair._edit("set_keypoints", kf.mnId, [0] * (kf.N + 1))
    if kind == 2:
        return pair._edit("set_keypoints", kf.mnId, [0] * (kf.N - 1) + [int(rng.choice([0x10, 0x20, 0x31]))]) if kf.N else ""
    if kind == 3:
        return pair.observations([5, -2])
    if kind == 4:
        return pair.keyframe_culling([kf.mnId, -1])
    if kind == 5:
        return pair.keyframe_culling([kf.mnId], None, int(rng.choice([0, 256, -3])))
    if kind == 6 and kf.mbBad:
        return pair._edit("set_keypoints", kf.mnId, [CM.KP_FAR] * kf.N)  # a bad row ignores the call
    return pair._edit("set_keypoints", kf.mnId, pm.keypoint_bytes(kf))  # the same row again


def one_round(rng, counts):
    if rng.random() < 0.3:
        os.environ["ORBGPU_DEBUG_COVIS_LDS_IDS"] = str(int(rng.choice([0, 1, 8])))
    else:
        os.environ.pop("ORBGPU_DEBUG_COVIS_LDS_IDS", None)
    pair = CullPair(initial_rows=int(rng.choice([0, 2, 2, 16])), initial_slots=int(rng.choice([0, 8, 64])))
    pm = CM.CullPointerMap(pair, mbMonocular=bool(rng.random() < 0.4))
    errs = []
    try:
        try:
            kfs = CM.random_map(rng, pm, n_kf=int(rng.integers(3, 25)), n_pts=int(rng.integers(10, 120)))
            counts["add_keyframe"] = counts.get("add_keyframe", 0) + len(kfs)
        except AssertionError as e:
            errs.append("planting: %s" % e)
            return errs
        for step in range(int(rng.integers(8, 40))):
            u = rng.random()
            try:
                if u < 0.45:
                    ids, ne = CM.random_candidates(rng, kfs)
                    cap = None if rng.random() < 0.7 else int(rng.integers(0, 4))
                    op, err = "culling", pair.keyframe_culling(ids, ne if rng.random() < 0.8 else None, int(rng.choice([1, 2, 3, 3, 3, 6])), cap)
                elif u < 0.60:
                    ids = [p.mnId for p in pm.mps.values()]
                    ask = [ids[int(i)] for i in rng.integers(0, len(ids), int(rng.integers(0, 40)))] + [-1, 10 ** 15]
                    op, err = "observations", pair.observations(ask)
                elif u < 0.70:
                    op, err = "refused", refused_call(rng, pair, pm)
                elif u < 0.80:
                    frame = M.random_frame(rng, pm)
                    op, err = "local_map", pair.local_map(pm.frame_kp_ids(frame), [])
                    if not err:
                        ids = list(pm.kfs)
                        err = pair.connections(ids[int(rng.integers(len(ids)))], int(rng.choice([1, 3, 15])))
                elif u < 0.93:
                    # the reference's loop on the pointer map: its hooks edit both graphs; V8 predicted the result
                    ids, ne = CM.random_candidates(rng, kfs)
                    op, err = "reference_culling", pair.keyframe_culling(ids, ne)
                    if not err:
                        res = pair.model.keyframe_culling(ids, ne)
                        want = pair.model.predicted(ids, res)
                        for k, keep in zip(ids, ne):
                            if k in pm.kfs:
                                pm.kfs[k].mbNotErase = bool(keep)
                        out, bad = pm.KeyFrameCulling([pm.kfs.get(k) for k in ids])
                        if [o[0] for o in out] != res["verdict"].tolist() or bad != res["bad_point_ids"].tolist():
                            err = "the reference's loop gives %s, bad points %s; V8 %s, %s" % (
                                [o[0] for o in out], bad[:8], res["verdict"].tolist(), res["bad_point_ids"][:8])
                        elif pair.model.state() != want:
                            err = "the hooks did not reach the state V8 predicted"
                else:
                    more = CM.random_map(rng, pm, n_kf=int(rng.integers(1, 4)), n_pts=int(rng.integers(5, 40)),
                                         first_kf=max(pm.kfs) + 1, first_mp=max(pm.mps) + 1)
                    kfs += more
                    op, err = "add_keyframe", ""
                    counts[op] = counts.get(op, 0) + len(more) - 1
            except AssertionError as e:
                op, err = "hook", str(e)
            counts[op] = counts.get(op, 0) + 1
            if err:
                errs.append("step %d (%s): %s" % (step, op, err))
                break
        if not errs and pair.size():
            errs.append(pair.size())
    finally:
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
    print("%s %d rounds, %d culling calls, %d observation queries, %d refused calls, %d other calls in %.1f s (seed %d; vs "
          "tests/cull_model.py, exact equality)" % (
              "fuzz FAILED" if errs else "fuzz ok", rounds, counts.get("culling", 0) + counts.get("reference_culling", 0),
              counts.get("observations", 0), counts.get("refused", 0),
              sum(v for k, v in counts.items() if k not in ("culling", "reference_culling", "observations", "refused")),
              time.time() - t0, seed))
    sys.exit(1 if errs else 0)


if __name__ == "__main__":
    main()
