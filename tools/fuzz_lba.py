"""Randomised comparison of Optimizer::LocalBundleAdjustment on the device with the CPU model (tests/lba_model.py; g2o
boundary unpinned).

usage: python tools/fuzz_lba.py SECONDS SEED

Each round draws a batch of seeded local maps (free poses, fixed cameras, points, mono / stereo mix, share of gross
outliers, noise, start perturbation), runs them in ONE orbgpu_local_ba_batch_device call and compares every scene whose
model is stable under permuted summation order -- least margin |chi2 / threshold - 1| >= 1e-6 over the permutations and the
same accept / reject trace in all of them: erase, n_edges, n_erased, rounds, iterations and trials per round exactly; poses
and points within 16 x the model's own spread under those permutations (largest over the round's scenes); the float
outputs within 1 ulp of the rounded model.  Unstable scenes are counted and left out; exit status 1 on any mismatch or if
more than one scene in eight was left out."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lba_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402

MARGIN = 1e-6
SENTINEL = 7  # outputs of a stopped call and erase bytes of skipped edges must come back as they went in
LEFT_OUT_CAP = 1.0 / 8.0


def to_problem(sc):
    """The host part of the dict lib.local_ba_problem takes, from a scene of lba_model.make_scene."""
    return {"Tcw": sc["Tcw"], "n_local": sc["n_local"], "fixed": sc["fixed"], "cam": sc["cam"],
            "inv_level_sigma2": sc["inv_sigma2"], "world_pos": sc["world_pos"], "edge_point": sc["e_point"],
            "edge_pose": sc["e_pose"], "edge_octave": sc["e_oct"], "edge_xy": sc["e_xy"], "edge_u_right": sc["e_ur"],
            "n_poses": len(sc["Tcw"]), "n_points": len(sc["world_pos"]), "n_edges": len(sc["e_point"]),
            "nlevels": np.asarray(sc["inv_sigma2"]).shape[-1]}


def upload(torch, sc, stop=None):
    """Sentinel-filled device outputs of one scene; returns (problem dict, keep-alive dict).  stop: None (null flag) or
    the value of a device flag."""
    nl, m, e = sc["n_local"], len(sc["world_pos"]), len(sc["e_point"])
    d = {"Tcw_d": torch.full((max(nl, 1), 16), float(SENTINEL), dtype=torch.float64, device="cuda"),
         "Tcw": torch.full((max(nl, 1), 16), float(SENTINEL), dtype=torch.float32, device="cuda"),
         "pos_d": torch.full((max(m, 1), 3), float(SENTINEL), dtype=torch.float64, device="cuda"),
         "pos": torch.full((max(m, 1), 3), float(SENTINEL), dtype=torch.float32, device="cuda"),
         "erase": torch.full((max(e, 1),), SENTINEL, dtype=torch.uint8, device="cuda"),
         "res": torch.zeros(C.sizeof(G.LocalBAResult), dtype=torch.uint8, device="cuda")}
    p = to_problem(sc)
    if stop is not None:
        d["stop"] = torch.tensor([int(stop)], dtype=torch.int32, device="cuda")
        p["d_stop"] = d["stop"].data_ptr()
    p.update(d_Tcw_d=d["Tcw_d"].data_ptr(), d_Tcw=d["Tcw"].data_ptr(), d_pos_d=d["pos_d"].data_ptr(),
             d_pos=d["pos"].data_ptr(), d_erase=d["erase"].data_ptr(), d_result=d["res"].data_ptr())
    return p, d


def download(d, sc):
    """(every output byte, result dict, arrays dict)."""
    nl, m, e = sc["n_local"], len(sc["world_pos"]), len(sc["e_point"])
    raw = d["res"].cpu().numpy().tobytes()
    a = {"Tcw_d": d["Tcw_d"].cpu().numpy()[:nl].reshape(nl, 4, 4), "Tcw": d["Tcw"].cpu().numpy()[:nl].reshape(nl, 4, 4),
         "pos_d": d["pos_d"].cpu().numpy()[:m], "pos": d["pos"].cpu().numpy()[:m], "erase": d["erase"].cpu().numpy()[:e]}
    return raw + b"".join(a[k].tobytes() for k in ("Tcw_d", "Tcw", "pos_d", "pos", "erase")), \
        G.LocalBAResult.from_buffer_copy(raw).as_dict(), a


def run_batch(torch, scenes, stops=None):
    """All scenes in one batched call: list of (bytes, result dict, arrays dict)."""
    ups = [upload(torch, sc, None if stops is None else stops[i]) for i, sc in enumerate(scenes)]
    G.local_ba_batch_device([u[0] for u in ups], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [download(u[1], sc) for u, sc in zip(ups, scenes)]


def _ulp(a, b):
    """Largest distance in float32 steps between a and b; NaN against NaN and equal values count 0."""
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    if not a.size:
        return 0
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    d = np.where(np.signbit(a) == np.signbit(b), d, 2)
    d = np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0, d)
    d = np.where(np.isnan(a) != np.isnan(b), 1 << 30, d)
    return int(d.max())


def _dev(a, b):
    """Largest |a - b|; entries where both are NaN or both the same infinity count 0, where one is: inf."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    if not a.size:
        return 0.0
    with np.errstate(all="ignore"):
        d = np.abs(a - b)
    d = np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0.0, d)
    d = np.where(np.isnan(d), np.inf, d)
    return float(d.max())


_REFERENCE = {}


def reference(sc, n_perm, key=None):
    """The model's answer for a scene with its spread under n_perm permutations: (result, spread of the poses, of the
    points, stable).  key: cache the answer under this name (the tests share one reference per scene)."""
    if key is not None and key in _REFERENCE:
        return _REFERENCE[key]
    m = M.local_ba(sc)
    dT, dX, same, margin = M.permutation_spread(sc, m, n_perm=n_perm, seed=len(sc["e_point"]))
    out = (m, dT, dX, bool(same and margin >= MARGIN))
    if key is not None:
        _REFERENCE[key] = out
    return out


LBA_COUNTERS = ("n_edges", "n_erased", "rounds", "stopped", "n_bad_index", "iterations", "trials")


def _erase_wanted(m):
    return np.where(m["erase"] == 255, SENTINEL, m["erase"]).astype(np.uint8)


def compare(scenes, got, n_perm=3, keys=None):
    """Model vs device for a set of scenes.  Returns a dict: compared, left_out, mismatches (list of strings), spread_pose /
    spread_point (largest model deviation under permuted summation order), dev_pose / dev_point (largest device
    deviation from the model), float_ulp."""
    return compare_by_rule(scenes, got, reference, LBA_COUNTERS, "erase", "erase flags", _erase_wanted, n_perm, keys)


def compare_by_rule(scenes, got, reference, counters, flags, flags_label, flags_wanted, n_perm=3, keys=None):
    """The one text of the comparison rule, for any optimiser whose model returns poses, points and a byte array of flags.
    reference(sc, n_perm, key) -> (model result, spread of the poses, of the points, stable); counters: the result members
    compared exactly; flags: the name of the byte array, flags_label what a mismatch calls it, flags_wanted(model result)
    the bytes the device has to return."""
    rep = {"compared": 0, "left_out": 0, "mismatches": [], "spread_pose": 0.0, "spread_point": 0.0, "dev_pose": 0.0,
           "dev_point": 0.0, "float_ulp": 0}
    kept = []
    for i, (sc, (_, r, a)) in enumerate(zip(scenes, got)):
        m, dT, dX, stable = reference(sc, n_perm, None if keys is None else keys[i])
        if not stable:
            rep["left_out"] += 1
            continue
        rep["compared"] += 1
        rep["spread_pose"], rep["spread_point"] = max(rep["spread_pose"], dT), max(rep["spread_point"], dX)
        kept.append((i, m, r, a))
    for i, m, r, a in kept:
        tag = "scene %d (%d edges): " % (i, m["n_edges"])
        for k in counters:
            if r[k] != m[k]:
                rep["mismatches"].append(tag + "%s %r, model %r" % (k, r[k], m[k]))
        want = flags_wanted(m)
        if not np.array_equal(a[flags], want):
            rep["mismatches"].append(tag + "%d %s differ" % (int((a[flags] != want).sum()), flags_label))
        for what, dk, fk, sk in (("pose", "Tcw_d", "Tcw", "spread_pose"), ("point", "pos_d", "pos", "spread_point")):
            dev = _dev(a[dk], m[dk])
            rep["dev_" + what] = max(rep["dev_" + what], dev)
            if not dev <= 16 * rep[sk]:
                rep["mismatches"].append(tag + "%s off by %.3e, allowed 16 x %.3e" % (dk, dev, rep[sk]))
            with np.errstate(all="ignore"):
                if _ulp(a[fk], a[dk].astype(np.float32)) != 0:
                    rep["mismatches"].append(tag + "%s is not (float)%s" % (fk, dk))
            ulp = _ulp(a[fk], m[fk])
            rep["float_ulp"] = max(rep["float_ulp"], ulp)
            if ulp > 1:
                rep["mismatches"].append(tag + "float %s differs from the model's by %d ulp" % (what, ulp))
    return rep


def draw_scene(rng):
    nf, nx, npts = [(1, 1, 6), (2, 0, 8), (3, 2, 40), (5, 3, 120), (8, 4, 300)][int(rng.integers(5))]
    if rng.random() < 0.5:
        nf, nx, npts = int(rng.integers(1, 9)), int(rng.integers(0, 5)), int(rng.integers(6, 200))
    kf0 = nx == 0 or rng.random() < 0.2
    return M.make_scene(nf, nx, npts, int(rng.integers(1 << 31)), mode=str(rng.choice(["mono", "stereo", "mixed"])), kf0_fixed=kf0,
                        noise=float(rng.uniform(0.2, 1.0)), outlier_frac=float(rng.choice([0.0, 0.03, 0.08])),
                        obs_frac=float(rng.uniform(0.4, 0.9)), rot_sigma=float(rng.uniform(0.001, 0.006)),
                        trans_sigma=float(rng.uniform(0.003, 0.02)), point_sigma=float(rng.uniform(0.005, 0.03)))


def run(seconds, seed, batch=8):
    import torch
    rng = np.random.default_rng(seed)
    tot = {"rounds": 0, "compared": 0, "left_out": 0, "mismatches": [], "spread_pose": 0.0, "spread_point": 0.0,
           "dev_pose": 0.0, "dev_point": 0.0, "float_ulp": 0}
    t_end = time.time() + seconds
    while time.time() < t_end:
        scenes = [draw_scene(rng) for _ in range(batch)]
        rep = compare(scenes, run_batch(torch, scenes), n_perm=2)
        tot["rounds"] += 1
        for k in ("compared", "left_out"):
            tot[k] += rep[k]
        tot["mismatches"] += rep["mismatches"]
        for k in ("spread_pose", "spread_point", "dev_pose", "dev_point", "float_ulp"):
            tot[k] = max(tot[k], rep[k])
    return tot


def main():
    tot = run(float(sys.argv[1]), int(sys.argv[2]))
    print("rounds %d, scenes compared %d, left out (unstable under permutation) %d, mismatches %d" % (
        tot["rounds"], tot["compared"], tot["left_out"], len(tot["mismatches"])))
    print("model spread: poses <= %.3e, points <= %.3e; device deviation: poses <= %.3e, points <= %.3e; float outputs <= %d "
          "ulp (vs CPU restatement; g2o boundary unpinned)" % (tot["spread_pose"], tot["spread_point"], tot["dev_pose"],
                                                               tot["dev_point"], tot["float_ulp"]))
    for m in tot["mismatches"][:20]:
        print("  " + m)
    too_many = tot["left_out"] > LEFT_OUT_CAP * (tot["compared"] + tot["left_out"])
    sys.exit(1 if tot["mismatches"] or too_many else 0)


if __name__ == "__main__":
    main()
