"""Randomised comparison of Optimizer::OptimizeEssentialGraph on the device with the CPU model (tests/eg_model.py; g2o
boundary unpinned).

usage: python tools/fuzz_eg.py SECONDS SEED

Each round draws a batch of seeded pose graphs (a chain or a ring with extra edges, one or two fixed rows, the scale fixed
or free, the entry estimates off the map the edges measure, some points), runs them in ONE
orbgpu_essential_graph_batch_device call, corrects the points with orbgpu_essential_graph_correct_points_device and
compares by the rule of fuzz_lba.compare_by_rule: n_edges, iterations, trials, stopped, n_bad_index, n_free_active and the
rows that come out bit-equal to their input exactly; poses and points within 16 x the model's own spread under permuted
summation order (largest over the round's scenes); the float outputs equal to (float) of the double ones and within 1 ulp
of the rounded model.  "Pose" is the double pre-image of Tiw -- R and t (1 / s) of G10 -- and "point" the double pre-image of
a corrected point (G11), both formed on the host from the device's own states, so the (float) rule is the exact formula on
the device's own doubles.

The drawn graphs are CONSISTENT (their edges measure one map) and run just down to it (draw_scene): an inconsistent loop
carries the 1e-7 noise of the 1e-9 difference quotient into its minimum, past a float step, and a graph that has converged
decides its further trials between equal chi2.  Both are judged with the model alone, never reach the device and count as left out under
fuzz_lba's one-in-eight cap: a trace that changes under permutation, and a spread past CONDITION_BOUND.  The parity
scenes of tests/test_gpu_eg.py cover the inconsistent loops with their own rule."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import eg_model as M  # noqa: E402
from fuzz_lba import LEFT_OUT_CAP, SENTINEL, _dev, _ulp, compare_by_rule  # noqa: E402, F401
from orb_slam2_map_amd import lib as G  # noqa: E402

HOST = ("Scw", "Snc", "fixed", "edge_i", "edge_j", "edge_kind", "n_iterations", "fix_scale")
EG_COUNTERS = ("n_edges", "iterations", "trials", "stopped", "n_bad_index", "n_free_active", "n_bad_ref")
N_PERM = 4
CONDITION_BOUND = 2.0 ** -22 / 16  # fuzz_ba's: a sixteenth of the float step between 2 and 4


def to_problem(sc):
    """The host part of the dict lib.essential_graph_problem takes."""
    return {k: sc[k] for k in HOST}


def n_points(sc):
    return 0 if sc.get("world_pos") is None else len(sc["world_pos"])


def upload(torch, sc, stop=None):
    """Sentinel-filled device outputs of one scene (and its points, if it has any); returns (problem dict, keep-alive dict).
    stop: None (null flag) or the value of a device flag."""
    V, m = len(sc["Scw"]), n_points(sc)
    d = {"Siw_d": torch.full((max(V, 1), 8), float(SENTINEL), dtype=torch.float64, device="cuda"),
         "Tiw": torch.full((max(V, 1), 16), float(SENTINEL), dtype=torch.float32, device="cuda"),
         "res": torch.zeros(C.sizeof(G.EssentialGraphResult), dtype=torch.uint8, device="cuda"),
         "Scw": torch.from_numpy(np.ascontiguousarray(sc["Scw"], np.float64).reshape(-1, 8)).cuda(),
         "n_bad_ref": torch.zeros(1, dtype=torch.int32, device="cuda")}
    if m:
        d["pos_in"] = torch.from_numpy(np.ascontiguousarray(sc["world_pos"], np.float32)).cuda()
        d["ref"] = torch.from_numpy(np.ascontiguousarray(sc["point_ref"], np.int32)).cuda()
        d["pos"] = torch.full((m, 3), float(SENTINEL), dtype=torch.float32, device="cuda")
    p = to_problem(sc)
    if stop is not None:
        d["stop"] = torch.tensor([int(stop)], dtype=torch.int32, device="cuda")
        p["d_stop"] = d["stop"].data_ptr()
    p.update(d_Siw_d=d["Siw_d"].data_ptr(), d_Tiw=d["Tiw"].data_ptr(), d_result=d["res"].data_ptr())
    return p, d


def correct_points(torch, sc, d):
    """G11 on the scene's device arrays, after the optimiser on the current stream."""
    if n_points(sc):
        G.essential_graph_correct_points_device(len(sc["Scw"]), d["Scw"].data_ptr(), d["Siw_d"].data_ptr(), n_points(sc),
                                                d["pos_in"].data_ptr(), d["ref"].data_ptr(), d["pos"].data_ptr(),
                                                d["n_bad_ref"].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)


def download(d, sc):
    """(every output byte, result dict, arrays dict); n_bad_ref of the result is the points call's count."""
    V, m = len(sc["Scw"]), n_points(sc)
    raw = d["res"].cpu().numpy().tobytes()
    a = {"Siw_d": d["Siw_d"].cpu().numpy()[:V], "Tiw": d["Tiw"].cpu().numpy()[:V],
         "pos": d["pos"].cpu().numpy() if m else np.zeros((0, 3), np.float32)}
    r = G.EssentialGraphResult.from_buffer_copy(raw).as_dict()
    r["n_bad_ref"] = int(d["n_bad_ref"].cpu().numpy()[0])
    return raw + b"".join(a[k].tobytes() for k in ("Siw_d", "Tiw", "pos")), r, a


def run_batch(torch, scenes, stops=None):
    """All scenes in one batched call, then their points: list of (bytes, result dict, arrays dict)."""
    ups = [upload(torch, sc, None if stops is None else stops[i]) for i, sc in enumerate(scenes)]
    G.essential_graph_batch_device([u[0] for u in ups], stream=torch.cuda.current_stream().cuda_stream)
    for i, (u, sc) in enumerate(zip(ups, scenes)):
        if stops is None or not stops[i]:
            correct_points(torch, sc, u[1])
    torch.cuda.synchronize()
    return [download(u[1], sc) for u, sc in zip(ups, scenes)]


# ---- the double pre-images of the float outputs -------------------------------------------------------------------------
def tiw_d(S):
    """R and t (1 / s) of G10 in double, [V][16]."""
    S = np.asarray(S, np.float64).reshape(-1, 8)
    T = np.zeros((len(S), 4, 4))
    with np.errstate(all="ignore"):
        T[:, :3, :3] = M.qmat(S[:, :4])
        T[:, :3, 3] = S[:, 4:7] * (1.0 / S[:, 7:8])
    T[:, 3, 3] = 1.0
    return T.reshape(len(S), 16)


def pos_d(Siw, sc):
    """The corrected points of G11 in double, [M][3]; a point with a row out of range keeps its position."""
    if not n_points(sc):
        return np.zeros((0, 3))
    pos = np.asarray(sc["world_pos"], np.float32).astype(np.float64)
    ref = np.asarray(sc["point_ref"], np.int64)
    ok = (ref >= 0) & (ref < len(sc["Scw"]))
    out = pos.copy()
    if ok.any():
        out[ok] = M.s_map(M.s_inv(np.asarray(Siw, np.float64)[ref[ok]]),
                          M.s_map(np.asarray(sc["Scw"], np.float64).reshape(-1, 8)[ref[ok]], pos[ok]))
    return out


def as_rule_arrays(Siw, Tiw, pos, sc):
    """What compare_by_rule reads: Tcw_d / Tcw, pos_d / pos and the flags (1 where a row left as it came, bit for bit)."""
    Siw = np.asarray(Siw, np.float64).reshape(-1, 8)
    same = np.array([Siw[v].tobytes() == np.asarray(sc["Scw"], np.float64).reshape(-1, 8)[v].tobytes()
                     for v in range(len(Siw))], np.uint8)
    return {"Tcw_d": tiw_d(Siw), "Tcw": np.asarray(Tiw, np.float32).reshape(-1, 16), "pos_d": pos_d(Siw, sc),
            "pos": np.asarray(pos, np.float32).reshape(-1, 3), "unchanged": same, "Siw_d": Siw}


_REFERENCE = {}


def reference(sc, n_perm, key=None):
    """The model's answer for a scene in compare_by_rule's terms, with its spread under n_perm permutations plus
    libm_nudge = +-1: (result, spread of the poses, of the points, stable).  The result also carries state_spread."""
    if key is not None and key in _REFERENCE:
        return _REFERENCE[key]
    m = M.essential_graph(sc)
    rng = np.random.default_rng(20_000 + m["n_edges"])
    runs = [M.essential_graph(sc, order=rng.permutation(m["n_edges"])) for _ in range(n_perm)]
    runs += [M.essential_graph(sc, libm_nudge=-1), M.essential_graph(sc, libm_nudge=1)]
    base = as_rule_arrays(m["Siw_d"], m["Tiw"], m["pos"] if m["pos"] is not None else np.zeros((0, 3), np.float32), sc)
    dT = dX = dS = 0.0
    stable = True
    for r in runs:
        a = as_rule_arrays(r["Siw_d"], r["Tiw"], r["pos"] if r["pos"] is not None else np.zeros((0, 3), np.float32), sc)
        dT, dX = max(dT, _dev(a["Tcw_d"], base["Tcw_d"])), max(dX, _dev(a["pos_d"], base["pos_d"]))
        dS = max(dS, _dev(a["Siw_d"], base["Siw_d"]))
        stable = stable and all(r[k] == m[k] for k in M.DISCRETE)
    res = dict(m)
    res.update(base)
    res.update(stopped=0, state_spread=dS)
    out = (res, dT, dX, bool(stable))
    if key is not None:
        _REFERENCE[key] = out
    return out


def rule_view(got, scenes):
    """The device's results with the arrays compare_by_rule reads."""
    return [(b, r, as_rule_arrays(a["Siw_d"], a["Tiw"], a["pos"], sc)) for (b, r, a), sc in zip(got, scenes)]


def compare(scenes, got, n_perm=N_PERM, keys=None):
    """Model vs device by fuzz_lba.compare_by_rule (the one text of the rule) with this optimiser's counters and the rows
    that leave as they came.  Returns what fuzz_lba.compare returns."""
    return compare_by_rule(scenes, rule_view(got, scenes), reference, EG_COUNTERS, "unchanged", "unchanged rows",
                           lambda m: m["unchanged"], n_perm, keys)


def compare_parity(names, scenes, got, n_perm=8):
    """The parity rule of tests/test_gpu_eg.py: nothing left out; discrete outputs exactly; every state within 16 x the
    model's own spread (8 permutations plus libm_nudge = +-1, largest over the set); Tiw and the corrected points the
    exact G10 / G11 formulas on the device's own doubles.  Returns a report dict."""
    refs = [reference(sc, n_perm, "parity-" + n) for n, sc in zip(names, scenes)]
    spread = max(r[0]["state_spread"] for r in refs)
    rep = {"spread": spread, "flips": sum(not r[3] for r in refs), "device_dev": 0.0, "mismatches": [], "per_scene": {}}
    for n, sc, (m, _, _, stable), (_, r, a) in zip(names, scenes, refs, got):
        v = as_rule_arrays(a["Siw_d"], a["Tiw"], a["pos"], sc)
        dev = _dev(v["Siw_d"], m["Siw_d"])
        rep["device_dev"] = max(rep["device_dev"], dev)
        for k in EG_COUNTERS:
            if r[k] != m[k]:
                rep["mismatches"].append("%s: %s %r, model %r" % (n, k, r[k], m[k]))
        if not dev <= 16 * spread:
            rep["mismatches"].append("%s: states off by %.3e, allowed 16 x %.3e" % (n, dev, spread))
        if not np.array_equal(v["unchanged"], m["unchanged"]):
            rep["mismatches"].append("%s: rows that leave as they came differ" % n)
        with np.errstate(all="ignore"):
            if _ulp(v["Tcw"], v["Tcw_d"].astype(np.float32)) != 0:
                rep["mismatches"].append("%s: Tiw is not G10 of the device's own states" % n)
            if _ulp(v["pos"], v["pos_d"].astype(np.float32)) != 0:
                rep["mismatches"].append("%s: points are not G11 of the device's own states" % n)
        with np.errstate(all="ignore"):
            chi_rel = abs(r["chi2_end"] - m["chi2_end"]) / max(abs(m["chi2_end"]), 1e-300)
        rep["per_scene"][n] = {"vertices": len(sc["Scw"]), "edges": m["n_edges"], "free_active": m["n_free_active"],
                               "model_spread": m["state_spread"], "stable": bool(stable), "device_deviation": dev,
                               "iterations": r["iterations"], "trials": r["trials"], "model_trace": m["trace"],
                               "envelope": r["envelope"], "bandwidth": r["bandwidth"],
                               "chi2_start": r["chi2_start"], "chi2_end": r["chi2_end"],
                               "chi2_end_relative_to_model": None if np.isnan(chi_rel) else float(chi_rel),
                               "log_cases": [int(c) for c in m["log_cases"]], "exp_cases": [int(c) for c in m["exp_cases"]]}
    return rep


def draw_scene(rng):
    """A consistent graph: the edges measure the map Snc, the entry estimates are off it, one or two iterations."""
    V = int(rng.choice([2, 3, 5, 8, 13, 20]))
    closed = V >= 5 and rng.random() < 0.6
    # Every drawn graph runs down to the map its edges measure, where the difference quotient's 1e-7 no longer shows (what an
    # iteration leaves is that noise times the error it started from); stopped earlier, the states would differ from the
    # model's by 1e-9 and more, which is many float steps for an entry near zero.  Scale fixed: steps of 0.01 to 0.03 and
    # three iterations (errors of about 1e-3, 1e-6, 1e-12).  Scale free: once an error has |sigma| >= 1e-5 and an angle
    # between 1e-4 and 4e-3 it falls where G3's published B is off, Gauss-Newton oversteps and lambda grows -- so those
    # graphs enter on the map's scale with steps of 1e-4 and run two iterations, all inside the small-angle, small-sigma
    # case, which exercises the seventh column; the parity scenes of tests/test_gpu_eg.py enter the other cases.
    fix_scale = bool(rng.random() < 0.6)
    sc = M.make_scene(V, int(rng.integers(1 << 31)), reach=int(rng.integers(1, 3)) if V >= 5 else 1, fix_scale=fix_scale,
                      rot_drift=0.0, trans_drift=0.0, scale_drift=0.0, n_corrected=0, closed=closed,
                      perturb=float(rng.uniform(0.01, 0.03) if fix_scale else rng.uniform(5e-5, 3e-4)), perturb_scale=False,
                      n_iterations=3 if fix_scale else 2, n_points=int(rng.integers(0, 40)))
    sc["edge_kind"] = np.ones_like(sc["edge_kind"])  # every edge measures Snc: a corrected row would make the loop inconsistent
    if V >= 8 and rng.random() < 0.5:
        sc.update({k: v for k, v in M.with_edges(sc, len(sc["edge_i"]) + int(rng.integers(1, 12)), int(rng.integers(1 << 31))).items()
                   if k.startswith("edge_")})
    if V >= 5 and rng.random() < 0.3:
        v = int(rng.integers(1, V))  # a second fixed row, on the map: the graph stays consistent
        sc["fixed"] = sc["fixed"].copy()
        sc["fixed"][v] = 1
        sc["Scw"][v] = sc["Snc"][v]
    return sc


def run(seconds, seed, batch=8, rounds=None):
    """Rounds of `batch` drawn graphs for `seconds`, or exactly `rounds` of them when that is given (the same graphs on
    every machine)."""
    import torch
    rng = np.random.default_rng(seed)
    tot = {"rounds": 0, "compared": 0, "left_out": 0, "ill_conditioned": 0, "mismatches": [], "spread_pose": 0.0,
           "spread_point": 0.0, "dev_pose": 0.0, "dev_point": 0.0, "float_ulp": 0}
    t_end = None if rounds is not None else time.time() + seconds
    while (tot["rounds"] < rounds) if rounds is not None else (time.time() < t_end):
        scenes, keys = [], []
        for i in range(batch):
            sc, key = draw_scene(rng), "fuzz-%d" % i
            _, dT, dX, stable = reference(sc, N_PERM, key)
            if stable and max(dT, dX) > CONDITION_BOUND:
                tot["ill_conditioned"] += 1
                tot["left_out"] += 1
                continue
            scenes.append(sc)
            keys.append(key)
        rep = compare(scenes, run_batch(torch, scenes) if scenes else [], n_perm=N_PERM, keys=keys)
        for i in range(batch):
            _REFERENCE.pop("fuzz-%d" % i, None)
        tot["rounds"] += 1
        for k in ("compared", "left_out"):
            tot[k] += rep[k]
        tot["mismatches"] += rep["mismatches"]
        for k in ("spread_pose", "spread_point", "dev_pose", "dev_point", "float_ulp"):
            tot[k] = max(tot[k], rep[k])
    return tot


def main():
    tot = run(float(sys.argv[1]), int(sys.argv[2]))
    print("rounds %d, scenes compared %d, left out %d (ill conditioned %d, the others unstable under permutation), "
          "mismatches %d" % (tot["rounds"], tot["compared"], tot["left_out"], tot["ill_conditioned"], len(tot["mismatches"])))
    print("model spread: poses <= %.3e, points <= %.3e; device deviation: poses <= %.3e, points <= %.3e; float outputs <= %d "
          "ulp (vs CPU restatement; g2o boundary unpinned)" % (tot["spread_pose"], tot["spread_point"], tot["dev_pose"],
                                                               tot["dev_point"], tot["float_ulp"]))
    for m in tot["mismatches"][:20]:
        print("  " + m)
    too_many = tot["left_out"] > LEFT_OUT_CAP * (tot["compared"] + tot["left_out"])
    sys.exit(1 if tot["mismatches"] or too_many else 0)


if __name__ == "__main__":
    main()
