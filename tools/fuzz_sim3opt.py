"""Randomised comparison of Optimizer::OptimizeSim3 on the device with the CPU model (tests/sim3opt_model.py; g2o
boundary unpinned).

usage: python tools/fuzz_sim3opt.py SECONDS SEED

Each round draws a batch of seeded scenes (size, free or fixed scale, share of gross outliers, noise, start
perturbation), runs them in ONE orbgpu_sim3_optimize_batch_device call and compares, per scene whose margin (least
|chi2 / th2 - 1| over all classifications of the model) is >= 1e-6: n_correspondences, n_bad, n_inliers, stages,
n_bad_index and every inlier byte exactly; R12_d, t12_d, s12_d within 16 x the model's own spread (8 permutations of the
summation order plus libm_nudge = +-1, largest over the round's scenes); the float outputs as the exact casts of the
device's doubles; T12 and Scw as the model's formula applied to the device's doubles.  Scenes below the margin are
counted and left out; the report goes to profiles/sim3opt_fuzz.txt; exit status 1 on any mismatch or if more than 1 % of
the scenes were left out."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sim3opt_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402

MARGIN = 1e-6
SENTINEL = 7  # inlier bytes of rows that are no correspondence must come back as they went in
ROWS = ("valid", "Xw1", "Xw2", "octave1", "octave2", "kp1_xy", "kp2_xy")
DTYPES = {"valid": np.uint8, "Xw1": np.float32, "Xw2": np.float32, "octave1": np.int32, "octave2": np.int32,
          "kp1_xy": np.float32, "kp2_xy": np.float32}


def host_problem(sc):
    """The scalar members of a problem dict from a scene."""
    return {"n1": len(sc["valid"]), "T1w": sc["T1w"], "T2w": sc["T2w"], "K1": sc["K1"], "K2": sc["K2"],
            "inv_level_sigma2": sc["inv_level_sigma2"], "R12": sc["R12"], "t12": sc["t12"], "s12": sc["s12"],
            "th2": sc["th2"], "fix_scale": sc["fix_scale"]}


def upload(torch, sc):
    """Device arrays of one scene; returns (problem dict, keep-alive dict)."""
    n1 = len(sc["valid"])
    d = {k: torch.from_numpy(np.ascontiguousarray(sc[k], DTYPES[k]).reshape(-1).copy() if n1 else np.zeros(4, DTYPES[k])).cuda()
         for k in ROWS}
    d["inlier"] = torch.full((max(n1, 1),), SENTINEL, dtype=torch.uint8, device="cuda")
    d["result"] = torch.zeros(C.sizeof(G.Sim3OptResult), dtype=torch.uint8, device="cuda")
    p = host_problem(sc)
    for k in ROWS + ("inlier", "result"):
        p[k] = d[k].data_ptr()
    return p, d


def download(d, n1):
    raw = d["result"].cpu().numpy().tobytes()
    return raw, G.Sim3OptResult.from_buffer_copy(raw).as_dict(), d["inlier"].cpu().numpy()[:n1].copy()


def run_batch(torch, scenes):
    """All scenes in one batched call: list of (raw result bytes, result dict, inlier [n1])."""
    ups = [upload(torch, sc) for sc in scenes]
    G.sim3_optimize_batch_device([u[0] for u in ups], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [download(u[1], len(sc["valid"])) for u, sc in zip(ups, scenes)]


def check_outputs(r, T2w):
    """O9 on the device's own doubles: the float casts, T12 and Scw.  Returns a list of complaints."""
    bad = []
    with np.errstate(all="ignore"):
        if not (np.array_equal(r["R12"], r["R12_d"].astype(np.float32), equal_nan=True)
                and np.array_equal(r["t12"], r["t12_d"].astype(np.float32), equal_nan=True)
                and np.array_equal(np.float32(r["s12"]), np.float32(r["s12_d"]), equal_nan=True)):
            bad.append("float outputs are not the casts of the doubles")
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = (r["s12_d"] * r["R12_d"]).astype(np.float32)
        T[:3, 3] = r["t12_d"].astype(np.float32)
    if not np.array_equal(r["T12"], T, equal_nan=True):
        bad.append("T12 is not toCvMat of the doubles")
    return bad


def compare(scenes, got, n_perm=8, models=None):
    """Model vs device for a set of scenes.  Returns a dict: compared, left_out, mismatches (list of strings), spread (the
    model's own, largest over the set), device_dev (largest deviation of R12_d / t12_d / s12_d), scw_dev."""
    rep = {"compared": 0, "left_out": 0, "mismatches": [], "spread": 0.0, "device_dev": 0.0, "scw_dev": 0.0, "flips": 0}
    kept = []
    for i, (sc, (raw, r, inl)) in enumerate(zip(scenes, got)):
        m = M.optimize_sim3(sc) if models is None else models[i]
        if m["margin"] < MARGIN:
            rep["left_out"] += 1
            continue
        rep["compared"] += 1
        if m["n_correspondences"] >= 1:
            dev, flips = M.model_spread(sc, m, n_perm=n_perm, seed=i)
            if np.isfinite(dev):
                rep["spread"] = max(rep["spread"], dev)
            rep["flips"] += flips
        kept.append((i, sc, m, r, inl))
    for i, sc, m, r, inl in kept:
        tag = "scene %d (N %d): " % (i, m["n_correspondences"])
        for k in M.DISCRETE:
            if r[k] != m[k]:
                rep["mismatches"].append(tag + "%s %d, model %d" % (k, r[k], m[k]))
        want = np.where(m["inlier"] == 255, SENTINEL, m["inlier"]).astype(np.uint8)
        if not np.array_equal(inl, want):
            rep["mismatches"].append(tag + "%d inlier bytes differ" % int((inl != want).sum()))
        dev = M.state_deviation(r, m)
        finite = np.isfinite(m["R12_d"]).all() and np.isfinite(m["t12_d"]).all() and np.isfinite(m["s12_d"])
        if finite:
            rep["device_dev"] = max(rep["device_dev"], dev)
            if not dev <= 16 * rep["spread"]:
                rep["mismatches"].append(tag + "state off by %.3e, allowed 16 x %.3e" % (dev, rep["spread"]))
        rep["mismatches"] += [tag + c for c in check_outputs(r, sc["T2w"])]
        scw = M.scw_of((M.quat_from_matrix(r["R12_d"]), r["t12_d"], r["s12_d"]), sc["T2w"])
        # the quaternion of a matrix is the state only up to the rounding of the round trip: Scw is compared with the
        # formula on the device's doubles to float resolution, T12 (no quaternion product) exactly
        if finite:
            with np.errstate(all="ignore"):
                sdev = float(np.abs(r["Scw"].astype(np.float64) - scw.astype(np.float64)).max())
                lim = 4 * np.finfo(np.float32).eps * max(1.0, float(np.abs(scw).max()))
            rep["scw_dev"] = max(rep["scw_dev"], sdev)
            if not sdev <= lim:
                rep["mismatches"].append(tag + "Scw off by %.3e from the formula on the device's doubles" % sdev)
    return rep


def draw_scene(rng):
    n = int(rng.choice(M.PARITY_SIZES) if rng.random() < 0.4 else rng.integers(1, 900))
    return M.make_scene(n, int(rng.integers(1 << 31)), fix_scale=bool(rng.random() < 0.5),
                        outlier_frac=float(rng.choice([0.0, 0.1, 0.3, 0.5])), noise_px=float(rng.uniform(0.1, 1.0)),
                        rot_sigma=float(rng.uniform(0.001, 0.02)), trans_sigma=float(rng.uniform(0.002, 0.04)),
                        scale_sigma=float(rng.uniform(0.002, 0.04)))


def run(seconds, seed, batch=16):
    import torch
    rng = np.random.default_rng(seed)
    tot = {"rounds": 0, "compared": 0, "left_out": 0, "mismatches": [], "spread": 0.0, "device_dev": 0.0, "scw_dev": 0.0}
    t_end = time.time() + seconds
    while time.time() < t_end:
        scenes = [draw_scene(rng) for _ in range(batch)]
        rep = compare(scenes, run_batch(torch, scenes))
        tot["rounds"] += 1
        for k in ("compared", "left_out"):
            tot[k] += rep[k]
        tot["mismatches"] += ["round %d, %s" % (tot["rounds"], m) for m in rep["mismatches"]]
        for k in ("spread", "device_dev", "scw_dev"):
            tot[k] = max(tot[k], rep[k])
    return tot


def report(tot):
    lines = ["rounds %d, scenes compared %d, left out (margin < %g) %d, mismatches %d" % (
        tot["rounds"], tot["compared"], MARGIN, tot["left_out"], len(tot["mismatches"])),
        "model spread <= %.3e, device deviation <= %.3e, Scw deviation <= %.3e (vs CPU restatement; g2o boundary unpinned)"
        % (tot["spread"], tot["device_dev"], tot["scw_dev"])]
    return lines + ["  " + m for m in tot["mismatches"][:50]]


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    tot = run(seconds, seed)
    lines = ["fuzz_sim3opt %g s, seed %d" % (seconds, seed)] + report(tot)
    print("\n".join(lines))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sim3opt_fuzz.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    too_many = tot["left_out"] > 0.01 * (tot["compared"] + tot["left_out"])
    sys.exit(1 if tot["mismatches"] or too_many else 0)


if __name__ == "__main__":
    main()
