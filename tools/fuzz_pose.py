"""Randomised comparison of Optimizer::PoseOptimization on the device with the CPU model (tests/pose_model.py; g2o
boundary unpinned).

usage: python tools/fuzz_pose.py SECONDS SEED

Each round draws a batch of seeded scenes (size, mono / stereo mix, share of associations and of gross outliers, noise,
start perturbation), runs them in ONE orbgpu_pose_optimization_batch_device call and compares, per scene whose margin
(least |chi2 / threshold - 1| over all classifications of the model) is >= 1e-6: n_initial, n_inliers, rounds and every
mvbOutlier exactly, Tcw_d within 16 x the model's own spread under 8 permutations of the summation order (largest over
the round's scenes).  Scenes below the margin are counted and left out; exit status 1 on any mismatch or if more than 1 %
of the scenes were left out."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pose_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402

MARGIN = 1e-6
SENTINEL = 7  # outlier bytes of key points without an edge must come back as they went in


def upload(torch, sc, cap=None):
    """Device arrays of one scene in the layout of the device entry points; returns (problem dict, keep-alive dict)."""
    n = sc["n"]
    cap = max(n, 1) if cap is None else cap
    kps = np.zeros(cap, G.KEYPOINT_DTYPE)
    kps["x"][:n], kps["y"][:n], kps["octave"][:n] = sc["kps_xy"][:, 0], sc["kps_xy"][:, 1], sc["octave"]
    ur = np.full(cap, -1, np.float32)
    ur[:n] = sc["u_right"]
    k2m = np.full(cap, -1, np.int32)
    k2m[:n] = sc["kp_to_mp"]
    d = {"kps": torch.from_numpy(kps.view(np.float32).reshape(cap, 7)).cuda(), "ur": torch.from_numpy(ur).cuda(),
         "k2m": torch.from_numpy(k2m).cuda(), "n": torch.tensor([n], dtype=torch.int32, device="cuda"),
         "wp": torch.from_numpy(np.ascontiguousarray(sc["world_pos"], np.float32)).cuda(),
         "out": torch.full((cap,), SENTINEL, dtype=torch.uint8, device="cuda"),
         "res": torch.zeros(C.sizeof(G.PoseResult), dtype=torch.uint8, device="cuda")}
    fv = G.DeviceFrameView()
    fv.cap, fv.n, fv.kps, fv.u_right, fv.nlevels = cap, d["n"].data_ptr(), d["kps"].data_ptr(), d["ur"].data_ptr(), len(sc["inv_level_sigma2"])
    d["fv"] = fv
    fx, fy, cx, cy, bf = (float(k) for k in sc["K"])
    p = {"frame": fv, "d_kp_to_mp": d["k2m"].data_ptr(), "d_world_pos": d["wp"].data_ptr(), "rows": len(sc["world_pos"]),
         "Tcw": sc["Tcw"], "inv_level_sigma2": sc["inv_level_sigma2"], "fx": fx, "fy": fy, "cx": cx, "cy": cy, "mbf": bf,
         "d_outlier": d["out"].data_ptr(), "d_result": d["res"].data_ptr()}
    return p, d


def download(d, n):
    raw = d["res"].cpu().numpy().tobytes()
    return raw, G.PoseResult.from_buffer_copy(raw).as_dict(), d["out"].cpu().numpy()[:n].copy()


def run_batch(torch, scenes, caps=None):
    """All scenes in one batched call: list of (raw result bytes, result dict, outlier [n])."""
    ups = [upload(torch, sc, None if caps is None else caps[i]) for i, sc in enumerate(scenes)]
    G.pose_optimization_batch_device([u[0] for u in ups], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [download(u[1], sc["n"]) for u, sc in zip(ups, scenes)]


def compare(scenes, got, n_perm=8):
    """Model vs device for a set of scenes.  Returns a dict: compared, left_out, mismatches (list of strings), spread
    (largest model deviation under permuted summation order), device_dev (largest |Tcw_d - model|), float_ulp."""
    rep = {"compared": 0, "left_out": 0, "mismatches": [], "spread": 0.0, "device_dev": 0.0, "float_ulp": 0}
    kept = []
    for i, (sc, (raw, r, out)) in enumerate(zip(scenes, got)):
        m = M.run_model(sc)
        if m["margin"] < MARGIN:
            rep["left_out"] += 1
            continue
        rep["compared"] += 1
        if m["n_initial"] >= 3:
            dev, _ = M.permutation_spread(sc, m, n_perm=n_perm, seed=i)
            rep["spread"] = max(rep["spread"], dev)
        kept.append((i, m, r, out))
    for i, m, r, out in kept:
        tag = "scene %d (n_initial %d): " % (i, m["n_initial"])
        for k in ("n_initial", "n_inliers", "rounds", "n_bad_index"):
            if r[k] != m[k]:
                rep["mismatches"].append(tag + "%s %d, model %d" % (k, r[k], m[k]))
        want = np.where(m["outlier"] == 255, SENTINEL, m["outlier"]).astype(np.uint8)
        if not np.array_equal(out, want):
            rep["mismatches"].append(tag + "%d outlier flags differ" % int((out != want).sum()))
        dev = float(np.abs(r["Tcw_d"] - m["Tcw_d"]).max())
        rep["device_dev"] = max(rep["device_dev"], dev)
        if not dev <= 16 * rep["spread"]:
            rep["mismatches"].append(tag + "Tcw_d off by %.3e, allowed 16 x %.3e" % (dev, rep["spread"]))
        if not np.array_equal(r["Tcw"], r["Tcw_d"].astype(np.float32)):
            rep["mismatches"].append(tag + "Tcw is not (float)Tcw_d")
        ulp = np.abs(r["Tcw"].view(np.int32).astype(np.int64) - m["Tcw"].view(np.int32).astype(np.int64))
        same_sign = np.signbit(r["Tcw"]) == np.signbit(m["Tcw"])
        ulp = np.where(same_sign, ulp, 2)
        ulp = np.where((r["Tcw"] == 0) & (m["Tcw"] == 0), 0, ulp)
        rep["float_ulp"] = max(rep["float_ulp"], int(ulp.max()))
        if ulp.max() > 1:
            rep["mismatches"].append(tag + "float pose differs from the model's by %d ulp" % int(ulp.max()))
    return rep


def draw_scene(rng):
    n = int(rng.choice([3, 9, 10, 40, 150, 400, 1000, 1800]) if rng.random() < 0.5 else rng.integers(3, 2000))
    return M.make_scene(n, int(rng.integers(1 << 31)), mode=str(rng.choice(["mono", "stereo", "mixed"])),
                        assoc_frac=float(rng.choice([1.0, 0.8, 0.4])), outlier_frac=float(rng.choice([0.0, 0.1, 0.2, 0.35])),
                        noise=float(rng.uniform(0.2, 1.0)), rot_sigma=float(rng.uniform(0.001, 0.02)),
                        trans_sigma=float(rng.uniform(0.003, 0.05)))


def run(seconds, seed, batch=24):
    import torch
    rng = np.random.default_rng(seed)
    tot = {"rounds": 0, "compared": 0, "left_out": 0, "mismatches": [], "spread": 0.0, "device_dev": 0.0, "float_ulp": 0}
    t_end = time.time() + seconds
    while time.time() < t_end:
        scenes = [draw_scene(rng) for _ in range(batch)]
        rep = compare(scenes, run_batch(torch, scenes))
        tot["rounds"] += 1
        for k in ("compared", "left_out"):
            tot[k] += rep[k]
        tot["mismatches"] += rep["mismatches"]
        for k in ("spread", "device_dev", "float_ulp"):
            tot[k] = max(tot[k], rep[k])
    return tot


def main():
    tot = run(float(sys.argv[1]), int(sys.argv[2]))
    print("rounds %d, scenes compared %d, left out (margin < %g) %d, mismatches %d" % (
        tot["rounds"], tot["compared"], MARGIN, tot["left_out"], len(tot["mismatches"])))
    print("model spread <= %.3e, device deviation <= %.3e, float pose <= %d ulp (vs CPU restatement; g2o boundary unpinned)"
          % (tot["spread"], tot["device_dev"], tot["float_ulp"]))
    for m in tot["mismatches"][:20]:
        print("  " + m)
    too_many = tot["left_out"] > 0.01 * (tot["compared"] + tot["left_out"])
    sys.exit(1 if tot["mismatches"] or too_many else 0)


if __name__ == "__main__":
    main()
