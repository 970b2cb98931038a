"""Randomised comparison of the Initializer on the device (orbgpu_initializer_batch_device) with the CPU model
(tests/init_model.py) -- vs CPU restatement; OpenCV boundary unpinned.

usage: python tools/fuzz_init.py SECONDS SEED

Each round draws a batch of seeded two-view scenes (size, kind, noise, share of outliers, number of hypotheses), runs them
in ONE batched call and compares them with the model as compare() describes.  The constants of the comparison (GAP,
BOUND_FACTOR, MARGIN_FACTOR, LEFT_OUT_CAP) and their reasoning are in tests/init_model.py and tests/pnp_model.py.  Exit
status 1 on any mismatch."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import init_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402


def upload(torch, sc):
    """Device arrays of one scene; returns (problem dict for lib.initializer_batch_device, keep-alive dict)."""
    k1, k2 = np.asarray(sc["kp1"], np.float32).reshape(-1, 2), np.asarray(sc["kp2"], np.float32).reshape(-1, 2)
    sets = np.ascontiguousarray(sc["sets"], np.int32).reshape(-1, 8)
    n1, n2, H = len(k1), len(k2), len(sets)
    words = (n1 + 63) // 64
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device="cuda")  # noqa: E731
    d = {"kp1": dev(k1) if n1 else z(2, torch.float32), "kp2": dev(k2) if n2 else z(2, torch.float32),
         "matches12": dev(np.asarray(sc["matches12"], np.int32)) if n1 else z(1, torch.int32),
         "sets": dev(sets) if H else z(8, torch.int32),
         "scores_h": torch.full((max(H, 1),), -7.0, dtype=torch.float32, device="cuda"),
         "scores_f": torch.full((max(H, 1),), -7.0, dtype=torch.float32, device="cuda"),
         "masks_h": z(H * words, torch.int64), "masks_f": z(H * words, torch.int64), "R21": z(9, torch.float32),
         "t21": z(3, torch.float32), "P3D": torch.full((max(3 * n1, 1),), -7.0, dtype=torch.float32, device="cuda"),
         "triangulated": torch.full((max(n1, 1),), 7, dtype=torch.uint8, device="cuda"),
         "result": torch.zeros(C.sizeof(G.InitResult), dtype=torch.uint8, device="cuda")}
    p = {k: sc[k] for k in ("K", "sigma", "min_parallax", "min_triangulated") if k in sc}
    p.update(n1=n1, n2=n2, n_hyp=H)
    p.update({k: v.data_ptr() for k, v in d.items()})
    return p, d


def download(d, sc):
    n1, H = len(np.asarray(sc["kp1"]).reshape(-1, 2)), len(np.asarray(sc["sets"]).reshape(-1, 8))
    words = (n1 + 63) // 64
    r = G.InitResult.from_buffer_copy(d["result"].cpu().numpy().tobytes()).as_dict()
    r.update(scores_h=d["scores_h"].cpu().numpy()[:H].copy(), scores_f=d["scores_f"].cpu().numpy()[:H].copy(),
             masks_h=d["masks_h"].cpu().numpy()[:H * words].view(np.uint64).reshape(H, words),
             masks_f=d["masks_f"].cpu().numpy()[:H * words].view(np.uint64).reshape(H, words),
             R21_out=d["R21"].cpu().numpy().reshape(3, 3), t21_out=d["t21"].cpu().numpy().copy(),
             P3D=d["P3D"].cpu().numpy()[:3 * n1].reshape(n1, 3), triangulated=d["triangulated"].cpu().numpy()[:n1].copy())
    return r


RESULT_KEYS = ("n", "n_bad_index", "n_bad_set", "best_h", "best_f", "used_homography", "n_inliers", "best_motion",
               "second_best_good", "success")
ARRAY_KEYS = ("scores_h", "scores_f", "masks_h", "masks_f", "P3D", "triangulated", "n_good", "cos_parallax", "H21", "F21", "R21",
              "t21", "SH", "SF", "RH")


def result_bytes(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ARRAY_KEYS) + repr([int(r[k]) for k in RESULT_KEYS]).encode()


def run_batch(torch, scenes):
    ups = [upload(torch, sc) for sc in scenes]
    G.initializer_batch_device([u[0] for u in ups], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [download(u[1], sc) for u, sc in zip(ups, scenes)]


def _clear_winner(scores, best, bound):
    """the winner of a strict > scan stays the winner when every score moves by at most bound x max(1, |score|)"""
    if best < 0:
        return not (np.asarray(scores, np.float64) > 0).any() or bound == 0.0
    s = np.asarray(scores, np.float64)
    others = np.delete(s, best)
    return bound == 0.0 or not len(others) or s[best] - others.max() > 2.0 * bound * max(1.0, abs(s[best]))


def compare(scenes, got, passes=None, fp64=None):
    """Model against device.  passes: [(model, spread)] from M.model_pass, computed here if missing.  Per hypothesis and
    model (H, F): mask words byte-equal and the score within the bound, outside the hypotheses M.left_out names.  The
    results that follow from the selection (best_h / best_f, the branch, n_good, best_motion, success, triangulated
    exactly; the matrices, R21, t21, P3D within the bound) are compared when no hypothesis is left out, the winners are
    clear of the bound, and no eigenvalue gap or threshold of the reconstruction is closer than GAP / the margin.
    fp64: the module tests/init_fp64.py; main() and the fuzz test pass it (the tool itself needs nothing of tests/ but the
    model).  A scene where something is left out is then held to float64 instead, stage by stage on its own result (rungs
    3, 4, 6 and 7; the winners' matrices are in the result, so nothing more is launched): fp64_scenes counts them,
    fp64_hypotheses the left-out hypotheses in them.
    Returns a dict: spread, bound, margin (the largest of the scenes; each scene is compared within its own), device_dev,
    left_out (largest share of a scene), mismatches (strings)."""
    if passes is None:
        passes = [M.model_pass(sc) for sc in scenes]
    spread = max([s for _, s in passes] + [0.0])
    rep = {"spread": spread, "bound": M.BOUND_FACTOR * spread, "margin": M.MARGIN_FACTOR * M.BOUND_FACTOR * spread, "device_dev": 0.0,
           "left_out": 0.0, "hypotheses": 0, "hypotheses_left_out": 0, "downstream_compared": 0, "fp64_scenes": 0,
           "fp64_hypotheses": 0, "mismatches": []}
    bad = rep["mismatches"]
    for i, (sc, (m, own), r) in enumerate(zip(scenes, passes, got)):
        tag = "scene %d (%s, N %d): " % (i, sc.get("kind", "?"), m["N"])
        # every scene is held to its own spread, never to a wider one of the batch: a scene whose two model paths agree in
        # every float is compared bit for bit
        bound = M.BOUND_FACTOR * own
        margin = M.MARGIN_FACTOR * bound
        for k, mk in (("n", "N"), ("n_bad_index", "n_bad_index"), ("n_bad_set", "n_bad_set")):
            if r[k] != m[mk]:
                bad.append(tag + "%s %d, model %d" % (k, r[k], m[mk]))
        H = len(m["scores_h"])
        outs = M.left_out(m, bound)
        n_out = int(outs[0].sum() + outs[1].sum())
        rep["hypotheses"] += 2 * H
        rep["hypotheses_left_out"] += n_out
        if H:
            share = n_out / (2.0 * H)
            rep["left_out"] = max(rep["left_out"], share)
            if share > M.LEFT_OUT_CAP:
                bad.append(tag + "%d of %d hypotheses left out" % (n_out, 2 * H))
        if n_out and fp64 is not None:
            rungs = fp64.ladder(sc, r, None, G.initializer_cos_limits(sc.get("min_parallax", 1.0)), only=("rung3", "rung4", "rung6", "rung7"))
            bad += [tag + "float64 " + v for v in fp64.violations(rungs)]
            rep["fp64_scenes"] += 1
            rep["fp64_hypotheses"] += n_out
        for out, name in zip(outs, "hf"):
            keep = ~out
            if not np.array_equal(r["masks_" + name][keep], m["masks_" + name][keep]):
                w = np.flatnonzero((r["masks_" + name][keep] != m["masks_" + name][keep]).any(1))
                bad.append(tag + "%d %s masks differ, first hypothesis %d" % (len(w), name.upper(), np.flatnonzero(keep)[w[0]]))
            dv = M.dev(m["scores_" + name][keep], r["scores_" + name][keep])
            rep["device_dev"] = max(rep["device_dev"], dv)
            if not dv <= bound:
                bad.append(tag + "%s scores off by %.3e, allowed %.3e" % (name.upper(), dv, bound))
        clear = n_out == 0 and _clear_winner(m["scores_h"], m["best_h"], bound) and _clear_winner(m["scores_f"], m["best_f"], bound)
        clear = clear and (bound == 0.0 or abs(float(m["RH"]) - 0.40) > 2.0 * bound)
        clear = clear and m["svd_gap"] >= M.GAP and m["rt_gap"] >= M.GAP and m["rt_near"] >= margin
        if not clear:
            continue
        rep["downstream_compared"] += 1
        for k in ("best_h", "best_f", "used_homography", "n_inliers", "best_motion", "second_best_good", "success"):
            if int(r[k]) != int(m[k]):
                bad.append(tag + "%s %d, model %d" % (k, int(r[k]), int(m[k])))
        if not np.array_equal(r["n_good"], m["n_good"]):
            bad.append(tag + "n_good %s, model %s" % (r["n_good"].tolist(), m["n_good"].tolist()))
        if not np.array_equal(r["triangulated"], m["triangulated"]):
            bad.append(tag + "triangulated differs")
        for k in ("SH", "SF", "H21", "F21", "R21", "t21", "P3D", "cos_parallax"):
            dv = M.dev(m[k], r[k])
            rep["device_dev"] = max(rep["device_dev"], dv)
            if not dv <= bound:
                bad.append(tag + "%s off by %.3e, allowed %.3e" % (k, dv, bound))
        if M.dev(r["R21"], r["R21_out"]) != 0.0 or M.dev(r["t21"], r["t21_out"]) != 0.0:
            bad.append(tag + "the R21 / t21 arrays differ from the result's")
    return rep


def draw_scene(rng):
    n = int(rng.choice([8, 9, 63, 64, 65, 300, 1000]) if rng.random() < 0.5 else rng.integers(8, 1200))
    kind = str(rng.choice(["general", "general", "planar", "rotation", "few"]))
    return M.make_scene(n, int(rng.integers(1 << 31)), kind, n_hyp=int(rng.choice([1, 5, 24, 200])),
                        n1=n + int(rng.integers(0, n + 5)), n2=n + int(rng.integers(0, n + 5)),
                        noise_px=float(rng.uniform(0.1, 1.0)), outlier_frac=float(rng.choice([0.0, 0.1, 0.3])))


def run(seconds, seed, batch=4, fp64=None):
    import torch
    rng = np.random.default_rng(seed)
    tot = {"rounds": 0, "scenes": 0, "hypotheses": 0, "hypotheses_left_out": 0, "downstream_compared": 0, "fp64_scenes": 0,
           "fp64_hypotheses": 0, "spread": 0.0, "device_dev": 0.0, "left_out": 0.0, "mismatches": []}
    t_end = time.time() + seconds
    while True:
        scenes = [draw_scene(rng) for _ in range(batch)]
        rep = compare(scenes, run_batch(torch, scenes), fp64=fp64)
        tot["rounds"] += 1
        tot["scenes"] += len(scenes)
        # a drawn scene may leave out more than the cap (the committed parity scenes may not): that is reported, not failed
        tot["mismatches"] += [m for m in rep["mismatches"] if "hypotheses left out" not in m]
        for k in ("hypotheses", "hypotheses_left_out", "downstream_compared", "fp64_scenes", "fp64_hypotheses"):
            tot[k] += rep[k]
        for k in ("spread", "device_dev", "left_out"):
            tot[k] = max(tot[k], rep[k])
        if time.time() >= t_end:
            return tot


def report(tot):
    return ["rounds %d, scenes %d (%d compared to the end), hypotheses %d, left out %d (largest share of a scene %.3f), "
            "mismatches %d" % (tot["rounds"], tot["scenes"], tot["downstream_compared"], tot["hypotheses"],
                               tot["hypotheses_left_out"], tot["left_out"], len(tot["mismatches"])),
            "model spread <= %.3e, device deviation <= %.3e (vs CPU restatement; OpenCV boundary unpinned)" % (
                tot["spread"], tot["device_dev"]),
            "float64 by stage (checks of the winners, selection, CheckRT, accept rule) on the %d scenes that left something out: "
            "they hold %d of the %d left-out hypotheses" % (tot["fp64_scenes"], tot["fp64_hypotheses"], tot["hypotheses_left_out"])] + [
                "  " + m for m in tot["mismatches"][:20]]


def main():
    import init_fp64
    tot = run(float(sys.argv[1]), int(sys.argv[2]), fp64=init_fp64)
    print("\n".join(report(tot)))
    sys.exit(1 if tot["mismatches"] else 0)


if __name__ == "__main__":
    main()
