"""Randomised comparison of the PnP solver on the device (orbgpu_pnp_solve_batch_device) with the CPU model
(tests/pnp_model.py) -- vs CPU restatement; OpenCV boundary unpinned.

usage: python tools/fuzz_pnp.py SECONDS SEED

Each round draws a batch of seeded frames (size, share of invalid rows and of gross outliers, noise, minimal set of 4, 5
or 6, number of hypotheses), solves them in ONE batched call and compares them with the model as compare() describes.
The constants of the comparison (GAP, BOUND_FACTOR, MARGIN_FACTOR, LEFT_OUT_CAP) and their reasoning are in
tests/pnp_model.py, next to the scenes they are derived for.  Exit status 1 on any mismatch."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pnp_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402


def upload(torch, sc, start_iteration=0, best_so_far=0, n_iterations=0):
    """Device arrays of one scene; returns (problem dict for lib.pnp_solve_batch_device, keep-alive dict)."""
    n1, sets = len(sc["valid"]), np.ascontiguousarray(sc["sets"], np.int32).reshape(-1, int(sc["min_set"]))
    H, words = len(sets), (n1 + 63) // 64
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device="cuda")  # noqa: E731
    d = {"valid": dev(np.asarray(sc["valid"], np.uint8)) if n1 else z(1, torch.uint8),
         "Xw": dev(np.asarray(sc["Xw"], np.float32)) if n1 else z(3, torch.float32),
         "kp": dev(np.asarray(sc["kp"], np.float32)) if n1 else z(2, torch.float32),
         "octave": dev(np.asarray(sc["octave"], np.int32)) if n1 else z(1, torch.int32),
         "sets": dev(sets) if H else z(4, torch.int32),
         "counts": torch.full((max(H, 1),), -7, dtype=torch.int32, device="cuda"), "Tcw": z(16 * H, torch.float32),
         "masks": z(H * words, torch.int64), "refined_mask": z(words, torch.int64),
         "indices": torch.full((max(n1, 1),), -1, dtype=torch.int32, device="cuda"),
         "result": torch.zeros(C.sizeof(G.PnpResult), dtype=torch.uint8, device="cuda")}
    p = {k: sc[k] for k in ("K", "level_sigma2", "min_set", "min_inliers", "max_iterations", "epsilon", "th2", "probability")}
    p.update(n1=n1, n_hyp=H, start_iteration=start_iteration, best_so_far=best_so_far, n_iterations=n_iterations)
    if "nlevels" in sc:
        p["nlevels"] = sc["nlevels"]
    p.update({k: v.data_ptr() for k, v in d.items()})
    return p, d


def download(d, sc):
    n1, H = len(sc["valid"]), len(np.asarray(sc["sets"]).reshape(-1, int(sc["min_set"])))
    words = (n1 + 63) // 64
    r = G.PnpResult.from_buffer_copy(d["result"].cpu().numpy().tobytes()).as_dict()
    r.update(counts=d["counts"].cpu().numpy()[:H].copy(), Tcw_all=d["Tcw"].cpu().numpy()[:16 * H].reshape(H, 4, 4),
             masks=d["masks"].cpu().numpy()[:H * words].view(np.uint64).reshape(H, words),
             refined_mask=d["refined_mask"].cpu().numpy()[:words].view(np.uint64).copy(),
             indices=d["indices"].cpu().numpy()[:n1].copy())
    return r


RESULT_KEYS = ("n", "min_inliers", "max_its", "n_bad_index", "n_bad_set", "accepted", "n_inliers", "best_inliers",
               "best_iteration", "iterations", "no_more")


def result_bytes(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("counts", "Tcw_all", "masks", "refined_mask", "indices", "Tcw")) + \
        repr([r[k] for k in RESULT_KEYS]).encode()


def run_batch(torch, scenes, **kw):
    ups = [upload(torch, sc, **kw) for sc in scenes]
    G.pnp_solve_batch_device([u[0] for u in ups], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [download(u[1], sc) for u, sc in zip(ups, scenes)]


def compare(scenes, got, passes=None):
    """Model against device.  passes: [(model, spread)] from M.model_pass, computed here if missing.  Returns a dict:
    spread, bound, margin, device_dev, left_out (largest share of a scene), mismatches (strings)."""
    if passes is None:
        passes = [M.model_pass(sc) for sc in scenes]
    spread = max([s for _, s in passes] + [0.0])
    bound = M.BOUND_FACTOR * spread
    rep = {"spread": spread, "bound": bound, "margin": M.MARGIN_FACTOR * bound, "device_dev": 0.0, "left_out": 0.0,
           "hypotheses": 0, "hypotheses_left_out": 0, "mismatches": []}
    bad = rep["mismatches"]
    for i, (sc, (m, _), r) in enumerate(zip(scenes, passes, got)):
        tag = "scene %d (N %d, set %d): " % (i, m["N"], sc["min_set"])
        for k, mk in (("n", "N"), ("min_inliers", "min_inliers"), ("max_its", "max_its"), ("n_bad_index", "n_bad_index"),
                      ("n_bad_set", "n_bad_set")):
            if r[k] != m[mk]:
                bad.append(tag + "%s %d, model %d" % (k, r[k], m[mk]))
        if not np.array_equal(r["indices"][:m["N"]], m["indices"]):
            bad.append(tag + "indices differ")
        u = m["n_use"]
        out = M.left_out(m, bound)
        rep["hypotheses"] += u
        rep["hypotheses_left_out"] += int(out.sum())
        if u:
            rep["left_out"] = max(rep["left_out"], float(out.mean()))
            if out.mean() > M.LEFT_OUT_CAP:
                bad.append(tag + "%d of %d hypotheses left out" % (out.sum(), u))
        keep = ~out
        if not np.array_equal(r["counts"][:u][keep], m["counts"][:u][keep]):
            w = np.flatnonzero(r["counts"][:u][keep] != m["counts"][:u][keep])
            bad.append(tag + "%d counts differ, first hypothesis %d: %d, model %d" % (
                len(w), np.flatnonzero(keep)[w[0]], r["counts"][:u][keep][w[0]], m["counts"][:u][keep][w[0]]))
        if (r["counts"][u:] != 0).any():
            bad.append(tag + "counts beyond n_use are not 0")
        if not np.array_equal(r["masks"][:u][keep], m["masks"][:u][keep]):
            bad.append(tag + "mask words differ")
        pop = np.unpackbits(np.ascontiguousarray(r["masks"][:u]).view(np.uint8).reshape(u, -1), axis=1).sum(1) if u else np.zeros(0)
        if (pop != r["counts"][:u]).any():
            bad.append(tag + "a count is not the popcount of its mask")
        dv = M.dev(m["Tcw"][:u][keep], r["Tcw_all"][:u][keep])
        rep["device_dev"] = max(rep["device_dev"], dv)
        if not dv <= bound:
            bad.append(tag + "Tcw off by %.3e, allowed %.3e" % (dv, bound))
        # the record-dependent results: compared when no hypothesis the model's scan read was left out and no refine it
        # ran was ill-conditioned or near a threshold
        scanned = out[:m["iterations"]].any()
        for h, rf in m["refined"].items():
            scanned |= rf["gap"] < M.GAP or rf["thr"] < M.THR_DECADES or rf["choice"] <= bound or rf["near"] < M.MARGIN_FACTOR * bound
        if not scanned:
            for k in ("accepted", "n_inliers", "best_inliers", "best_iteration", "iterations", "no_more"):
                if r[k] != int(m[k]):
                    bad.append(tag + "%s %d, model %d" % (k, r[k], int(m[k])))
            if not np.array_equal(r["refined_mask"], m["refined_mask"]):
                bad.append(tag + "the returned mask differs")
            dv = M.dev(m["refined_Tcw"], r["Tcw"])
            rep["device_dev"] = max(rep["device_dev"], dv)
            if not dv <= bound:
                bad.append(tag + "returned Tcw off by %.3e, allowed %.3e" % (dv, bound))
    return rep


def draw_scene(rng):
    n = int(rng.choice([3, 9, 10, 11, 63, 64, 65, 300, 1000]) if rng.random() < 0.5 else rng.integers(3, 1200))
    return M.make_scene(n, int(rng.integers(1 << 31)), n1=n + int(rng.integers(0, n + 5)), n_hyp=int(rng.choice([1, 5, 60, 300])),
                        min_set=int(rng.choice([4, 4, 5, 6])), outlier_frac=float(rng.choice([0.0, 0.1, 0.3, 0.5])),
                        noise_px=float(rng.uniform(0.2, 1.0)))


def run(seconds, seed, batch=4):
    import torch
    rng = np.random.default_rng(seed)
    tot = {"rounds": 0, "scenes": 0, "hypotheses": 0, "hypotheses_left_out": 0, "spread": 0.0, "device_dev": 0.0, "left_out": 0.0,
           "mismatches": []}
    t_end = time.time() + seconds
    while True:
        scenes = [draw_scene(rng) for _ in range(batch)]
        rep = compare(scenes, run_batch(torch, scenes))
        tot["rounds"] += 1
        tot["scenes"] += len(scenes)
        # a drawn scene may leave out more than the cap (the committed parity scenes may not): that is reported, not failed
        tot["mismatches"] += [m for m in rep["mismatches"] if "hypotheses left out" not in m]
        for k in ("hypotheses", "hypotheses_left_out"):
            tot[k] += rep[k]
        for k in ("spread", "device_dev", "left_out"):
            tot[k] = max(tot[k], rep[k])
        if time.time() >= t_end:
            return tot


def main():
    tot = run(float(sys.argv[1]), int(sys.argv[2]))
    print("rounds %d, scenes %d, hypotheses %d, left out %d (largest share of a scene %.3f), mismatches %d" % (
        tot["rounds"], tot["scenes"], tot["hypotheses"], tot["hypotheses_left_out"], tot["left_out"], len(tot["mismatches"])))
    print("model spread <= %.3e, device deviation <= %.3e (vs CPU restatement; OpenCV boundary unpinned)" % (
        tot["spread"], tot["device_dev"]))
    for m in tot["mismatches"][:20]:
        print("  " + m)
    sys.exit(1 if tot["mismatches"] else 0)


if __name__ == "__main__":
    main()
