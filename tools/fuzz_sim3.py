"""Randomised comparison of the Sim3 solver on the device (orbgpu_sim3_solve_batch_device) with the CPU model
(tests/sim3_model.py) -- vs CPU restatement; OpenCV boundary unpinned.

usage: python tools/fuzz_sim3.py SECONDS SEED

Each round draws a batch of seeded key-frame pairs (size, share of invalid rows and of gross outliers, noise, fixed or free
scale, number of hypotheses), solves them in ONE batched call and compares them with the model as compare() describes.
Exit status 1 on any mismatch or if a scene leaves out more than 10 % of its hypotheses."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sim3_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402

# A hypothesis whose two largest eigenvalues differ by less than GAP (relative to the largest magnitude) is left out:
# an eigenvector moves by about 2^-53 / gap under a change of algorithm, and at 1e-6 that is 1e-10, three orders below
# the resolution of the float32 R it is rounded to; below that gap the vector is not a property of the definition.
GAP = 1e-6
# Continuous outputs may deviate by BOUND_FACTOR x the model's own spread (Jacobi against numpy.linalg.eigh), both
# measured as |a - b| / max(1, |a|) over R, t, s and T12.
BOUND_FACTOR = 16.0
# From that bound B to err: an entry of T12 / T21 moves by at most B max(1, |entry|), so a camera-frame coordinate by at
# most B (|X| + |Y| + |Z| + max(1, |t|)) <= 16 B in make_scene's geometry (coordinates within 2 + 2 + 8, |t| < 4); a pixel
# by at most fx / z (1 + |x / z|) times that <= 500 / 1 x 4 x 16 B (depth >= 1, |x / z| <= 3); err = d'd by 2 |d| times the
# pixel shift, so err / maxError at the threshold (|d| = sqrt(maxError) >= 3) by 2 x 32000 B / 3 < 2.2e4 B.  A (hypothesis,
# point) pair with |err / maxError - 1| below MARGIN_FACTOR x B is not compared, nor is a hypothesis that holds one.
MARGIN_FACTOR = 2.2e4
LEFT_OUT_CAP = 0.10


def upload(torch, sc, start_iteration=0, best_so_far=0):
    """Device arrays of one scene; returns (problem dict for lib.sim3_solve_batch_device, keep-alive dict)."""
    n1, tri = len(sc["valid"]), np.ascontiguousarray(sc["triples"], np.int32).reshape(-1, 3)
    H, words = len(tri), (len(sc["valid"]) + 63) // 64
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device="cuda")  # noqa: E731
    d = {"valid": dev(np.asarray(sc["valid"], np.uint8)) if n1 else z(1, torch.uint8),
         "Xw1": dev(np.asarray(sc["Xw1"], np.float32)) if n1 else z(3, torch.float32),
         "Xw2": dev(np.asarray(sc["Xw2"], np.float32)) if n1 else z(3, torch.float32),
         "octave1": dev(np.asarray(sc["octave1"], np.int32)) if n1 else z(1, torch.int32),
         "octave2": dev(np.asarray(sc["octave2"], np.int32)) if n1 else z(1, torch.int32),
         "triples": dev(tri) if H else z(3, torch.int32),
         "counts": torch.full((max(H, 1),), -7, dtype=torch.int32, device="cuda"), "R": z(9 * H, torch.float32),
         "t": z(3 * H, torch.float32), "s": z(H, torch.float32), "T12": z(16 * H, torch.float32),
         "masks": z(H * words, torch.int64), "indices1": torch.full((max(n1, 1),), -1, dtype=torch.int32, device="cuda"),
         "result": torch.zeros(C.sizeof(G.Sim3Result), dtype=torch.uint8, device="cuda")}
    p = {k: sc[k] for k in ("T1w", "T2w", "K1", "K2", "level_sigma2", "fix_scale", "probability", "min_inliers", "max_iterations")}
    p.update(n1=n1, n_hyp=H, start_iteration=start_iteration, best_so_far=best_so_far)
    if "nlevels" in sc:
        p["nlevels"] = sc["nlevels"]
    p.update({k: v.data_ptr() for k, v in d.items()})
    return p, d


def download(d, sc):
    n1, H = len(sc["valid"]), len(np.asarray(sc["triples"]).reshape(-1, 3))
    words = (n1 + 63) // 64
    raw = d["result"].cpu().numpy().tobytes()
    r = G.Sim3Result.from_buffer_copy(raw).as_dict()
    r.update(counts=d["counts"].cpu().numpy()[:H].copy(), R=d["R"].cpu().numpy()[:9 * H].reshape(H, 3, 3),
             t=d["t"].cpu().numpy()[:3 * H].reshape(H, 3), s=d["s"].cpu().numpy()[:H], T12=d["T12"].cpu().numpy()[:16 * H].reshape(H, 4, 4),
             masks=d["masks"].cpu().numpy()[:H * words].view(np.uint64).reshape(H, words), indices1=d["indices1"].cpu().numpy()[:n1].copy())
    return r


def result_bytes(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("counts", "R", "t", "s", "T12", "masks", "indices1")) + repr(
        [r[k] for k, _ in G.Sim3Result._fields_]).encode()


def run_batch(torch, scenes, **kw):
    ups = [upload(torch, sc, **kw) for sc in scenes]
    G.sim3_solve_batch_device([u[0] for u in ups], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [download(u[1], sc) for u, sc in zip(ups, scenes)]


def _dev(a, b):
    """largest |a - b| / max(1, |a|); NaN against NaN is no deviation, NaN against a number is infinite"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    na, nb = np.isnan(a), np.isnan(b)
    if (na != nb).any():
        return float("inf")
    ok = ~na
    with np.errstate(all="ignore"):
        d = np.abs(a[ok] - b[ok]) / np.maximum(1.0, np.abs(a[ok]))
    d = np.where(np.isnan(d), 0.0 if np.array_equal(a[ok], b[ok]) else np.inf, d)
    return float(d.max()) if d.size else 0.0


def model_pass(scenes):
    """The CPU half: per scene the model, and the spread between the model and itself with eigh in place of its Jacobi
    over the hypotheses with gap >= GAP.  Returns (models, spread)."""
    models, spread = [], 0.0
    for sc in scenes:
        m, e = M.solve(sc), M.solve(sc, eig="eigh")
        u = m["n_use"]
        ok = m["gap"][:u] >= GAP
        m["well"] = ok
        for k in ("R", "t", "s", "T12"):
            spread = max(spread, _dev(m[k][:u][ok], e[k][:u][ok]))
        models.append(m)
    return models, spread


def left_out(m, margin):
    """mask over the used hypotheses: ill-conditioned, or holding a near-threshold pair"""
    u = m["n_use"]
    return ~m["well"] | (m["near"][:u] < margin)


def compare(scenes, got, models=None, spread=None):
    """Model against device.  Returns a dict: spread, bound, margin, device_dev, left_out (largest share of a scene),
    mismatches (strings)."""
    if models is None:
        models, spread = model_pass(scenes)
    bound = BOUND_FACTOR * spread
    margin = MARGIN_FACTOR * bound
    rep = {"spread": spread, "bound": bound, "margin": margin, "device_dev": 0.0, "left_out": 0.0, "hypotheses": 0,
           "hypotheses_left_out": 0, "mismatches": []}
    for i, (sc, m, r) in enumerate(zip(scenes, models, got)):
        tag = "scene %d (N %d): " % (i, m["N"])
        bad = rep["mismatches"]
        for k, mk in (("n", "N"), ("max_its", "max_its"), ("n_bad_index", "n_bad_index"), ("n_bad_triple", "n_bad_triple")):
            if r[k] != m[mk]:
                bad.append(tag + "%s %d, model %d" % (k, r[k], m[mk]))
        if not np.array_equal(r["indices1"][:m["N"]], m["indices1"]):
            bad.append(tag + "indices1 differ")
        u = m["n_use"]
        out = left_out(m, margin)
        rep["hypotheses"] += u
        rep["hypotheses_left_out"] += int(out.sum())
        if u:
            rep["left_out"] = max(rep["left_out"], float(out.mean()))
            if out.mean() > LEFT_OUT_CAP:
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
        for k in ("R", "t", "s", "T12"):
            dv = _dev(m[k][:u][keep], r[k][:u][keep])
            rep["device_dev"] = max(rep["device_dev"], dv)
            if not dv <= bound:
                bad.append(tag + "%s off by %.3e, allowed %.3e" % (k, dv, bound))
        # the acceptance rule over the device's own counts, always; against the model's when no hypothesis that the scan
        # read was left out
        st = M.RansacState(r["n"], sc["min_inliers"], r["max_its"])
        acc, n_inl, no_more = st.iterate(u, r["counts"]) if (u or r["n"] < sc["min_inliers"]) else (-1, 0, False)
        want = {"accepted": acc, "n_inliers": n_inl, "no_more": int(no_more), "best_inliers": st.best,
                "best_iteration": st.best_iteration, "iterations": st.iterations}
        for k, v in want.items():
            if r[k] != v:
                bad.append(tag + "%s %d, replayed over the device's counts %d" % (k, r[k], v))
        if not out[:m["iterations"]].any():
            for k in want:
                if r[k] != int(m[k]):
                    bad.append(tag + "%s %d, model %d" % (k, r[k], int(m[k])))
    return rep


def draw_scene(rng):
    n = int(rng.choice([3, 19, 20, 21, 63, 64, 65, 300, 1000]) if rng.random() < 0.5 else rng.integers(3, 1200))
    return M.make_scene(n, int(rng.integers(1 << 31)), n1=n + int(rng.integers(0, n + 5)), n_hyp=int(rng.choice([1, 5, 60, 300])),
                        fix_scale=bool(rng.integers(2)), outlier_frac=float(rng.choice([0.0, 0.1, 0.3, 0.5])),
                        noise_px=float(rng.uniform(0.2, 1.0)))


def run(seconds, seed, batch=8):
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
        tot["mismatches"] += rep["mismatches"]
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
