"""Randomised comparison of Frame::ComputeStereoMatches on the device with the CPU model (tests/stereo_model.py).

usage: python tools/fuzz_stereo.py SECONDS SEED

Each round draws an image size, feature count, scale factor, level count, depth range, mbf, and shared or separate
extractor handles (now and then a scene mirrored about its middle column, where crafted key points reach the
zero-disparity clamp); extracts a synthetic stereo pair (GPU and oracle key points must agree), then compares u_right /
depth bit for bit on the extractor's lists and on crafted lists (stereo_model.craft_lists).  Separate handles go
through the host entry point, a shared handle (one call of 2 frames) through the batched device entry point.
Prints the count of every model branch reached and the mismatches; exit status 1 on any mismatch."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stereo_model as M  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402
from orb_slam2_map_amd.synth import StereoStream  # noqa: E402


def device_pair(torch, ext, left, right, kl, dl, kr, dr, mbf, fx):
    """The batched device entry point on frames 0 / 1 of one handle's last call, for host lists."""
    cap = max(len(kl), len(kr), 1)

    def up(a, shape, dtype):
        t = torch.zeros(shape, dtype=dtype, device="cuda")
        if len(a):
            t[:len(a)] = torch.from_numpy(np.ascontiguousarray(a))
        return t
    k_l = up(kl.view(np.float32).reshape(-1, 7), (cap, 7), torch.float32)
    k_r = up(kr.view(np.float32).reshape(-1, 7), (cap, 7), torch.float32)
    d_l = up(dl, (cap, 32), torch.uint8)
    d_r = up(dr, (cap, 32), torch.uint8)
    n = torch.tensor([len(kl), len(kr)], dtype=torch.int32, device="cuda")
    u = torch.zeros(cap, dtype=torch.float32, device="cuda")
    z = torch.zeros(cap, dtype=torch.float32, device="cuda")
    G.stereo_matches_batch_device(ext, 0, ext, 1, 1, cap, k_l.data_ptr(), n.data_ptr(), d_l.data_ptr(), k_r.data_ptr(),
                                  n.data_ptr() + 4, d_r.data_ptr(), mbf, fx, u.data_ptr(), z.data_ptr(), None, 0)
    torch.cuda.synchronize()
    return u.cpu().numpy()[:len(kl)], z.cpu().numpy()[:len(kl)]


def main():
    seconds, seed = float(sys.argv[1]), int(sys.argv[2])
    import torch
    rng = np.random.default_rng(seed)
    seen = np.zeros(len(M.REASONS), np.int64)
    rounds = lists = mismatches = 0
    t_end = time.time() + seconds
    while time.time() < t_end:
        w, h = int(rng.integers(240, 1300)), int(rng.integers(200, 500))
        nf = int(rng.integers(200, 2500))
        sf = float(rng.choice([1.1, 1.2, 1.25, 1.3, 1.4]))
        nl = int(rng.integers(2, 9))
        if min(w, h) / sf ** (nl - 1) < 70:
            continue
        zmin = float(rng.uniform(3, 15))
        st = StereoStream(w, h, int(rng.integers(0, 1 << 30)), zmin=zmin, zmax=zmin * float(rng.uniform(2, 10)))
        left, right, _ = st.frame(int(rng.integers(0, 50)))
        mirrored = rng.random() < 0.15  # a scene symmetric about its middle column: zero disparities (the 0.01 clamp)
        if mirrored:
            left, right = M.mirrored_pair(w, h, w // 2, int(rng.integers(0, 1 << 30)))
        mbf = np.float32(st.bf * float(rng.choice([1.0, 1.0, 0.5, 0.05, 3.0])))
        shared = bool(rng.integers(0, 2))
        try:  # sizes the extractor refuses (a level's aspect ratio leaves no FAST cell, EINVAL) are not stereo cases
            if shared:
                ext = G.ORBextractor(nf, sf, nl, max_batch=2)
                (kl, kr), (dl, dr) = ext.extract_batch(np.stack([left, right]))
            else:
                el, er = G.ORBextractor(nf, sf, nl), G.ORBextractor(nf, sf, nl)
                kl, dl = el(left)
                kr, dr = er(right)
        except G.OrbGpuError as e:
            if e.status != G.EINVAL:
                raise
            continue
        ol, orr = O.Extractor(nf, sf, nl), O.Extractor(nf, sf, nl)
        okl, odl = ol.extract(left)
        okr, odr = orr.extract(right)
        if kl.tobytes() != okl.tobytes() or kr.tobytes() != okr.tobytes():
            print("extractor mismatch (not a stereo finding): %dx%d nf %d sf %g nl %d" % (w, h, nf, sf, nl))
            mismatches += 1
            continue
        pl, pr = M.oracle_planes(ol), M.oracle_planes(orr)
        rounds += 1
        extra = M.clamp_keys(kl, dl, kr, dr, w // 2, h) if mirrored else M.craft_lists(kl, dl, kr, dr, rng, w, h, nl)
        for lst in ((kl, dl, kr, dr), extra):
            u, d, reason = M.stereo_matches(*lst, pl, pr, ol.scale_factors(), ol.inv_scale_factors(), mbf, st.fx)
            if shared:
                gu, gd = device_pair(torch, ext, left, right, *lst, mbf, st.fx)
            else:
                gu, gd = G.compute_stereo_matches(el, er, *lst, mbf, st.fx)
            lists += 1
            seen += np.bincount(reason, minlength=len(M.REASONS))
            if not (np.array_equal(gu.view(np.int32), u.view(np.int32)) and np.array_equal(gd.view(np.int32), d.view(np.int32))):
                mismatches += 1
                bad = np.nonzero((gu.view(np.int32) != u.view(np.int32)) | (gd.view(np.int32) != d.view(np.int32)))[0]
                print("MISMATCH %dx%d nf %d sf %g nl %d mbf %g shared %d: %d key points, first %s" %
                      (w, h, nf, sf, nl, mbf, shared, len(bad), bad[:5].tolist()))
    print("branches: " + ", ".join("%s %d" % (r, c) for r, c in zip(M.REASONS, seen)))
    print("rounds %d lists %d mismatches %d" % (rounds, lists, mismatches))
    return 1 if mismatches else 0


if __name__ == "__main__":
    sys.exit(main())
