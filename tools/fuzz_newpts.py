"""Randomised comparison of LocalMapping::CreateNewMapPoints on the device with the CPU model (tests/newpts_model.py; vs
CPU restatement, OpenCV boundary unpinned).

usage: python tools/fuzz_newpts.py SECONDS SEED
       python tools/fuzz_newpts.py --record      (the parity scenes' figures -> profiles/newpts_parity.json)

Each round draws a seeded scene (sensor mix, key-point counts, neighbour count, noise, flags), runs it through the device
flavour and compares it with newpts_model.compare: match12, status and the counts exactly outside the margins, x3d within
16 x the model's spread (bit for bit at spread 0), every stage on the device's own upstream output.  The host flavour must
give the device flavour's bytes.  Exit status 1 on any mismatch."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import newpts_model as M  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402

OUT_KEYS = ("match12", "status", "x3d", "n_matches", "n_created")


def _device_frame(torch, f, keep):
    d = dict(f)
    d["n"] = len(f["kp_x"])
    for (k, t) in G._NP_ARRAYS:
        a = f.get(k)
        if a is None or len(a) == 0:
            d[k] = None
            continue
        tens = torch.from_numpy(np.ascontiguousarray(a, t)).cuda()
        keep.append(tens)
        d[k] = tens.data_ptr()
    return d


def run_device(torch, sc, stop=None, sentinel=True):
    """The device flavour on the current stream; outputs start as garbage (the call must overwrite all of them)."""
    keep = []
    nn, n1 = len(sc["neighbours"]), len(sc["kf1"]["kp_x"])
    fill = 77 if sentinel else 0
    o = {"match12": torch.full((max(nn * n1, 1),), fill, dtype=torch.int32, device="cuda"),
         "status": torch.full((max(nn * n1, 1),), fill, dtype=torch.int32, device="cuda"),
         "x3d": torch.full((max(nn * n1 * 3, 1),), float(fill), dtype=torch.float32, device="cuda"),
         "n_matches": torch.full((max(nn, 1),), fill, dtype=torch.int32, device="cuda"),
         "n_created": torch.full((max(nn, 1),), fill, dtype=torch.int32, device="cuda"),
         "n_done": torch.full((1,), fill, dtype=torch.int32, device="cuda")}
    ptrs = {k: v.data_ptr() for k, v in o.items()}
    if stop is not None:
        flag = torch.tensor([int(stop)], dtype=torch.int32, device="cuda")
        keep.append(flag)
        ptrs["stop"] = flag.data_ptr()
    G.create_new_map_points_device(_device_frame(torch, sc["kf1"], keep), [_device_frame(torch, f, keep) for f in sc["neighbours"]],
                                   sc["ratio_factor"], sc["only_stereo"], sc["check_ori"],
                                   stream=torch.cuda.current_stream().cuda_stream, **ptrs)
    torch.cuda.synchronize()
    return {"match12": o["match12"].cpu().numpy()[:nn * n1].reshape(nn, n1), "status": o["status"].cpu().numpy()[:nn * n1].reshape(nn, n1),
            "x3d": o["x3d"].cpu().numpy()[:nn * n1 * 3].reshape(nn, n1, 3), "n_matches": o["n_matches"].cpu().numpy()[:nn],
            "n_created": o["n_created"].cpu().numpy()[:nn], "n_done": int(o["n_done"].cpu().numpy()[0])}


def run_host(sc, stop=None):
    return G.create_new_map_points(sc["kf1"], sc["neighbours"], sc["ratio_factor"], sc["only_stereo"], sc["check_ori"], stop=stop)


def same_bytes(a, b):
    return a["n_done"] == b["n_done"] and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in OUT_KEYS)


def check_scene(torch, sc):
    """figures of one scene (model spread, margin bound, the comparison's); raises AssertionError on a mismatch"""
    _, spread, _, _ = M.model_pass(sc)
    bound = M.BOUND_FACTOR * spread
    d = run_device(torch, sc)
    fig = M.compare(sc, d, bound)
    assert same_bytes(d, run_host(sc)), "host and device flavours differ"
    fig.update(spread=spread, bound=bound, reproj_margin=M.REPROJ_MARGIN_FACTOR * bound, created=int(d["n_created"].sum()))
    return fig


def draw_scene(rng):
    nn = int(rng.integers(1, 5))
    return M.make_scene(int(rng.integers(1, 1 << 30)), mix=("mono", "stereo", "mixed")[int(rng.integers(0, 3))],
                        n1=int(rng.integers(1, 200)), n2=tuple(int(rng.integers(0, 180)) for _ in range(nn)),
                        noise=float(rng.choice([0.0, 0.3, 0.8])), only_stereo=bool(rng.random() < 0.2),
                        check_ori=bool(rng.random() < 0.7), has_frac=float(rng.choice([0.0, 0.2, 0.6])))


def run(seconds, seed):
    import torch
    rng = np.random.default_rng(seed)
    tot = {"scenes": 0, "matched": 0, "left_out": 0, "created": 0, "x3d_deviation": 0.0, "mismatches": []}
    t0 = time.time()
    while time.time() - t0 < seconds:
        sc = draw_scene(rng)
        tot["scenes"] += 1
        try:
            fig = check_scene(torch, sc)
        except AssertionError as e:
            tot["mismatches"].append("scene %d: %s" % (tot["scenes"], e))
            continue
        tot["matched"] += fig["matched"]
        tot["left_out"] += fig["left_out"]
        tot["created"] += fig["created"]
        tot["x3d_deviation"] = max(tot["x3d_deviation"], fig["x3d_deviation"])
    return tot


def record():
    import torch
    doc = {"note": "vs CPU restatement; OpenCV boundary unpinned", "bound_factor": M.BOUND_FACTOR, "scenes": {}}
    for name in M.SCENES:
        doc["scenes"][name] = check_scene(torch, M.scene(name))
    path = os.path.join(ROOT, "profiles", "newpts_parity.json")
    out = os.environ.get("NEWPTS_PARITY_OUT", path)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


def main():
    if sys.argv[1:] == ["--record"]:
        record()
        return 0
    tot = run(float(sys.argv[1]), int(sys.argv[2]))
    print(json.dumps({k: v for k, v in tot.items() if k != "mismatches"}))
    for m in tot["mismatches"][:20]:
        print(m)
    return 1 if tot["mismatches"] else 0


if __name__ == "__main__":
    sys.exit(main())
