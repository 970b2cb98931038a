"""Times LocalMapping::CreateNewMapPoints on the device: one orbgpu_create_new_map_points call against the sum of the nn
orbgpu_search_for_triangulation calls an integrator had to make before (the same inputs; that path has no triangulation and
no chain between the neighbours, so it does less work).

usage: python tools/bench_newpts.py [--reps R] [--out profiles/newpts_times.json]

Per case (nn = 10 at 1000 key points per frame, nn = 20 at 2000): medians over R calls of
  new_host_ms         the C call of the host flavour (one staged upload, the chain, one download)
  new_device_ms       the device flavour between two events on its stream (arrays already on the device)
  new_enqueue_ms      host time of the device flavour's call (the launches are queued, nothing is waited for)
  old_sum_ms          the nn C calls of orbgpu_search_for_triangulation, summed
  prepare_new_ms / prepare_old_ms   building the argument structures in Python, apart from the calls
Scenes: tests/newpts_model.make_scene."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import newpts_model as M  # noqa: E402
import fuzz_newpts as F  # noqa: E402
from orb_slam2_map_amd import lib as G  # noqa: E402

CASES = {"nn10_n1000": (10, 1000), "nn20_n2000": (20, 2000)}


def _ms(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def _view(f, keep):
    v = G.FrameView()
    v.n = len(f["kp_x"])
    a = [np.ascontiguousarray(f[k]) for k in ("kp_x", "kp_y", "kp_octave", "kp_angle", "u_right", "desc", "scale_factors")]
    keep.append(a)
    v.kp_x, v.kp_y, v.kp_octave, v.kp_angle, v.u_right, v.desc, v.scale_factors = (x.ctypes.data for x in a)
    v.nlevels = len(f["scale_factors"])
    return v


def bench_case(torch, nn, n, reps):
    sc = M.make_scene(4000 + nn, mix="mixed", n1=n, n2=(n,) * nn, n_points=n + n // 8, far=n // 16)
    kf1, nbs = sc["kf1"], sc["neighbours"]
    L = G.lib()
    L.orbgpu_create_new_map_points.argtypes = [C.c_void_p, C.c_int32]
    L.orbgpu_search_for_triangulation.argtypes = [C.c_void_p] * 7 + [C.c_float, C.c_float, C.c_void_p, C.c_int32, C.c_int32,
                                                                     C.c_void_p, C.c_void_p, C.c_int32]
    out = {k: np.zeros(nn * n * w, t) for k, w, t in (("match12", 1, np.int32), ("status", 1, np.int32), ("x3d", 3, np.float32))}
    cnt = {k: np.zeros(nn, np.int32) for k in ("n_matches", "n_created")}
    done = C.c_int32()

    def prepare_new():
        keep = []
        q = G.new_points_problem(kf1, nbs, sc["ratio_factor"], False, True, keep, False, n_done=C.addressof(done),
                                 **{k: v.ctypes.data for k, v in list(out.items()) + list(cnt.items())})
        return q, keep
    q, keep = prepare_new()

    def new_host():
        G.check(L.orbgpu_create_new_map_points(C.byref(q), 0))

    def prepare_old():
        keep2 = []
        return _view(kf1, keep2), [_view(f, keep2) for f in nbs], keep2
    v1, v2, keep2 = prepare_old()
    m12, nm = np.zeros(n, np.int32), C.c_int32()
    F12 = [np.ascontiguousarray(f["F12"], np.float32) for f in nbs]

    def old_sum():
        for k, f in enumerate(nbs):
            G.check(L.orbgpu_search_for_triangulation(C.byref(v1), kf1["has_mp"].ctypes.data, kf1["node"].ctypes.data, C.byref(v2[k]),
                                                      f["has_mp"].ctypes.data, f["node"].ctypes.data, F12[k].ctypes.data,
                                                      float(f["ex"]), float(f["ey"]), f["level_sigma2"].ctypes.data, 0, 1,
                                                      m12.ctypes.data, C.byref(nm), 0))
    new_host(), old_sum()  # warm-up: workspaces, code objects
    res = {"nn": nn, "keypoints": n, "reps": reps, "new_host_ms": _ms(new_host, reps), "old_sum_ms": _ms(old_sum, reps),
           "prepare_new_ms": _ms(prepare_new, reps), "prepare_old_ms": _ms(prepare_old, reps),
           "matches": int(cnt["n_matches"].sum()), "created": int(cnt["n_created"].sum())}
    # the device flavour between events
    keepd = []
    d1, d2 = F._device_frame(torch, kf1, keepd), [F._device_frame(torch, f, keepd) for f in nbs]
    o = {k: torch.zeros(max(v.size, 1), dtype=torch.int32 if v.dtype == np.int32 else torch.float32, device="cuda")
         for k, v in list(out.items()) + list(cnt.items())}
    o["n_done"] = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptrs = {k: v.data_ptr() for k, v in o.items()}
    qd = G.new_points_problem(d1, d2, sc["ratio_factor"], False, True, keepd, True, **ptrs)
    fn = L.orbgpu_create_new_map_points_device
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    dev_ms, enq_ms = [], []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        G.check(fn(C.byref(qd), 0, stream))
        t1 = time.perf_counter()
        b.record()
        torch.cuda.synchronize()
        if r:
            dev_ms.append(a.elapsed_time(b)), enq_ms.append((t1 - t0) * 1e3)
    res["new_device_ms"], res["new_enqueue_ms"] = statistics.median(dev_ms), statistics.median(enq_ms)
    assert o["n_created"].cpu().numpy().tobytes() == cnt["n_created"].tobytes()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newpts_times.json"))
    a = ap.parse_args()
    import torch
    doc = {"note": "first, unrepeated record; medians of --reps calls; old_sum is the parent's path and has no triangulation",
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, (nn, n) in CASES.items():
        doc["cases"][name] = bench_case(torch, nn, n, a.reps)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
