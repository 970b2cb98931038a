"""The seven host flavours (orbgpu_sim3_solve / _all, orbgpu_sim3_optimize, orbgpu_pnp_solve / _all, orbgpu_initializer /
_all, orbgpu_local_ba, orbgpu_bundle_adjustment, orbgpu_essential_graph) are staging around their families' device
flavours.  Every caller array is a view of exactly its documented length inside a buffer filled with a
canary byte; each entry point is called once with every optional output given and once with every one null.  The canaries
stay, the two calls agree, and the result and the arrays equal, byte for byte, what the device flavour leaves in torch
buffers for the same problem -- no tolerance: the same kernels ran on the same bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

CANARY, PAD, SENTINEL = 0xC5, 64, 7
VP = C.c_void_p


@pytest.fixture(scope="module")
def G():
    from orb_slam2_map_amd import lib
    if lib.device_count() < 1:
        pytest.skip("no HIP device")
    return lib


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


class Arrays:
    """The caller's arrays of one call: each exactly as long as documented, between PAD canary bytes on either side"""

    def __init__(self):
        self.blocks = []

    def put(self, a, dtype):
        a = np.ascontiguousarray(a, dtype)
        buf = np.full(a.nbytes + 2 * PAD, CANARY, np.uint8)
        v = buf[PAD:PAD + a.nbytes].view(dtype).reshape(a.shape)
        v[...] = a
        self.blocks.append((buf, a.nbytes))
        return v

    def out(self, shape, dtype, given=True):
        """an output that starts as SENTINEL; None when the caller does not ask for it"""
        return self.put(np.full(shape, SENTINEL, dtype), dtype) if given else None

    def intact(self):
        return all((b[:PAD] == CANARY).all() and (b[PAD + n:] == CANARY).all() for b, n in self.blocks)


def ptr(a):
    return None if a is None else VP(a.ctypes.data)  # a zero-length view still has an address


def call(G, name, n_pointers, *args):
    fn = getattr(G.lib(), name)
    fn.argtypes = [VP] * n_pointers + [C.c_int32]
    return fn(*args, 0)


def same_result(cls, res, dev, skip=()):
    """the host flavour's result structure against the device flavour's, as dicts of the same class, field by field"""
    h = res.as_dict()
    assert h and set(h) <= {k for k, _ in cls._fields_}
    for k in h:
        if k not in skip:
            assert np.asarray(h[k]).tobytes() == np.asarray(dev[k]).tobytes(), k


def same_where_written(host, dev, fill, zeroed=True):
    """What the kernels wrote is the same; what they left alone still holds `fill` in the device flavour's torch buffer and,
    behind an entry point that clears its staging block first (zeroed), comes back as zeros"""
    d = np.ascontiguousarray(dev).reshape(host.shape)
    w = d != fill
    assert host[w].tobytes() == d[w].tobytes()
    assert not zeroed or not host[~w].any()


def bits(mask_words, n):
    i = np.arange(n)
    return ((mask_words[i // 64] >> (i % 64).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


def device_or_none(G, run):
    """what the device flavour gives; None (and a line that says so) when it refuses the size"""
    try:
        return run()
    except G.OrbGpuError as e:
        assert e.status == G.EINVAL
        print("the device flavour refuses this size: %s" % e)
        return None


def cut(sc, rows, n1, sets, H):
    """the scene's first n1 rows and first H minimal sets"""
    out = dict(sc)
    for k in rows:
        out[k] = np.asarray(sc[k])[:n1].copy()
    out[sets] = np.asarray(sc[sets])[:H].copy()
    return out


SIZES = [(n1, H) for n1 in (0, 1, 65) for H in (0, 3)]


# ---- Sim3Solver -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,H", SIZES)
def test_sim3_solve(G, torch, n1, H):
    import fuzz_sim3 as F
    import sim3_model as M
    sc = cut(M.make_scene(60, 7, n1=65, n_hyp=3), ("valid", "Xw1", "Xw2", "octave1", "octave2"), n1, "triples", H)
    words = (n1 + 63) // 64

    def host(every, given):
        A = Arrays()
        ins = {"valid": A.put(sc["valid"], np.uint8), "Xw1": A.put(sc["Xw1"], np.float32), "Xw2": A.put(sc["Xw2"], np.float32),
               "octave1": A.put(sc["octave1"], np.int32), "octave2": A.put(sc["octave2"], np.int32),
               "triples": A.put(np.asarray(sc["triples"]).reshape(-1, 3), np.int32)}
        p = {k: sc[k] for k in ("T1w", "T2w", "K1", "K2", "level_sigma2", "fix_scale", "probability", "min_inliers", "max_iterations")}
        p.update(n1=n1, n_hyp=H, **{k: v.ctypes.data for k, v in ins.items()})
        q, res, lead = G.sim3_problem(p), G.Sim3Result(), ((H,) if every else ())
        o = {"counts": A.out((H,), np.int32, given), "R": A.out(lead + (3, 3), np.float32, given),
             "t": A.out(lead + (3,), np.float32, given), "s": A.out(lead + (1,), np.float32, given),
             "T12": A.out(lead + (4, 4), np.float32, given),
             "last": A.out((H, words), np.uint64, given) if every else A.out((n1,), np.uint8, given)}
        rc = call(G, "orbgpu_sim3_solve_all" if every else "orbgpu_sim3_solve", 8, C.byref(q), ptr(o["counts"]), ptr(o["R"]), ptr(o["t"]),
                  ptr(o["s"]), ptr(o["T12"]), ptr(o["last"]), C.byref(res))
        assert A.intact()
        return rc, res, o

    dev = device_or_none(G, lambda: F.run_batch(torch, [sc])[0])
    for every in (False, True):
        (rc, res, o), (rc0, res0, _) = host(every, True), host(every, False)
        assert rc == rc0 == (G.OK if dev is not None else G.EINVAL)
        if dev is None:
            continue
        same_result(G.Sim3Result, res, dev), same_result(G.Sim3Result, res0, dev)
        same_where_written(o["counts"], dev["counts"], -7, zeroed=every)  # only orbgpu_sim3_solve_all clears the block
        if every:
            for k in ("R", "t", "s", "T12"):
                assert o[k].tobytes() == dev[k].tobytes(), k
            assert o["last"].tobytes() == dev["masks"].tobytes()
        else:
            b, acc = dev["best_iteration"], dev["accepted"]
            for k in ("R", "t", "s", "T12"):
                want = dev[k][b] if 0 <= b < H else np.full(o[k].shape, SENTINEL, np.float32)
                assert o[k].tobytes() == np.asarray(want).tobytes(), k
            assert np.array_equal(o["last"], bits(dev["masks"][acc], n1) if acc >= 0 and words else np.zeros(n1, np.uint8))


# ---- Optimizer::OptimizeSim3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1", (0, 1, 65))
def test_sim3_optimize(G, torch, n1):
    import fuzz_sim3opt as F
    import sim3opt_model as M
    base = M.make_scene(50, 11, n1=65)
    sc = dict(base, **{k: np.asarray(base[k])[:n1].copy() for k in F.ROWS})

    def host(given):
        A = Arrays()
        p = F.host_problem(sc)
        p.update({k: A.put(np.asarray(sc[k]).reshape(-1), F.DTYPES[k]).ctypes.data for k in F.ROWS})
        q, res, ni = G.sim3_opt_problem(p), G.Sim3OptResult(), C.c_int32(-1)
        inl = A.out((n1,), np.uint8, given or n1 > 0)  # required when there are rows
        rc = call(G, "orbgpu_sim3_optimize", 4, C.byref(q), ptr(inl), C.byref(ni), C.byref(res) if given else None)
        assert A.intact()
        return rc, res, ni.value, inl

    dev = device_or_none(G, lambda: F.run_batch(torch, [sc])[0])
    (rc, res, ni, inl), (rc0, _, ni0, inl0) = host(True), host(False)
    assert rc == rc0 == (G.OK if dev is not None else G.EINVAL)
    if dev is not None:
        raw, r, d_inl = dev
        same_result(G.Sim3OptResult, res, r)
        assert ni == ni0 == r["n_inliers"] and inl.tobytes() == d_inl.tobytes()
        assert inl0 is None or inl0.tobytes() == inl.tobytes()


# ---- PnPsolver --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,H", SIZES)
def test_pnp_solve(G, torch, n1, H):
    import fuzz_pnp as F
    import pnp_model as M
    sc = cut(M.make_scene(60, 7, n1=65, n_hyp=3), ("valid", "Xw", "kp", "octave"), n1, "sets", H)
    words = (n1 + 63) // 64

    def host(every, given):
        A, keep = Arrays(), []
        s = dict(sc, valid=A.put(sc["valid"], np.uint8), Xw=A.put(sc["Xw"], np.float32), kp=A.put(sc["kp"], np.float32),
                 octave=A.put(sc["octave"], np.int32), sets=A.put(np.asarray(sc["sets"]).reshape(-1, sc["min_set"]), np.int32))
        q, res = G._pnp_host_problem(s, keep), G.PnpResult()
        q.valid, q.Xw, q.kp, q.octave, q.sets = (s[k].ctypes.data for k in ("valid", "Xw", "kp", "octave", "sets"))
        o = {"counts": A.out((H,), np.int32, given), "Tcw": A.out(((H,) if every else ()) + (4, 4), np.float32, given)}
        if every:
            o["masks"], o["refined"] = A.out((H, words), np.uint64, given), A.out((words,), np.uint64, given)
            rc = call(G, "orbgpu_pnp_solve_all", 6, C.byref(q), ptr(o["counts"]), ptr(o["Tcw"]), ptr(o["masks"]), ptr(o["refined"]),
                      C.byref(res))
        else:
            o["inliers"] = A.out((n1,), np.uint8, given)
            rc = call(G, "orbgpu_pnp_solve", 5, C.byref(q), ptr(o["counts"]), ptr(o["Tcw"]), ptr(o["inliers"]), C.byref(res))
        assert A.intact()
        return rc, res, o

    dev = device_or_none(G, lambda: F.run_batch(torch, [sc])[0])
    for every in (False, True):
        (rc, res, o), (rc0, res0, _) = host(every, True), host(every, False)
        assert rc == rc0 == (G.OK if dev is not None else G.EINVAL)
        if dev is None:
            continue
        same_result(G.PnpResult, res, dev), same_result(G.PnpResult, res0, dev)
        same_where_written(o["counts"], dev["counts"], -7)
        if every:
            assert o["Tcw"].tobytes() == dev["Tcw_all"].tobytes() and o["masks"].tobytes() == dev["masks"].tobytes()
            assert o["refined"].tobytes() == dev["refined_mask"].tobytes()
        else:
            assert o["Tcw"].tobytes() == np.asarray(dev["Tcw"], np.float32).tobytes()
            assert np.array_equal(o["inliers"], bits(dev["refined_mask"], n1))


# ---- Initializer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,H", SIZES)
def test_initializer(G, torch, n1, H):
    import fuzz_init as F
    import init_model as M
    sc = cut(M.make_scene(50, 7, n1=65, n_hyp=3), ("kp1", "matches12"), n1, "sets", H)
    words = (n1 + 63) // 64

    def host(every, given):
        A, keep = Arrays(), []
        s = dict(sc, kp1=A.put(np.asarray(sc["kp1"]).reshape(-1, 2), np.float32), kp2=A.put(np.asarray(sc["kp2"]).reshape(-1, 2), np.float32),
                 matches12=A.put(sc["matches12"], np.int32), sets=A.put(np.asarray(sc["sets"]).reshape(-1, 8), np.int32))
        q, res = G._init_host_problem(s, keep), G.InitResult()
        q.kp1, q.kp2, q.matches12, q.sets = (s[k].ctypes.data for k in ("kp1", "kp2", "matches12", "sets"))
        o = {"P3D": A.out((n1, 3), np.float32, given), "triangulated": A.out((n1,), np.uint8, given)}
        if every:
            o.update(scores_h=A.out((H,), np.float32, given), scores_f=A.out((H,), np.float32, given),
                     masks_h=A.out((H, words), np.uint64, given), masks_f=A.out((H, words), np.uint64, given))
            rc = call(G, "orbgpu_initializer_all", 8, C.byref(q), ptr(o["scores_h"]), ptr(o["scores_f"]), ptr(o["masks_h"]),
                      ptr(o["masks_f"]), ptr(o["P3D"]), ptr(o["triangulated"]), C.byref(res))
        else:
            rc = call(G, "orbgpu_initializer", 4, C.byref(q), ptr(o["P3D"]), ptr(o["triangulated"]), C.byref(res))
        assert A.intact()
        return rc, res, o

    dev = device_or_none(G, lambda: F.run_batch(torch, [sc])[0])
    for every in (False, True):
        (rc, res, o), (rc0, res0, _) = host(every, True), host(every, False)
        assert rc == rc0 == (G.OK if dev is not None else G.EINVAL)
        if dev is None:
            continue
        # parallax_deg is the host flavours' own (include/orbgpu.h): the same in both calls, not the device flavour's
        same_result(G.InitResult, res, dev, skip=("parallax_deg",)), same_result(G.InitResult, res0, res.as_dict())
        for k in o:  # fuzz_init.upload's fills
            same_where_written(o[k], dev[k], {"P3D": -7.0, "triangulated": 7, "scores_h": -7.0, "scores_f": -7.0}.get(k, 0))


# ---- the two bundle adjustments ---------------------------------------------------------------------------------------------
def _empty_lba_scene():
    z = lambda *shape: np.zeros(shape, np.float32)  # noqa: E731
    return {"Tcw": z(0, 4, 4), "n_local": 0, "fixed": np.zeros(0, np.uint8), "cam": z(0, 5), "inv_sigma2": z(0, 8), "world_pos": z(0, 3),
            "e_point": np.zeros(0, np.int32), "e_pose": np.zeros(0, np.int32), "e_oct": np.zeros(0, np.int32), "e_xy": z(0, 2),
            "e_ur": z(0), "n_iterations": 4, "robust": True}


def _ba_host(G, F, sc, entry, make_problem, result_cls, n_rows, flag_len, given):
    A, keep = Arrays(), []
    p = F.to_problem(sc)
    for k, t in G._LBA_HOST:
        p[k] = A.put(p[k], t)
    q, res = make_problem(p, keep), result_cls()
    for k, _ in G._LBA_HOST:
        setattr(q, k, p[k].ctypes.data)  # the views themselves, zero-length ones included
    M = len(sc["world_pos"])
    o = {"Tcw_d": A.out((n_rows, 4, 4), np.float64, given), "Tcw": A.out((n_rows, 4, 4), np.float32),
         "pos_d": A.out((M, 3), np.float64, given), "pos": A.out((M, 3), np.float32), "flag": A.out((flag_len,), np.uint8)}
    rc = call(G, entry, 8, C.byref(q), None, ptr(o["Tcw_d"]), ptr(o["Tcw"]), ptr(o["pos_d"]), ptr(o["pos"]), ptr(o["flag"]),
              C.byref(res) if given else None)
    assert A.intact()
    return rc, res, o


def _ba_check(G, dev, calls, result_cls, flag):
    (rc, res, o), (rc0, _, o0) = calls
    assert rc == rc0 == (G.OK if dev is not None else G.EINVAL)
    if dev is None:
        return
    _, r, a = dev
    same_result(result_cls, res, r)
    for k in ("Tcw_d", "Tcw", "pos_d", "pos"):
        assert o[k].tobytes() == np.ascontiguousarray(a[k]).tobytes(), k
    assert o["flag"].tobytes() == np.ascontiguousarray(a[flag]).tobytes()
    for k in ("Tcw", "pos", "flag"):
        assert o0[k].tobytes() == o[k].tobytes(), k


@pytest.mark.parametrize("empty", (True, False))
def test_local_ba(G, torch, empty):
    import fuzz_lba as F
    import lba_model as M
    sc = _empty_lba_scene() if empty else M.make_scene(2, 2, 30, 5, mode="mixed")
    dev = device_or_none(G, lambda: F.run_batch(torch, [sc])[0])
    calls = [_ba_host(G, F, sc, "orbgpu_local_ba", G.local_ba_problem, G.LocalBAResult, sc["n_local"], len(sc["e_point"]), given)
             for given in (True, False)]
    _ba_check(G, dev, calls, G.LocalBAResult, "erase")


@pytest.mark.parametrize("empty", (True, False))
def test_bundle_adjustment(G, torch, empty):
    import fuzz_ba as F
    sc = _empty_lba_scene() if empty else F.make_scene(2, 2, 30, 5, n_iterations=4, mode="mixed")
    dev = device_or_none(G, lambda: F.run_batch(torch, [sc])[0])
    calls = [_ba_host(G, F, sc, "orbgpu_bundle_adjustment", G.bundle_adjustment_problem, G.BundleAdjustmentResult, len(sc["Tcw"]),
                      len(sc["world_pos"]), given) for given in (True, False)]
    _ba_check(G, dev, calls, G.BundleAdjustmentResult, "not_included")


# ---- Optimizer::OptimizeEssentialGraph --------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,M", [(V, M) for V in (0, 3) for M in (0, 5)])
def test_essential_graph(G, torch, V, M):
    import eg_model
    import fuzz_eg as F
    if V:
        sc = eg_model.make_scene(V, 9, n_iterations=2, n_points=M)
    else:
        sc = {"Scw": np.zeros((0, 8)), "Snc": np.zeros((0, 8)), "fixed": np.zeros(0, np.uint8), "edge_i": np.zeros(0, np.int32),
              "edge_j": np.zeros(0, np.int32), "edge_kind": np.zeros(0, np.int32), "n_iterations": 2, "fix_scale": False}
        if M:
            sc.update(world_pos=np.ones((M, 3), np.float32), point_ref=np.zeros(M, np.int32))

    def host(given):
        A, keep = Arrays(), []
        p = F.to_problem(sc)
        for k, t in G._EG_HOST:
            p[k] = A.put(p[k], t)
        q, res = G.essential_graph_problem(p, keep), G.EssentialGraphResult()
        for k, _ in G._EG_HOST:
            setattr(q, k, p[k].ctypes.data)
        X = A.put(sc["world_pos"], np.float32) if M else None
        ref = A.put(sc["point_ref"], np.int32) if M else None
        o = {"Siw_d": A.out((V, 8), np.float64, given), "Tiw": A.out((V, 4, 4), np.float32), "pos": A.out((M, 3), np.float32, M > 0)}
        fn = G.lib().orbgpu_essential_graph
        fn.argtypes = [VP] * 4 + [C.c_int32] + [VP] * 4 + [C.c_int32]
        rc = fn(C.byref(q), None, ptr(o["Siw_d"]), ptr(o["Tiw"]), M, ptr(X), ptr(ref), ptr(o["pos"]), C.byref(res) if given else None, 0)
        assert A.intact()
        return rc, res, o

    dev = device_or_none(G, lambda: F.run_batch(torch, [sc])[0])
    (rc, res, o), (rc0, _, o0) = host(True), host(False)
    assert rc == rc0 == (G.OK if dev is not None else G.EINVAL)
    if dev is not None:
        _, r, a = dev
        same_result(G.EssentialGraphResult, res, r)
        assert o["Siw_d"].tobytes() == np.ascontiguousarray(a["Siw_d"]).tobytes()
        assert o["Tiw"].tobytes() == np.ascontiguousarray(a["Tiw"]).tobytes() == o0["Tiw"].tobytes()
        if M:
            assert o["pos"].tobytes() == np.ascontiguousarray(a["pos"]).tobytes() == o0["pos"].tobytes()
