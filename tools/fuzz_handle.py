"""Randomised call sequences on a few long-lived extractor handles against the oracle (the state a handle keeps between
calls: recorded graph, configured tables, direct-mode level 0, cell counters):
    python tools/fuzz_handle.py [seconds] [seed]
Calls are drawn from: host or device entry point, image sizes from a small set (wide and flat against tall, more and
fewer pyramid bytes), batches of 1-40 frames, a cap just below or above what the frames need, the three options
(fast early-out, concurrent blur, profiling) toggled, and allocation failures forced with ORBGPU_DEBUG_FAIL_ALLOC_OVER.
After every call: key points (u32 patterns), descriptors and mvImagePyramid levels 0, 1 and the last of the first and
last frame against the oracle.  Not part of the test suite (it needs a GPU and runs as long as asked); prints the first
failing call and the sequence that led to it."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from orb_slam2_map_amd import lib as G
from orb_slam2_map_amd.synth import Stream
from oracle import oracle_py as O
import ctypes as C

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rng = np.random.default_rng(seed)
FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
HOOK = "ORBGPU_DEBUG_FAIL_ALLOC_OVER"
os.environ.pop(HOOK, None)

# (nfeatures, nlevels, max_batch, sizes): 1000x200 has more columns and fewer pyramid bytes than 640x480; 400x600 is tall
HANDLES = [(1000, 8, 1, [(640, 480), (400, 600), (752, 480)]),
           (600, 4, 8, [(640, 480), (1000, 200), (400, 600)]),
           (1500, 8, 4, [(640, 480), (1280, 960), (752, 480)])]
POOL = 40
_images, _oracle = {}, {}


def images(w, h):
    if (w, h) not in _images:
        st = Stream(w, h, int(rng.integers(1, 1 << 30)))
        _images[(w, h)] = np.stack([st.frame(i)[0] for i in range(POOL)])
    return _images[(w, h)]


def oracle(nfeat, nl, w, h, i):
    key = (nfeat, nl, w, h, i)
    if key not in _oracle:
        oe = O.Extractor(nfeat, 1.2, nl)
        k, d = oe.extract(images(w, h)[i])
        lv = {}
        for l in (0, 1, nl - 1):
            lw, lh = C.c_int(), C.c_int()
            oe.L.ora_blurred_level(oe.h, l, C.byref(lw), C.byref(lh))
            lv[l] = oe.pyramid_level(l)[19:19 + lh.value, 19:19 + lw.value].copy()
        _oracle[key] = (k, d, lv)
    return _oracle[key]


def same(gk, gd, ok, od):
    return len(gk) == len(ok) and all(np.array_equal(np.ascontiguousarray(gk[f]).view(np.uint32),
                                                     np.ascontiguousarray(ok[f]).view(np.uint32)) for f in FIELDS) \
        and np.array_equal(gd, od)


class Handle:
    def __init__(self, spec):
        self.nfeat, self.nl, self.max_batch, self.sizes = spec
        self.ge = G.ORBextractor(self.nfeat, 1.2, self.nl, max_batch=self.max_batch)
        self.keep = []  # caller buffers of the recent device calls (level 0 of a direct-mode call is read from them)
        self.log = []
        self.last = None  # (size, batch, cap, entry) of the last call: repeated half of the time, so graphs are recorded and replayed


def fail(h, msg):
    print("FAIL", msg)
    print("handle nfeat %d nlevels %d max_batch %d, seed %d; its calls so far:" % (h.nfeat, h.nl, h.max_batch, seed))
    for line in h.log[-40:]:
        print("   ", line)
    sys.exit(1)


def one_call(h):
    ge = h.ge
    repeat = h.last is not None and rng.random() < 0.5
    if repeat:
        (w, hh), b, cap, entry = h.last
    else:
        w, hh = h.sizes[int(rng.integers(len(h.sizes)))]
        b = int(rng.choice([1, 1, 1, 2, 3, 7, 8, 8, 9, 16, 40])) if rng.random() < 0.8 else int(rng.integers(1, 41))
    idx = rng.integers(0, POOL, b)
    imgs = np.ascontiguousarray(images(w, hh)[idx])
    need = max(len(oracle(h.nfeat, h.nl, w, hh, int(i))[0]) for i in idx)
    if not repeat:
        r = rng.random()
        cap = max(need - 1 - int(rng.integers(0, 3)), 1) if r < 0.12 else (need + int(rng.integers(0, 40)) if r < 0.5 else ge.max_keypoints(w, hh))
        entry = "host" if rng.random() < 0.6 else "device"
    h.last = ((w, hh), b, cap, entry)
    toggles = []
    for name, fn in (("early_out", ge.set_fast_early_out), ("blur", ge.set_concurrent_blur), ("profiling", ge.set_profiling)):
        if rng.random() < 0.06:
            on = int(rng.integers(0, 2))
            fn(on)
            toggles.append("%s=%d" % (name, on))
    hook = None
    if rng.random() < 0.08:
        hook = int(rng.choice([0, 1 << 16, 1 << 20, 1 << 22, 1 << 24]))
        os.environ[HOOK] = str(hook)
    desc = "%s %dx%d batch %d cap %d (need %d)%s%s" % (entry, w, hh, b, cap, need, " " + " ".join(toggles) if toggles else "",
                                                       " alloc<=%d" % hook if hook is not None else "")
    h.log.append(desc)
    try:
        if entry == "host":
            kps = np.zeros((b, cap), G.KEYPOINT_DTYPE)
            dsc = np.zeros((b, cap, 32), np.uint8)
            n = np.zeros(b, np.int32)
            rc = ge.L.orbgpu_extract_batch(ge.h, imgs.ctypes.data_as(C.c_void_p), b, w, hh, w, w * hh,
                                           kps.ctypes.data_as(C.c_void_p), dsc.ctypes.data_as(C.c_void_p), cap,
                                           n.ctypes.data_as(C.c_void_p))
            gk = [kps[f, :n[f]] for f in range(b)] if rc == G.OK else None
            gd = [dsc[f, :n[f]] for f in range(b)] if rc == G.OK else None
        else:
            buf = torch.from_numpy(imgs).cuda()
            kps_t = torch.zeros((b, cap, 7), dtype=torch.float32, device="cuda")
            dsc_t = torch.zeros((b, cap, 32), dtype=torch.uint8, device="cuda")
            n_t = torch.zeros(b, dtype=torch.int32, device="cuda")
            h.keep = (h.keep + [(buf, kps_t, dsc_t, n_t)])[-16:]
            rc = ge.L.orbgpu_extract_batch_device(ge.h, buf.data_ptr(), b, w, hh, w, w * hh, kps_t.data_ptr(), dsc_t.data_ptr(),
                                                  cap, n_t.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            n = n_t.cpu().numpy()
            gk = [np.frombuffer(kps_t[f, :max(n[f], 0)].cpu().numpy().tobytes(), G.KEYPOINT_DTYPE) for f in range(b)]
            gd = [dsc_t[f, :max(n[f], 0)].cpu().numpy() for f in range(b)]
    finally:
        os.environ.pop(HOOK, None)
    err = ge.L.orbgpu_last_error_string().decode("utf-8", "replace") if rc != G.OK else ""
    if rc == G.ENOMEM and hook is not None:
        h.log[-1] += " -> ENOMEM"
        return
    if entry == "host" and need > cap:
        if rc != G.ECAPACITY:
            fail(h, "%s: expected ECAPACITY, got %d %s" % (desc, rc, err))
        h.log[-1] += " -> ECAPACITY"
        return
    if rc != G.OK:
        fail(h, "%s: status %d %s" % (desc, rc, err))
    for f in range(b):
        ok, od, _ = oracle(h.nfeat, h.nl, w, hh, int(idx[f]))
        if entry == "device" and len(ok) > cap:
            if n[f] >= 0:
                fail(h, "%s frame %d: count %d for a frame over cap (oracle %d)" % (desc, f, n[f], len(ok)))
            continue
        if not same(gk[f], gd[f], ok, od):
            fail(h, "%s frame %d: %d key points, oracle %d, or descriptors differ" % (desc, f, len(gk[f]), len(ok)))
    for f in sorted({0, b - 1}):
        lv = oracle(h.nfeat, h.nl, w, hh, int(idx[f]))[2]
        for l, ref in lv.items():
            g, _, _ = ge.get_pyramid_level(f, l)
            if not np.array_equal(g, ref):
                fail(h, "%s: mvImagePyramid[%d] of frame %d differs" % (desc, l, f))
    try:
        ge.get_pyramid_level(b, 0)
        fail(h, "%s: frame %d of a batch of %d was readable" % (desc, b, b))
    except G.OrbGpuError as ex:
        if ex.status != G.EINVAL:
            fail(h, "%s: frame past the batch: status %d" % (desc, ex.status))


t0, n_calls, graphs = time.time(), 0, np.zeros(2, np.int64)
handles = [Handle(s) for s in HANDLES]
while time.time() - t0 < budget:
    h = handles[int(rng.integers(len(handles)))]
    one_call(h)
    n_calls += 1
    if rng.random() < 0.002:  # now and then a fresh handle in its place (first-call paths again)
        i = handles.index(h)
        graphs += h.ge.graph_counts()
        h.ge.close()
        handles[i] = Handle(HANDLES[i])
for h in handles:
    graphs += h.ge.graph_counts()
print("host entry graphs: %d recorded, %d replays" % tuple(graphs))
print("fuzz ok: %d calls in %.0f s" % (n_calls, time.time() - t0))
