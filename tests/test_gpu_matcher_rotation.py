"""GPU parity of the matchers' rotation-consistency check (k_bf_resolve, proj_resolve_body's finish, k_tri_finish; all
through rot_bin / three_maxima of matcher_common.h) on planted histograms: the scenes of the other matcher tests with
the angle arrays replaced by rot_plan's, so that the second and third maximum, ties, the 10 % cut at equality, the
+360 wrap, bin 12 and the half-way value of round() all decide which matches survive.  The oracle, pinned to a
second statement of the rule by test_rot_plan.py, is the reference; every comparison is exact."""
import numpy as np
import pytest

import rot_plan as RP
import rot_scenes as S

pytestmark = pytest.mark.gpu

ALL = sorted(RP.CASES)
FOUR = ["four_way_tie", "half_way_split", "ten_percent_edge", "top_bin_split"]
THREE = ["tie_for_third", "half_way_split", "top_bin_split"]
_cache = {}


def scene(gpu, key, make):
    """One scene (and its device-side call) per module run: the scene, its unchecked pairs and the planted angles do
    not depend on the case under test."""
    if key not in _cache:
        sc = make()
        _cache[key] = (sc, sc.gpu_flavours(gpu))
    return _cache[key]


def check(sc, run, case, min_removed=1):
    p = S.plan(sc, case)
    assert len(p["pairs"]) >= RP.CASES[case][1]
    want = sc.oracle(p["aa"], p["ab"], True)
    got = run(p["aa"], p["ab"], True)
    print("%s: %d pairs, oracle keeps %d, device keeps %d" % (case, len(p["pairs"]), want[0], got[0]))
    assert S.same(got, want), "%s: %d vs %d, %d entries differ" % (case, got[0], want[0], int((got[1] != want[1]).sum()))
    if RP.CASES[case][2]:
        assert want[0] <= p["count_off"] - min_removed
    return p, want


@pytest.mark.parametrize("case", ALL)
def test_bf_host(gpu, oracle, case):
    sc, fl = scene(gpu, "bf", lambda: S.BFScene(400))
    check(sc, fl["host"], case)


def test_bf_more_rows_than_finishing_threads(gpu, oracle):
    """1500 rows (the limit is 4096): the finish walks them with a stride of its 1024 threads."""
    sc, fl = scene(gpu, "bf1500", lambda: S.BFScene(1500, seed=5))
    for case in ("four_way_tie", "ten_percent_edge"):
        p, want = check(sc, fl["host"], case)
        removed = np.nonzero(~p["keep"])[0]
        assert removed.min() < 1024 < removed.max()


@pytest.mark.parametrize("stride", [28, 4])
@pytest.mark.parametrize("cases", [("ten_percent_edge", "single_bin", "four_way_tie", "half_way_split"),
                                   ("top_bin_split", "tie_for_third", "single_bin", "second_below")])
def test_bf_batched_device_path(gpu, oracle, stride, cases):
    """Four pairs in one call, each with its own histogram (single_bin between two that remove: a histogram that is
    not reset per pair would show); angles read from 28-byte key-point records or from plain float arrays."""
    torch = pytest.importorskip("torch")
    B, cap = 4, 448
    sizes = [400, 260, 333, 128]
    desc = np.zeros((B, cap, 32), np.uint8)
    nrow = np.array(sizes, np.int32)
    ang_a, ang_b, want = np.zeros((B, cap), np.float32), np.zeros((B, cap), np.float32), []
    for p in range(B):
        sc = S.BFScene(sizes[p], seed=40 + p)
        desc[p, :sizes[p]] = sc.d
        pl = S.plan(sc, cases[p], seed=p)
        ang_a[p, :sizes[p]], ang_b[p, :sizes[p]] = pl["aa"], pl["ab"]
        want.append(sc.oracle(pl["aa"], pl["ab"], True))
        assert (want[-1][0] < sizes[p]) == RP.CASES[cases[p]][2]
    d_desc, d_n = torch.from_numpy(desc).cuda(), torch.from_numpy(nrow).cuda()
    if stride == 28:
        rng = np.random.default_rng(1)
        ra, rb = (rng.uniform(0, 360, (B, cap, 7)).astype(np.float32) for _ in range(2))  # the other fields: anything
        ra[:, :, 3], rb[:, :, 3] = ang_a, ang_b
        d_a, d_b = torch.from_numpy(ra).cuda(), torch.from_numpy(rb).cuda()
        pa, pb = d_a.data_ptr() + 12, d_b.data_ptr() + 12
    else:
        d_a, d_b = torch.from_numpy(ang_a).cuda(), torch.from_numpy(ang_b).cuda()
        pa, pb = d_a.data_ptr(), d_b.data_ptr()
    bm = gpu.BatchMatcher(B, cap)
    match_b = torch.full((B, cap), -7, dtype=torch.int32, device="cuda")
    nm = torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in range(2):
        bm.match(B, cap, d_desc.data_ptr(), pa, None, d_n.data_ptr(), d_desc.data_ptr(), pb, d_n.data_ptr(), stride, 50, 0.7,
                 True, match_b.data_ptr(), nm.data_ptr(), s)
        torch.cuda.synchronize()
        runs.append((nm.cpu().numpy().tobytes(), match_b.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]
    mb, n = match_b.cpu().numpy(), nm.cpu().numpy()
    for p in range(B):
        assert n[p] == want[p][0] and np.array_equal(mb[p, :sizes[p]], want[p][1]), (p, cases[p], n[p], want[p][0])
        assert np.all(mb[p, sizes[p]:] == -1)
    bm.close()


@pytest.mark.parametrize("case", FOUR + ["tie_for_third", "wrap_and_top_bin"])
def test_search_by_bow(gpu, oracle, case):
    sc, fl = scene(gpu, "bow", lambda: S.BowScene(gpu))
    check(sc, fl["host"], case)


@pytest.mark.parametrize("case", FOUR)
def test_search_by_bow_near_duplicates(gpu, oracle, case):
    """The scene of test_search_by_bow_conflicts_within_nodes with the check on.  ORBmatcher.cc:209-210 skips a frame
    key point that has a match, so no two rows share one here (test_rot_plan.py shows it); what the scene adds is
    the greedy claim order inside few, crowded nodes feeding the histogram."""
    sc, fl = scene(gpu, "bowdup", S.BowDuplicatesScene)
    check(sc, fl["host"], case)


@pytest.mark.parametrize("case", FOUR + ["second_below"])
def test_search_by_bow_keyframes(gpu, oracle, case):
    sc, fl = scene(gpu, "bowkf", lambda: S.BowKeyFramesScene(gpu))
    check(sc, fl["host"], case)


@pytest.mark.parametrize("case", FOUR)
@pytest.mark.parametrize("flavour", ["host", "table", "device"])
def test_search_by_projection_last(gpu, oracle, flavour, case):
    """obs_zero = 0.4: many key points are taken by two rows; the plan puts one of the two into a removed bin, and the
    key point must end up unassigned whichever of them it was."""
    if flavour == "device":
        pytest.importorskip("torch")
    sc, fl = scene(gpu, "last", lambda: S.LastFrameScene(gpu))
    p, want = check(sc, fl[flavour], case)
    pairs = p["pairs"]
    js, cnt = np.unique(pairs[:, 1], return_counts=True)
    split = [j for j in js[cnt > 1] if len(set(p["keep"][pairs[:, 1] == j])) == 2]
    assert len(split) >= 5 and np.all(want[1][split] == -1)


@pytest.mark.parametrize("case", THREE)
def test_search_by_projection_keyframe(gpu, oracle, case):
    sc, fl = scene(gpu, "keyframe", lambda: S.KeyFrameScene(gpu))
    p, want = check(sc, fl["host"], case)
    assert np.all(want[1][sc.k0 == -2] == -2)


@pytest.mark.parametrize("case", THREE)
@pytest.mark.parametrize("only_stereo", [False, True])
def test_search_for_triangulation(gpu, oracle, only_stereo, case):
    sc, fl = scene(gpu, ("tri", only_stereo), lambda: S.TriangulationScene(gpu, only_stereo))
    check(sc, fl["host"], case)


@pytest.mark.parametrize("case", THREE)
def test_search_for_initialization(gpu, oracle, case):
    sc, fl = scene(gpu, "init", lambda: S.InitializationScene(gpu))
    check(sc, fl["host"], case)


def test_search_for_initialization_stale_votes(gpu, oracle):
    """The crafted steal scene: eight robbed rows keep their votes, which makes their bin the third maximum and
    pushes a bin of live matches out (test_rot_plan.py::test_steal_scene_bites shows that it does)."""
    sc = S.StealScene()
    run = sc.gpu_flavours(gpu)["host"]
    aa, ab = sc.angles()
    for chk in (True, False):
        want, got = sc.oracle(aa, ab, chk), run(aa, ab, chk)
        assert S.same(got, want), (chk, got[0], want[0])
    assert sc.oracle(aa, ab, True)[0] == 25


def test_no_pairs(gpu, oracle):
    """Nothing to match: count 0, outputs as they were."""
    rng = np.random.default_rng(1)
    for make in (S.EmptyBFScene, lambda: S.BowScene(gpu, empty=True), lambda: S.BowKeyFramesScene(gpu, empty=True),
                 lambda: S.LastFrameScene(gpu, empty=True), lambda: S.KeyFrameScene(gpu, empty=True),
                 lambda: S.TriangulationScene(gpu, False, empty=True), lambda: S.InitializationScene(gpu, empty=True)):
        sc = make()
        aa, ab = (rng.uniform(0, 360, n).astype(np.float32) for n in (sc.n_a, sc.n_b))
        want = sc.oracle(aa, ab, True)
        assert want[0] == 0
        for name, run in sc.gpu_flavours(gpu).items():
            if name == "device":
                pytest.importorskip("torch")
            assert S.same(run(aa, ab, True), want), (type(sc).__name__, name)


def test_same_bytes_twice(gpu, oracle):
    """The histogram is built with LDS atomics: the result must not depend on their order."""
    keys = [("bf", "host"), ("bow", "host"), ("bowkf", "host"), ("last", "host"), ("last", "table"), ("last", "device"),
            ("keyframe", "host"), (("tri", False), "host"), ("init", "host")]
    makers = {"bf": lambda: S.BFScene(400), "bow": lambda: S.BowScene(gpu), "bowkf": lambda: S.BowKeyFramesScene(gpu),
              "last": lambda: S.LastFrameScene(gpu), "keyframe": lambda: S.KeyFrameScene(gpu),
              ("tri", False): lambda: S.TriangulationScene(gpu, False), "init": lambda: S.InitializationScene(gpu)}
    for key, flavour in keys:
        sc, fl = scene(gpu, key, makers[key])
        p = S.plan(sc, "four_way_tie")
        a, b = fl[flavour](p["aa"], p["ab"], True), fl[flavour](p["aa"], p["ab"], True)
        assert a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])), (key, flavour)
