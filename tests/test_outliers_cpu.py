"""The judge of the density kernels (tests/outliers_oracle.py) judged itself, without a GPU: its radius counts against scipy's k-d
tree in float64, every rule of f3dgs_radius_count and f3dgs_knn_outliers on hand-built cases, the argument checks of the C ABI and
of the Python layer that answer before any device work - and the precondition of tests/test_gpu_outliers.py: on every input that
file uses, no score lies near its group's threshold.  The builders of those inputs live here; the GPU file imports them."""
import ctypes
import math
import os

import numpy as np
import pytest

import neighbors_oracle as no
import outliers_oracle as oo
from test_knn import _points
from util import ROOT

FLT_MAX = np.finfo(np.float32).max
_cache = {}


def _once(key, make):
    """computed once per input and left unchanged"""
    if key not in _cache:
        _cache[key] = make()
        for a in (_cache[key] if isinstance(_cache[key], tuple) else (_cache[key],)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _cache[key]


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------

COUNT_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000]      # the wave edge, the leaf edge, a partial last leaf
CAPS = [None, 1, 5]
RATIOS = [0.0, 1.0, 2.5]
SCORE_KS = [1, 3, 8, 16]
NUM_GROUPS = 7
GROUP_VALUES = np.array([0, 1, 2, 3, 4, 6, 9])                # seven labels: 9 is out of range, group 5 stays empty


def size_points(P):
    return _points(P, 11 + P, "uniform") if P else np.zeros((0, 3), np.float32)


def radius_of_mean_count(p, target=8):
    """the float32 radius within which a point has `target` others on average: the (target P / 2)-th smallest pair distance"""
    d = oo.pair_dist2(p, 0.0, np.inf)
    if not len(d):
        return np.float32(1.0)
    return np.float32(math.sqrt(float(d[min(len(d) - 1, target * len(p) // 2)])))


def radii_of(key, p):
    """0, a quarter of the mean nearest distance, the radius of mean count ~ 8, +inf"""
    def make():
        if len(p) < 2:
            return (0.0, 0.25, 1.0, math.inf)
        nearest = np.sqrt(no.knn(p, 1)[1][:, 0].astype(np.float64)).mean()
        return (0.0, float(np.float32(nearest / 4)), float(radius_of_mean_count(p)), math.inf)
    return _once(("radii", key), make)


def radius2_of(radius):
    """the Python layer's: the radius squared in float32"""
    r = np.float32(radius)
    with np.errstate(over="ignore"):
        return np.float32(r * r)


def count_labels(P, seed=3):
    """labels with 10 % set to -1, and values up to 2^31 - 1"""
    g = np.random.default_rng(seed)
    lab = np.array([0, 1, 5, 2**31 - 1])[g.integers(0, 4, P)]
    lab[g.random(P) < 0.1] = -1
    return lab


def score_lists():
    """the judge's lists of 2000 clustered points at K = 16 (a row's first K entries are its list at K)"""
    def make():
        p = _points(2000, 13, "clustered")
        return (p,) + no.knn(p, 16)
    return _once("score lists", make)


def score_labels(P):
    g = np.random.default_rng(21)
    lab = GROUP_VALUES[g.integers(0, len(GROUP_VALUES), P)]
    lab[g.random(P) < 0.05] = -1
    return lab


def corrupt(idx, d2, seed):
    """idx of -7, P and self, a NaN distance, the search's empty slot (-1, FLT_MAX): 40 rows each"""
    g = np.random.default_rng(seed)
    idx, d2 = idx.copy(), d2.copy()
    P, K = idx.shape
    rows = g.choice(P, 200, replace=False)
    slots = g.integers(0, K, 200)
    idx[rows[:40], slots[:40]] = -7
    idx[rows[40:80], slots[40:80]] = P
    idx[rows[80:120], slots[80:120]] = rows[80:120]
    d2[rows[120:160], slots[120:160]] = np.nan
    idx[rows[160:], slots[160:]] = -1
    d2[rows[160:], slots[160:]] = FLT_MAX
    return idx, d2


def score_cases():
    """(name, idx, dist2, labels or None, num_groups) of every score case of the GPU tests"""
    p, idx16, d16 = score_lists()
    labels = score_labels(len(p))
    for K in SCORE_KS:
        for labelled in (False, True):
            for bad in (False, True):
                idx, d2 = np.ascontiguousarray(idx16[:, :K]), np.ascontiguousarray(d16[:, :K])
                if bad:
                    idx, d2 = corrupt(idx, d2, 40 + K)
                yield f"K{K}-{'labels' if labelled else 'all'}-{'corrupted' if bad else 'clean'}", idx, d2, \
                    (labels if labelled else None), (NUM_GROUPS if labelled else 1)


def judged(name, idx, d2, labels, G, ratio):
    """the judge's (score, keep, stats) of a case, computed once"""
    sc = _once(("score", name), lambda: oo.scores(idx, d2, labels, G))
    return _once(("outliers", name, ratio), lambda: oo.outliers(idx, d2, labels, G, ratio, sc=sc))


def floater_scene():
    """A synth scene's means as the body, and around it what a component filter cannot remove: a sparse HALO on a sphere about the
    body, joined to it by a BRIDGE (a line of points from the body's centre to a halo point), and 50 FAR points.  Returns (points,
    kind): kind 0 body, 1 bridge, 2 halo, 3 far; and the halo's spacing."""
    def make():
        import torch  # noqa: F401
        from synth import make_scene
        body = make_scene(3000, 4, 64, 64, seed=3)["means3D"].numpy().astype(np.float32)
        g = np.random.default_rng(17)
        c = body.astype(np.float64).mean(0)
        R = 1.3 * np.sqrt(((body - c) ** 2).sum(1)).max()
        n_halo = 400
        k = np.arange(n_halo) + 0.5                                 # a Fibonacci sphere: evenly spread directions
        phi, z = k * math.pi * (3 - math.sqrt(5)), 1 - 2 * k / n_halo
        dirs = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
        h = R * math.sqrt(4 * math.pi / n_halo)                      # the halo's spacing
        halo = c + R * dirs + g.normal(0, 0.01 * h, (n_halo, 3))
        steps = int(math.ceil(R / (0.4 * h)))
        bridge = c + np.linspace(0, 1, steps, endpoint=False)[:, None] * R * dirs[n_halo // 2] + g.normal(0, 0.01 * h, (steps, 3))
        u = g.normal(0, 1, (50, 3))
        far = c + u / np.sqrt((u * u).sum(1))[:, None] * R * g.uniform(5, 10, (50, 1))
        pts = np.concatenate([body, bridge, halo, far]).astype(np.float32)
        kind = np.concatenate([np.zeros(len(body)), np.ones(steps), np.full(n_halo, 2), np.full(50, 3)]).astype(np.int64)
        order = g.permutation(len(pts))
        return pts[order], kind[order], float(h)
    return _once("floater scene", make)


def scene_lists(K=8):
    return _once(("scene lists", K), lambda: no.knn(floater_scene()[0], K))


def capture_points(which):
    return _points(1000, 51 + which, "clustered")


def keep_inputs():
    """every (name, idx, dist2, labels, num_groups, ratio) whose `keep` the GPU tests compare"""
    for name, idx, d2, labels, G in score_cases():
        for ratio in RATIOS:
            yield name, idx, d2, labels, G, ratio
    pts, kind, _ = floater_scene()
    idx, d2 = scene_lists()
    yield "scene-all", idx, d2, None, 1, 2.0
    yield "scene-mask", idx, d2, (kind != 3).astype(np.int64) - 1, 1, 2.0
    yield "scene-labels", idx, d2, np.minimum(kind, 2), 3, 2.0
    for which in (0, 1):
        p = capture_points(which)
        idx, d2 = _once(("capture lists", which), lambda: no.knn(p, 8))
        yield f"capture-{which}", idx, d2, None, 1, 2.0


# ---- the judge against the k-d tree -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["uniform", "clustered", "planar"])
def test_counts_equal_the_kdtree(kind):
    """P = 5000, seed 11, the radius of mean count ~ 8 moved into the widest gap between pair distances nearby: no pair lies within
    1e-5 relative of it (asserted), so the float32 distances and the tree's float64 ones put every pair on the same side."""
    from scipy.spatial import cKDTree
    p = _points(5000, 11, kind)
    r = oo.clear_radius(p, radius_of_mean_count(p))
    assert oo.radius_clearance(p, r) > 1e-5
    got = oo.radius_count(p, radius2_of(r))
    p64 = p.astype(np.float64)
    want = cKDTree(p64).query_ball_point(p64, math.sqrt(float(radius2_of(r))), return_length=True) - 1
    assert np.array_equal(got, want)
    assert 6 < got.mean() < 10 and got.min() < got.max()
    for cap in (1, 5):
        assert np.array_equal(oo.radius_count(p, radius2_of(r), cap=cap), np.minimum(want, cap))


# ---- hand cases of every rule -------------------------------------------------------------------------------------------------

def test_duplicates_are_counted_at_radius_zero():
    base = _points(5, 2)
    p = np.concatenate([base, base, base])
    assert oo.radius_count(p, 0.0).tolist() == [2] * 15
    assert oo.radius_count(base, 0.0).tolist() == [0] * 5
    assert oo.radius_count(np.zeros((6, 3), np.float32), 0.0).tolist() == [5] * 6
    assert oo.radius_count(np.zeros((0, 3), np.float32), 1.0).shape == (0,)


def test_the_radius_is_inclusive_and_the_cap_saturates():
    p = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [10, 0, 0]], np.float32)
    assert oo.radius_count(p, 1.0).tolist() == [1, 2, 2, 1, 0]            # a pair exactly on the radius is counted
    assert oo.radius_count(p, np.float32(0.99) ** 2).tolist() == [0] * 5
    assert oo.radius_count(p, 4.0).tolist() == [2, 3, 3, 2, 0]
    assert oo.radius_count(p, 4.0, cap=2).tolist() == [2, 2, 2, 2, 0]
    assert oo.radius_count(p, 4.0, cap=1).tolist() == [1, 1, 1, 1, 0]
    assert oo.radius_count(p, np.inf).tolist() == [4] * 5
    assert oo.radius_count(p, np.inf, cap=3).tolist() == [3] * 5


def test_labels_join_equal_non_negative_labels_only():
    p = np.zeros((6, 3), np.float32)
    assert oo.radius_count(p, 0.0, labels=[0, 0, 1, -1, -1, 2**31 - 1]).tolist() == [1, 1, 0, 0, 0, 0]
    assert oo.radius_count(p, 0.0, labels=[-5, -5, -5, 7, 7, 7]).tolist() == [0, 0, 0, 2, 2, 2]


def test_non_finite_points_count_nobody_and_are_counted_by_nobody():
    p = _points(40, 6)
    p[7, 1] = np.nan
    p[23, 0] = np.inf
    rest = np.delete(np.arange(40), [7, 23])
    for r2 in (1.0, 9.0, np.inf):
        c = oo.radius_count(p, r2)
        assert c[7] == 0 and c[23] == 0
        assert np.array_equal(c[rest], oo.radius_count(p[rest], r2))      # the others: as if the two were not there
    assert oo.radius_count(p, np.inf)[rest].tolist() == [37] * 38
    far = np.array([[3e19, 0, 0], [-3e19, 0, 0], [3e19, 1, 0]], np.float32)       # finite points whose distance overflows
    assert oo.radius_count(far, 4.0).tolist() == [1, 0, 1]
    assert oo.radius_count(far, np.inf).tolist() == [2, 2, 2]                     # +inf counts every finite point


def test_slot_rules():
    P = 5
    d = np.float32
    idx = np.array([[1, 2, 3], [-7, P, 1], [0, 1, 3], [4, 4, -1], [3, 0, 1]], np.int32)
    d2 = np.array([[1, 4, 9], [1, 1, 1], [4, np.nan, 16], [np.inf, 0.25, FLT_MAX], [0.25, 1, 1]], d)
    sc = oo.scores(idx, d2)
    assert sc[0] == d((1.0 + 2.0 + 3.0) / 3)
    assert sc[1] == np.inf                                  # -7, P and self: no valid slot
    assert sc[2] == d(3.0)                                  # the NaN distance is left out: (2 + 4) / 2
    assert sc[3] == d(0.5)                                  # inf is left out, FLT_MAX beside -1 fails the index test
    assert sc[4] == d((0.5 + 1.0 + 1.0) / 3)
    # FLT_MAX with a real index is a distance like any other
    big = oo.scores(np.array([[1], [0]], np.int32), np.array([[FLT_MAX], [FLT_MAX]], d))
    assert big[0] == d(math.sqrt(float(FLT_MAX)))
    # labels: a slot counts only within the group; a point out of range is no member
    lab = [0, 0, 1, 1, 5]
    sc = oo.scores(idx, d2, lab, 2)
    assert sc[0] == d(1.0) and sc[2] == d(4.0) and sc[4] == np.inf and sc[3] == np.inf
    assert oo.scores(idx, d2, [-1] * 5, 2).tolist() == [np.inf] * 5
    # the score is the fp64 mean rounded once
    idx1 = np.array([[1, 2], [0, 2], [0, 1]], np.int32)
    d21 = np.array([[2, 3], [2, 5], [3, 5]], d)
    assert oo.scores(idx1, d21)[0] == d((math.sqrt(2.0) + math.sqrt(3.0)) / 2)


def test_group_statistics():
    idx = np.array([[1], [0], [3], [2], [4], [0]], np.int32)
    d2 = np.array([[1], [1], [4], [16], [1], [9]], np.float32)
    lab = [0, 0, 1, 1, 2, 3]                                # group 2: one member without a valid slot (self); 3: one member; 4: empty
    sc, keep, stats = oo.outliers(idx, d2, lab, 5, 1.0)
    assert sc.tolist() == [1, 1, 2, 4, np.inf, np.inf]      # (point 5's neighbour 0 carries another label)
    assert stats[0].tolist() == [2, 1, 0, 1]
    assert stats[1].tolist() == [2, 3, math.sqrt(2.0), 3 + math.sqrt(2.0)]        # n == 2: the N - 1 form
    assert stats[2].tolist() == [0, 0, 0, 0] and stats[3].tolist() == [0, 0, 0, 0] and stats[4].tolist() == [0, 0, 0, 0]
    assert keep.tolist() == [True, True, True, True, False, False]
    _, keep0, stats0 = oo.outliers(idx, d2, lab, 5, 0.0)
    assert keep0.tolist() == [True, True, True, False, False, False] and stats0[1, 3] == 3
    # nobody has a neighbour of its own label: every group is empty
    sc, keep, stats = oo.outliers(np.array([[1], [0], [0]], np.int32), np.array([[4], [4], [9]], np.float32), [0, 1, 1], 2, 0.0)
    assert sc.tolist() == [np.inf, np.inf, np.inf] and not keep.any() and not stats.any()
    sc, keep, stats = oo.outliers(np.array([[1, 2], [0, 2], [0, 1]], np.int32), np.array([[4, 9], [4, 1], [9, 1]], np.float32), [0, 0, 1], 2, 0.0)
    assert sc.tolist() == [2, 2, np.inf] and stats[0].tolist() == [2, 2, 0, 2] and keep.tolist() == [True, True, False]
    # a group of one member with a finite score: std 0, the member is kept at every ratio
    sc, keep, stats = oo.outliers(np.array([[1], [0]], np.int32), np.array([[4], [np.nan]], np.float32), None, 1, 2.5)
    assert stats[0].tolist() == [1, 2, 0, 2] and keep.tolist() == [True, False]


# ---- the precondition of the GPU tests ----------------------------------------------------------------------------------------

def test_no_gpu_case_has_a_score_near_its_threshold():
    """For every input whose `keep` tests/test_gpu_outliers.py compares: no finite score lies within n 2^-50 (mean + std) of its
    group's threshold - the device's threshold, an fp64 evaluation in another order, decides every point as the judge does."""
    seen = 0
    for name, idx, d2, labels, G, ratio in keep_inputs():
        sc, keep, stats = judged(name, idx, d2, labels, G, ratio)
        assert oo.threshold_clearance(sc, labels, G, stats) > 1, (name, ratio)
        seen += 1
    assert seen == len(SCORE_KS) * 4 * len(RATIOS) + 5


def test_the_planted_scene_is_what_it_claims():
    pts, kind, h = floater_scene()
    assert (kind == 3).sum() == 50 and (kind == 2).sum() == 400 and len(pts) == 3000 + (kind == 1).sum() + 450
    # over all points the far ones go - and inflate the deviation so much that the halo stays; among the rest the halo goes
    sc, keep, stats = judged("scene-all", *scene_lists(), None, 1, 2.0)
    assert not keep[kind == 3].any() and keep[kind == 0].all()
    sc, keep, stats = judged("scene-mask", *scene_lists(), (kind != 3).astype(np.int64) - 1, 1, 2.0)
    assert not keep[kind == 3].any() and keep[kind == 2].mean() < 0.1 and keep[kind == 0].mean() > 0.9
    cnt = oo.radius_count(pts, radius2_of(0.6 * h), cap=4)
    assert not (cnt[kind == 3] >= 4).any() and (cnt[kind == 2] >= 4).mean() < 0.1 and (cnt[kind == 0] >= 4).mean() > 0.9


# ---- the C ABI: what is refused before any device work ------------------------------------------------------------------------

def _lib():
    so = os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import torch  # noqa: F401  (its bundled HIP runtime must be the one the library binds to)
    lib = ctypes.CDLL(so)
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_version.restype = ci
    lib.f3dgs_knn_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_radius_count_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_radius_count_scratch_bytes.argtypes = [ci]
    lib.f3dgs_radius_count.argtypes = [ci, vp, cf, vp, ci, vp, vp, vp]
    lib.f3dgs_knn_outliers_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_knn_outliers_scratch_bytes.argtypes = [ci]
    lib.f3dgs_knn_outliers.argtypes = [ci, ci, vp, vp, vp, ci, cf, vp, vp, vp, vp, vp]
    return lib


def test_c_abi_refuses_bad_arguments_without_gpu():
    lib = _lib()
    assert lib.f3dgs_version() >= 32500
    A = 0x10000                                    # an aligned, never dereferenced address
    INV, UNS = -1, -4                              # F3DGS_ERR_INVALID_ARGUMENT, F3DGS_ERR_UNSUPPORTED
    err = lib.f3dgs_last_error
    # the count
    assert lib.f3dgs_radius_count_scratch_bytes(1000) >= lib.f3dgs_knn_scratch_bytes(1000) + 4 * 1000
    assert lib.f3dgs_radius_count_scratch_bytes(-3) == lib.f3dgs_radius_count_scratch_bytes(0)
    assert lib.f3dgs_radius_count(0, None, 1.0, None, 0, None, None, None) == 0                     # P == 0: a no-op
    assert lib.f3dgs_radius_count(-1, A, 1.0, None, 0, A, A, None) == INV and b"P < 0" in err()
    assert lib.f3dgs_radius_count(2**30 + 1, A, 1.0, None, 0, A, A, None) == UNS and b"2^30" in err()
    for bad in (-1.0, np.nan, -np.inf):
        assert lib.f3dgs_radius_count(10, A, bad, None, 0, A, A, None) == INV and b"radius2" in err()
    assert lib.f3dgs_radius_count(10, A, 1.0, None, -1, A, A, None) == INV and b"cap" in err()
    for args in ((None, A, A), (A, None, A), (A, A, None)):
        assert lib.f3dgs_radius_count(10, args[0], np.inf, None, 3, args[1], args[2], None) == INV and b"null" in err()
    assert lib.f3dgs_radius_count(10, A, 1.0, A, 0, A, A + 4, None) == INV and b"16-byte" in err()
    # the scores
    assert lib.f3dgs_knn_outliers_scratch_bytes(7) >= 7 * 20 and lib.f3dgs_knn_outliers_scratch_bytes(-1) == lib.f3dgs_knn_outliers_scratch_bytes(0) > 0
    ok = (A, A, None, 1, 2.0, A, A, A, A)

    def call(P=10, K=3, a=ok):
        return lib.f3dgs_knn_outliers(P, K, *a, None)
    assert call(P=-1) == INV and b"P < 0" in err()
    assert call(P=2**30 + 1) == UNS and b"2^30" in err()
    for K in (0, 17, -2):
        assert call(K=K) == INV and b"1 .. 16" in err()
    assert call(a=(A, A, A, 0, 2.0, A, A, A, A)) == INV and b"num_groups" in err()
    assert call(a=(A, A, None, 2, 2.0, A, A, A, A)) == INV and b"without labels" in err()
    for bad in (-0.5, np.nan, np.inf):
        assert call(a=(A, A, None, 1, bad, A, A, A, A)) == INV and b"ratio" in err()
    for hole in (0, 1, 5, 6, 7, 8):                # idx, dist2, score, stats, keep, scratch
        a = list(ok)
        a[hole] = None
        assert call(a=tuple(a)) == INV and b"null" in err(), hole
    assert call(a=(A, A, None, 1, 2.0, A, A, A, A + 4)) == INV and b"8-byte" in err()


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import torch
    import neighbors
    pts, idx, d2 = torch.zeros(10, 3), torch.zeros(10, 3, dtype=torch.int32), torch.zeros(10, 3)
    with pytest.raises(ValueError, match="HIP device.*torch.float32 \\(10, 3\\) on cpu"):
        neighbors.radius_count(pts, 1.0)
    with pytest.raises(ValueError, match="HIP device"):
        neighbors.outlier_scores(idx, d2)
    with pytest.raises(ValueError, match="HIP device"):
        neighbors.remove_statistical_outliers(None, pts)
    with pytest.raises(ValueError, match="HIP device"):
        neighbors.remove_radius_outliers(torch.zeros(10, dtype=torch.bool), pts, 1.0, 3)
    for name in ("Outliers", "radius_count", "outlier_scores", "remove_statistical_outliers", "remove_radius_outliers"):
        assert name in neighbors.__all__
    assert neighbors.Outliers._fields == ("score", "keep", "stats")
