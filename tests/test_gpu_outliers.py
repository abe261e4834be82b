"""The density kernels on the GPU (csrc/outliers.hip; neighbors.py: radius_count, outlier_scores, remove_statistical_outliers,
remove_radius_outliers).  The judge is tests/outliers_oracle.py - numpy, brute force, the kernel's float32 operation order, fp64
scores rounded once - and every integer, byte and score comparison is exact, the score as bits.  Only the group statistics carry a
bound: that of an fp64 sum of n non-negative terms taken in any order.  tests/test_outliers_cpu.py builds the inputs and asserts,
for every one of them, that no score lies near its group's threshold: `keep` is compared exactly, no point left out."""
import math

import numpy as np
import pytest
import torch

import outliers_oracle as oo
import test_outliers_cpu as cases
from test_knn import _points
from test_neighbors_cpu import lattice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)                   # (a copy: the judge's arrays are read-only)
    return t if dtype is None else t.to(dtype)


def _want_count(key, p, radius, labels=None):
    """the judge's uncapped counts, computed once per input and left unchanged; a cap is their minimum with it"""
    k = ("count", key, float(radius), labels is not None)
    if k not in _cache:
        _cache[k] = oo.radius_count(p, cases.radius2_of(radius), labels)
        _cache[k].setflags(write=False)
    return _cache[k]


def _count(p, radius, labels=None, cap=None, dtype=torch.int64):
    import neighbors
    out = neighbors.radius_count(_dev(p), radius, None if labels is None else _dev(labels, dtype), cap=cap)
    torch.cuda.synchronize()
    assert out.dtype == torch.int32 and tuple(out.shape) == (len(p),)
    return out.cpu().numpy()


def _check_counts(key, p, radii, labels=None, caps=cases.CAPS, dtype=torch.int64):
    for r in radii:
        want = _want_count(key, p, r, labels)
        for cap in caps:
            got = _count(p, r, labels, cap, dtype)
            capped = want if cap is None else np.minimum(want, cap)
            assert np.array_equal(got, capped), f"{key}, radius {r}, cap {cap}: {int((got != capped).sum())} counts differ"
    return want


# ---- counts -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", cases.COUNT_SIZES)
def test_count_sizes(P):
    p = cases.size_points(P)
    _check_counts(("uniform", P), p, cases.radii_of(("uniform", P), p))
    if P > 1:
        assert (_want_count(("uniform", P), p, math.inf) == P - 1).all()


@pytest.mark.parametrize("kind", ["clustered", "planar"])
def test_count_pruning_far_from_the_origin(kind):
    p = _points(5000, 11, kind)
    radii = cases.radii_of((kind, 5000), p)
    _check_counts((kind, 5000), p, radii)
    assert 6 < _want_count((kind, 5000), p, radii[2]).mean() < 10


def test_count_shuffled_lattice_every_pair_on_the_radius():
    """12 x 12 x 12 integer points, shuffled: at radius 1 every counted pair lies exactly ON the radius, many of them across leaves.
    Fails where a pair is tested with <, where a leaf is pruned with <, where the box bound is not monotone with the distances."""
    p = lattice(12, 7)
    want = _check_counts(("lattice", 12), p, (1.0,))
    interior = ((p >= 1) & (p <= 10)).all(1)
    assert (want[interior] == 6).all() and want.min() == 3
    assert (_check_counts(("lattice", 12), p, (0.99,)) == 0).all()


def test_count_duplicates_and_non_finite_points():
    p = np.repeat(_points(300, 5), 4, axis=0)                     # every point four times
    assert (_check_counts(("dup", 300), p, (0.0,)) == 3).all()
    q = _points(500, 8).copy()
    q[123, 2] = np.nan
    q[377, 0] = -np.inf
    radii = cases.radii_of(("uniform", 500, 8), _points(500, 8))
    for r in (radii[2], math.inf):
        want = _check_counts(("nonfinite", 500), q, (r,))
        assert want[123] == 0 and want[377] == 0
    assert (np.delete(want, [123, 377]) == 497).all()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_count_labels(dtype):
    """10 % of the labels -1, values up to 2^31 - 1; int32 and int64 through the Python layer"""
    for key, p in ((("uniform", 1000), cases.size_points(1000)), (("clustered", 5000), _points(5000, 11, "clustered"))):
        labels = cases.count_labels(len(p))
        radii = cases.radii_of(key, p)
        want = _check_counts(key, p, (radii[2] * 2, math.inf), labels, dtype=dtype)
        assert (want[labels < 0] == 0).all() and (want[labels >= 0] > 0).any()
        assert (want[labels == 2**31 - 1] == (labels == 2**31 - 1).sum() - 1).all()      # radius inf: the label's other points


# ---- scores -------------------------------------------------------------------------------------------------------------------

def _scores(idx, d2, labels, G, ratio, dtype=torch.int64):
    import neighbors
    out = neighbors.outlier_scores(idx if torch.is_tensor(idx) else _dev(idx), d2 if torch.is_tensor(d2) else _dev(d2),
                                   None if labels is None else _dev(labels, dtype), G if labels is not None else None, ratio)
    torch.cuda.synchronize()
    P = idx.shape[0]
    assert isinstance(out, neighbors.Outliers)
    assert out.score.dtype == torch.float32 and tuple(out.score.shape) == (P,)
    assert out.keep.dtype == torch.bool and tuple(out.keep.shape) == (P,)
    assert out.stats.dtype == torch.float64 and tuple(out.stats.shape) == (G, 4) and out.stats.device == out.score.device
    return out.score.cpu().numpy(), out.keep.cpu().numpy(), out.stats.cpu().numpy()


def _check_outliers(got, want, what):
    (sc, keep, stats), (wsc, wkeep, wstats) = got, want
    assert np.array_equal(_bits(sc), _bits(wsc)), f"{what}: {int((_bits(sc) != _bits(wsc)).sum())} scores differ"
    n, mean, std, thr = (wstats[:, c] for c in range(4))
    assert np.array_equal(stats[:, 0], n), what
    e_mean = n * 2.0 ** -52 * mean
    e_std = n * 2.0 ** -51 * (mean + std)
    assert (np.abs(stats[:, 1] - mean) <= e_mean).all(), what
    assert (np.abs(stats[:, 2] - std) <= e_std).all(), what
    assert (np.abs(stats[:, 3] - thr) <= e_mean + e_std).all(), what
    assert np.array_equal(keep, wkeep), f"{what}: {int((keep != wkeep).sum())} decisions differ"


@pytest.mark.parametrize("K", cases.SCORE_KS)
def test_scores_on_the_search_own_lists(K):
    """neighbors.knn's lists of 2000 clustered points - the judge's, bit for bit -, without labels and with seven labels of which
    one is out of range and one empty, as they are and with idx of -7, P and self, NaN distances and empty slots written in."""
    import neighbors
    p = cases.score_lists()[0]
    dev_idx, dev_d2 = neighbors.knn(_dev(p), K)
    for name, idx, d2, labels, G in cases.score_cases():
        if not name.startswith(f"K{K}-"):
            continue
        clean = name.endswith("clean")
        if clean:
            assert np.array_equal(dev_idx.cpu().numpy(), idx) and np.array_equal(_bits(dev_d2.cpu().numpy()), _bits(d2))
        for ratio in cases.RATIOS:
            got = _scores(dev_idx if clean else idx, dev_d2 if clean else d2, labels, G, ratio)
            _check_outliers(got, cases.judged(name, idx, d2, labels, G, ratio), f"{name}, ratio {ratio}")
        if labels is not None:
            assert got[2][5].tolist() == [0, 0, 0, 0] and (got[0][labels == 9] == np.inf).all()      # the empty group, the label out of range
            if K >= 3:
                assert (got[2][[0, 1, 2, 3, 4, 6], 0] > 50).all()      # (about 270 members a label, 37 % of them with a neighbour of their label at K = 3)
            _check_outliers(_scores(idx, d2, labels, G, 1.0, torch.int32), cases.judged(name, idx, d2, labels, G, 1.0), name + ", int32")


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def test_floaters_a_component_filter_keeps():
    """A synth scene with 50 far points and a sparse halo joined to the body by a bridge.  keep_largest removes the far points and
    KEEPS the bridge and the halo - one component with the body; the two density filters drop exactly what the judge drops, and
    with it the halo.  A bool mask in, a bool mask out; labels in, int64 labels out with -1 for the outliers; None in, keep out."""
    import neighbors
    pts, kind, h = cases.floater_scene()
    xyz = _dev(pts)
    idx, d2 = neighbors.knn(xyz, 8)
    everything = torch.ones(len(pts), dtype=torch.bool, device=DEV)
    largest = neighbors.keep_largest(everything, idx, dist2=d2, max_dist=1.2 * h).cpu().numpy()
    assert largest[kind == 1].all() and largest[kind == 2].all() and not largest[kind == 3].any() and largest[kind == 0].mean() > 0.9
    lists = cases.scene_lists()
    mask = kind != 3
    labels = np.minimum(kind, 2)
    # statistical
    keep = neighbors.remove_statistical_outliers(None, xyz, k=8, ratio=2.0)
    assert keep.dtype == torch.bool
    assert np.array_equal(keep.cpu().numpy(), cases.judged("scene-all", *lists, None, 1, 2.0)[1])
    out = neighbors.remove_statistical_outliers(_dev(mask), xyz, k=8, ratio=2.0)
    want = cases.judged("scene-mask", *lists, mask.astype(np.int64) - 1, 1, 2.0)[1]
    assert out.dtype == torch.bool and np.array_equal(out.cpu().numpy(), want)
    assert not want[kind == 3].any() and want[kind == 2].mean() < 0.1 and want[kind == 0].mean() > 0.9
    for dtype in (torch.int32, torch.int64):
        out = neighbors.remove_statistical_outliers(_dev(labels, dtype), xyz, k=8, ratio=2.0, num_labels=3)
        want = cases.judged("scene-labels", *lists, labels, 3, 2.0)[1]
        assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), np.where(want, labels, -1))
    # radius
    radius, least = 0.6 * h, 4
    r2 = cases.radius2_of(radius)
    want = oo.radius_count(pts, r2) >= least
    keep = neighbors.remove_radius_outliers(None, xyz, radius, least)
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), want)
    assert not want[kind >= 2].any() and want[kind == 0].mean() > 0.9
    want = oo.radius_count(pts, r2, mask.astype(np.int64) - 1) >= least
    out = neighbors.remove_radius_outliers(_dev(mask), xyz, radius, least)
    assert out.dtype == torch.bool and np.array_equal(out.cpu().numpy(), want) and not want[~mask].any()
    want = oo.radius_count(pts, r2, labels) >= least
    out = neighbors.remove_radius_outliers(_dev(labels), xyz, radius, least)
    assert out.dtype == torch.int64 and np.array_equal(out.cpu().numpy(), np.where(want, labels, -1))


def test_python_layer_refuses_bad_arguments():
    import neighbors
    xyz = _dev(_points(10, 1))
    idx, d2 = neighbors.knn(xyz, 3)
    for bad in (-1.0, math.nan, "1", True):
        with pytest.raises(ValueError, match="radius"):
            neighbors.radius_count(xyz, bad)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="cap"):
            neighbors.radius_count(xyz, 1.0, cap=bad)
        with pytest.raises(ValueError, match="min_neighbors"):
            neighbors.remove_radius_outliers(None, xyz, 1.0, bad)
    with pytest.raises(ValueError, match=r"points.*torch.float64 \(10, 3\) on cuda:0"):
        neighbors.radius_count(xyz.double(), 1.0)
    with pytest.raises(ValueError, match=r"labels.*torch.float32 \(10,\) on cuda:0"):
        neighbors.radius_count(xyz, 1.0, labels=torch.zeros(10, device=DEV))
    with pytest.raises(ValueError, match=r"labels.*\(9,\)"):
        neighbors.radius_count(xyz, 1.0, labels=torch.zeros(9, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match=r"labels.*on cpu"):
        neighbors.radius_count(xyz, 1.0, labels=torch.zeros(10, dtype=torch.int64))
    for bad in (-1.0, math.inf, math.nan, None):
        with pytest.raises(ValueError, match="ratio"):
            neighbors.outlier_scores(idx, d2, ratio=bad)
    with pytest.raises(ValueError, match="dist2"):
        neighbors.outlier_scores(idx, None)
    with pytest.raises(ValueError, match=r"dist2.*torch.float64"):
        neighbors.outlier_scores(idx, d2.double())
    with pytest.raises(ValueError, match="num_labels"):
        neighbors.outlier_scores(idx, d2, labels=torch.zeros(10, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="num_labels"):
        neighbors.outlier_scores(idx, d2, num_labels=3)
    with pytest.raises(ValueError, match="num_labels"):
        neighbors.remove_statistical_outliers(torch.zeros(10, dtype=torch.int64, device=DEV), xyz, k=3)
    with pytest.raises(ValueError, match=r"mask.*\(9,\)"):
        neighbors.remove_statistical_outliers(torch.zeros(9, dtype=torch.bool, device=DEV), xyz, k=3)
    with pytest.raises(ValueError, match="k = 17"):
        neighbors.remove_statistical_outliers(None, xyz, k=17)
    # the smallest clouds: nothing to score, nothing kept
    for P in (0, 1):
        few = xyz[:P]
        assert neighbors.remove_statistical_outliers(None, few, k=3).tolist() == [False] * P
        assert neighbors.remove_radius_outliers(None, few, 1.0, 1).tolist() == [False] * P
        out = neighbors.outlier_scores(*neighbors.knn(few, 3))
        assert out.stats.cpu().tolist() == [[0, 0, 0, 0]] and out.score.tolist() == [math.inf] * P


# ---- capture ------------------------------------------------------------------------------------------------------------------

def test_capture_and_replay():
    """knn + outlier_scores + radius_count captured as one linear graph on one stream, replayed on new points behind the same
    pointers: the judge's results for the new points."""
    import neighbors
    sets = [cases.capture_points(0), cases.capture_points(1)]
    radius = cases.radii_of(("capture", 0), sets[0])[2]
    xyz = _dev(sets[0])

    def run():
        idx, d2 = neighbors.knn(xyz, 8)
        out = neighbors.outlier_scores(idx, d2, ratio=2.0)
        return out.score, out.keep, out.stats, neighbors.radius_count(xyz, radius, cap=5)

    want = []
    for which in (0, 1):
        p = sets[which]
        idx, d2 = cases._once(("capture lists", which), lambda: cases.no.knn(p, 8))
        want.append(cases.judged(f"capture-{which}", idx, d2, None, 1, 2.0) + (oo.radius_count(p, cases.radius2_of(radius), cap=5),))
    assert not np.array_equal(want[0][1], want[1][1]) and not np.array_equal(want[0][3], want[1][3])
    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # one stream, no parallel branches
        captured = run()
    for which in (0, 1, 0):
        xyz.copy_(_dev(sets[which]))
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        sc, keep, stats, cnt = (t.cpu().numpy() for t in captured)
        _check_outliers((sc, keep, stats), want[which][:3], f"replay of set {which}")
        assert np.array_equal(cnt, want[which][3])
