"""The neighbourhood kernels on the GPU (csrc/neighbors.hip; neighbors.py: knn, mode_filter, smooth_labels, clean_selection).
The judge is tests/neighbors_oracle.py - numpy, brute force, the kernel's float32 operation order - and EVERY comparison is exact:
idx equal, dist2 equal as bits, labels equal, share equal as bits.  The result is defined as a function of the inputs alone, so
there is nothing to tolerate."""
import types

import numpy as np
import pytest
import torch

import neighbors_oracle as no
from test_gpu_contrib import _Model, _camera
from test_knn import _points
from test_neighbors_cpu import lattice

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLT_MAX = np.finfo(np.float32).max
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _knn(p, K, dist2=True):
    import neighbors
    idx, d2 = neighbors.knn(torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(DEV), K, return_dist2=dist2)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (len(p), K)
    if not dist2:
        assert d2 is None
        return idx.cpu().numpy(), None
    assert d2.dtype == torch.float32 and d2.shape == idx.shape
    return idx.cpu().numpy(), d2.cpu().numpy()


def _want(key, make):
    """the judge's answer, computed once per input and left unchanged"""
    if key not in _cache:
        _cache[key] = make()
        for a in _cache[key]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _cache[key]


def _check_knn(p, K, key, option=None):
    """option (the fixture): both walk orders are run - scheduling only, the same bits"""
    want_idx, want_d2 = _want(("knn", key, K), lambda: no.knn(p, K))
    for outward in ((1, 0) if option is not None else (None,)):
        if outward is not None:
            option("knn_outward", outward)
        idx, d2 = _knn(p, K)
        what = f"{key}, K = {K}, knn_outward = {outward}"
        assert np.array_equal(idx, want_idx), f"{what}: {int((idx != want_idx).any(1).sum())} rows differ"
        assert np.array_equal(_bits(d2), _bits(want_d2)), what
    return idx, d2


# around the wave edge (64), the leaf edge (256), a partial last leaf; around every list size of the kernel (4, 8, 16)
@pytest.mark.parametrize("P", [0, 1, 2, 16, 17, 63, 64, 65, 255, 256, 257, 1000])
def test_knn_sizes(P, option):
    p = _points(P, 11 + P, "uniform") if P else np.zeros((0, 3), np.float32)
    for K in (1, 3, 4, 5, 8, 9, 16):
        idx, d2 = _check_knn(p, K, ("uniform", P), option=option)
        if P - 1 < K:
            assert (idx[:, max(P - 1, 0):] == -1).all() and (d2[:, max(P - 1, 0):] == FLT_MAX).all()


@pytest.mark.parametrize("kind", ["clustered", "planar"])
def test_knn_pruning_far_from_the_origin(kind, option):
    _check_knn(_points(5000, 11, kind), 16, (kind, 5000), option=option)


@pytest.mark.parametrize("K", [6, 8, 16])
def test_knn_shuffled_lattice_every_row_tied(K, option):
    """12 x 12 x 12 integer points, shuffled: every row holds equal distances, many of them across leaves.  Fails where a leaf is
    pruned with <, where the box bound is not monotone with the distances, where ties follow the Morton order."""
    p = lattice(12, 7)
    idx, d2 = _check_knn(p, K, ("lattice", 12), option=option)
    assert (np.diff(d2, axis=1) == 0).any(1).all()


def test_knn_duplicates_non_finite_points_and_no_dist2():
    p = np.repeat(_points(300, 5), 4, axis=0)                     # every point four times
    idx, d2 = _check_knn(p, 5, ("dup", 300))
    assert (d2[:, :3] == 0).all() and (d2[:, 3] > 0).all()
    assert np.array_equal(idx[:, :3] // 4, np.arange(1200)[:, None] // 4 * np.ones((1, 3), np.int64))
    q = _points(500, 8).copy()
    q[123, 2] = np.nan
    q[377, 0] = -np.inf
    idx, d2 = _check_knn(q, 8, ("nonfinite", 500))
    assert (idx[[123, 377]] == -1).all() and not np.isin(idx, [123, 377]).any()
    idx_only, none = _knn(q, 8, dist2=False)
    assert none is None and np.array_equal(idx_only, idx)


def test_knn_agrees_with_distcuda2():
    """the existing product on the same points: its mean of three squared distances, within the bar tests/test_knn.py holds it to
    (the two units round differently by design)"""
    from simple_knn._C import distCUDA2
    for kind in ("uniform", "clustered"):
        p = _points(5000, 11, kind)
        _, d2 = _knn(p, 3)
        mean = distCUDA2(torch.from_numpy(p).to(DEV)).cpu().numpy()
        assert np.allclose(d2.sum(1) / 3, mean, rtol=2e-6, atol=0), kind


# ---- the mode filter ------------------------------------------------------------------------------------------------------

def _lists():
    def make():
        p = _points(2000, 13, "clustered")
        idx, d2 = no.knn(p, 8)
        return p, idx, d2
    return _want("filter lists", make)


def _filter(labels, idx, dtype=torch.int64, weight=None, dist2=None, **kw):
    import neighbors
    t = lambda a, dt=None: None if a is None else torch.as_tensor(np.array(a), dtype=dt).to(DEV)      # (a copy: the judge's arrays are read-only)
    out = neighbors.mode_filter(t(labels, dtype), t(idx, torch.int32), weight=t(weight, torch.float32), dist2=t(dist2, torch.float32),
                                return_share=True, **kw)
    torch.cuda.synchronize()
    assert out[0].dtype == torch.int64 and out[1].dtype == torch.float32
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def _check_filter(labels, idx, what, weight=None, dist2=None, max_dist=None, fill=True, iterations=1, dtype=torch.int64):
    with np.errstate(over="ignore"):
        max_dist2 = np.inf if max_dist is None else np.float32(max_dist) * np.float32(max_dist)
    want, want_share = no.mode_filter(labels, idx, weight, dist2, max_dist2, fill, iterations)
    got, share = _filter(labels, idx, dtype, weight, dist2, max_dist=max_dist, fill=fill, iterations=iterations)
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} labels differ"
    assert np.array_equal(_bits(share), _bits(want_share)), what
    return got


def test_filter_equals_the_judge():
    _, idx, d2 = _lists()
    g = np.random.default_rng(3)
    P = len(idx)
    labels = g.integers(0, 5, P)
    labels[g.random(P) < 0.1] = -1
    w = g.random(P).astype(np.float32)
    w[g.random(P) < 0.15] = 0
    ones = _check_filter(labels, idx, "weights all 1")
    assert (ones != labels).sum() > P // 10
    _check_filter(labels, idx, "int32 labels", dtype=torch.int32)
    _check_filter(labels, idx, "random weights with zeros", weight=w)
    _check_filter(labels, idx, "fill off", weight=w, fill=False)
    kept = _check_filter(labels, idx, "fill off, weights 1", fill=False)
    assert (kept[labels < 0] == -1).all()
    radius = float(np.sqrt(np.median(d2[:, 3])))                  # about half of the neighbours are beyond it
    _check_filter(labels, idx, "finite max_dist", weight=w, dist2=d2, max_dist=radius)
    _check_filter(labels, idx, "three iterations", weight=w, iterations=3)
    _check_filter(labels, idx, "three iterations, limited, no fill", dist2=d2, max_dist=radius, fill=False, iterations=3)
    big = np.where(labels >= 0, 2**31 - 1 - labels, -1)           # labels up to 2^31 - 1
    _check_filter(big, idx, "large labels", weight=w)
    assert _check_filter(big, idx, "large labels, int32", dtype=torch.int32).max() == 2**31 - 1
    for K in (1, 4, 5):                                           # the other list sizes of the kernel
        _check_filter(labels, idx[:, :K].copy(), f"K = {K}", weight=w)
    idx16, d16 = _want("filter lists 16", lambda: no.knn(_lists()[0], 16))
    _check_filter(labels, idx16, "K = 16", weight=w)
    _check_filter(labels, idx16, "K = 16, weights 1, limited", dist2=d16, max_dist=radius)


def test_filter_short_lists_and_corrupted_idx():
    p = _points(6, 2)
    idx, d2 = no.knn(p, 8)                                        # P <= K: the lists end in -1
    assert (idx[:, 5:] == -1).all()
    _check_filter([3, 3, -1, 7, 7, 7], idx, "P <= K")
    _check_filter([3, 3, -1, 7, 7, 7], idx, "P <= K, limited", dist2=d2, max_dist=1e30, fill=False)
    _, idx, _ = _lists()
    g = np.random.default_rng(4)
    P = len(idx)
    bad = idx.copy()
    bad[g.random(bad.shape) < 0.2] = -7
    bad[g.random(bad.shape) < 0.2] = P
    bad[0], bad[-1] = P, -7
    labels = g.integers(-1, 4, P)
    _check_filter(labels, bad, "idx with -7 and P", weight=g.random(P).astype(np.float32))      # the judge's answer: a result check


def test_lifter_end_to_end():
    """One 64 x 64 view of a synth scene through LabelLifter; smooth_labels and clean_selection against the judge applied to the
    lifter's own labels() / confidence() / select() read back."""
    import contrib
    import neighbors
    from synth import make_scene
    sc = make_scene(P=2000, C=0, width=64, height=64, seed=21, scale_lo=0.01, scale_hi=0.1)
    P, L = 2000, 6
    y, x = np.mgrid[0:64, 0:64]
    label_map = ((x // 11) % 3 + 3 * (y // 32)).astype(np.int64)
    lifter = contrib.LabelLifter(P, L, DEV)
    pc = _Model(sc)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    lifter.add_view(_camera(sc), pc, pipe, sc["bg"].to(DEV), torch.from_numpy(label_map).to(DEV))
    xyz = pc.get_xyz
    labels, conf, seen = lifter.labels().cpu().numpy(), lifter.confidence().cpu().numpy(), lifter.seen(0.05).cpu().numpy()
    assert 0.2 < (labels >= 0).mean() and len(np.unique(labels[labels >= 0])) >= 3
    idx, d2 = no.knn(sc["means3D"].numpy(), 8)
    entering = np.where(seen, labels, -1)
    for kw in (dict(), dict(iterations=2, fill=False), dict(max_dist=0.4)):
        got = neighbors.smooth_labels(lifter, xyz, k=8, min_weight=0.05, **kw)
        limit = np.inf if "max_dist" not in kw else np.float32(kw["max_dist"]) * np.float32(kw["max_dist"])
        want, _ = no.mode_filter(entering, idx, conf, d2, limit, kw.get("fill", True), kw.get("iterations", 1))
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), kw
        assert (want != entering).any()                           # (the filter does move labels of this scene)
    dev_idx, dev_d2 = neighbors.knn(xyz, 8)
    assert np.array_equal(dev_idx.cpu().numpy(), idx)
    for cls in (0, 4):
        mask = lifter.select(cls, threshold=0.5)
        got = neighbors.clean_selection(mask, dev_idx)
        want, _ = no.mode_filter(mask.cpu().numpy().astype(np.int64), idx)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want == 1)
        assert (got != mask).any()
        got = neighbors.clean_selection(mask, dev_idx, weight=lifter.confidence(), dist2=dev_d2, max_dist=0.4, iterations=2)
        want, _ = no.mode_filter(mask.cpu().numpy().astype(np.int64), idx, conf, d2, np.float32(0.4) * np.float32(0.4), True, 2)
        assert np.array_equal(got.cpu().numpy(), want == 1)


def test_errors():
    import neighbors
    from simple_knn import _C
    pts = torch.zeros(10, 3, device=DEV)
    idx = torch.zeros(10, 3, device=DEV, dtype=torch.int32)
    labels = torch.zeros(10, device=DEV, dtype=torch.int64)
    for bad in (torch.zeros(10, 3), torch.zeros(10, 4, device=DEV), torch.zeros(10, 3, device=DEV, dtype=torch.float64),
                torch.zeros(30, device=DEV)):
        with pytest.raises(ValueError):
            neighbors.knn(bad, 3)
    for k in (0, 17, 3.0):
        with pytest.raises(ValueError):
            neighbors.knn(pts, k)
    with pytest.raises(Exception, match="1 .. 16"):
        _C.knn_neighbors(pts, 17, True)
    for args, kw in (((labels.cpu(), idx), {}), ((labels, idx.cpu()), {}), ((labels.float(), idx), {}), ((labels, idx.long()), {}),
                     ((labels[:9], idx), {}), ((labels, idx), dict(weight=torch.ones(10, device=DEV, dtype=torch.float64))),
                     ((labels, idx), dict(weight=torch.ones(9, device=DEV))), ((labels, idx), dict(dist2=torch.ones(10, 2, device=DEV))),
                     ((labels, idx), dict(max_dist=1.0)), ((labels, idx), dict(max_dist=-1.0, dist2=torch.ones(10, 3, device=DEV))),
                     ((labels, idx), dict(iterations=0)), ((labels, torch.zeros(10, 17, device=DEV, dtype=torch.int32)), {})):
        with pytest.raises(ValueError):
            neighbors.mode_filter(*args, **kw)
    l32 = labels.int()
    with pytest.raises(Exception, match="in place"):
        _C.label_mode_filter(l32, None, idx, None, float("inf"), True, l32, None)
    with pytest.raises(Exception, match="needs dist2"):
        _C.label_mode_filter(l32, None, idx, None, 2.0, True, torch.empty_like(l32), None)
    with pytest.raises(ValueError):
        neighbors.clean_selection(labels, idx)
    with pytest.raises(ValueError):
        neighbors.smooth_labels(object(), pts)


def test_capture_and_replay():
    """knn and two filter iterations captured on one stream and replayed twice: the eager bits, also on new points behind the
    same pointers.  Nothing is allocated by the test inside the capture."""
    import neighbors
    p0, p1 = _points(3000, 31, "clustered"), _points(3000, 32, "uniform")
    g = np.random.default_rng(6)
    pts = torch.from_numpy(p0).to(DEV)
    labels = torch.from_numpy(g.integers(-1, 5, 3000)).to(DEV)
    weight = torch.from_numpy(g.random(3000).astype(np.float32)).to(DEV)

    def run():
        idx, d2 = neighbors.knn(pts, 8)
        out, share = neighbors.mode_filter(labels, idx, weight=weight, dist2=d2, max_dist=0.5, iterations=2, return_share=True)
        return idx, d2, out, share

    def eager(p):
        pts.copy_(torch.from_numpy(p).to(DEV))
        res = [t.clone() for t in run()]
        torch.cuda.synchronize()
        return res

    want = {0: eager(p0), 1: eager(p1)}
    assert not torch.equal(want[0][0], want[1][0])
    pts.copy_(torch.from_numpy(p0).to(DEV))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # one stream, no parallel branches
        captured = run()
    for which, p in ((0, p0), (1, p1)):
        pts.copy_(torch.from_numpy(p).to(DEV))
        for t in captured:
            t.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, want[which]):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
