"""The judge of the group statistics (tests/group_stats_oracle.py) judged itself, without a GPU: against an independent numpy
route (bincount, np.cov, minimum.at) and scipy's connected components, every rule of include/f3dgs.h (f3dgs_group_stats,
f3dgs_group_merge) on hand-built cases, and the argument checks of the C ABI and of groups.py that answer before any device work."""
import ctypes
import os

import numpy as np
import pytest

import group_stats_oracle as go
from util import ROOT

INF = np.inf
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def test_judge_equals_an_independent_numpy_route():
    P, G, C = 3000, 37, 5
    g = np.random.default_rng(5)
    ids = g.integers(-3, G + 3, P)
    xyz = (g.normal(0, 2, (P, 3)) + [10, -20, 5]).astype(np.float32)
    w = g.random(P).astype(np.float32)
    w[g.random(P) < 0.1] = 0
    f = g.normal(0, 1, (P, C)).astype(np.float32)
    got = go.group_stats(ids, xyz, G, w, f)
    ok = (ids >= 0) & (ids < G) & (w > 0)
    assert np.array_equal(ok, go.members(ids, xyz, G, w))
    gi, wd, xd, fd = ids[ok], w[ok].astype(np.float64), xyz[ok].astype(np.float64), f[ok].astype(np.float64)
    count = np.bincount(gi, minlength=G)
    M = np.bincount(gi, weights=wd, minlength=G)
    assert count.min() > 1 and np.array_equal(got["count"], count)
    assert np.allclose(got["mass"], M, rtol=2e-7, atol=0)
    lo, hi = np.full((G, 3), np.inf, np.float32), np.full((G, 3), -np.inf, np.float32)
    np.minimum.at(lo, gi, xyz[ok])
    np.maximum.at(hi, gi, xyz[ok])
    assert np.array_equal(got["aabb"], np.concatenate([lo, hi], 1))
    for a in range(3):
        assert np.allclose(got["centroid"][:, a], np.bincount(gi, weights=wd * xd[:, a], minlength=G) / M, rtol=2e-7, atol=0)
    for c in range(C):
        assert np.allclose(got["feature_mean"][:, c], np.bincount(gi, weights=wd * fd[:, c], minlength=G) / M, rtol=0, atol=1e-6)
    for k in range(G):
        cov = np.cov(xd[gi == k].T, aweights=wd[gi == k], bias=True)
        want = np.array([cov[a, b] for a, b in go.COV_PAIRS])
        assert np.allclose(got["cov"][k], want, rtol=1e-6, atol=1e-7), k
    # the bounds: positive, and small against the values - a bound of the size of the value would judge nothing
    assert (got["mass_bar"] > 0).all() and (got["mass_bar"] < 1e-6 * M).all()
    assert (got["centroid_bar"] < 1e-6 * np.abs(got["centroid"]) + 1e-12).all()
    assert (got["cov_bar"] < 1e-6 * got["cov"][:, [0]].clip(1) + 1e-12).all()
    assert (got["feature_bar"] < 1e-6).all()


def test_bound_is_ulp_plus_the_summation_term():
    """one group, two members, by hand"""
    xyz = np.array([[1, 0, 0], [3, 0, 0]], np.float32)
    got = go.group_stats([0, 0], xyz, 1, np.array([1, 3], np.float32))
    assert got["mass"][0] == 4 and got["centroid"][0, 0] == 2.5
    assert got["centroid_bar"][0, 0] == float(np.spacing(np.float32(2.5))) + 4 * 2 * 2.0 ** -53 * 10 / 4
    assert got["mass_bar"][0] == float(np.spacing(np.float32(4))) + 4 * 2 * 2.0 ** -53 * 4
    assert got["cov"][0, 0] == np.float32((1 * 1.5 ** 2 + 3 * 0.5 ** 2) / 4) and (got["cov"][0, 1:] == 0).all()
    assert go.ulp32(np.inf) == 0 and go.ulp32(np.nan) == 0 and go.ulp32(1.0) == 2.0 ** -23


def test_rules_of_membership_and_the_empty_values():
    nan = np.nan
    xyz = np.array([[1, 2, 3], [4, 5, 6], [nan, 0, 0], [0, INF, 0], [7, 8, 9], [1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4], [5, 5, 5]], np.float32)
    ids = np.array([0, 0, 0, 0, 2, -1, 3, I32_MIN, I32_MAX, 0])
    w = np.array([1, 2, 1, 1, 1, 1, 1, 1, 1, 0], np.float32)
    assert go.members(ids, xyz, 3, w).tolist() == [True, True, False, False, True, False, False, False, False, False]
    for bad in (0.0, -0.0, nan, INF, -1.0, -INF):
        w2 = w.copy()
        w2[0] = bad
        assert not go.members(ids, xyz, 3, w2)[0], bad
    got = go.group_stats(ids, xyz, 3, w)
    assert got["count"].tolist() == [2, 0, 1] and got["mass"].tolist() == [3, 0, 1]
    assert np.array_equal(got["centroid"], np.array([[3, 4, 5], [0, 0, 0], [7, 8, 9]], np.float32))
    assert np.array_equal(got["aabb"][1], np.array([INF] * 3 + [-INF] * 3, np.float32))            # an empty group
    assert np.array_equal(got["aabb"][0], np.array([1, 2, 3, 4, 5, 6], np.float32))
    assert (got["cov"][1] == 0).all() and (got["cov"][2] == 0).all()                                # empty; a single member
    assert np.allclose(got["cov"][0], 2.0)                                                          # (1, 2) weights about 3: 2 * 4 / 3 + 1 / 3 ... = 2
    assert got["feature_mean"] is None
    # without weights everybody with finite coordinates and an id in range is a member
    assert go.group_stats(ids, xyz, 3)["count"].tolist() == [3, 0, 1]
    # P == 0
    empty = go.group_stats(np.zeros(0, np.int64), np.zeros((0, 3), np.float32), 2, None, np.zeros((0, 4), np.float32))
    assert empty["count"].tolist() == [0, 0] and (empty["feature_mean"] == 0).all() and empty["feature_mean"].shape == (2, 4)
    assert np.array_equal(empty["aabb"], np.array([[INF] * 3 + [-INF] * 3] * 2, np.float32))


def test_box_orders_minus_zero_below_plus_zero_and_features_propagate():
    xyz = np.array([[0.0, -0.0, 1], [-0.0, 0.0, 1]], np.float32)
    box = go.group_stats([0, 0], xyz, 1)["aabb"][0]
    assert np.signbit(box[:2]).all() and not np.signbit(box[3:5]).any()
    assert go.order_key(np.float32(-0.0)) + 1 == go.order_key(np.float32(0.0))
    f = np.array([[1, INF, np.nan, INF], [3, 1, 1, -INF]], np.float32)
    fm = go.group_stats([0, 0], xyz, 1, None, f)["feature_mean"][0]
    assert fm[0] == 2 and fm[1] == INF and np.isnan(fm[2]) and np.isnan(fm[3])
    assert go.within(fm, fm, 0).all() and not go.within([INF], [-INF], 1).any() and not go.within([1.0], [np.nan], 1).any()


def _scipy_roots(G, pairs):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    a = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(G, G))
    n, part = connected_components(a, directed=False)
    first = np.full(n, G, np.int64)
    np.minimum.at(first, part, np.arange(G))
    return first[part]


@pytest.mark.parametrize("mutual", [False, True])
def test_merge_judge_equals_scipy(mutual):
    """The adjacency restated as a loop over the slots; the partition is scipy's on the thresholded group graph."""
    P, K, G, C = 2000, 4, 60, 6
    g = np.random.default_rng(9)
    ids = g.integers(-2, G + 2, P)
    idx = g.integers(-1, P + 1, (P, K)).astype(np.int32)
    idx[g.random((P, K)) < 0.9] = -1
    for i in g.choice(P, P // 4, replace=False):                    # a fair share of two-sided edges
        j = idx[i, 0]
        if 0 <= j < P:
            idx[j, g.integers(0, K)] = i
    dist2 = g.random((P, K)).astype(np.float32)
    dist2[g.random((P, K)) < 0.05] = np.nan
    fm = g.normal(0, 1, (G, C)).astype(np.float32)
    fm[7] = 0                                                       # a zero norm: merges with nobody
    limit, min_cos = np.float32(0.8), -0.1
    directed = set()
    for i in range(P):
        for s in range(K):
            j = int(idx[i, s])
            if 0 <= j < P and j != i and 0 <= ids[i] < G and 0 <= ids[j] < G and ids[i] != ids[j] and dist2[i, s] <= limit:
                directed.add((i, j))
    pairs = {(min(ids[a], ids[b]), max(ids[a], ids[b])) for a, b in directed if not mutual or (b, a) in directed}
    pairs = np.array(sorted(pairs), np.int64).reshape(-1, 2)
    assert len(pairs) >= 20
    assert np.array_equal(go.adjacency(ids, idx, G, dist2, limit, mutual), pairs)
    m = fm.astype(np.float64)
    keep = []
    for a, b in pairs:
        na, nb = m[a] @ m[a], m[b] @ m[b]
        if na > 0 and nb > 0 and m[a] @ m[b] / np.sqrt(na * nb) >= min_cos:
            keep.append((a, b))
    assert 3 <= len(keep) < len(pairs) and not any(7 in p for p in keep)
    want_root = _scipy_roots(G, np.array(keep, np.int64))
    out, root = go.group_merge(ids, idx, fm, min_cos, dist2, limit, mutual)
    assert np.array_equal(root, want_root) and root[7] == 7
    inside = (ids >= 0) & (ids < G)
    assert np.array_equal(out[inside], want_root[ids[inside]]) and (out[~inside] == -1).all()


def test_merge_judge_refuses_a_cosine_at_the_threshold():
    fm = np.array([[1, 0], [1, 0], [0, 1]], np.float32)
    ids, idx = np.array([0, 1, 2]), np.array([[1], [2], [0]], np.int32)
    out, root = go.group_merge(ids, idx, fm, 0.5)
    assert root.tolist() == [0, 0, 2] and out.tolist() == [0, 0, 2]
    with pytest.raises(AssertionError, match="within rounding"):
        go.group_merge(ids, idx, fm, 1.0)
    assert go.group_merge(np.array([5, -1, I32_MIN]), idx, fm, 0.5)[0].tolist() == [-1, -1, -1]


# ---- the C ABI: what is refused before any device work ---------------------------------------------------------------------

def _lib():
    so = os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import torch  # noqa: F401  (its bundled HIP runtime must be the one the library binds to)
    lib = ctypes.CDLL(so)
    vp, ci, cf, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_version.restype = ci
    lib.f3dgs_group_stats_scratch_bytes.restype = sz
    lib.f3dgs_group_stats_scratch_bytes.argtypes = [ci, ci]
    lib.f3dgs_group_stats.argtypes = [ci, ci, ci, vp, vp, vp, vp, ctypes.c_int64, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.f3dgs_group_merge_scratch_bytes.restype = sz
    lib.f3dgs_group_merge_scratch_bytes.argtypes = [ci]
    lib.f3dgs_group_merge.argtypes = [ci, ci, ci, ci, vp, vp, vp, cf, ci, vp, cf, vp, vp, vp, vp, sz, vp]
    return lib


def test_c_abi_refuses_bad_arguments_without_gpu():
    lib = _lib()
    assert lib.f3dgs_version() >= 32000
    A, B, D, F, S = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000        # aligned, never dereferenced addresses
    INV, UNS = -1, -4
    err = lib.f3dgs_last_error
    BIG = 1 << 40

    def stats(P=10, G=4, C=8, groups=A, xyz=B, weight=None, features=F, stride=8, count=D, mass=None, centroid=None, cov=None, aabb=None,
              fm=None, scratch=S, nbytes=BIG):
        return lib.f3dgs_group_stats(P, G, C, groups, xyz, weight, features, stride, count, mass, centroid, cov, aabb, fm, scratch, nbytes, None)

    need = lib.f3dgs_group_stats_scratch_bytes(300, 32)
    assert need >= 300 * (32 + 10) * 8 and lib.f3dgs_group_stats_scratch_bytes(1, 0) > 0
    assert lib.f3dgs_group_stats_scratch_bytes(65536, 4096) >= 65536 * 4096 * 8               # (no 32-bit overflow)
    assert stats(P=-1) == INV and b"P < 0" in err()
    for G in (0, -1, 65537):
        assert stats(G=G) == INV and b"1 .. 65536" in err()
    for C in (-1, 4097):
        assert stats(C=C) == INV and b"0 .. 4096" in err()
    assert stats(features=None) == INV and b"features" in err()
    assert stats(C=0, features=None, fm=D) == INV and b"C = 0" in err()
    assert stats(stride=7) == INV and b"feature_stride" in err()
    for kw in (dict(groups=None), dict(xyz=None)):
        assert stats(**kw) == INV and b"null" in err(), kw
    assert stats(count=None) == INV and b"every output" in err()
    assert stats(scratch=None) == INV and b"scratch" in err()
    assert stats(nbytes=lib.f3dgs_group_stats_scratch_bytes(4, 8) - 1) == INV and b"scratch" in err()
    assert stats(scratch=S + 4) == INV and b"8-byte" in err()

    def merge(P=10, K=3, G=4, C=8, groups=A, idx=B, dist2=None, max_dist2=INF, mutual=0, fm=F, min_cos=0.5, root=D, out=D + 0x1000,
              status=D + 0x2000, scratch=S, nbytes=BIG):
        return lib.f3dgs_group_merge(P, K, G, C, groups, idx, dist2, max_dist2, mutual, fm, min_cos, root, out, status, scratch, nbytes, None)

    assert lib.f3dgs_group_merge_scratch_bytes(4096) >= 4096 * 4096 // 8 + 4096 * 4
    assert merge(P=-1) == INV and b"P < 0" in err()
    for K in (0, 17):
        assert merge(K=K) == INV and b"1 .. 16" in err()
    for G in (0, 4097):
        assert merge(G=G) == INV and b"1 .. 4096" in err()
    for C in (0, 4097):
        assert merge(C=C) == INV and b"channels" in err()
    assert merge(P=(1 << 30) + 1) == UNS
    for bad in (-1.0, np.nan):
        assert merge(max_dist2=bad, dist2=A) == INV and b"negative or NaN" in err()
    assert merge(min_cos=np.nan) == INV and b"min_cos" in err()
    assert merge(max_dist2=2.0) == INV and b"needs dist2" in err()
    for kw in (dict(groups=None), dict(idx=None), dict(fm=None), dict(root=None), dict(out=None), dict(status=None)):
        assert merge(**kw) == INV and b"null" in err(), kw
    assert merge(scratch=None) == INV and b"scratch" in err()
    assert merge(nbytes=lib.f3dgs_group_merge_scratch_bytes(4) - 1) == INV and b"scratch" in err()
    assert merge(scratch=S + 2) == INV and b"4-byte" in err()


def test_python_surface_refuses_cpu_tensors():
    import torch
    import groups
    ids = torch.zeros(10, dtype=torch.int64)
    xyz = torch.zeros(10, 3)
    idx = torch.zeros(10, 3, dtype=torch.int32)
    fm = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="HIP device.*int64.*10.*cpu"):
        groups.group_stats(ids, xyz, 4)
    with pytest.raises(ValueError, match="HIP device"):
        groups.group_stats(ids > 0, xyz)
    with pytest.raises(ValueError, match="HIP device"):
        groups.merge_similar(ids, idx, fm, 0.5)
    with pytest.raises(ValueError, match="HIP device"):
        groups.select_groups(ids, fm, torch.zeros(2, 8))
    with pytest.raises(ValueError, match="labels\\(\\)"):
        groups.lifter_stats(object(), xyz)
    assert groups.GroupStats._fields == ("count", "mass", "centroid", "cov", "aabb_min", "aabb_max", "feature_mean")
    assert groups.MergedGroups._fields == ("groups", "group_root", "status")
    assert {"group_stats", "lifter_stats", "select_groups", "merge_similar"} <= set(groups.__all__)
