"""The judge of the neighbourhood kernels (tests/neighbors_oracle.py) judged itself, without a GPU: the brute-force float32 search
against scipy's k-d tree in float64, the rules of the lists and of the mode filter on hand-built cases, and the argument checks
of the C ABI that answer before any device work."""
import ctypes
import os

import numpy as np
import pytest

import neighbors_oracle as no
from test_knn import _points
from util import ROOT

FLT_MAX = np.finfo(np.float32).max


@pytest.mark.parametrize("kind", ["uniform", "clustered", "planar"])
def test_bruteforce_equals_the_kdtree_exactly(kind):
    """P = 5000, seed 11, K = 16: no row of these three families has a tied distance, and the float32 rounding of the distances
    reorders no pair: the index rows of the two searches are identical, in identical order, nothing left out."""
    from scipy.spatial import cKDTree
    p = _points(5000, 11, kind)
    idx, dist2 = no.knn(p, 16)
    _, want = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=17)
    assert np.array_equal(want[:, 0], np.arange(5000))            # the point itself, at distance 0
    assert np.array_equal(idx, want[:, 1:].astype(np.int32))
    assert (np.diff(dist2, axis=1) > 0).all()                     # strictly ascending: no tie anywhere
    exact = ((p[idx].astype(np.float64) - p[:, None, :].astype(np.float64)) ** 2).sum(2)
    assert np.allclose(dist2, exact, rtol=3e-7 * 4, atol=0)


def test_duplicates_are_neighbours_ordered_by_index():
    base = _points(5, 2)
    p = np.concatenate([base, base, base])                        # point i again at i + 5 and i + 10
    idx, dist2 = no.knn(p, 3)
    for i in range(15):
        twins = sorted({i % 5, i % 5 + 5, i % 5 + 10} - {i})
        assert idx[i, :2].tolist() == twins and (dist2[i, :2] == 0).all() and dist2[i, 2] > 0
    same = np.zeros((6, 3), np.float32)                           # every distance 0: the order is the index order, self left out
    idx, dist2 = no.knn(same, 4)
    assert idx.tolist() == [[j for j in range(6) if j != i][:4] for i in range(6)] and (dist2 == 0).all()


def lattice(n, seed):
    g = np.random.default_rng(seed)
    pts = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    return pts[g.permutation(len(pts))]


def test_shuffled_lattice_ties_resolve_by_index():
    p = lattice(5, 4)
    for K in (6, 8):
        idx, dist2 = no.knn(p, K)
        for i in range(len(p)):
            d = ((p - p[i]) ** 2).sum(1)                          # small integers: exact in any format
            d[i] = np.inf
            order = sorted(range(len(p)), key=lambda j: (d[j], j))[:K]
            assert idx[i].tolist() == order and dist2[i].tolist() == [d[j] for j in order]
        assert (np.diff(dist2, axis=1) == 0).any(1).all()         # a tie in every row


def test_fewer_points_than_neighbours():
    idx, dist2 = no.knn(np.zeros((0, 3), np.float32), 3)
    assert idx.shape == (0, 3) and dist2.shape == (0, 3)
    idx, dist2 = no.knn(np.ones((1, 3), np.float32), 2)
    assert idx.tolist() == [[-1, -1]] and (dist2 == FLT_MAX).all()
    p = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0]], np.float32)
    idx, dist2 = no.knn(p, 4)
    assert idx.tolist() == [[1, 2, -1, -1], [0, 2, -1, -1], [1, 0, -1, -1]]
    assert dist2[:, :2].tolist() == [[1, 9], [1, 4], [4, 9]] and (dist2[:, 2:] == FLT_MAX).all()


def test_non_finite_points_have_no_neighbours_and_are_nobodys():
    p = _points(40, 6)
    p[7, 1] = np.nan
    p[23, 0] = np.inf
    idx, dist2 = no.knn(p, 5)
    assert (idx[[7, 23]] == -1).all() and (dist2[[7, 23]] == FLT_MAX).all()
    rest = np.delete(np.arange(40), [7, 23])
    assert not np.isin(idx[rest], [7, 23]).any() and (idx[rest] >= 0).all()
    sub_idx, sub_d = no.knn(p[rest], 5)                           # the others: as if the two were not there
    assert np.array_equal(rest[sub_idx], idx[rest]) and np.array_equal(sub_d, dist2[rest])
    far = np.array([[3e19, 0, 0], [-3e19, 0, 0], [3e19, 1, 0]], np.float32)       # finite points whose distance overflows
    idx, dist2 = no.knn(far, 2)
    assert idx.tolist() == [[2, -1], [-1, -1], [0, -1]]


# ---- the mode filter ------------------------------------------------------------------------------------------------------

def _step(labels, idx, **kw):
    out, share = no.mode_filter_step(np.asarray(labels), np.asarray(idx, np.int32), **kw)
    return out.tolist(), share.tolist()


def test_filter_own_label_wins_a_tie_else_the_smallest_label():
    idx = [[1, 2, 3, 4]] + [[0, 0, 0, 0]] * 4
    # Gaussian 0: own 9, neighbours 5 5 9 7: scores 9 -> 2, 5 -> 2, 7 -> 1: the tie goes to the own label
    assert _step([9, 5, 5, 9, 7], idx)[0][0] == 9
    # own 7, neighbours 8 8 3 3: 8 -> 2, 3 -> 2, 7 -> 1: the own label is not among the tied: the smallest of them
    out, share = _step([7, 8, 8, 3, 3], idx)
    assert out[0] == 3 and share[0] == np.float32(2) / np.float32(5)
    # own label unlabelled, neighbours 8 8 3 3
    assert _step([-1, 8, 8, 3, 3], idx)[0][0] == 3
    # a clear majority beats the own label
    assert _step([7, 8, 8, 8, 3], idx)[0][0] == 8
    # the own label wins a tie through its neighbours even where the Gaussian itself has no vote (weight 0)
    w = np.array([0, 1, 1, 1, 1], np.float32)
    assert _step([4, 4, 2, 2, 4], idx, weight=w)[0][0] == 4
    assert _step([4, 4, 2, 2, 6], idx, weight=w)[0][0] == 2      # 2 -> 2 beats 4 -> 1


def test_filter_fill_and_no_voter():
    idx = [[1, 2], [0, 2], [0, 1]]
    assert _step([-1, 6, 6], idx)[0] == [6, 6, 6]
    out, share = _step([-1, 6, 6], idx, fill=False)
    assert out == [-1, 6, 6] and share[0] == 0.0
    out, share = _step([-1, -5, -1], idx)
    assert out == [-1, -1, -1] and share == [0.0, 0.0, 0.0]


def test_filter_weight_rule():
    idx = [[1, 2, 3, 4]] + [[0, 0, 0, 0]] * 4
    labels = [1, 2, 3, 4, 5]
    w = np.array([0.0, -1.0, np.nan, np.inf, 0.25], np.float32)      # only the last one votes
    out, share = _step(labels, idx, weight=w)
    assert out[0] == 5 and share[0] == 1.0
    w = np.array([0.5, 0.25, 0.125, 0.0, 0.0], np.float32)
    out, share = _step([1, 2, 2, 1, 1], idx, weight=w)               # 1 -> 0.5, 2 -> 0.375
    assert out[0] == 1 and share[0] == np.float32(0.5) / np.float32(0.875)


def test_filter_max_dist2_and_corrupted_idx():
    idx = np.array([[1, 2, 3]] + [[0, 0, 0]] * 3, np.int32)
    d2 = np.array([[1.0, 4.0, 9.0]] + [[1.0, 1.0, 1.0]] * 3, np.float32)
    labels = [0, 1, 2, 2]
    assert _step(labels, idx)[0][0] == 2
    assert _step(labels, idx, dist2=d2, max_dist2=4.0)[0][0] == 0      # 3 is out; 0, 1, 2 tie: the own label
    assert _step(labels, idx, dist2=d2, max_dist2=3.9)[0][0] == 0
    assert _step([-1, 1, 2, 2], idx, dist2=d2, max_dist2=3.9)[0][0] == 1
    assert _step([-1, 1, 2, 2], idx, dist2=d2, max_dist2=0.5)[0][0] == -1
    bad = np.array([[-7, 4, 2, 3]] + [[0, 0, 0, 0]] * 3, np.int32)     # -7 and P: no voters, nothing read
    assert _step(labels, bad)[0][0] == 2
    assert _step([5, 1, 2**31 - 1, 2**31 - 1], idx)[0][0] == 2**31 - 1


def test_filter_iterations_are_single_steps():
    g = np.random.default_rng(5)
    p = _points(300, 9, "clustered")
    idx, d2 = no.knn(p, 6)
    labels = g.integers(-1, 4, 300)
    w = g.random(300).astype(np.float32)
    three, share3 = no.mode_filter(labels, idx, w, iterations=3)
    cur = labels
    for _ in range(3):
        cur, share = no.mode_filter_step(cur, idx, w)
    assert np.array_equal(three, cur) and np.array_equal(share3, share)
    assert not np.array_equal(no.mode_filter_step(labels, idx, w)[0], cur)      # (the steps do move something)


# ---- the C ABI: what is refused before any device work ---------------------------------------------------------------------

def _lib():
    so = os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import torch  # noqa: F401  (its bundled HIP runtime must be the one the library binds to)
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_version.restype = ci
    lib.f3dgs_knn_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_knn_neighbors_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_knn_neighbors_scratch_bytes.argtypes = [ci, ci]
    lib.f3dgs_knn_neighbors.argtypes = [ci, ci, vp, vp, vp, vp, vp]
    lib.f3dgs_label_mode_filter.argtypes = [ci, ci, vp, vp, vp, vp, ctypes.c_float, ci, vp, vp, vp]
    return lib


def test_c_abi_refuses_bad_arguments_without_gpu():
    lib = _lib()
    assert lib.f3dgs_version() >= 31800
    A = 0x10000                                    # an aligned, never dereferenced address
    INV = -1                                       # F3DGS_ERR_INVALID_ARGUMENT
    assert lib.f3dgs_knn_neighbors_scratch_bytes(1000, 16) == lib.f3dgs_knn_scratch_bytes(1000) > 1000 * 16
    assert lib.f3dgs_knn_neighbors_scratch_bytes(-3, 4) == lib.f3dgs_knn_neighbors_scratch_bytes(0, 4)
    assert lib.f3dgs_knn_neighbors(0, 3, None, None, None, None, None) == 0                      # P == 0: a no-op
    assert lib.f3dgs_knn_neighbors(-1, 3, A, A, A, A, None) == INV and b"P < 0" in lib.f3dgs_last_error()
    for K in (0, 17, -2):
        assert lib.f3dgs_knn_neighbors(10, K, A, A, A, A, None) == INV and b"1 .. 16" in lib.f3dgs_last_error()
        assert lib.f3dgs_label_mode_filter(10, K, A, None, A, None, np.inf, 1, A + 64, None, None) == INV
    for args in ((None, A, A, A), (A, None, A, A), (A, A, A, None)):
        assert lib.f3dgs_knn_neighbors(10, 3, *args, None) == INV and b"null" in lib.f3dgs_last_error()
    assert lib.f3dgs_knn_neighbors(10, 3, A, A, None, A + 4, None) == INV and b"16-byte" in lib.f3dgs_last_error()
    # the filter
    assert lib.f3dgs_label_mode_filter(0, 3, None, None, None, None, np.inf, 1, None, None, None) == 0
    assert lib.f3dgs_label_mode_filter(-1, 3, A, None, A, None, np.inf, 1, A + 64, None, None) == INV
    assert lib.f3dgs_label_mode_filter(10, 3, A, None, A, None, np.inf, 1, A, None, None) == INV and b"in place" in lib.f3dgs_last_error()
    assert lib.f3dgs_label_mode_filter(10, 3, A, None, A, None, 2.0, 1, A + 64, None, None) == INV and b"needs dist2" in lib.f3dgs_last_error()
    for bad in (-1.0, np.nan):
        assert lib.f3dgs_label_mode_filter(10, 3, A, None, A, A, bad, 1, A + 64, None, None) == INV
    for args in ((None, A, A + 64), (A, None, A + 64), (A, A, None)):
        assert lib.f3dgs_label_mode_filter(10, 3, args[0], None, args[1], None, np.inf, 1, args[2], None, None) == INV
        assert b"null" in lib.f3dgs_last_error()


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import torch
    import neighbors
    with pytest.raises(ValueError, match="HIP device"):
        neighbors.knn(torch.zeros(10, 3), 3)
    with pytest.raises(ValueError, match="HIP device"):
        neighbors.mode_filter(torch.zeros(10, dtype=torch.int64), torch.zeros(10, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="HIP device"):
        neighbors.clean_selection(torch.zeros(10, dtype=torch.bool), torch.zeros(10, 3, dtype=torch.int32))
    assert neighbors.MAX_NEIGHBORS == 16 == neighbors._C.KNN_MAX_NEIGHBORS
