"""The judge of the component kernels (tests/components_oracle.py) judged itself, without a GPU: against scipy's connected
components on random lists, every rule of include/f3dgs.h (f3dgs_knn_components, f3dgs_component_filter) on hand-built cases, and
the argument checks of the C ABI and of neighbors.py that answer before any device work."""
import ctypes
import os

import numpy as np
import pytest

import components_oracle as co
from util import ROOT

INF = np.inf


def _random_lists(P, K, seed):
    g = np.random.default_rng(seed)
    idx = g.integers(0, P, (P, K)).astype(np.int32)
    # sparse enough for many components: most slots point nowhere
    idx[g.random((P, K)) < (0.0 if K == 1 else 0.75)] = -1
    dist2 = g.random((P, K)).astype(np.float32)
    labels = g.integers(0, 3, P)
    labels[g.random(P) < 0.1] = -1
    return idx, dist2, labels


def _scipy_parts(P, pairs):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    a = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(P, P))
    return connected_components(a, directed=False)


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("with_labels", [False, True])
def test_judge_equals_scipy(K, mutual, with_labels):
    """The edges are restated here as a loop over the slots; the partition, the roots and the sizes are scipy's."""
    P = 3000
    idx, dist2, labels = _random_lists(P, K, 100 + K)
    if mutual:                                         # make a fair share of the edges two-sided
        g = np.random.default_rng(K)
        for i in g.choice(P, P // 2, replace=False):
            j = idx[i, 0]
            if j >= 0:
                idx[j, g.integers(0, K)] = i
    lab = labels if with_labels else None
    limit = np.float32(0.8)
    active, lv = co.active_of(P, lab)
    directed = set()
    for i in range(P):
        for s in range(K):
            j = int(idx[i, s])
            if 0 <= j < P and j != i and active[i] and active[j] and lv[i] == lv[j] and dist2[i, s] <= limit:
                directed.add((i, j))
    pairs = {(min(a, b), max(a, b)) for a, b in directed if not mutual or (b, a) in directed}
    pairs = np.array(sorted(pairs), np.int64).reshape(-1, 2)
    assert len(pairs) >= 30
    assert np.array_equal(co.edges(idx, lab, dist2, limit, mutual), pairs)
    n, part = _scipy_parts(P, pairs)
    root, size, comp, comp_root, n_comp = co.components(idx, lab, dist2, limit, mutual)
    assert (root[~active] == -1).all() and (size[~active] == 0).all() and (comp[~active] == -1).all()
    assert n_comp == n - int((~active).sum()) and 1 < n_comp < active.sum()
    members = {}
    for i in np.flatnonzero(active):
        members.setdefault(part[i], []).append(i)
    for m in members.values():
        assert (root[m] == min(m)).all() and (size[m] == len(m)).all()       # equal partitions: every part one root, its minimum
    assert len({int(r) for r in root[active]}) == len(members)
    roots = np.unique(root[active])
    assert np.array_equal(comp_root[:n_comp], roots) and (comp_root[n_comp:] == -1).all()
    assert np.array_equal(comp[active], np.searchsorted(roots, root[active]))


def _roots(idx, **kw):
    return co.components(np.array(idx, np.int32), **kw)[0].tolist()


def test_rules_of_an_edge():
    assert _roots([[0], [1], [2]]) == [0, 1, 2]                                        # self edges
    assert _roots([[3], [-7], [1]]) == [0, 1, 1]                                       # out of range: P and -7; 2 -> 1 is an edge
    assert _roots([[1], [2], [0]], labels=[4, -1, 4]) == [0, -1, 0]                    # an inactive end: only 2 -> 0 is left
    assert _roots([[1], [2], [0]], labels=[4, 5, 4]) == [0, 1, 0]                      # label mismatch
    assert _roots([[1], [2], [2]]) == [0, 0, 0]                                        # either direction makes the edge
    assert _roots([[1], [2], [1]], mutual=True) == [0, 1, 1]                           # one-sided under mutual: 0 -> 1 is dropped
    root, size, comp, comp_root, n = co.components(np.array([[1], [2], [0]], np.int32), labels=[4, -1, 4])
    assert size.tolist() == [2, 0, 2] and comp.tolist() == [0, -1, 0] and comp_root.tolist() == [0, -1, -1] and n == 1


def test_rules_of_a_distance():
    idx = np.array([[1, 2], [0, 2], [0, 1]], np.int32)
    d2 = np.array([[4.0, 9.0], [4.0, 1.0], [9.0, 1.0]], np.float32)
    assert _roots(idx, dist2=d2, max_dist2=4.0) == [0, 0, 0]                           # exactly at max_dist2: an edge (<=)
    assert _roots(idx, dist2=d2, max_dist2=np.nextafter(np.float32(4), np.float32(0))) == [0, 1, 1]
    assert _roots(idx, dist2=d2, max_dist2=0.5) == [0, 1, 2]
    nan = d2.copy()
    nan[0, 0] = np.nan                                                                 # 0 -> 1 is gone, 1 -> 0 stays
    assert _roots(idx, dist2=nan, max_dist2=4.0) == [0, 0, 0]
    assert _roots(idx, dist2=nan, max_dist2=4.0, mutual=True) == [0, 1, 1]
    nan[1, 0] = np.nan
    assert _roots(idx, dist2=nan, max_dist2=4.0) == [0, 1, 1]
    one = d2.copy()
    one[1, 0] = 5.0                                                                    # each direction is judged on its own slot
    assert _roots(idx, dist2=one, max_dist2=4.0, mutual=True) == [0, 1, 1]
    assert _roots(idx, dist2=nan) == [0, 0, 0]                                         # no limit: the distances are not read


def test_rows_of_minus_one_and_empty():
    import neighbors_oracle as no
    idx, _ = no.knn(np.ones((1, 3), np.float32), 2)                                    # P <= K: a row of -1
    root, size, comp, comp_root, n = co.components(idx)
    assert (root.tolist(), size.tolist(), comp.tolist(), comp_root.tolist(), n) == ([0], [1], [0], [0], 1)
    idx, _ = no.knn(np.array([[0, 0, 0], [1, 0, 0], [9, 0, 0]], np.float32), 4)
    assert (idx[:, 2:] == -1).all() and co.components(idx)[0].tolist() == [0, 0, 0]
    root, size, comp, comp_root, n = co.components(np.zeros((0, 3), np.int32))
    assert len(root) == len(size) == len(comp) == len(comp_root) == 0 and n == 0
    assert len(co.component_filter(None, root, size)) == 0


def test_filter_rules():
    # three chains: {0, 1}, {2, 3} (a tie in size), {4}; all label 0
    idx = np.array([[1], [0], [3], [2], [4]], np.int32)
    root, size = co.components(idx)[:2]
    assert root.tolist() == [0, 0, 2, 2, 4] and size.tolist() == [2, 2, 2, 2, 1]
    assert co.component_filter(None, root, size, 1).tolist() == [0, 0, 0, 0, 0]
    assert co.component_filter(None, root, size, 2).tolist() == [0, 0, 0, 0, -1]
    assert co.component_filter(None, root, size, 3).tolist() == [-1] * 5
    assert co.component_filter(None, root, size, 1, True, 1).tolist() == [0, 0, -1, -1, -1]      # the tie: the smaller root
    assert co.component_filter(None, root, size, 3, True, 1).tolist() == [-1] * 5                # the best is too small
    labels = np.array([7, 7, 2, 2, -3])
    root, size = co.components(idx, labels)[:2]
    assert root.tolist() == [0, 0, 2, 2, -1]
    assert co.component_filter(labels, root, size, 1, True, 8).tolist() == [7, 7, 2, 2, -1]
    assert co.component_filter(labels, root, size, 1, True, 7).tolist() == [-1, -1, 2, 2, -1]    # a label >= num_labels
    assert co.component_filter(labels, root, size, 1, False, 0).tolist() == [7, 7, 2, 2, -1]     # num_labels: only with largest
    assert co.clean(np.array([1, 1, 0, 0, 1], bool), idx, 2).tolist() == [True, True, False, False, False]
    assert co.clean(np.array([1, 1, 1, 1, 1], bool), idx, 1, True).tolist() == [True, True, False, False, False]
    assert co.clean(labels, idx, 1, True, 7).tolist() == [-1, -1, 2, 2, -1]


# ---- the C ABI: what is refused before any device work ---------------------------------------------------------------------

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
    lib.f3dgs_knn_components_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_knn_components_scratch_bytes.argtypes = [ci, ci]
    lib.f3dgs_knn_components.argtypes = [ci, ci, vp, vp, cf, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.f3dgs_component_filter.argtypes = [ci, vp, vp, vp, ci, ci, ci, vp, vp, vp]
    lib.f3dgs_debug_knn_components_shape.argtypes = [ci, ci, vp, vp, cf, vp, ci, ci, vp, vp, vp, vp]
    return lib


def test_c_abi_refuses_bad_arguments_without_gpu():
    lib = _lib()
    assert lib.f3dgs_version() >= 31900
    A, B, C, D, S = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000        # aligned, never dereferenced addresses
    INV, UNS = -1, -4
    err = lib.f3dgs_last_error

    def comp(P=10, K=3, idx=A, dist2=None, max_dist2=INF, labels=None, mutual=0, root=B, size=C, comp=None, comp_root=None, n_comp=None,
             status=S, scratch=None):
        return lib.f3dgs_knn_components(P, K, idx, dist2, max_dist2, labels, mutual, root, size, comp, comp_root, n_comp, status, scratch, None)

    assert lib.f3dgs_knn_components_scratch_bytes(1 << 20, 0) >= (1 << 20) // 1024 * 4
    assert lib.f3dgs_knn_components_scratch_bytes(0, 300) >= 300 * 8
    assert lib.f3dgs_knn_components_scratch_bytes(-5, -5) == lib.f3dgs_knn_components_scratch_bytes(0, 0) > 0
    assert comp(P=-1) == INV and b"P < 0" in err()
    for K in (0, 17, -2):
        assert comp(K=K) == INV and b"1 .. 16" in err()
    assert comp(P=(1 << 30) + 1) == UNS
    for kw in (dict(idx=None), dict(root=None), dict(size=None), dict(status=None)):
        assert comp(**kw) == INV and b"null" in err(), kw
    assert comp(P=0, status=None) == INV and b"null" in err()
    assert comp(size=B) == INV and b"root is size" in err()
    assert comp(max_dist2=2.0) == INV and b"needs dist2" in err()
    for bad in (-1.0, np.nan):
        assert comp(max_dist2=bad, dist2=D) == INV and b"negative or NaN" in err()
    for kw in (dict(comp_root=None), dict(n_comp=None), dict(scratch=None)):                  # the dense outputs go together
        full = dict(comp=D, comp_root=D + 0x1000, n_comp=D + 0x2000, scratch=D + 0x3000)
        full.update(kw)
        assert comp(**full) == INV and b"null" in err(), kw
    assert comp(comp=B, comp_root=D, n_comp=D + 64, scratch=D + 128) == INV and b"of their own" in err()
    assert comp(comp=D, comp_root=D, n_comp=D + 64, scratch=D + 128) == INV and b"of their own" in err()
    assert comp(comp=D, comp_root=D + 0x1000, n_comp=D + 0x2000, scratch=D + 0x3004) == INV and b"8-byte" in err()
    assert lib.f3dgs_debug_knn_components_shape(10, 3, A, None, INF, None, 0, 3, B, C, S, None) == INV and b"shape" in err()
    assert lib.f3dgs_debug_knn_components_shape(10, 17, A, None, INF, None, 0, 1, B, C, S, None) == INV and b"1 .. 16" in err()

    def filt(P=10, labels=None, root=B, size=C, min_size=1, largest=0, num_labels=0, out=D, scratch=None):
        return lib.f3dgs_component_filter(P, labels, root, size, min_size, largest, num_labels, out, scratch, None)

    assert filt(P=0, root=None, size=None, out=None) == 0                                     # P == 0: a no-op
    assert filt(P=-1) == INV and b"P < 0" in err()
    for kw in (dict(root=None), dict(size=None), dict(out=None)):
        assert filt(**kw) == INV and b"null" in err(), kw
    assert filt(out=B) == INV and b"in place" in err()
    assert filt(out=C) == INV and b"in place" in err()
    assert filt(largest=1, num_labels=-1) == INV and b"num_labels" in err()
    assert filt(largest=1, num_labels=4) == INV and b"scratch" in err()
    assert filt(largest=1, num_labels=4, scratch=S + 4) == INV and b"8-byte" in err()


def test_python_surface_refuses_cpu_tensors():
    import torch
    import neighbors
    idx = torch.zeros(10, 3, dtype=torch.int32)
    labels = torch.zeros(10, dtype=torch.int64)
    mask = torch.zeros(10, dtype=torch.bool)
    with pytest.raises(ValueError, match="HIP device"):
        neighbors.components(idx)
    with pytest.raises(ValueError, match="HIP device"):
        neighbors.components(idx, labels=labels)
    for arg in (labels, mask):
        with pytest.raises(ValueError, match="HIP device"):
            neighbors.drop_small(arg, idx, 2)
        with pytest.raises(ValueError, match="HIP device"):
            neighbors.keep_largest(arg, idx, 4)
    with pytest.raises(ValueError, match="HIP device"):
        neighbors.split_labels(labels, idx)
    with pytest.raises(ValueError, match="min_size"):
        neighbors.drop_small(labels, idx, 0)
    assert {"components", "drop_small", "keep_largest", "split_labels"} <= set(neighbors.__all__)
    assert neighbors.Components._fields == ("root", "size", "comp", "comp_root", "n_comp", "status")
    assert neighbors.SplitLabels._fields == ("comp", "n_comp", "comp_label")
