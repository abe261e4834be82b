"""The component kernels on the GPU (csrc/components.hip; neighbors.py: components, drop_small, keep_largest, split_labels).
The judge is tests/components_oracle.py - numpy, the rules of include/f3dgs.h as array expressions - and EVERY comparison is exact:
the result is integers and a function of the inputs alone."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import components_oracle as co
import neighbors_oracle as no
from test_gpu_contrib import _Model, _camera
from test_knn import _points
from test_neighbors_cpu import lattice
from util import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def _t(a, dtype):
    return None if a is None else torch.as_tensor(np.array(a), dtype=dtype).to(DEV)      # (a copy: cached arrays are read-only)


def _want(key, make):
    """computed once per input and left unchanged"""
    if key not in _cache:
        _cache[key] = make()
        for a in _cache[key] if isinstance(_cache[key], tuple) else (_cache[key],):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _cache[key]


def _dev_knn(p, K):
    import neighbors
    idx, d2 = neighbors.knn(_t(p, torch.float32).reshape(-1, 3), K)
    return idx.cpu().numpy(), d2.cpu().numpy()


def _limit2(max_dist):
    with np.errstate(over="ignore"):
        return np.inf if max_dist is None else np.float32(max_dist) * np.float32(max_dist)


def _check(idx, what, labels=None, dist2=None, max_dist=None, mutual=False, label_dtype=torch.int64):
    """neighbors.components, dense and not, against the judge.  Returns the judge's (root, size, comp, comp_root, n_comp)."""
    import neighbors
    want = co.components(idx, labels, dist2, _limit2(max_dist), mutual)
    P = len(idx)
    args = (_t(idx, torch.int32),)
    kw = dict(labels=_t(labels, label_dtype), dist2=_t(dist2, torch.float32), max_dist=max_dist, mutual=mutual)
    res = neighbors.components(*args, dense=True, **kw)
    torch.cuda.synchronize()
    assert isinstance(res, neighbors.Components) and all(t.dtype == torch.int64 for t in res)
    assert res.n_comp.shape == () and res.status.shape == () and all(tuple(t.shape) == (P,) for t in res[:4])
    assert int(res.status) == 0, what
    assert int(res.n_comp) == want[4], f"{what}: n_comp {int(res.n_comp)}, the judge {want[4]}"
    for name, got, w in zip(res._fields, res[:4], want[:4]):
        got = got.cpu().numpy()
        assert np.array_equal(got, w), f"{what}: {name}: {int((got != w).sum())} of {P} differ"
    plain = neighbors.components(*args, **kw)
    torch.cuda.synchronize()
    assert plain.comp is None and plain.comp_root is None and plain.n_comp is None and int(plain.status) == 0
    assert torch.equal(plain.root, res.root) and torch.equal(plain.size, res.size), what
    return want


# around the wave edge (64), the block edge (256), more than one block; every list size of the link kernel (4, 8, 16)
@pytest.mark.parametrize("P", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes(P):
    g = np.random.default_rng(50 + P)
    labels = g.integers(0, 3, P)
    labels[g.random(P) < 0.1] = -1
    for K in (1, 3, 8, 16):
        idx, d2 = _dev_knn(_points(P, 11 + P, "uniform") if P else np.zeros((0, 3), np.float32), K)
        for mutual in (False, True):
            _check(idx, f"P = {P}, K = {K}, mutual = {mutual}", mutual=mutual)
            _check(idx, f"P = {P}, K = {K}, mutual = {mutual}, labels", labels=labels, mutual=mutual)
        if P:
            _check(idx, f"P = {P}, K = {K}, int32 labels, limited", labels=labels, dist2=d2, max_dist=float(np.sqrt(np.median(d2[:, 0]))),
                   label_dtype=torch.int32)


def _blobs():
    def make():
        g = np.random.default_rng(17)
        p = np.concatenate([g.normal(0, 1, (1000, 3)), g.normal(0, 1, (1000, 3)) + [40, 0, 0]]).astype(np.float32)
        order = g.permutation(2000)
        p = p[order]
        idx, d2 = no.knn(p, 8)                                    # the exact float32 lists
        return p, (order >= 1000).astype(np.int64), idx, d2
    return _want("blobs", make)


def test_two_blobs():
    """1000 points of N(0, 1) each, 40 apart, shuffled, K = 8: two components of 1000; more under mutual"""
    p, blob, idx, d2 = _blobs()
    dev_idx, _ = _dev_knn(p, 8)
    assert np.array_equal(dev_idx, idx)
    root, size, comp, comp_root, n_comp = _check(idx, "two blobs")
    assert n_comp == 2 and (size == 1000).all() and np.array_equal(comp, blob ^ blob[0])
    assert _check(idx, "two blobs, mutual", mutual=True)[4] > 2


def test_shuffled_lattice():
    """12 x 12 x 12 integer points at K = 6: every inner point's list is its six lattice neighbours at distance 1, a point of the
    surface also holds neighbours at sqrt(2).  One component.  max_dist 1.0 keeps the lattice edges (dist2 == max_dist2: <=), 0.99
    keeps none.  Under labels = (x + y + z) % 2 the lattice edges join different labels: with max_dist 1.0 every node is a
    singleton (without it the sqrt(2) edges of the surface join equal parities: the judge decides)."""
    p = lattice(12, 7)
    P = len(p)
    idx, d2 = _want("lattice lists", lambda: _dev_knn(p, 6))
    parity = p.astype(np.int64).sum(1) % 2
    assert _check(idx, "lattice")[4] == 1
    assert _check(idx, "lattice, max_dist 1.0", dist2=d2, max_dist=1.0)[4] == 1
    assert _check(idx, "lattice, max_dist 0.99", dist2=d2, max_dist=0.99)[4] == P
    assert _check(idx, "lattice, parity, max_dist 1.0", labels=parity, dist2=d2, max_dist=1.0)[4] == P
    assert 2 <= _check(idx, "lattice, parity", labels=parity)[4] < P
    _check(idx, "lattice, mutual", mutual=True)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_line_deep_walks(order):
    """4096 points on a line at K = 2: one chain, the deepest walks the union-find meets; with one gap two chains"""
    n = 4096
    pos = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "shuffled": np.random.default_rng(3).permutation(n)}[order]
    for gap in (False, True):
        x = pos.astype(np.float32) + (5.0 if gap else 0.0) * (pos >= 1500)
        idx, d2 = _dev_knn(np.stack([x, 0 * x, 0 * x], 1), 2)
        root, size, comp, comp_root, n_comp = _check(idx, f"line {order}, gap = {gap}", dist2=d2, max_dist=2.5)
        assert n_comp == (2 if gap else 1) and sorted(set(size.tolist())) == ([1500, n - 1500] if gap else [n])
        _check(idx, f"line {order}, gap = {gap}, mutual", mutual=True)


def test_contention_on_one_word():
    P = 5000
    for target in (0, P - 1):
        idx = np.full((P, 1), target, np.int32)
        root, size, _, _, n_comp = _check(idx, f"every node links to {target}")
        assert n_comp == 1 and (root == 0).all() and (size == P).all()
    p = np.repeat(_points(300, 5), 4, axis=0)                     # every point four times: distance 0, ties by index
    for K in (3, 5):
        idx, d2 = _dev_knn(p, K)
        n_comp = _check(idx, f"duplicates, K = {K}")[4]
        assert n_comp == 300 if K == 3 else n_comp < 300
        assert _check(idx, f"duplicates, K = {K}, max_dist 0", dist2=d2, max_dist=0.0, mutual=True)[4] == 300


def _lists():
    def make():
        p = _points(2000, 13, "clustered")
        idx, d2 = _dev_knn(p, 8)
        return p, idx, d2
    return _want("filter lists", make)


def test_corrupted_lists():
    _, idx, d2 = _lists()
    g = np.random.default_rng(4)
    P = len(idx)
    bad = idx.copy()
    bad[g.random(bad.shape) < 0.2] = -7
    bad[g.random(bad.shape) < 0.2] = P
    own = g.random(bad.shape) < 0.2
    bad[own] = np.repeat(np.arange(P), 8).reshape(P, 8)[own]
    bad[g.random(P) < 0.1] = -1                                   # rows of -1
    bad[0], bad[-1] = P, -7
    bad[1, 0] = 2**31 - 1
    bad[2, 0] = -2**31
    labels = g.integers(-1, 4, P)
    for mutual in (False, True):
        assert _check(bad, f"idx with -7, P and own, mutual = {mutual}", mutual=mutual)[4] > 1
        _check(bad, f"idx with -7, P and own, labels, limited, mutual = {mutual}", labels=labels, dist2=d2, max_dist=0.3, mutual=mutual)
    nan = d2.copy()
    nan[g.random(nan.shape) < 0.3] = np.nan
    _check(idx, "NaN distances", dist2=nan, max_dist=1e9)
    _check(np.full((P, 3), -1, np.int32), "rows of -1 only")


def test_link_shapes_agree():
    """f3dgs_debug_knn_components_shape: the link stage as one thread per node (0) and per (node, slot) (1): the judge's root and
    size from both; 2 (no link): every active node a component of its own."""
    torch.zeros(1, device=DEV)
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.f3dgs_debug_knn_components_shape.argtypes = [ci, ci, vp, vp, ctypes.c_float, vp, ci, ci, vp, vp, vp, vp]
    _, idx8, d2 = _lists()
    g = np.random.default_rng(8)
    P = len(idx8)
    labels = g.integers(-1, 3, P)
    for K in (3, 8):
        idx = np.ascontiguousarray(idx8[:, :K])
        dist2 = np.ascontiguousarray(d2[:, :K])
        for mutual in (0, 1):
            want = co.components(idx, labels, dist2, np.float32(0.09), bool(mutual))
            t_idx, t_d2, t_lab = _t(idx, torch.int32), _t(dist2, torch.float32), _t(labels, torch.int32)
            for shape in (0, 1, 2):
                root, size = torch.full((P,), -9, device=DEV, dtype=torch.int32), torch.full((P,), -9, device=DEV, dtype=torch.int32)
                status = torch.full((), -9, device=DEV, dtype=torch.int32)
                rc = lib.f3dgs_debug_knn_components_shape(P, K, t_idx.data_ptr(), t_d2.data_ptr(), 0.09, t_lab.data_ptr(), mutual, shape,
                                                          root.data_ptr(), size.data_ptr(), status.data_ptr(),
                                                          torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert rc == 0 and int(status) == 0
                if shape == 2:
                    assert np.array_equal(root.cpu().numpy(), np.where(labels >= 0, np.arange(P), -1))
                    assert np.array_equal(size.cpu().numpy(), (labels >= 0).astype(np.int32))
                else:
                    assert np.array_equal(root.cpu().numpy(), want[0]) and np.array_equal(size.cpu().numpy(), want[1]), (K, mutual, shape)


# ---- the filter --------------------------------------------------------------------------------------------------------------

def _check_clean(labels_or_mask, idx, what, min_size=1, largest=False, num_labels=None, dtype=torch.int64, **kw):
    import neighbors
    a = np.asarray(labels_or_mask)
    want = co.clean(a, idx, min_size, largest, num_labels or 0, kw.get("dist2"), _limit2(kw.get("max_dist")), kw.get("mutual", False))
    arg = _t(a, torch.bool if a.dtype == bool else dtype)
    before = arg.clone()
    dkw = dict(dist2=_t(kw.get("dist2"), torch.float32), max_dist=kw.get("max_dist"), mutual=kw.get("mutual", False))
    if largest:
        got = neighbors.keep_largest(arg, _t(idx, torch.int32), num_labels=num_labels, min_size=min_size, **dkw)
    else:
        got = neighbors.drop_small(arg, _t(idx, torch.int32), min_size, **dkw)
    torch.cuda.synchronize()
    assert got.dtype == (torch.bool if a.dtype == bool else torch.int64) and torch.equal(arg, before), what
    got = got.cpu().numpy()
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} differ"
    return got


def test_filter_equals_the_judge():
    _, idx, d2 = _lists()
    g = np.random.default_rng(9)
    P = len(idx)
    labels = g.integers(0, 6, P)
    labels[g.random(P) < 0.1] = -1
    mask = g.random(P) < 0.4
    sparse = idx[:, :2].copy()                                    # many small components
    for min_size in (1, 2, 5):
        got = _check_clean(labels, sparse, f"labels, min_size {min_size}", min_size, max_dist=0.05, dist2=d2[:, :2].copy())
        assert min_size == 1 or 0 < (got != np.maximum(labels, -1)).sum() < P
        _check_clean(labels, sparse, f"int32 labels, min_size {min_size}", min_size, dtype=torch.int32)
        _check_clean(mask, sparse, f"mask, min_size {min_size}", min_size)
        _check_clean(labels, sparse, f"labels, largest, min_size {min_size}", min_size, True, 6, mutual=True)
        _check_clean(mask, idx, f"mask, largest, min_size {min_size}", min_size, True)
    got = _check_clean(labels, idx, "largest, one label beyond num_labels", 1, True, 5)
    assert (got[labels == 5] == -1).all() and (got >= 0).any()
    assert (_check_clean(labels, idx, "largest, num_labels 0", 1, True, 0) == -1).all()
    big = np.where(labels >= 0, 2**31 - 1 - labels, -1)           # labels up to 2^31 - 1: beyond any table
    assert (_check_clean(big, idx, "large labels, largest", 1, True, 1000) == -1).all()
    _check_clean(big, sparse, "large labels, min_size 2", 2)


def test_filter_two_equal_blobs_and_aliasing():
    """two components of 1000 under one label: the one that holds the lower root (node 0) stays"""
    import neighbors
    from simple_knn import _C
    _, blob, idx, _ = _blobs()
    keep = _check_clean(np.ones(2000, bool), idx, "two equal blobs, mask", 1, True)
    assert np.array_equal(keep, blob == blob[0])
    got = _check_clean(np.full(2000, 3), idx, "two equal blobs, labels", 1, True, 4)
    assert np.array_equal(got, np.where(blob == blob[0], 3, -1))
    assert not _check_clean(np.ones(2000, bool), idx, "two equal blobs, min_size 1001", 1001, True).any()
    # the binding itself: a separate output and labels_out aliasing labels give the same labels; NULL labels are label 0
    labels = _t(np.where(blob == 1, 2, 0), torch.int32)
    res = neighbors.components(_t(idx, torch.int32), labels=labels)
    root, size = res.root.int(), res.size.int()
    out = torch.full_like(labels, -9)
    _C.component_filter(labels, root, size, 1, True, 2, out)
    alias = labels.clone()
    _C.component_filter(alias, root, size, 1, True, 2, alias)
    torch.cuda.synchronize()
    assert torch.equal(out, alias) and np.array_equal(out.cpu().numpy(), np.where(blob == 1, -1, 0))
    res = neighbors.components(_t(idx, torch.int32))
    _C.component_filter(None, res.root.int(), res.size.int(), 1, True, 1, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.where(blob == blob[0], 0, -1))


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def test_lifter_end_to_end():
    """One 64 x 64 view of a synth scene through LabelLifter; drop_small and keep_largest against the judge applied to the
    lifter's own labels() / select() read back."""
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
    idx, d2 = neighbors.knn(pc.get_xyz, 4)
    labels = lifter.labels()
    lab, lists, dist2 = labels.cpu().numpy(), idx.cpu().numpy(), d2.cpu().numpy()
    assert 0.2 < (lab >= 0).mean() and len(np.unique(lab[lab >= 0])) >= 3
    got = neighbors.drop_small(labels, idx, 5)
    want = co.clean(lab, lists, 5)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want) and 0 < (want != lab).sum() < (lab >= 0).sum()
    got = neighbors.keep_largest(labels, idx, num_labels=L, dist2=d2, max_dist=0.4)
    want = co.clean(lab, lists, 1, True, L, dist2, _limit2(0.4))
    assert np.array_equal(got.cpu().numpy(), want) and (want != lab).any() and len(np.unique(want[want >= 0])) >= 3
    for cls in (0, 4):
        mask = lifter.select(cls, threshold=0.5)
        m = mask.cpu().numpy()
        got = neighbors.keep_largest(mask, idx)
        want = co.clean(m, lists, 1, True)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want) and 0 < want.sum() < m.sum()
        got = neighbors.drop_small(mask, idx, 3, mutual=True)
        assert np.array_equal(got.cpu().numpy(), co.clean(m, lists, 3, mutual=True))


def test_split_labels_gives_two_far_slabs_two_ids():
    """an instance field in which two far slabs carry ONE id (two chairs that shared a mask), a third slab another, some
    Gaussians none: split_labels gives every body an id of its own and tells which id it came from"""
    import neighbors
    g = np.random.default_rng(12)
    slab = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    n = len(slab)
    p = np.concatenate([slab, slab + [30, 0, 0], slab + [60, 0, 0]])
    ids = np.repeat([5, 2, 5], n)
    body = np.repeat([0, 1, 2], n)
    ids[[7, n + 9]] = -1                                          # (corners of the slabs: nothing falls apart)
    order = g.permutation(3 * n)
    p, ids, body = p[order], ids[order], body[order]
    idx, _ = neighbors.knn(_t(p, torch.float32), 6)
    res = neighbors.split_labels(_t(ids, torch.int64), idx)
    torch.cuda.synchronize()
    assert isinstance(res, neighbors.SplitLabels) and all(t.dtype == torch.int64 for t in res)
    comp, n_comp, comp_label = res.comp.cpu().numpy(), int(res.n_comp), res.comp_label.cpu().numpy()
    want = co.components(idx.cpu().numpy(), ids)
    assert n_comp == want[4] == 3 and np.array_equal(comp, want[2])
    assert np.array_equal(comp_label, np.where(want[3] >= 0, ids[np.maximum(want[3], 0)], -1))
    assert sorted(comp_label[:3].tolist()) == [2, 5, 5] and (comp_label[3:] == -1).all()
    for b in range(3):                                            # one new id per body
        assert len(set(comp[(body == b) & (ids >= 0)].tolist())) == 1
    assert len(set(comp[ids == 5].tolist())) == 2 and (comp[ids < 0] == -1).all()
    empty = neighbors.split_labels(torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV))
    assert int(empty.n_comp) == 0 and empty.comp.shape == (0,) and empty.comp_label.shape == (0,)


def test_errors():
    import neighbors
    from simple_knn import _C
    idx = torch.zeros(10, 3, device=DEV, dtype=torch.int32)
    labels = torch.zeros(10, device=DEV, dtype=torch.int64)
    mask = torch.zeros(10, device=DEV, dtype=torch.bool)
    d2 = torch.ones(10, 3, device=DEV)
    for args, kw in (((idx.cpu(),), {}), ((idx.long(),), {}), ((idx[0],), {}), ((torch.zeros(10, 17, device=DEV, dtype=torch.int32),), {}),
                     ((idx,), dict(labels=labels.cpu())), ((idx,), dict(labels=labels.float())), ((idx,), dict(labels=labels[:9])),
                     ((idx,), dict(dist2=d2[:, :2])), ((idx,), dict(dist2=d2.double())), ((idx,), dict(max_dist=1.0)),
                     ((idx,), dict(max_dist=-1.0, dist2=d2))):
        with pytest.raises(ValueError, match="expected|HIP device|needs dist2"):
            neighbors.components(*args, **kw)
    with pytest.raises(ValueError, match=r"torch.float32 \(10,\) on cuda:0"):      # dtype, shape and device are named
        neighbors.drop_small(labels.float(), idx, 2)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="min_size"):
            neighbors.drop_small(labels, idx, bad)
    with pytest.raises(ValueError, match="num_labels"):
        neighbors.keep_largest(labels, idx)
    with pytest.raises(ValueError, match="num_labels"):
        neighbors.keep_largest(labels, idx, num_labels=-1)
    with pytest.raises(ValueError):
        neighbors.keep_largest(mask, idx[:9])
    with pytest.raises(ValueError):
        neighbors.split_labels(mask, idx)
    with pytest.raises(Exception, match="1 .. 16"):
        _C.knn_components(torch.zeros(10, 17, device=DEV, dtype=torch.int32), None, float("inf"), None, False, False)
    l32 = labels.int()
    with pytest.raises(Exception, match="in place"):
        _C.component_filter(l32, l32, torch.ones_like(l32), 1, False, 0, l32)


def test_capture_and_replay():
    """components(dense=True) and keep_largest captured as one linear graph on one stream, replayed on new lists behind the same
    pointers: the eager results.  Nothing is allocated by the test inside the capture."""
    import neighbors
    g = np.random.default_rng(6)
    lists = [_dev_knn(_points(3000, 31, "clustered"), 8), _dev_knn(_points(3000, 32, "uniform"), 8)]
    idx, d2 = _t(lists[0][0], torch.int32), _t(lists[0][1], torch.float32)
    labels = _t(g.integers(-1, 5, 3000), torch.int64)

    def run():
        res = neighbors.components(idx, labels=labels, dist2=d2, max_dist=0.08, dense=True)
        return tuple(res) + (neighbors.keep_largest(labels, idx, num_labels=5, dist2=d2, max_dist=0.08),)

    def load(which):
        idx.copy_(torch.from_numpy(lists[which][0]).to(DEV))
        d2.copy_(torch.from_numpy(lists[which][1]).to(DEV))

    want = {}
    for which in (0, 1):
        load(which)
        want[which] = [t.clone() for t in run()]
        torch.cuda.synchronize()
        assert int(want[which][5]) == 0 and int(want[which][4]) > 5
    assert not torch.equal(want[0][0], want[1][0])
    load(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # one stream, no parallel branches
        captured = run()
    for which in (0, 1, 0):
        load(which)
        for t in captured:
            t.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, want[which]):
            assert torch.equal(a, b)
