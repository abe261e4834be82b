"""The segmentation scores and palette pictures on the GPU (feature-3dgs_amd/seg_metrics.py, csrc/seg_metrics.hip) against the
numpy oracle (tests/seg_metrics_oracle.py, itself held to the reference's own code on the CPU), the reference's fixture values
and segment.label_agreement.

Bars.  Every counter: integer equality.  accuracy, accuracy_masked: bit for bit (one fp64 division of exact integers).  iou,
iou_masked: 1e-10 absolute with NaN where the oracle has NaN - at most 256 terms in [0, 1] summed in fp64 in another order differ
by less than 256 * 256 * 2^-53 = 7e-12.  Pictures: byte for byte.

Launch shape of the count kernel: a workgroup stages 1024 pixels at a time and a view is shared by at most 32 workgroups, so a
view of more than 32 x 1024 pixels makes a workgroup take a second tile."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

import seg_metrics_oracle as O
from util import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_seg_metrics.npz")
DEV = "cuda:0"
IOU_TOL = 1e-10
DTYPES = (torch.uint8, torch.int32, torch.int64)
CASES = ("big", "seven", "few", "same", "nomatch", "gtonly")


def _maps(N, HW, L, seed, shape=None):
    """(teacher, student, gt) int64 numpy (N,) + shape: piecewise-constant teacher (runs of one label, as a segmentation has
    them) over a skewed label distribution, student and gt with a share of pixels redrawn; labels 0 and L - 1 present."""
    rng = np.random.default_rng(seed)
    p = rng.dirichlet(np.full(L, 0.3))
    runs = rng.choice(L, size=(N, HW), p=p)
    hold = rng.random((N, HW)) < 0.8                       # keep the previous pixel's label: runs of mean length 5
    start = np.where(hold, 0, np.arange(HW)[None])          # index of the pixel whose draw a pixel shows
    start[:, 0] = 0
    t = np.take_along_axis(runs, np.maximum.accumulate(start, axis=1), axis=1)

    def redraw(share):
        out = t.copy()
        w = rng.random(t.shape) < share
        out[w] = rng.choice(L, size=int(w.sum()), p=p)
        return out

    s, g = redraw(0.3), redraw(0.25)
    for m in (t, s, g):
        m[:, 0] = 0
        m[:, -1] = L - 1
    shape = shape or (1, HW)
    return tuple(m.reshape((N,) + tuple(shape)).astype(np.int64) for m in (t, s, g))


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _close(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= IOU_TOL


def _check_row(got, want, has_gt, where):
    """got: a SegScores / SegPooled row already on the host as Python values; want: the oracle's dict"""
    assert _same(got["accuracy"], want["accuracy"]), (where, got["accuracy"], want["accuracy"])
    assert _close(got["iou"], want["iou"]), (where, got["iou"], want["iou"])
    assert got["invalid"] == want["invalid"], where
    assert got["labels_ranked"] == want["labels_ranked"].tolist(), where
    assert np.allclose(got["iou_per_label"], want["iou_per_label"], rtol=0, atol=0, equal_nan=True), where
    if has_gt:
        assert _same(got["accuracy_masked"], want["accuracy_masked"]), where
        assert _close(got["iou_masked"], want["iou_masked"]), (where, got["iou_masked"], want["iou_masked"])
        assert got["labels_ranked_masked"] == want["labels_ranked_masked"].tolist(), where
        assert np.allclose(got["iou_per_label_masked"], want["iou_per_label_masked"], rtol=0, atol=0, equal_nan=True), where
    else:
        assert got["accuracy_masked"] is None and got["iou_masked"] is None


SCORE_FIELDS = ("accuracy", "iou", "accuracy_masked", "iou_masked", "invalid", "iou_per_label", "labels_ranked",
                "iou_per_label_masked", "labels_ranked_masked")


def _host_rows(sc, N):
    cpu = {k: (getattr(sc, k).cpu() if getattr(sc, k) is not None else None) for k in SCORE_FIELDS}
    rows = [{k: (v[n].tolist() if v is not None else None) for k, v in cpu.items()} for n in range(N)]
    pooled = {k: (getattr(sc.pooled, k).cpu().tolist() if getattr(sc.pooled, k) is not None else None) for k in SCORE_FIELDS}
    return rows, pooled


def _check(t, s, g, L, nc, dt=(torch.int64, torch.int64, torch.int64), device_maps=None, where=""):
    """Counts and scores of (N,...) numpy maps against the oracle.  device_maps: the tensors to pass instead of fresh copies."""
    from seg_metrics import segmentation_counts, segmentation_scores
    N = t.shape[0]
    tv, sv, gv = device_maps or (_dev(t, dt[0]), _dev(s, dt[1]), None if g is None else _dev(g, dt[2]))
    want_rows, want_pooled, want_counts = O.scores(t, s, g, L, nc)
    c = segmentation_counts(tv, sv, gv, num_labels=L)
    for name in O.COUNT_NAMES + O.SCALAR_NAMES:
        got = getattr(c, name)
        if g is None and name in ("n_g", "m_g", "m_s", "m_gs", "matched", "correct"):
            assert got is None
            continue
        assert got.dtype == torch.int64 and got.shape == ((N, L) if name in O.COUNT_NAMES else (N,))
        want = np.stack([np.asarray(wc[name]) for wc in want_counts])
        assert np.array_equal(got.cpu().numpy(), want), (where, name)
    sc = segmentation_scores(tv, sv, gv, num_labels=L, num_classes=nc)
    assert sc.accuracy.dtype == torch.float64 and tuple(sc.labels_ranked.shape) == (N, nc) and tuple(sc.iou_per_label.shape) == (N, L)
    rows, pooled = _host_rows(sc, N)
    for n in range(N):
        _check_row(rows[n], want_rows[n], g is not None, (where, n))
    _check_row(pooled, want_pooled, g is not None, (where, "pooled"))
    return sc


# ---- the reference itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_recorded_cases_match_the_reference(name):
    import seg_metrics as M
    z = np.load(GOLDEN)
    t, s, g, L = z[f"{name}/teacher"], z[f"{name}/student"], z[f"{name}/gt"], int(z[f"{name}/L"])
    for nc in z[f"{name}/num_classes"].tolist():
        want = {k: float(z[f"{name}/{k}"]) for k in ("accuracy", "accuracy_masked")}
        want["iou"], want["iou_masked"] = float(z[f"{name}/iou_{nc}"]), float(z[f"{name}/iou_masked_{nc}"])
        sc = M.segmentation_scores(_dev(t, torch.uint8), _dev(s, torch.uint8), _dev(g, torch.uint8), num_labels=L, num_classes=nc)
        for k, same in (("accuracy", _same), ("accuracy_masked", _same), ("iou", _close), ("iou_masked", _close)):
            assert same(float(getattr(sc, k)[0]), want[k]), (k, float(getattr(sc, k)[0]), want[k])
            assert same(float(getattr(sc.pooled, k)), want[k]), ("pooled", k)
        assert int(sc.invalid[0]) == 0
        # the four drop-ins, fed as the reference's script feeds them: (1,H,W) int64 numpy; and device tensors
        t64, s64, g64 = (m.astype(np.int64)[None] for m in (t, s, g))
        assert _same(M.calculate_accuracy(t64, s64), want["accuracy"])
        assert _same(M.calculate_accuracy_mask(g64, t64, s64, 0), want["accuracy_masked"])
        assert _close(M.calculate_iou(t64, s64, nc), want["iou"])
        assert _close(M.calculate_iou_mask(g64, t64, s64, nc), want["iou_masked"])
        assert _close(M.calculate_iou(_dev(t, torch.int32), _dev(s, torch.uint8), nc), want["iou"])
        assert _close(M.calculate_iou_mask(_dev(g), _dev(t, torch.int16), _dev(s), nc), want["iou_masked"])
    _check(t[None].astype(np.int64), s[None].astype(np.int64), g[None].astype(np.int64), L, nc, where=name)


# ---- launch shape ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 32 * 1024 - 1, 32 * 1024, 32 * 1024 + 1])
def test_pixel_counts_at_every_edge_of_the_launch_shape(HW):
    t, s, g = _maps(1, HW, 9, seed=HW)
    _check(t, s, g, 9, 4, where=HW)
    _check(t, s, None, 9, 4, where=HW)


def test_three_views_that_start_inside_a_tile_and_a_vector():
    t, s, g = _maps(3, 257, 9, seed=3)
    _check(t, s, g, 9, 4)
    _check(t, s, g, 9, 4, dt=(torch.uint8, torch.int32, torch.uint8))


def test_a_view_of_360_by_480():
    t, s, g = _maps(1, 360 * 480, 150, seed=11, shape=(360, 480))
    _check(t, s, g, 150, 7)


@pytest.mark.parametrize("L", [1, 2, 255, 256])
def test_label_range(L):
    t, s, g = _maps(2, 700, L, seed=L)
    for m in (t, s, g):
        assert m.min() == 0 and m.max() == L - 1
    for nc in {1, L}:
        _check(t, s, g, L, nc, where=(L, nc))
    if L > 200:
        _check(t, s, g, L, L, dt=(torch.uint8, torch.uint8, torch.int32), where=L)


# ---- types and alignment ------------------------------------------------------------------------------------------------------
def test_every_type_pair_and_gt_in_each_type():
    t, s, g = _maps(2, 37 * 53, 21, seed=5, shape=(37, 53))
    for dt_t, dt_s in itertools.product(DTYPES, DTYPES):
        _check(t, s, None, 21, 7, dt=(dt_t, dt_s, None), where=(dt_t, dt_s))
    for dt_g in DTYPES:
        _check(t, s, g, 21, 7, dt=(torch.int64, torch.uint8, dt_g), where=dt_g)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_maps_at_an_odd_storage_offset(dtype, offset):
    """A map sliced out of a longer buffer starts `offset` elements behind an aligned address: head and tail of every tile and of
    the whole block are read element by element.  The buffer ends with the map, so a vector load past the end would leave it."""
    N, H, W = 2, 13, 41
    t, s, g = _maps(N, H * W, 17, seed=offset, shape=(H, W))

    def sliced(a, off):
        buf = torch.full((off + a.size,), 99, dtype=dtype, device=DEV)
        buf[off:] = _dev(a.reshape(-1), dtype)
        v = buf[off:].view(N, H, W)
        assert v.data_ptr() % (4 * v.element_size()) == off * v.element_size() % (4 * v.element_size())
        return v

    _check(t, s, g, 17, 7, device_maps=(sliced(t, offset), sliced(s, (offset + 1) % 4), sliced(g, offset)), where=(dtype, offset))


# ---- counter width and contention -----------------------------------------------------------------------------------------------
def test_one_label_everywhere_and_a_view_of_two_labels():
    from seg_metrics import segmentation_counts
    one = np.full((1, 300, 300), 5, np.int64)
    _check(one, one, one, 8, 3)
    c = segmentation_counts(_dev(one), _dev(one), _dev(one), num_labels=8)
    for name in O.COUNT_NAMES:                      # 90 000 > 2^16: a packed 16-bit counter would show
        assert int(getattr(c, name)[0, 5]) == 90000 and int(getattr(c, name).sum()) == 90000
    for name in ("valid", "equal", "matched", "correct"):
        assert int(getattr(c, name)[0]) == 90000
    two = one.copy()
    two[:, 150:] = 2
    other = one.copy()
    other[:, :, 100:] = 2
    _check(two, other, two, 8, 3)


# ---- invalid labels -----------------------------------------------------------------------------------------------------------
def test_invalid_labels_are_counted_and_left_out():
    import seg_metrics as M
    L = 200
    t, s, g = _maps(2, 3000, L, seed=21)
    rng = np.random.default_rng(1)
    bad = [L, 255, -1, 1 << 40, -(1 << 40), (1 << 32) + 3, (1 << 63) - 1]
    for m in (t, s, g):
        idx = rng.choice(m.size, size=40, replace=False)
        m.reshape(-1)[idx] = rng.choice(bad, size=40)
    want = [O.counts(t[n], s[n], g[n], L)["invalid"] for n in range(2)]
    assert min(want) > 40
    sc = _check(t, s, g, L, 7)
    assert sc.invalid.tolist() == want
    _check(t, s, None, L, 7)
    # narrower types hold the values that fit them: 255 and L as uint8, -1 as int32
    t8, s32 = np.clip(t, 0, 255), np.clip(s, -1, 255)
    _check(t8, s32, None, L, 7, dt=(torch.uint8, torch.int32, None))
    with pytest.raises(ValueError, match=rf"view 0: {want[0]} pixels with a label outside \[0, {L}\)"):
        M.evaluate_segmentation([_dev(t[0]), _dev(t[1])], [_dev(s[0]), _dev(s[1])], [_dev(g[0]), _dev(g[1])], num_labels=L)


# ---- ties ---------------------------------------------------------------------------------------------------------------------
def test_tie_across_the_cut_keeps_the_lower_label():
    from seg_metrics import segmentation_scores
    from segment import label_agreement
    # labels 4 and 6 both count 40 at ranks 2 and 3 (num_classes = 2); 6 agrees fully, 4 half: the choice decides the mean
    t = np.array([1] * 50 + [6] * 20 + [4] * 20 + [0] * 10, np.int64).reshape(1, 10, 10)
    s = np.array([1] * 50 + [6] * 20 + [4] * 10 + [0] * 10 + [4] * 10, np.int64).reshape(1, 10, 10)
    sc = _check(t, s, t, 8, 2)
    assert sc.labels_ranked[0].tolist() == [1, 4]
    acc, iou = label_agreement(_dev(t[0]), _dev(s[0]), 2)
    assert _same(float(sc.accuracy[0]), acc) and _close(float(sc.iou[0]), iou)
    assert not _close(iou, 1.0)                      # (keeping label 6 instead would give 1)
    assert segmentation_scores(_dev(t), _dev(s), num_labels=8, num_classes=3).labels_ranked[0].tolist() == [1, 4, 6]


def test_drop_ins_agree_with_label_agreement_on_tie_free_maps():
    """calculate_accuracy and calculate_iou against label_agreement's two floats: accuracy bit for bit, IoU within 1e-10.
    label_agreement is given the maps on the host: there torch's `mean` divides the sum by the count, the reference's own
    equal / total.  On the device torch forms the mean as sum * (1 / count), two roundings: for the first of these maps that is
    0.7511473737888833 where 1473 / 1961 = 0.7511473737888832 (the reference's value, and the kernel's), so against the
    device route the accuracy is held to those two roundings, 2^-52 absolute for a value below 1."""
    import seg_metrics as M
    from segment import label_agreement
    done = 0
    for seed in range(40):
        t, s, _ = _maps(1, 37 * 53, 30, seed=100 + seed, shape=(37, 53))
        counts = np.sort(np.bincount(np.concatenate((t.reshape(-1), s.reshape(-1)))))[::-1]
        if counts[6] == counts[7] or len(set(counts[:8].tolist())) < 8:
            continue                                 # a tie at or inside the cut: not this test's subject
        tv, sv = _dev(t[0]), _dev(s[0])
        got_acc, got_iou = M.calculate_accuracy(tv, sv), M.calculate_iou(tv, sv, 7)
        acc, iou = label_agreement(torch.from_numpy(t[0]), torch.from_numpy(s[0]), 7)
        assert _same(got_acc, acc) and _close(got_iou, iou), (got_acc, acc, got_iou, iou)
        acc_dev, iou_dev = label_agreement(tv, sv, 7)
        assert abs(got_acc - acc_dev) <= 2.0 ** -52 and _close(got_iou, iou_dev), (got_acc, acc_dev, got_iou, iou_dev)
        done += 1
        if done == 3:
            break
    assert done == 3


# ---- pooling, evaluate_segmentation -------------------------------------------------------------------------------------------
def test_pooled_row_sums_counters_not_scores():
    t, s, g = _maps(5, 1500, 12, seed=9)
    s[3] = np.where(np.arange(1500) % 3 == 0, s[3], (s[3] + 1) % 12)          # views of different quality
    sc = _check(t, s, g, 12, 5)                      # (the pooled row against the oracle run on the summed counters)
    mean_of_views = float(sc.iou.mean())
    assert abs(float(sc.pooled.iou) - mean_of_views) > 1e-6


@pytest.mark.parametrize("with_gt", [False, True])
def test_chained_calls_pool_as_one_call_on_all_views(with_gt):
    """`carry`: the pooled row of a call that is handed the pooled counters of the calls before it equals, bit for bit, the pooled
    row of one call on all views - and the oracle's; the per-view rows are the call's own views."""
    from seg_metrics import segmentation_scores
    L, nc = 25, 6
    t, s, g = _maps(5, 900, L, seed=77)
    if not with_gt:
        g = None
    kw = dict(num_labels=L, num_classes=nc)
    dev = lambda m, sl: None if m is None else _dev(m[sl])
    whole = segmentation_scores(_dev(t), _dev(s), dev(g, slice(None)), **kw)
    first = segmentation_scores(_dev(t[:2]), _dev(s[:2]), dev(g, slice(0, 2)), **kw)
    second = segmentation_scores(_dev(t[2:3], torch.uint8), _dev(s[2:3], torch.int32), dev(g, slice(2, 3)),
                                 carry=(first.pooled.counts, first.pooled.scalars), **kw)
    third = segmentation_scores(_dev(t[3:]), _dev(s[3:]), dev(g, slice(3, 5)), carry=(second.pooled.counts, second.pooled.scalars), **kw)
    for k in SCORE_FIELDS + ("counts", "scalars"):
        a, b = getattr(third.pooled, k), getattr(whole.pooled, k)
        if a is None:
            assert b is None and not with_gt
            continue
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b), k
    assert not torch.equal(first.pooled.counts, whole.pooled.counts)
    assert torch.equal(third.accuracy.view(torch.int64), whole.accuracy[3:].view(torch.int64)) and torch.equal(third.invalid, whole.invalid[3:])
    _, want_pooled, want_counts = O.scores(t, s, g, L, nc)
    _check_row(_host_rows(third, 2)[1], want_pooled, with_gt, "chained")
    names = O.COUNT_NAMES[:7 if with_gt else 3]
    assert np.array_equal(third.pooled.counts.cpu().numpy(), np.stack([O.pool(want_counts)[n] for n in names]))


def test_counts_alone_skip_the_scores_and_still_pool():
    """segmentation_counts hands the library no score outputs (include/f3dgs.h: all three NULL): the finish kernel then only sums
    the views' counters into the pooled row."""
    from diff_gaussian_rasterization import _C
    L = 11
    t, s, g = _maps(3, 1300, L, seed=31)
    for gv in (_dev(g, torch.uint8), torch.Tensor([])):
        e = torch.Tensor([])          # (no carry)
        counts, scalars, scores, per_label, ranked = _C.seg_metrics(_dev(t), _dev(s, torch.int32), gv, L, 1, e, e, False)
        assert scores.numel() == 0 and per_label.numel() == 0 and ranked.numel() == 0
        want = [O.counts(t[n], s[n], g[n] if gv.numel() else None, L) for n in range(3)]
        names = O.COUNT_NAMES[:7 if gv.numel() else 3]
        assert tuple(counts.shape) == (len(names), 4, L) and tuple(scalars.shape) == (5, 4)
        for a, name in enumerate(names):
            assert np.array_equal(counts[a, :3].cpu().numpy(), np.stack([w[name] for w in want])), name
            assert np.array_equal(counts[a, 3].cpu().numpy(), O.pool(want)[name]), ("pooled", name)
        for a, name in enumerate(O.SCALAR_NAMES):
            got = scalars[a].tolist()
            assert got[:3] == [w.get(name, 0) for w in want] and got[3] == sum(w.get(name, 0) for w in want), name


def test_evaluate_segmentation_with_views_of_mixed_sizes_and_types():
    import seg_metrics as M
    L, nc = 40, 7
    specs = [((20, 30), torch.int64), ((20, 30), torch.int64), ((17, 23), torch.int64), ((20, 30), torch.uint8), ((20, 30), torch.uint8),
             ((20, 30), torch.int32), ((1, 5), torch.int64)]
    T, S, G = [], [], []
    for i, (shape, _) in enumerate(specs):
        t, s, g = _maps(1, shape[0] * shape[1], L, seed=50 + i, shape=shape)
        T.append(t[0]); S.append(s[0]); G.append(g[0])
    for gts in (G, None):
        rep = M.evaluate_segmentation([_dev(a, dt) for a, (_, dt) in zip(T, specs)], [_dev(a, torch.int64) for a in S],
                                      None if gts is None else [_dev(a, dt) for a, (_, dt) in zip(gts, specs)], num_labels=L, num_classes=nc)
        names = ("accuracy", "iou") + (("accuracy_masked", "iou_masked") if gts else ())
        assert set(rep) == set(names) | {"per_view", "pooled"}
        want = [O.finish(O.counts(T[i], S[i], None if gts is None else gts[i], L), nc) for i in range(len(T))]
        pooled = O.finish(O.pool([O.counts(T[i], S[i], None if gts is None else gts[i], L) for i in range(len(T))]), nc)
        for k in names:
            same = _same if k.startswith("accuracy") else _close
            assert len(rep["per_view"][k]) == len(T)
            for i in range(len(T)):
                assert same(rep["per_view"][k][i], want[i][k]), (k, i)
            accum = 0.0
            for v in rep["per_view"][k]:
                accum += v
            assert _same(rep[k], accum / len(T))          # a running sum divided by the count, in Python floats
            assert same(rep["pooled"][k], pooled[k]), ("pooled", k)


# ---- determinism and capture ----------------------------------------------------------------------------------------------------
def _bits(sc):
    out = []
    for k in SCORE_FIELDS:
        for row in (sc, sc.pooled):
            v = getattr(row, k)
            out.append(v.clone().view(torch.int64) if v.dtype == torch.float64 else v.clone())
    out += [sc.pooled.counts.clone(), sc.pooled.scalars.clone()]
    return out


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_two_calls_and_a_graph_replay_give_the_same_bits():
    from seg_metrics import segmentation_scores
    t, s, g = _maps(3, 37 * 131, 30, seed=8, shape=(37, 131))
    tv, sv, gv = _dev(t), _dev(s, torch.int32), _dev(g, torch.uint8)
    kw = dict(num_labels=30, num_classes=7)
    a = _bits(segmentation_scores(tv, sv, gv, **kw))
    assert _same_bits(a, _bits(segmentation_scores(tv, sv, gv, **kw)))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # one stream, no parallel branches
        c = segmentation_scores(tv, sv, gv, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(_bits(c), a)
    for step in (1, 2):                                     # new content behind the same pointers: the counters start from zero
        sv.copy_(torch.roll(sv, shifts=1, dims=0))          # (the student's views moved on by one, then by two, of three)
        graph.replay()
        torch.cuda.synchronize()
        got = _bits(c)
        assert _same_bits(got, _bits(segmentation_scores(tv, sv, gv, **kw))) and not _same_bits(got, a)
        rows, pooled = _host_rows(c, 3)
        want_rows, want_pooled, _ = O.scores(t, sv.cpu().numpy(), g, 30, 7)
        for n in range(3):
            _check_row(rows[n], want_rows[n], True, ("replay", step, n))
        _check_row(pooled, want_pooled, True, ("replay", step))


# ---- pictures -------------------------------------------------------------------------------------------------------------------
def test_recorded_pictures_match_the_reference():
    import seg_metrics as M
    z = np.load(GOLDEN)
    for name in ("color_a", "color_b"):
        labels, palette, image = _dev(z[f"{name}/labels"], torch.uint8), torch.from_numpy(z[f"{name}/palette"]), torch.from_numpy(z[f"{name}/image"]).to(DEV)
        assert np.array_equal(M.colorize(labels, palette).cpu().numpy(), z[f"{name}/mask"])
        strip = M.overlay(labels, palette, image, strip=True)
        assert strip.dtype == torch.uint8 and tuple(strip.shape) == (labels.shape[0], 3 * labels.shape[1], 3)
        assert np.array_equal(strip.cpu().numpy(), z[f"{name}/strip"])
        W = labels.shape[1]
        assert np.array_equal(M.overlay(labels.to(torch.int64), palette.to(DEV), image).cpu().numpy(), z[f"{name}/strip"][:, W:2 * W])


@pytest.mark.parametrize("shape", [(5, 7), (16, 64), (33, 65)])
def test_pictures_against_the_oracle(shape):
    import seg_metrics as M
    H, W = shape
    N, L = 2, 256
    rng = np.random.default_rng(H)
    palette = rng.integers(0, 256, size=(L, 3)).astype(np.uint8)
    palette[0], palette[255] = (0, 0, 0), (255, 255, 255)
    labels = rng.integers(0, L, size=(N, H, W)).astype(np.int64)
    labels.reshape(-1)[:2] = (0, 255)
    image = rng.random((N, 3, H, W)).astype(np.float32)
    flat = image.reshape(-1)
    flat[:4] = (0.0, 1.0, 1.0, 0.0)
    n = flat.size // 3
    flat[4:4 + n] = rng.integers(0, 256, size=n).astype(np.float32) / np.float32(255.0)          # exact k / 255
    img = torch.from_numpy(image).to(DEV)
    for dtype in DTYPES:
        lab = _dev(labels, dtype)
        assert np.array_equal(M.colorize(lab, palette).cpu().numpy(), O.colorize(labels, palette))
        for weights in ((0.4, 0.6), (1, 0)):
            for strip in (False, True):
                got = M.overlay(lab, palette, img, weights=weights, strip=strip)
                assert tuple(got.shape) == (N, H, 3 * W if strip else W, 3)
                assert np.array_equal(got.cpu().numpy(), O.overlay(labels, palette, image, weights, strip)), (dtype, weights, strip)
    # a single (H,W) map, a short palette: labels outside it take `fill`
    short = palette[:100]
    wild = labels[0].copy()
    wild.reshape(-1)[3:8] = (100, -1, 1 << 40, -(1 << 40), 255)
    for fill in ((0, 0, 0), (7, 200, 255)):
        got = M.colorize(_dev(wild), short, fill=fill)
        assert tuple(got.shape) == (H, W, 3) and np.array_equal(got.cpu().numpy(), O.colorize(wild, short, fill))
        got = M.overlay(_dev(wild), short, img[0], strip=True, fill=fill)
        assert np.array_equal(got.cpu().numpy(), O.overlay(wild, short, image[0], strip=True, fill=fill))
    # an image outside [0, 1] is clamped (the reference leaves it undefined), NaN gives 0
    odd = img[0].clone()
    odd.view(-1)[:4] = torch.tensor([-0.5, 1.5, float("nan"), 300.0], device=DEV)
    got = M.overlay(_dev(labels[0]), palette, odd, weights=(1, 0)).cpu().numpy()
    assert got[0, :4, 0].tolist() == [0, 255, 0, 255]


# ---- pipeline -------------------------------------------------------------------------------------------------------------------
def test_labels_of_segment_go_straight_in():
    from seg_metrics import segmentation_scores
    from segment import segment
    g = torch.Generator().manual_seed(4)
    K, C, H, W = 12, 16, 23, 31
    text = torch.randn(K, C, generator=g)
    teacher_map = torch.randn(C, H, W, generator=g)
    student_map = teacher_map + 0.7 * torch.randn(C, H, W, generator=g)
    lt = segment(teacher_map.to(DEV), text.to(DEV), half=False)
    ls = segment(student_map.to(DEV), text.to(DEV), half=False)
    assert lt.dtype == torch.int64 and tuple(lt.shape) == (H, W)
    sc = segmentation_scores(lt, ls, num_labels=K)
    (want,), pooled, _ = O.scores([lt.cpu().numpy()], [ls.cpu().numpy()], None, K, 7)
    rows, got_pooled = _host_rows(sc, 1)
    _check_row(rows[0], want, False, "pipeline")
    _check_row(got_pooled, pooled, False, "pipeline pooled")
    assert 0.0 < want["accuracy"] < 1.0
