"""The instance association without a GPU: the judge (tests/instance_assoc_oracle.py) against hand-worked tables, its invariance
under a renumbering of the view's masks, the argument errors of f3dgs_instance_associate / f3dgs_instance_merge (raised before any
device work), those of the Python layer, and the soundness of the end-to-end inputs of tests/test_gpu_instance_assoc.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import instance_assoc_oracle as io
from util import ROOT

A = 0x10000                     # a never dereferenced address, aligned for every element


# ---------------------------------------------------------------- the judge against tables worked by hand

def test_first_view_every_mask_of_weight_is_new():
    M, L = 4, 6
    T = np.zeros((M + 1, L + 1))
    T[0, L], T[2, L], T[3, L], T[M, L] = 5, 2, 1, 7          # count = 0: all weight sits on unlabelled Gaussians
    o = io.match(T, M, L, 0)
    assert o["mapping"].tolist() == [0, -1, 1, 2] and o["best_label"].tolist() == [-1] * 4 and not o["best_iou"].any()
    assert o["count"] == 3 and o["dropped"] == 0
    o = io.match(T, M, L, 0, min_weight=1.0)                 # rowall <= min_weight: no instance, and not dropped
    assert o["mapping"].tolist() == [0, -1, 1, -1] and o["count"] == 2 and o["dropped"] == 0
    T2 = np.zeros((M + 1, 3))                                # two slots only (the table's column L is then column 2)
    T2[:, 2] = T[:, L]
    o = io.match(T2, M, 2, 0)
    assert o["mapping"].tolist() == [0, -1, 1, -1] and o["count"] == 2 and o["dropped"] == 1


def test_iou_counts_uncovered_instance_weight_but_not_unlabelled_mask_weight():
    M, L, count = 2, 3, 2
    T = np.array([[6., 0, 0, 10],      # mask 0: 6 on instance 0, 10 on unlabelled Gaussians (does not count against it)
                  [1., 3, 0, 0],       # mask 1: 1 on instance 0, 3 on instance 1
                  [2., 1, 0, 4]])      # under no mask: 2 of instance 0, 1 of instance 1 (counts against them)
    iou, rowall = io.iou_table(T, M, L, count)
    assert rowall.tolist() == [16, 4]
    assert np.array_equal(iou, np.array([[6 / (6 + 9 - 6), 0], [1 / (4 + 9 - 1), 3 / (4 + 4 - 3)]]))
    o = io.match(T, M, L, count, iou_thresh=0.5)
    assert o["best_label"].tolist() == [0, 1] and o["mapping"].tolist() == [0, 1] and o["count"] == 2 and o["dropped"] == 0
    assert o["best_iou"].tolist() == [6 / 9, 3 / 5]
    o = io.match(T, M, L, count, iou_thresh=0.65)            # mask 1 (0.6) fails the threshold: a new instance
    assert o["mapping"].tolist() == [0, 2] and o["count"] == 3
    assert abs(o["gap"] - min(6 / 9 - 0.65, 0.65 - 0.6)) < 1e-15


def test_exact_ties_go_to_the_lowest_index_on_both_sides():
    M, L, count = 3, 4, 3
    # mask 0 overlaps instances 1 and 2 alike: the LOWER instance is its best.  Masks 1 and 2 claim instance 0 with the same IoU:
    # the LOWER mask wins, the other opens a new instance.
    T = np.array([[0., 4, 4, 0, 0],
                  [2., 0, 0, 0, 0],
                  [2., 0, 0, 0, 0],
                  [0., 0, 0, 0, 0]])
    iou, _ = io.iou_table(T, M, L, count)
    assert iou[0, 1] == iou[0, 2] == 0.5 and iou[1, 0] == iou[2, 0] == 0.5
    o = io.match(T, M, L, count, iou_thresh=0.5)
    assert o["best_label"].tolist() == [1, 0, 0] and o["best_iou"].tolist() == [0.5, 0.5, 0.5]
    assert o["mapping"].tolist() == [1, 0, 3] and o["count"] == 4 and o["dropped"] == 0 and o["gap"] == 0.0
    # without the tie the larger IoU wins whatever its index: col[0] = 6, 2 / (2 + 6 - 2) = 1 / 3 against 3 / (3 + 6 - 3) = 1 / 2
    T[1, 0], T[2, 0], T[3, 0] = 2, 3, 1
    o = io.match(T, M, L, count, iou_thresh=0.3)
    assert o["mapping"].tolist() == [1, 3, 0]


def test_overflow_at_full_count():
    M, L = 3, 2
    T = np.array([[5., 0, 0], [0., 0, 3], [0., 1, 2], [0., 4, 0]])
    o = io.match(T, M, L, L, iou_thresh=0.5)       # mask 0 keeps instance 0; masks 1, 2 find no slot (mask 2: IoU 1 / 7)
    assert o["mapping"].tolist() == [0, -1, -1] and o["count"] == 2 and o["dropped"] == 2
    o = io.match(T, M, L, L, iou_thresh=0.5, min_weight=3.0)
    assert o["mapping"].tolist() == [0, -1, -1] and o["dropped"] == 0          # rowall 3 <= 3: not counted


def test_overlap_table_by_hand():
    M, L = 2, 3
    #                 m0  m1  total
    av = np.array([[1., 2., 4.],       # g0: label 1 (the first of the two largest); 1 under no mask
                   [3., 0., 3.],       # g1: no 3D label yet -> column L
                   [5., 5., 0.],       # g2: total 0 - not seen, takes no part
                   [0., 2., 1.],       # g3: the residual is clamped at 0
                   [0., 0., 6.]], np.float32)   # g4: seen under no mask at all
    acc = np.array([[0., 7, 7, 9], [0., 0, 0, 0], [9., 0, 0, 9], [2., 1, 0, 3], [0, 0, 4., 4]], np.float32)
    assert io.global_labels(acc, L).tolist() == [1, -1, 0, 0, 2]
    T = io.overlap_table(av, acc, M, L)
    want = np.zeros((M + 1, L + 1))
    want[0, 1], want[1, 1], want[2, 1] = 1, 2, 1
    want[0, 3] = 3
    want[1, 0] = 2
    want[2, 2] = 6
    assert np.array_equal(T, want)
    merged = io.merge(av, [2, 7], acc, M, L)       # 7 lies outside [0, L): ignored
    assert np.array_equal(merged, np.array([[0., 7, 8, 13], [0, 0, 3, 3], [9, 0, 0, 9], [2, 1, 0, 4], [0, 0, 4, 10]]))
    both = io.merge(av, [1, 1], acc, M, L)         # a repeated target: both are added
    assert both[0].tolist() == [0, 10, 7, 13] and both[3].tolist() == [2, 3, 0, 4]
    # the residual is a float32 sum in ascending m: 2^24 + 1 + 1 stays 2^24 there, and the total 2^24 + 2 leaves 2, not 0
    big = np.array([[2.0 ** 24, 1, 1, 2.0 ** 24 + 2]], np.float32)
    assert io.overlap_table(big, np.zeros((1, 2), np.float32), 3, 1)[3, 1] == 2.0


def _random_case(rng, P, M, L, count):
    """non-negative float votes with about a third of the rows unseen, an accumulator with `count` columns in use"""
    av = rng.random((P, M + 1)).astype(np.float32) * (rng.random((P, M + 1)) < 0.4)
    av[:, M] = av[:, :M].sum(1) + rng.random(P).astype(np.float32)
    av[rng.random(P) < 0.3] = 0
    acc = np.zeros((P, L + 1), np.float32)
    acc[:, :count] = rng.random((P, count)) * (rng.random((P, count)) < 0.5)
    acc[:, L] = acc[:, :L].sum(1)
    return av, acc


@pytest.mark.parametrize("seed", range(5))
def test_the_judge_does_not_depend_on_the_numbering_of_the_view_s_masks(seed):
    rng = np.random.default_rng(seed)
    P, M, L, count = 400, 7, 12, 5
    av, acc = _random_case(rng, P, M, L, count)
    acc[:, :count] += 20 * np.eye(count, dtype=np.float32)[rng.integers(0, count, P)]          # clear 3D labels
    hit = rng.integers(0, M, P)
    av[np.arange(P), hit] += np.where(av[:, M] > 0, 6, 0).astype(np.float32) * (hit % count == acc[:, :count].argmax(1))
    av[:, M] = np.where(av[:, M] > 0, av[:, :M].sum(1) + 0.25, 0).astype(np.float32)
    one = io.associate(av, acc, M, L, count, iou_thresh=0.2)
    assert one["gap"] > 1e-9 and (one["mapping"] >= 0).sum() >= 3 and ((one["mapping"] >= 0) & (one["mapping"] < count)).any()
    perm = rng.permutation(M)                       # mask m of the view becomes mask perm[m]
    pv = np.empty_like(av)
    pv[:, perm], pv[:, M] = av[:, :M], av[:, M]
    two = io.associate(pv, acc, M, L, count, iou_thresh=0.2)
    assert np.array_equal(two["table"][perm], one["table"][:M]) and np.allclose(two["table"][M], one["table"][M], rtol=1e-6)
    # (the float32 residual and the column sums add in another order under the renumbering: equal to rounding, not to the bit)
    assert np.array_equal(two["best_label"][perm], one["best_label"]) and np.allclose(two["best_iou"][perm], one["best_iou"], rtol=1e-6, atol=0)
    old = one["mapping"] < count                    # matched masks keep their instance; the others are new (or none) in both
    assert np.array_equal(two["mapping"][perm][old & (one["mapping"] >= 0)], one["mapping"][old & (one["mapping"] >= 0)])
    assert np.array_equal(two["mapping"][perm] >= count, one["mapping"] >= count)
    assert np.array_equal(two["mapping"][perm] == -1, one["mapping"] == -1)
    assert (two["count"], two["dropped"]) == (one["count"], one["dropped"])
    assert sorted(two["mapping"][two["mapping"] >= count].tolist()) == list(range(count, two["count"]))


def test_sequence_first_view_needs_no_special_case():
    rng = np.random.default_rng(11)
    P, M, L = 60, 3, 5
    own = rng.integers(0, 3, P)
    view = lambda perm: np.concatenate([4.0 * np.eye(M)[np.asarray(perm)[own]], np.full((P, 1), 4.0)], 1).astype(np.float32)
    outs, acc, count, dropped = io.sequence([view([0, 1, 2]), view([2, 0, 1]), view([1, 2, 0])], P, M, L)
    assert [o["mapping"].tolist() for o in outs] == [[0, 1, 2], [1, 2, 0], [2, 0, 1]] and count == 3 and dropped == 0
    assert all(o["best_iou"].tolist() == [1.0, 1.0, 1.0] for o in outs[1:])
    assert np.array_equal(acc[:, :3], 12.0 * np.eye(3)[own]) and (acc[:, L] == 12).all() and not acc[:, 3:L].any()


# ---------------------------------------------------------------- the C ABI's argument errors, before any device work

def _lib():
    import diff_gaussian_rasterization  # noqa: F401  (its bundled HIP runtime must be the one the library binds to)
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.f3dgs_instance_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_instance_scratch_bytes.argtypes = [ci, ci]
    lib.f3dgs_instance_associate.restype = ci
    lib.f3dgs_instance_associate.argtypes = [ci] * 3 + [vp, vp, cd, cd] + [vp] * 8
    lib.f3dgs_instance_merge.restype = ci
    lib.f3dgs_instance_merge.argtypes = [ci] * 3 + [vp, ci, vp, vp, vp]
    lib.f3dgs_version.restype = ci
    return lib


def test_argument_errors_before_any_device_work():
    lib = _lib()
    err = lib.f3dgs_last_error
    good = dict(P=5, M=3, L=4, acc_view=A, acc=A, iou=0.5, minw=0.0, count=A, dropped=A, mapping=A, best_label=A, best_iou=A, table=A,
                scratch=A)

    def assoc(**kw):
        a = dict(good, **kw)
        return lib.f3dgs_instance_associate(a["P"], a["M"], a["L"], a["acc_view"], a["acc"], a["iou"], a["minw"], a["count"], a["dropped"],
                                            a["mapping"], a["best_label"], a["best_iou"], a["table"], a["scratch"], None)

    assert assoc(P=-1) == -1 and b"P < 0" in err()
    for M in (0, -2, 1025):
        assert assoc(M=M) == -1 and b"M outside 1 .. 1024" in err()
    for L in (0, -1, 4097):
        assert assoc(L=L) == -1 and b"L outside 1 .. 4096" in err()
    for name in ("acc_view", "acc", "count", "dropped", "mapping", "best_label", "best_iou", "table", "scratch"):
        assert assoc(**{name: None}) == -1 and b"null pointer" in err(), name
    for off in (4, 8, 1):
        assert assoc(scratch=A + off) == -1 and b"16-byte aligned" in err()
    for bad in (-0.1, float("nan"), -float("inf")):
        assert assoc(iou=bad) == -1 and b"iou_thresh" in err()
        assert assoc(minw=bad) == -1 and b"min_weight" in err()
    # P == 0 still answers the checks first (acc_view and acc may be null there, the outputs may not)
    assert assoc(P=0, acc_view=None, acc=None, table=None) == -1 and b"null pointer" in err()
    assert assoc(P=0, acc_view=None, acc=None, M=0) == -1

    merge = lambda P=5, M=3, L=4, acc_view=A, clear=1, mapping=A, acc=A: lib.f3dgs_instance_merge(P, M, L, acc_view, clear, mapping, acc, None)
    assert merge(P=-1) == -1 and b"P < 0" in err()
    for M in (0, 1025):
        assert merge(M=M) == -1 and b"M outside" in err()
    for L in (0, 4097):
        assert merge(L=L) == -1 and b"L outside" in err()
    for kw in (dict(acc_view=None), dict(mapping=None), dict(acc=None), dict(P=0, mapping=None)):
        assert merge(**kw) == -1 and b"null pointer" in err()
    assert merge(P=0, acc_view=None, acc=None) == 0            # no rows: nothing to add, no device touched

    assert lib.f3dgs_instance_scratch_bytes(0, 4) == 0 and lib.f3dgs_instance_scratch_bytes(3, 4097) == 0
    small, large = lib.f3dgs_instance_scratch_bytes(1, 1), lib.f3dgs_instance_scratch_bytes(1024, 4096)
    assert 0 < small <= large and large >= 8 * (2 * 1024 + 4096) + 4 * 4096 and large < (1 << 20)      # vectors of M and L only
    assert lib.f3dgs_version() >= 31700


# ---------------------------------------------------------------- the Python layer

def _past_the_device_check(fn):
    """runs fn with contrib._need_device switched off: the dtype / shape / device rules behind it, without a device"""
    import contrib
    keep = contrib._need_device
    contrib._need_device = lambda t, name: None
    try:
        return fn()
    finally:
        contrib._need_device = keep


def test_wrapper_errors_and_no_cpu_path():
    import instances as ins
    av, acc = torch.zeros(6, 4), torch.zeros(6, 9)
    count = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="HIP device"):
        ins.associate_votes(av, acc, count)
    with pytest.raises(ValueError, match="HIP device"):
        ins.merge_votes(av, torch.zeros(3, dtype=torch.int32), acc)
    for bad in (torch.zeros(6), torch.zeros(6, 1), torch.zeros(2, 3, 4), np.zeros((6, 4), np.float32)):
        with pytest.raises(ValueError, match=r"acc_view: a contiguous float32 \(P, M \+ 1\)"):
            ins.associate_votes(bad, acc, count)
        with pytest.raises(ValueError, match=r"acc: a contiguous float32 \(P, L \+ 1\)"):
            ins.merge_votes(av, torch.zeros(3, dtype=torch.int32), bad)
    with pytest.raises(ValueError, match=r"M = 1025 masks, 1 \.\. 1024"):
        ins.associate_votes(torch.zeros(2, 1026), acc, count)
    with pytest.raises(ValueError, match=r"L = 4097 instances, 1 \.\. 4096"):
        ins.associate_votes(av, torch.zeros(6, 4098), count)
    for kw in (dict(iou_thresh=-0.5), dict(iou_thresh=float("nan")), dict(min_weight=-1.0), dict(min_weight="much")):
        with pytest.raises(ValueError, match="a number >= 0 expected"):
            ins.associate_votes(av, acc, count, **kw)
    # behind the device check: the rules of contrib._check_votes, naming dtype, shape and device
    with pytest.raises(ValueError, match=r"acc_view: acc must be a contiguous float32 \(6, 4\).*torch.float64 \(6, 4\) on cpu"):
        _past_the_device_check(lambda: ins.associate_votes(av.double(), acc, count))
    with pytest.raises(ValueError, match=r"acc_view: acc must be a contiguous float32 \(6, 4\)"):
        _past_the_device_check(lambda: ins.associate_votes(torch.zeros(4, 6).t(), acc, count))
    with pytest.raises(ValueError, match=r"acc must be a contiguous float32 \(6, 9\).*\(5, 9\) on cpu"):
        _past_the_device_check(lambda: ins.associate_votes(av, torch.zeros(5, 9), count))
    for bad in (torch.zeros(1), torch.zeros(2, dtype=torch.int32), 3):
        with pytest.raises(ValueError, match="count must be one int32"):
            _past_the_device_check(lambda: ins.associate_votes(av, acc, bad))
    with pytest.raises(ValueError, match="dropped must be one int32"):
        _past_the_device_check(lambda: ins.associate_votes(av, acc, count, dropped=torch.zeros(1, dtype=torch.int64)))
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), [0, 1, 2]):
        with pytest.raises(ValueError, match=r"mapping must be a contiguous int32 \(3,\)"):
            _past_the_device_check(lambda: ins.merge_votes(av, bad, acc))
    with pytest.raises(ValueError, match="max_instances=4097"):
        ins.InstanceLifter(5, 4097, 8, "cuda")
    with pytest.raises(ValueError, match="max_masks=0"):
        ins.InstanceLifter(5, 8, 0, "cuda")
    with pytest.raises(ValueError, match="a number >= 0 expected"):
        ins.InstanceLifter(5, 8, 8, "cuda", iou_thresh=-1)
    with pytest.raises(ValueError, match=r"LabelLifter\(P=-1"):
        ins.InstanceLifter(-1, 8, 8, "cuda")
    with pytest.raises(ValueError, match="HIP device"):
        ins.InstanceLifter(5, 8, 8, "cpu")
    import contrib
    assert issubclass(ins.InstanceLifter, contrib.LabelLifter) and (ins.MAX_MASKS, ins.MAX_INSTANCES) == (1024, 4096)


# ---------------------------------------------------------------- the end-to-end inputs are sound by the judge alone

def test_end_to_end_inputs_map_back_to_the_first_view_s_ids(oracle_lib):
    import instance_cases as ic
    c = ic.build()
    P, M, L = c["P"], ic.MAX_MASKS, ic.MAX_INSTANCES
    assert sorted(np.bincount(c["slab"]).tolist()) == [P // ic.SLABS] * ic.SLABS
    for m, p, perm in zip(c["maps"], c["plain"], ic.PERMS):
        assert set(np.unique(p).tolist()) == {-1, 0, 1, 2, 3, 4}                  # every slab shows, and some pixels blend nothing
        assert np.array_equal(m, np.where(p >= 0, np.asarray(perm)[np.maximum(p, 0)], -1)) and sorted(perm) == list(range(ic.SLABS))
    outs, acc, count, dropped = io.sequence([v.astype(np.float32) for v in c["votes"]], P, M, L, ic.IOU_THRESH, 0.0)
    assert count == ic.SLABS and dropped == 0
    first = outs[0]["mapping"]
    assert sorted(first[:ic.SLABS].tolist()) == list(range(ic.SLABS)) and (first[ic.SLABS:] == -1).all()
    slab_id = first[np.asarray(ic.PERMS[0])]                                       # the global id of every slab
    for o, perm in zip(outs[1:], ic.PERMS[1:]):
        assert np.array_equal(o["mapping"][np.asarray(perm)], slab_id) and (o["mapping"][ic.SLABS:] == -1).all()
        matched = o["best_iou"][np.asarray(perm)]
        print("matched IoU:", np.round(matched, 3))
        assert (matched >= ic.IOU_THRESH + 0.05).all()
    # the 3D labels this gives are the slabs' (in global ids) for most of the seen Gaussians
    lab = np.where(acc[:, :L].max(1) > 0, acc[:, :L].argmax(1), -1)
    seen = lab >= 0
    assert seen.sum() > P // 2 and (lab[seen] == slab_id[c["slab"]][seen]).mean() > 0.8
