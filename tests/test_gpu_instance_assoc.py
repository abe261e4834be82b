"""The instance association on the GPU (csrc/instances.hip; instances.py: associate_votes, merge_votes, InstanceLifter).  The
judge is tests/instance_assoc_oracle.py in float64.  Integer-valued weights make every sum exact in any order: there the table,
the mapping, count and dropped must equal the judge's to the bit.  With float weights the table is held to the project's
gradient bar and the DECISIONS are judged from the device's own table, on inputs whose decisions the judge finds clear."""
import types

import numpy as np
import pytest
import torch

import instance_assoc_oracle as io
import refutil as ru

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 1), (3, 4), (7, 8), (64, 63), (200, 300), (1024, 16), (5, 4096)]
ROWS = (0, 1, 63, 65, 5000)


def _counts(L):
    return sorted({0, L // 2, L})


def _structured(rng, P, M, L, count, integer):
    """votes and accumulator of P Gaussians that belong to objects: an object shows as one mask of the view and - below `count` -
    as one 3D instance, with sparse clutter in both; about 30 % of the rows are not seen (all zero), some seen rows carry no 3D
    label yet, some lie under no mask, and two 3D columns often hold the same maximum (the lowest index is the label)."""
    K = max(1, min(M, L, 12))
    obj = rng.integers(0, K, P)
    mask_of = rng.permutation(M)[:K] if M >= K else rng.integers(0, M, K)
    inst_of = rng.integers(0, max(count, 1), K)
    draw = (lambda *s: rng.integers(1, 4, s).astype(np.float32)) if integer else (lambda *s: (0.05 + rng.random(s)).astype(np.float32))
    av = np.zeros((P, M + 1), np.float32)
    clutter = rng.random((P, M)) < min(0.4, 2.0 / M)
    av[:, :M] = np.where(clutter, draw(P, M), 0)
    av[np.arange(P), mask_of[obj]] += np.where(rng.random(P) < 0.85, 3 * draw(P), 0)
    av[:, M] = av[:, :M].sum(1, dtype=np.float32) + np.where(rng.random(P) < 0.5, draw(P), 0)
    av[rng.random(P) < 0.3] = 0
    acc = np.zeros((P, L + 1), np.float32)
    if count:
        clutter = rng.random((P, count)) < min(0.4, 2.0 / count)
        acc[:, :count] = np.where(clutter, draw(P, count), 0)
        acc[np.arange(P), inst_of[obj]] += np.where(rng.random(P) < 0.8, 3 * draw(P), 0)
        if integer and count > 1:      # a second column at the row's maximum
            tie = rng.random(P) < 0.2
            acc[tie, rng.integers(0, count, int(tie.sum()))] = acc[tie, :count].max(1)
    acc[:, L] = acc[:, :L].sum(1, dtype=np.float32) + draw(P)
    return av, acc


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _associate(av, acc, count, iou_thresh, min_weight=0.0, dropped=0):
    import instances as ins
    c, d = _dev([count], torch.int32), _dev([dropped], torch.int32)
    out = ins.associate_votes(_dev(av), _dev(acc), c, iou_thresh=iou_thresh, min_weight=min_weight, dropped=d)
    torch.cuda.synchronize()
    assert out["dropped"] is d
    res = {k: out[k].cpu().numpy() for k in ("mapping", "best_label", "best_iou", "table")}
    res["count"], res["dropped"] = int(c.item()), int(d.item())
    assert res["mapping"].dtype == np.int32 and res["best_label"].dtype == np.int32 and res["best_iou"].dtype == np.float64
    assert res["table"].dtype == np.float32
    return res


def _bar(got, want, what):
    """every element within 1e-3 |g| + 1e-5 max|g| (the project's gradient bar)"""
    mx, worst = ru.grad_errors(got, want)
    print(f"{what}: max err / max|g| = {mx:.2e}, worst element {worst:.3f} x the bar")
    assert worst <= 1.0 and mx <= 1e-3, f"{what}: max err / max|g| = {mx:.2e}, worst element {worst:.2f} x outside the bar"


@pytest.mark.parametrize("M,L", SHAPES)
def test_integer_weights_equal_the_judge_exactly(M, L):
    import instances as ins
    rng = np.random.default_rng(1000 * M + L)
    ties = overflow = matched = 0
    for P in ROWS:
        for count in _counts(L):
            av, acc = _structured(rng, P, M, L, count, integer=True)
            for iou_thresh, min_weight in ((0.25, 0.0), (0.5, 3.0), (0.999, 0.0)):      # the last: next to nothing matches
                want = io.associate(av, acc, M, L, count, iou_thresh, min_weight)
                got = _associate(av, acc, count, iou_thresh, min_weight, dropped=7)
                what = f"P = {P}, M = {M}, L = {L}, count = {count}, iou_thresh = {iou_thresh}, min_weight = {min_weight}"
                assert got["table"].shape == (M + 1, L + 1) and np.array_equal(got["table"], want["table"]), what
                assert np.array_equal(got["best_label"], want["best_label"]), what
                assert np.array_equal(got["mapping"], want["mapping"]), what
                assert np.abs(got["best_iou"] - want["best_iou"]).max() <= 1e-15, what
                assert (got["count"], got["dropped"]) == (want["count"], 7 + want["dropped"]), what
                ties += want["gap"] == 0.0
                overflow += want["dropped"] > 0
                matched += int(((want["mapping"] >= 0) & (want["mapping"] < count)).sum())
            # the merge under that mapping: exact, and the view buffer is all zero afterwards
            v, a = _dev(av), _dev(acc)
            ins.merge_votes(v, _dev(want["mapping"], torch.int32), a, clear_view=True)
            torch.cuda.synchronize()
            assert np.array_equal(a.cpu().numpy(), io.merge(av, want["mapping"], acc, M, L)) and not v.any()
    print(f"M = {M}, L = {L}: {ties} cases with an exact tie, {overflow} that overflow, {matched} matched masks")
    assert overflow > 0
    if min(M, L) > 1:
        assert matched > 0


def test_hand_built_ties_of_both_kinds_and_the_overflow():
    M, L, count = 3, 4, 3
    #                 m0 m1 m2 total
    av = np.array([[4., 0, 0, 4], [4., 0, 0, 4], [0., 2, 2, 4], [0., 0, 0, 0]], np.float32)
    acc = np.array([[0., 5, 0, 0, 5], [0., 0, 5, 0, 5], [5., 0, 0, 0, 5], [5., 5, 5, 0, 15]], np.float32)
    want = io.associate(av, acc, M, L, count, 0.5)
    assert want["mapping"].tolist() == [1, 0, 3] and want["best_label"].tolist() == [1, 0, 0] and want["gap"] == 0.0
    got = _associate(av, acc, count, 0.5)
    assert np.array_equal(got["table"], want["table"]) and got["table"][0].tolist() == [0, 4, 4, 0, 0]
    assert got["mapping"].tolist() == [1, 0, 3] and got["best_label"].tolist() == [1, 0, 0] and got["best_iou"].tolist() == [0.5] * 3
    assert (got["count"], got["dropped"]) == (4, 0)
    # no slot left: the loser of the tie is dropped
    acc4 = acc.copy()
    acc4[3] = [0, 0, 0, 9, 9]
    got = _associate(av, acc4, 4, 0.5, dropped=2)
    assert got["mapping"].tolist() == [1, 0, -1] and (got["count"], got["dropped"]) == (4, 3)


@pytest.mark.parametrize("M,L", SHAPES)
def test_float_weights_table_at_the_bar_and_decisions_from_the_device_s_table(M, L):
    rng = np.random.default_rng(77 * M + L)
    clear = 0
    for P in ROWS[1:]:
        for count in _counts(L):
            av, acc = _structured(rng, P, M, L, count, integer=False)
            iou_thresh = 0.3
            want = io.associate(av, acc, M, L, count, iou_thresh)
            got = _associate(av, acc, count, iou_thresh)
            what = f"P = {P}, M = {M}, L = {L}, count = {count}"
            _bar(got["table"], want["table"], what)
            judged = io.match(got["table"], M, L, count, iou_thresh)
            print(f"{what}: the judge's smallest gap {want['gap']:.3e}, on the device's table {judged['gap']:.3e}")
            assert want["gap"] > 1e-9 and judged["gap"] > 1e-9, f"{what}: the inputs leave a decision within 1e-9 of its threshold"
            assert np.array_equal(got["mapping"], judged["mapping"]) and np.array_equal(got["best_label"], judged["best_label"]), what
            assert np.abs(got["best_iou"] - judged["best_iou"]).max() <= 1e-6, what
            assert (got["count"], got["dropped"]) == (judged["count"], judged["dropped"]), what
            clear += 1
    assert clear == (len(ROWS) - 1) * len(_counts(L))


@pytest.mark.parametrize("M,L", [(3, 4), (64, 63), (200, 300), (1024, 16), (5, 4096)])
def test_merge(M, L):
    import instances as ins
    rng = np.random.default_rng(5 * M + L)
    for P in (1, 65, 5000):
        av, _ = _structured(rng, P, M, L, L // 2, integer=False)
        acc = rng.standard_normal((P, L + 1)).astype(np.float32)          # any bits: untouched elements must keep them
        seen = av[:, M] > 0
        assert seen.any() or P == 1
        # injective, with entries that are ignored: -1, L and values far outside
        mapping = np.full(M, -1, np.int64)
        k = min(M, L)
        mapping[rng.permutation(M)[:k]] = rng.permutation(L)[:k]
        if M > k:
            mapping[mapping < 0] = rng.choice([-1, L, L + 1, 1 << 20, -7], int((mapping < 0).sum()))
        elif M > 1:
            mapping[rng.integers(0, M)] = rng.choice([L, -7, 1 << 20])
        want = acc.copy()
        for m in np.flatnonzero((mapping >= 0) & (mapping < L)):
            want[seen, mapping[m]] = acc[seen, mapping[m]] + av[seen, m]                     # ONE float32 add per element
        want[seen, L] = acc[seen, L] + av[seen, M]
        v, a = _dev(av), _dev(acc)
        assert ins.merge_votes(v, _dev(mapping, torch.int32), a) is a
        torch.cuda.synchronize()
        assert np.array_equal(a.cpu().numpy().view(np.uint32), want.view(np.uint32)), f"P = {P}: an injective merge is a single fp32 add"
        assert np.array_equal(v.cpu().numpy(), av), "without clear_view the view's votes are only read"
        _bar(a.cpu().numpy(), io.merge(av, mapping, acc, M, L), f"merge P = {P}, M = {M}, L = {L} against the judge")
        if M < 2:
            continue
        # repeated targets add up (at the bar: their adds arrive in any order); clear_view leaves all zeros
        rep = rng.integers(0, min(L, 3), M)
        a = _dev(acc)
        ins.merge_votes(v, _dev(rep, torch.int32), a, clear_view=True)
        torch.cuda.synchronize()
        got = a.cpu().numpy()
        _bar(got, io.merge(av, rep, acc, M, L), f"merge with repeated targets P = {P}, M = {M}, L = {L}")
        untouched = np.ones_like(acc, bool)
        untouched[np.ix_(seen, np.r_[np.unique(rep), L])] = False
        assert np.array_equal(got.view(np.uint32)[untouched], acc.view(np.uint32)[untouched])
        assert not v.any(), "clear_view leaves the view buffer all zero"


def test_no_rows():
    import instances as ins
    M, L = 5, 6
    got = _associate(np.zeros((0, M + 1), np.float32), np.zeros((0, L + 1), np.float32), 2, 0.5, dropped=4)
    assert not got["table"].any() and got["table"].shape == (M + 1, L + 1)
    assert (got["mapping"] == -1).all() and (got["best_label"] == -1).all() and not got["best_iou"].any()
    assert (got["count"], got["dropped"]) == (2, 4)
    a = torch.zeros(0, L + 1, device=DEV)
    assert ins.merge_votes(torch.zeros(0, M + 1, device=DEV), torch.zeros(M, device=DEV, dtype=torch.int32), a, clear_view=True) is a


def _int_views(rng, P, M, objects, n):
    """n views of P Gaussians of `objects` objects, integer weights: view v shows object k as mask perms[v][k]"""
    own = rng.integers(0, objects, P)
    views = []
    for _ in range(n):
        perm = rng.permutation(M)[:objects]
        av = np.zeros((P, M + 1), np.float32)
        av[np.arange(P), perm[own]] = rng.integers(2, 6, P)
        stray = rng.random(P) < 0.15
        av[stray, rng.integers(0, M, int(stray.sum()))] += 1
        av[:, M] = av[:, :M].sum(1) + rng.integers(0, 2, P)
        av[rng.random(P) < 0.25] = 0
        views.append(av)
    return views


def test_two_views_in_sequence_equal_the_judge_s_sequence():
    import instances as ins
    rng = np.random.default_rng(21)
    P, M, L = 3000, 9, 10                # six objects and three stray masks per view, ten slots: the second view overflows
    views = _int_views(rng, P, M, 6, 2)
    outs, acc_want, count_want, dropped_want = io.sequence(views, P, M, L, 0.5, 2.0)
    assert (outs[1]["mapping"][outs[1]["mapping"] >= 0] < outs[0]["count"]).sum() >= 5 and outs[0]["count"] >= 6
    acc = torch.zeros(P, L + 1, device=DEV)
    count, dropped = torch.zeros(1, device=DEV, dtype=torch.int32), torch.zeros(1, device=DEV, dtype=torch.int32)
    for av, o in zip(views, outs):
        v = _dev(av)
        r = ins.associate_votes(v, acc, count, iou_thresh=0.5, min_weight=2.0, dropped=dropped)
        ins.merge_votes(v, r["mapping"], acc, clear_view=True)
        torch.cuda.synchronize()
        assert np.array_equal(r["mapping"].cpu().numpy(), o["mapping"]) and np.array_equal(r["table"].cpu().numpy(), o["table"])
        assert not v.any()
    assert np.array_equal(acc.cpu().numpy(), acc_want) and (int(count.item()), int(dropped.item())) == (count_want, dropped_want)


def test_one_linear_capture_replays_to_the_same_mapping():
    import instances as ins
    rng = np.random.default_rng(22)
    P, M, L = 3000, 9, 12
    views = _int_views(rng, P, M, 6, 2)
    outs, acc_want, _, _ = io.sequence(views, P, M, L, 0.5, 0.0)
    first = io.merge(views[0], outs[0]["mapping"], np.zeros((P, L + 1)), M, L).astype(np.float32)
    v, acc = torch.zeros(P, M + 1, device=DEV), torch.zeros(P, L + 1, device=DEV)
    count, dropped = torch.zeros(1, device=DEV, dtype=torch.int32), torch.zeros(1, device=DEV, dtype=torch.int32)

    def load():          # the state in front of the second view
        v.copy_(_dev(views[1]))
        acc.copy_(_dev(first))
        count.fill_(outs[0]["count"])
        dropped.zero_()

    def step():
        r = ins.associate_votes(v, acc, count, iou_thresh=0.5, dropped=dropped)
        ins.merge_votes(v, r["mapping"], acc, clear_view=True)
        return r

    load()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # once outside the capture, as torch.cuda.graph asks
        eager = step()["mapping"].clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert np.array_equal(eager.cpu().numpy(), outs[1]["mapping"])
    load()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = step()
    for _ in range(2):
        load()
        r["mapping"].fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(r["mapping"].cpu().numpy(), outs[1]["mapping"])
        assert np.array_equal(acc.cpu().numpy(), acc_want) and int(count.item()) == outs[1]["count"] and not v.any()


# ---------------------------------------------------------------- end to end: three views through InstanceLifter

def test_instance_lifter_over_three_views(oracle_lib):
    """The inputs of tests/instance_cases.py (checked on the CPU by tests/test_instance_assoc_cpu.py): the same five slabs under
    another numbering in every view."""
    import contrib
    import instance_cases as ic
    import instances as ins
    from test_gpu_contrib import _Model, _camera
    c = ic.build()
    sc, P, W, H, M, L = c["scene"], c["P"], c["W"], c["H"], ic.MAX_MASKS, ic.MAX_INSTANCES
    pc = _Model(sc)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = sc["bg"].to(DEV)
    lifter = ins.InstanceLifter(P, L, M, DEV, iou_thresh=ic.IOU_THRESH)
    plain = contrib.LabelLifter(P, ic.SLABS, DEV)
    dtypes = [torch.int64, torch.int32, torch.int64]
    slab_id = None
    for cam, m, p, perm, dtype in zip(c["cams"], c["maps"], c["plain"], ic.PERMS, dtypes):
        view = _camera(cam)
        imap = torch.from_numpy(m).to(DEV).to(dtype)
        # the device's own vote of this view, and the state in front of it: what the judge decides from
        own = contrib.render_label_votes(view, pc, pipe, bg, imap, M)["acc"]
        before, count_before = lifter.acc.clone(), lifter.num_instances()
        out = lifter.add_view(view, pc, pipe, bg, imap)
        plain.add_view(view, pc, pipe, bg, torch.from_numpy(p).to(DEV))
        torch.cuda.synchronize()
        want = io.associate(own.cpu().numpy(), before.cpu().numpy(), M, L, count_before, ic.IOU_THRESH)
        mapping = out["mapping"].cpu().numpy()
        assert np.array_equal(mapping, want["mapping"]) and out["acc"] is lifter.acc and out["render"].shape == (3, H, W)
        assert np.abs(out["best_iou"].cpu().numpy() - want["best_iou"]).max() <= 1e-3          # two votes: atomics in another order
        assert not lifter.view.any(), "the view buffer is all zero again"
        if slab_id is None:
            slab_id = mapping[np.asarray(perm)]
        assert np.array_equal(mapping[np.asarray(perm)], slab_id) and (mapping[ic.SLABS:] == -1).all()
        gm = out["global_map"].cpu().numpy()
        assert gm.dtype == np.int64 and np.array_equal(gm, np.where(m >= 0, mapping[np.maximum(m, 0)], -1))
    assert lifter.views == 3 and lifter.num_instances() == ic.SLABS and lifter.num_dropped() == 0 and int(lifter.dropped.item()) == 0
    lab, ref, conf = lifter.labels().cpu().numpy(), plain.labels().cpu().numpy(), plain.confidence().cpu().numpy()
    sure = conf >= 0.6
    assert sure.sum() > P // 4
    assert np.array_equal(lab[sure], slab_id[ref[sure]])
    assert np.array_equal(lifter.seen().cpu().numpy(), plain.seen().cpu().numpy())
    sel = lifter.select(int(slab_id[2]))
    assert sel.dtype == torch.bool and sel.any() and (c["slab"][sel.cpu().numpy()] == 2).mean() > 0.8
