"""The label vote on the GPU (csrc/contrib.hip: label_votes_kernel; contrib.py: label_votes, LabelLifter).  The judge is never
the new kernel: it is the float64 walk of tests/contrib_oracle.py over the CPU oracle's forward state with the one-hot masks of
the label map, and the bar is the project's gradient bar (every element within 1e-3 |g| + 1e-5 max|g|), as for `acc` of the
contribution pass.  One walk per scene judges every map of that scene: the one-hot stacks are concatenated."""
import math
import types

import numpy as np
import pytest
import torch

import contrib_oracle as co
import label_maps as lm
import refutil as ru
from test_gpu_contrib import CASES, _Model, _camera, _forward
from util import general_camera

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SCENES = ("ragged", "tiles", "chunks", "opacity01", "heavy_tail_round")
MAPS = [("ladder", 20), ("ladder", 150), ("ladder", 300), ("noise", 20), ("noise", 150), ("noise", 300),
        ("constant", 1), ("constant", 20), ("constant", 150), ("constant", 300)]
_ref_cache = {}


def _dtypes(L):
    return ([torch.uint8] if L <= 256 else []) + [torch.int32, torch.int64]


def _labels(kind, W, H, L):
    return lm.KINDS[kind](W, H, L)


def _reference(name):
    """Scene and, for every map of MAPS, the judge's (P, L + 1) sums: one float64 walk over the oracle's state."""
    if name in _ref_cache:
        return _ref_cache[name]
    from oracle.oracle import Oracle, scene_kwargs
    sc = CASES[name]()
    W, H, P = sc["image_width"], sc["image_height"], sc["P"]
    o = Oracle()
    o.forward(**scene_kwargs(sc))
    maps = {(kind, L): _labels(kind, W, H, L) for kind, L in MAPS}
    j = co.walk(co.oracle_state(o), W, H, np.concatenate([lm.one_hot(maps[k], k[1]) for k in MAPS]))["acc"]
    judge, at = {}, 0
    for k in MAPS:
        judge[k] = np.concatenate([j[:, at:at + k[1]], j[:, -1:]], axis=1)
        at += k[1]
    ref = dict(scene=sc, W=W, H=H, P=P, maps=maps, judge=judge)
    _ref_cache[name] = ref
    return ref


def _votes(sc, fwd, labels, L, acc=None, dtype=torch.int64):
    from diff_gaussian_rasterization import _C
    n, _, _, _, _, geom, binning, img = fwd
    lab = labels if torch.is_tensor(labels) else torch.from_numpy(lm.as_dtype(labels, {torch.uint8: np.uint8, torch.int32: np.int32,
                                                                                      torch.int64: np.int64}[dtype])).to(DEV)
    if acc is None:
        acc = torch.zeros(sc["P"], L + 1, device=DEV)
    _C.label_votes(geom, binning, img, sc["P"], int(n), sc["image_height"], sc["image_width"], lab, L, acc)
    torch.cuda.synchronize()
    return acc


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _bar(got, want, what):
    """every element within 1e-3 |g| + 1e-5 max|g| (the project's gradient bar)"""
    mx, worst = ru.grad_errors(got, want)
    print(f"{what}: max err / max|g| = {mx:.2e}, worst element {worst:.3f} x the bar")
    assert worst <= 1.0 and mx <= 1e-3, f"{what}: max err / max|g| = {mx:.2e}, worst element {worst:.2f} x outside the bar"


@pytest.mark.parametrize("kind,L", MAPS)
@pytest.mark.parametrize("name", SCENES)
def test_votes_against_the_float64_walk(name, kind, L, option, oracle_lib):
    option("tile_cull", 0)            # the judge walks the oracle's lists: the reference's
    r = _reference(name)
    sc, P, labels, want = r["scene"], r["P"], r["maps"][(kind, L)], r["judge"][(kind, L)]
    assert want[:, L].max() > 0
    fwd = _forward(sc)
    for dtype in _dtypes(L):
        acc = _np(_votes(sc, fwd, labels, L, dtype=dtype))
        assert acc.shape == (P, L + 1) and np.isfinite(acc).all() and (acc >= 0).all()
        _bar(acc, want, f"{name} {kind} L = {L} {dtype}")
        unused = np.setdiff1d(np.arange(L), labels)
        assert not acc[:, unused].any(), "a class no pixel holds received weight"
        if kind != "noise":         # every label valid: the classes share out the total
            _bar(acc[:, :L].sum(1), acc[:, L], f"{name} {kind} L = {L} {dtype}: the classes' sum against the total")
        else:                       # invalid labels count in the total alone: the classes hold no more than it, up to the bar
            assert (acc[:, :L].sum(1) - acc[:, L] <= 1e-3 * acc[:, L] + 1e-5 * acc[:, L].max()).all()


def test_two_calls_add_and_the_total_is_the_contribution_pass_s(oracle_lib):
    from diff_gaussian_rasterization import _C
    r = _reference("chunks")
    sc, P, W, H = r["scene"], r["P"], r["W"], r["H"]
    labels, L = r["maps"][("ladder", 150)], 150
    fwd = _forward(sc)
    one = _votes(sc, fwd, labels, L)
    two = _votes(sc, fwd, labels, L)
    _votes(sc, fwd, labels, L, acc=two)
    _bar(_np(two), 2.0 * _np(one), "two calls into one acc against twice one call")
    n, _, _, _, _, geom, binning, img = fwd
    total = torch.zeros(P, 1, device=DEV)
    _C.contributions(geom, binning, img, P, int(n), H, W, None, total, None, False)
    torch.cuda.synchronize()
    _bar(_np(one)[:, L], _np(total)[:, 0], "the total column against contributions with K = 0")
    noisy = _votes(sc, fwd, r["maps"][("noise", 150)], L)
    _bar(_np(noisy)[:, L], _np(total)[:, 0], "the total column under invalid labels against contributions with K = 0")


def _wrapper_inputs(sc):
    import diff_gaussian_rasterization as dgr
    t = lambda x: x.to(DEV)
    st = dgr.GaussianRasterizationSettings(sc["image_height"], sc["image_width"], sc["tanfovx"], sc["tanfovy"], t(sc["bg"]), 1.0,
                                           t(sc["viewmatrix"]), t(sc["projmatrix"]), 3, t(sc["campos"]), False, False)
    kw = dict(means3D=t(sc["means3D"]), opacities=t(sc["opacities"]), shs=t(sc["shs"]), scales=t(sc["scales"]), rotations=t(sc["rotations"]))
    return st, kw


@pytest.mark.parametrize("kind", ["ladder", "noise"])
def test_against_the_grouped_route_on_the_device(kind, oracle_lib):
    """contributions(masks=MaskLifter.from_label_map(...)): 22 walks in groups of seven masks, against the one walk."""
    import contrib
    r = _reference("chunks")
    sc, P, L = r["scene"], r["P"], 150
    labels = torch.from_numpy(r["maps"][(kind, L)]).to(DEV)
    st, kw = _wrapper_inputs(sc)
    grouped = contrib.contributions(st, masks=contrib.MaskLifter.from_label_map(labels, L), pixel_outputs=False, **kw)["acc"]
    out = contrib.label_votes(st, labels=labels, num_classes=L, **kw)
    torch.cuda.synchronize()
    assert out["acc"].shape == (P, L + 1) and out["render"].shape == (3, r["H"], r["W"]) and set(out) == {"render", "feature_map", "depth", "radii", "acc"}
    _bar(_np(out["acc"]), _np(grouped), f"{kind}: one walk against the grouped route")
    # a given acc is added to, and returned
    again = contrib.label_votes(st, labels=labels.to(torch.int32), num_classes=L, acc=out["acc"], **kw)
    torch.cuda.synchronize()
    assert again["acc"] is out["acc"]
    _bar(_np(out["acc"]), 2.0 * _np(grouped), f"{kind}: a second view added")
    with pytest.raises(ValueError, match=r"torch.float32 \(70, 100\)"):
        contrib.label_votes(st, labels=labels.float(), num_classes=L, **kw)
    with pytest.raises(ValueError, match=r"\(70, 100\) tensor expected.*\(70, 99\)"):
        contrib.label_votes(st, labels=labels[:, :99], num_classes=L, **kw)
    with pytest.raises(ValueError, match=r"\(3000, 151\)"):
        contrib.label_votes(st, labels=labels, num_classes=L, acc=torch.zeros(P, L, device=DEV), **kw)
    with pytest.raises(ValueError, match="HIP device"):
        contrib.label_votes(st, labels=labels.cpu(), num_classes=L, **kw)


@pytest.mark.parametrize("name", ["chunks", "heavy_tail_round"])
def test_culled_and_reference_lists_agree(name, option, oracle_lib):
    r = _reference(name)
    sc, L = r["scene"], 150
    res = []
    for cull in (0, 1):
        option("tile_cull", cull)
        res.append(_np(_votes(sc, _forward(sc), r["maps"][("ladder", L)], L)))
    _bar(res[1], res[0], f"{name}: acc on the culled lists against the reference's lists")


def test_tile_bands(oracle_lib):
    from diff_gaussian_rasterization import _C
    r = _reference("chunks")
    sc, H, P, L = r["scene"], r["H"], r["P"], 150
    labels = r["maps"][("noise", L)]
    gy = (H + 15) // 16
    full = _np(_votes(sc, _forward(sc), labels, L))
    parts = np.zeros((P, L + 1))
    try:
        for r0, r1 in ((0, 2), (2, gy)):
            _C.set_tile_band(r0, r1)
            part = _np(_votes(sc, _forward(sc), labels, L))
            assert part.any()
            parts += part
    finally:
        _C.set_tile_band(0, 0)
    _bar(parts, full, "the bands' acc against the whole view's")


def test_no_gaussians_and_nothing_in_front_of_the_camera():
    import contrib
    from test_gpu_contrib import _synth
    sc = _synth(300, 40, 24, 17)
    W, H, L = 40, 24, 20
    st, kw = _wrapper_inputs(sc)
    labels = torch.from_numpy(lm.ladder(W, H, L)).to(DEV)
    behind = sc["means3D"].clone()
    behind[:, 2] = -behind[:, 2].abs() - 1.0
    for P, means in ((0, sc["means3D"][:0]), (300, behind)):
        k = {n: v[:P] for n, v in kw.items()}
        k["means3D"] = means.to(DEV)
        pre = torch.full((P, L + 1), 0.5, device=DEV)
        out = contrib.label_votes(st, labels=labels, num_classes=L, acc=pre, **k)
        torch.cuda.synchronize()
        assert out["acc"] is pre and out["acc"].shape == (P, L + 1) and (pre == 0.5).all()          # added to: nothing was added
        assert not (out["radii"] > 0).any()
        assert contrib.label_votes(st, labels=labels, num_classes=L, **k)["acc"].shape == (P, L + 1)
    lifter = contrib.LabelLifter(0, L, DEV)
    assert lifter.labels().shape == (0,) and lifter.label_image(torch.full((H, W), -1, device=DEV, dtype=torch.int32)).eq(-1).all()


# ---------------------------------------------------------------- LabelLifter: several views of one model

@pytest.mark.parametrize("name", ["opacity01", "chunks"])
def test_label_lifter_over_three_views(name, oracle_lib):
    """labels() against the judge's argmax wherever the judge's two largest columns differ by more than 1e-3 relative; that
    rule may leave out at most 1 % of the seen Gaussians (by the judge alone: 0.56 % at worst, 2 of 359)."""
    import contrib
    import edit
    from oracle.oracle import Oracle, scene_kwargs
    sc = CASES[name]()
    W, H, P, L = sc["image_width"], sc["image_height"], sc["P"], 150
    labels = lm.ladder(W, H, L)
    hot = lm.one_hot(labels, L)
    views = [dict(yaw=0.0, pitch=0.0, roll=0.0, campos=(0.0, 0.0, 0.0)), dict(yaw=6.0, pitch=-3.0, roll=10.0, campos=(0.3, -0.2, -0.5)),
             dict(yaw=-8.0, pitch=4.0, roll=-5.0, campos=(-0.4, 0.1, 0.4))]
    lifter = contrib.LabelLifter(P, L, DEV)
    pc = _Model(sc)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = sc["bg"].to(DEV)
    judge = np.zeros((P, L + 1))
    dtypes = [torch.int64, torch.uint8, torch.int32]
    for v, dtype in zip(views, dtypes):
        cam = general_camera(W, H, **v)
        for k in ("R", "t", "fovx", "fovy"):
            cam.pop(k)
        view = _camera(cam)
        out = lifter.add_view(view, pc, pipe, bg, torch.from_numpy(labels).to(DEV).to(dtype))
        assert out["render"].shape == (3, H, W) and out["acc"] is lifter.acc
        so = dict(sc, **cam)
        so["tanfovx"], so["tanfovy"] = math.tan(view.FoVx * 0.5), math.tan(view.FoVy * 0.5)      # as render() forms them
        o = Oracle()
        o.forward(**scene_kwargs(so))
        judge += co.walk(co.oracle_state(o), W, H, hot)["acc"]
    torch.cuda.synchronize()
    assert lifter.views == 3
    den = judge[:, L]
    seen = den > 0
    assert np.array_equal(lifter.seen().cpu().numpy(), seen) and seen.sum() > P // 4
    top = np.sort(judge[:, :L], 1)
    clear = seen & (top[:, -1] - top[:, -2] > 1e-3 * top[:, -1])
    left_out = int((seen & ~clear).sum())
    print(f"{name}: {left_out} of {int(seen.sum())} seen Gaussians have their two largest classes within 1e-3 relative")
    assert left_out <= 0.01 * seen.sum()
    lab = lifter.labels().cpu().numpy()
    assert lab.dtype == np.int64 and (lab[~seen] == -1).all() and (lab[seen] >= 0).all()
    assert np.array_equal(lab[clear], judge[:, :L].argmax(1)[clear])
    # confidence and ratios: the winning share, within the mask lifter's 2e-3
    want = np.where(seen[:, None], judge[:, :L] / np.maximum(den[:, None], 1e-300), 0.0)
    ratios = _np(lifter.ratios())
    e = np.abs(ratios - want).max()
    print(f"{name}: worst |ratio - judge| = {e:.2e}")
    assert ratios.shape == (P, L) and e <= 2e-3
    conf = _np(lifter.confidence())
    assert np.abs(conf - want.max(1)).max() <= 2e-3 and not conf[~seen].any() and (conf[seen] > 0).all() and (conf <= 1 + 1e-6).all()
    # select(cls): one column of ratios() >= threshold, driving the existing edit unchanged
    cls = int(np.bincount(lab[seen]).argmax())
    sel = lifter.select(cls)
    near = np.abs(want[:, cls] - 0.5) <= 2e-3
    assert sel.dtype == torch.bool and sel.shape == (P,)
    assert np.array_equal(sel.cpu().numpy()[~near], ((want[:, cls] >= 0.5) & seen)[~near])
    assert torch.equal(sel, (lifter.ratios()[:, cls] >= 0.5) & lifter.seen())
    assert not lifter.select(cls, min_weight=1e9).any() and lifter.select(cls, threshold=0.0).cpu().numpy().tolist() == seen.tolist()
    with pytest.raises(ValueError, match="cls = 150"):
        lifter.select(L)
    opacity, before = pc.get_opacity.clone(), pc.get_opacity.clone()
    edit.apply_edit(opacity, pc.get_features, sel, {"deletion": True})
    assert sel.any() and not opacity[sel].any() and torch.equal(opacity[~sel], before[~sel])
    # label_image(ids): the 3D labels seen from the first view
    cam = general_camera(W, H, **views[0])
    for k in ("R", "t", "fovx", "fovy"):
        cam.pop(k)
    ids = contrib.render_contributions(_camera(cam), pc, pipe, bg)["ids"]
    picture = lifter.label_image(ids)
    ids_np = ids.cpu().numpy()
    assert picture.dtype == torch.int64 and picture.shape == (H, W) and (ids_np >= 0).any()
    assert np.array_equal(picture.cpu().numpy(), np.where(ids_np >= 0, lab[np.maximum(ids_np, 0)], -1))
    assert torch.equal(lifter.label_image(ids.long()), picture)
