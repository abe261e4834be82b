"""The contribution pass on the GPU (csrc/contrib.hip, contrib.py).  The judge is never the new kernel: per Gaussian it is
the CPU oracle's backward with the masks as upstream feature gradient (a), per pixel the float64 walk of
tests/contrib_oracle.py over the oracle's forward state (b); and the forward call's own final_T / n_contrib, which the pass
must reproduce bit for bit."""
import math
import types

import numpy as np
import pytest
import torch

import contrib_oracle as co
import refutil as ru
from util import general_camera, harsh_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = {
    "ragged": lambda: _synth(50, 17, 23, 11),                                      # one and a bit tiles
    "tiles": lambda: _synth(400, 129, 64, 12),                                     # 8 T + 1 columns, empty tiles
    "chunks": lambda: _synth(3000, 100, 70, 13),                                   # lists of several chunks
    "dense": lambda: _synth(2500, 64, 64, 14, scale_lo=0.02, scale_hi=0.4),        # every pixel ends early
    "opacity01": lambda: harsh_scene("opacity01", 1500, 0, 70, 33, seed=15),
    "heavy_tail_round": lambda: harsh_scene("heavy_tail_round", 1500, 0, 70, 33, seed=16),
}
SYNTH = ("ragged", "tiles", "chunks", "dense")


def _synth(P, W, H, seed, **kw):
    from synth import make_scene
    return make_scene(P=P, C=0, width=W, height=H, seed=seed, **kw)


def _masks(W, H, seed=0):
    """the seven masks of every case: all ones, the checker, a half plane cut at x = 21, uniform soft values, all zeros, and
    the checker and the half plane inverted"""
    y, x = np.mgrid[0:H, 0:W]
    checker, half = ((x // 5 + y // 3) & 1).astype(np.float32), (x < 21).astype(np.float32)
    soft = np.random.default_rng(seed).random((H, W)).astype(np.float32)
    return np.stack([np.ones((H, W), np.float32), checker, half, soft, np.zeros((H, W), np.float32), 1 - checker, 1 - half])


ZERO_COLUMN = 4
_ref_cache = {}


def _reference(name):
    """Scene, masks and both judges of a case, computed once."""
    if name in _ref_cache:
        return _ref_cache[name]
    from oracle.oracle import Oracle, scene_kwargs
    sc = CASES[name]()
    W, H, P = sc["image_width"], sc["image_height"], sc["P"]
    masks = _masks(W, H)
    K = len(masks)
    so = dict(sc, C=K + 1, semantic_feature=torch.zeros(P, 1, K + 1))
    o = Oracle()
    out = o.forward(**scene_kwargs(so))
    state = co.oracle_state(o)
    judge = co.walk(state, W, H, masks)
    grad = None
    if name in SYNTH:
        up = np.concatenate([masks, np.ones((1, H, W), np.float32)])
        grad = o.backward(np.zeros((3, H, W), np.float32), up, np.zeros((1, H, W), np.float32))["dL_dsemantic_feature"]
        grad = grad.reshape(P, K + 1).astype(np.float64)
    ref = dict(scene=sc, masks=masks, state=state, judge=judge, grad=grad, radii=out["radii"], W=W, H=H, P=P)
    _ref_cache[name] = ref
    return ref


def _forward(sc):
    d = ru.device_inputs(sc, sc["C"], DEV)
    return ru.raw_forward(ru.product_module(), sc, d)


def _pass(sc, fwd, masks=None, acc=None, wmax=None, pixel=True):
    from diff_gaussian_rasterization import _C
    n, _, _, _, _, geom, binning, img = fwd
    m = None if masks is None else torch.as_tensor(masks, device=DEV).contiguous()
    out = _C.contributions(geom, binning, img, sc["P"], int(n), sc["image_height"], sc["image_width"], m, acc, wmax, pixel)
    torch.cuda.synchronize()
    return out


def _np(t):
    return t.cpu().numpy()


def _zeros(*shape):
    return torch.zeros(*shape, device=DEV)


def _bar(got, want, what):
    """every element within 1e-3 |g| + 1e-5 max|g| (the project's gradient bar)"""
    mx, worst = ru.grad_errors(got, want)
    print(f"{what}: max err / max|g| = {mx:.2e}, worst element {worst:.3f} x the bar")
    assert worst <= 1.0 and mx <= 1e-3, f"{what}: max err / max|g| = {mx:.2e}, worst element {worst:.2f} x outside the bar"
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_case_against_the_forward_and_both_judges(name, option, oracle_lib):
    option("tile_cull", 0)            # n_contrib is a list position: comparable with the oracle's only on the reference's lists
    r = _reference(name)
    sc, masks, j, W, H, P = r["scene"], r["masks"], r["judge"], r["W"], r["H"], r["P"]
    K = len(masks)
    fwd = _forward(sc)
    img = ru.product_image_state(sc, fwd)
    final_T, n_contrib = img["final_T"].reshape(H, W), img["n_contrib"].reshape(H, W)
    acc, wmax = _zeros(P, K + 1), _zeros(P)
    alpha, median, ids, idw = (_np(t) for t in _pass(sc, fwd, masks, acc, wmax))
    acc, wmax = _np(acc).astype(np.float64), _np(wmax)
    assert ids.dtype == np.int32 and alpha.shape == median.shape == ids.shape == idw.shape == (H, W)

    # ---- exact consistency with the forward call
    assert np.array_equal(alpha, np.float32(1.0) - final_T), "alpha is not 1 - final_T bit for bit"
    assert all(np.isfinite(a).all() for a in (alpha, median, idw, acc, wmax))
    assert ((ids == -1) | ((ids >= 0) & (ids < P))).all()
    assert not (ids[n_contrib == 0] != -1).any()
    assert np.array_equal(ids == -1, idw == 0) and np.array_equal(ids == -1, final_T == 1.0)     # nothing blended <=> T stayed 1
    # 0 <= id_weight <= alpha.  Both sides are the forward's float32 values: alpha = fl(1 - T) with T a product of n_contrib
    # rounded factors, each rounding at most 2^-24 in absolute terms (T <= 1), and one more for the subtraction - a pixel with a
    # single contributor has id_weight = a exactly and alpha = fl(1 - fl(1 - a)), which may lie one rounding below a
    assert (idw >= 0).all() and (idw <= alpha + (n_contrib + 1.0) * 2.0 ** -24).all()
    seen = ids >= 0
    assert (wmax[ids[seen]] >= idw[seen]).all()
    dom = np.zeros(P, np.float32)
    np.maximum.at(dom, ids[seen], idw[seen])           # largest weight a Gaussian has where it is the dominant one
    assert (wmax >= dom).all()
    own_max = seen & (idw == wmax[np.where(seen, ids, 0)])      # pixels where the dominant Gaussian reaches its own maximum
    assert np.array_equal(wmax[ids[own_max]], dom[ids[own_max]])
    dead = (sc["opacities"].numpy().reshape(-1) == 0) | (r["radii"] == 0)
    assert not acc[dead].any() and not wmax[dead].any()
    assert not acc[:, ZERO_COLUMN].any()
    assert (acc >= 0).all() and (wmax >= 0).all() and (wmax <= 0.99).all()

    # ---- per pixel against the float64 walk (b)
    border = j["borderline"] | (n_contrib != r["state"]["n_contrib"].reshape(H, W))
    nb = int(border.sum())
    print(f"{name}: {nb} borderline pixels of {W * H}")
    assert nb <= 0.01 * W * H
    ok = ~border
    e_alpha = np.abs(alpha - j["alpha"])[ok].max()
    e_idw = np.abs(idw - j["top1"])[ok].max()
    print(f"{name}: worst |alpha - judge| = {e_alpha:.2e}, worst |id_weight - judge| = {e_idw:.2e}")
    assert e_alpha <= 1e-5 and e_idw <= 1e-5
    assert np.array_equal(ids[ok], j["ids"][ok])
    assert np.array_equal(median[ok].view(np.uint32), j["median_depth"][ok].view(np.uint32))
    if nb:
        two = co.top_two(r["state"], W, H, np.flatnonzero(border.reshape(-1)))
        for p, pair in two.items():
            assert ids.reshape(-1)[p] in pair or ids.reshape(-1)[p] == -1 and pair == (-1, -1), (p, ids.reshape(-1)[p], pair)
    # a Gaussian's largest weight, where the judge finds it at a pixel that is not borderline
    g_ok = (j["wmax_pixel"] >= 0) & ~border.reshape(-1)[np.maximum(j["wmax_pixel"], 0)]
    never = j["wmax_pixel"] < 0
    e_wmax = np.abs(wmax - j["wmax"])[g_ok].max() if g_ok.any() else 0.0
    print(f"{name}: worst |wmax - judge| = {e_wmax:.2e} over {int(g_ok.sum())} Gaussians")
    assert e_wmax <= 1e-5
    if nb == 0:
        assert not wmax[never].any()

    # ---- per Gaussian
    if r["grad"] is not None:
        _bar(acc, r["grad"], f"{name}: acc against the oracle's backward")
        _bar(acc[:, 0], acc[:, K], f"{name}: the all-ones mask against the weight total")
    else:
        mass = abs(acc[:, K].sum() - alpha.astype(np.float64).sum())
        print(f"{name}: |sum acc[:, K] - sum alpha| = {mass:.3e} (bar {1e-5 * W * H:.3e})")
        assert mass <= 1e-5 * W * H
    want = r["grad"] if r["grad"] is not None else acc          # harsh cases: the columns of the K = 7 call

    # ---- the other column counts: K = 0, 1, 3 (the judge's columns of the same masks), without the per-pixel outputs
    for k in (0, 1, 3):
        a = _zeros(P, k + 1)
        out = _pass(sc, fwd, masks[:k] if k else None, a, None, pixel=False)
        assert out == (None, None, None, None)
        cols = list(range(k)) + [K]
        _bar(_np(a), want[:, cols], f"{name}: K = {k}")
    # wmax alone, and the per-pixel outputs alone: reproducible, so bit-identical to the combined call
    w2 = _zeros(P)
    _pass(sc, fwd, None, None, w2, pixel=False)
    assert np.array_equal(_np(w2), wmax)
    again = [_np(t) for t in _pass(sc, fwd)]
    for a, b in zip(again, (alpha, median, ids, idw)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["ragged", "chunks"])
def test_every_column_count_walks_the_same_list(name):
    """One walk feeds every contrib_kernel<NC, PIX>, with the entry's depth (PIX) and without: the reproducible outputs - the
    four per-pixel ones, and wmax, a max of non-negative floats - must not depend on which instantiation formed them."""
    sc = CASES[name]()
    W, H, P = sc["image_width"], sc["image_height"], sc["P"]
    masks = _masks(W, H)
    fwd = _forward(sc)
    pix_only = [_np(t) for t in _pass(sc, fwd)]                                   # <0, true>
    wmax_only = _zeros(P)
    assert _pass(sc, fwd, None, None, wmax_only, pixel=False) == (None, None, None, None)      # <0, false>
    assert pix_only[0].any() and wmax_only.any()
    for k in (0, 1, 3, 7):                                                        # NC = 1, 2, 4, 8
        m = masks[:k] if k else None
        pix = _pass(sc, fwd, m, _zeros(P, k + 1), None)                           # <NC, true>
        for what, a, b in zip(("alpha", "median_depth", "ids", "id_weight"), pix, pix_only):
            assert np.array_equal(_np(a).view(np.uint32), b.view(np.uint32)), f"{name}: {what} with K = {k} differs from the per-pixel-only call"
        wmax = _zeros(P)
        _pass(sc, fwd, m, _zeros(P, k + 1), wmax, pixel=False)                    # <NC, false>
        assert torch.equal(wmax.view(torch.int32), wmax_only.view(torch.int32)), f"{name}: wmax beside K = {k} differs from the wmax-only call"


def test_no_gaussians_and_nothing_in_front_of_the_camera():
    import contrib
    import diff_gaussian_rasterization as dgr
    sc = _synth(300, 40, 24, 17)
    W, H = 40, 24
    t = lambda x: x.to(DEV)
    st = dgr.GaussianRasterizationSettings(H, W, sc["tanfovx"], sc["tanfovy"], t(sc["bg"]), 1.0, t(sc["viewmatrix"]), t(sc["projmatrix"]),
                                           3, t(sc["campos"]), False, False)
    masks = torch.ones(2, H, W, device=DEV)
    behind = sc["means3D"].clone()
    behind[:, 2] = -behind[:, 2].abs() - 1.0
    for P, means in ((0, sc["means3D"][:0]), (300, behind)):
        kw = dict(means3D=t(means), opacities=t(sc["opacities"][:P]), shs=t(sc["shs"][:P]), scales=t(sc["scales"][:P]),
                  rotations=t(sc["rotations"][:P]))
        wmax = _zeros(P)
        out = contrib.contributions(st, masks=masks, wmax=wmax, **kw)
        torch.cuda.synchronize()
        assert out["alpha"].shape == (H, W) and not out["alpha"].any() and not out["median_depth"].any() and not out["id_weight"].any()
        assert (out["ids"] == -1).all() and out["ids"].dtype == torch.int32
        assert out["acc"].shape == (P, 3) and not out["acc"].any() and not wmax.any()
        assert not (out["radii"] > 0).any()


def test_accumulation_and_grouping(oracle_lib):
    import contrib
    import diff_gaussian_rasterization as dgr
    r = _reference("chunks")
    sc, masks, W, H, P = r["scene"], r["masks"], r["W"], r["H"], r["P"]
    fwd = _forward(sc)
    one, two = _zeros(P, 4), _zeros(P, 4)
    _pass(sc, fwd, masks[:3], one, None, pixel=False)
    _pass(sc, fwd, masks[:3], two, None, pixel=False)
    _pass(sc, fwd, masks[:3], two, None, pixel=False)
    _bar(_np(two), 2.0 * _np(one).astype(np.float64), "two calls into one acc")
    # a pre-filled wmax is never lowered, and is raised where the view's weight is larger
    clean, pre = _zeros(P), torch.full((P,), 0.25, device=DEV)
    _pass(sc, fwd, None, None, clean, pixel=False)
    _pass(sc, fwd, None, None, pre, pixel=False)
    assert torch.equal(pre, torch.clamp_min(clean, 0.25)) and (clean > 0.25).any() and (clean < 0.25).any()
    # nine masks through the wrapper's grouping against nine K = 1 calls; the weight total is added once
    t = lambda x: x.to(DEV)
    st = dgr.GaussianRasterizationSettings(H, W, sc["tanfovx"], sc["tanfovy"], t(sc["bg"]), 1.0, t(sc["viewmatrix"]), t(sc["projmatrix"]),
                                           3, t(sc["campos"]), False, False)
    kw = dict(means3D=t(sc["means3D"]), opacities=t(sc["opacities"]), shs=t(sc["shs"]), scales=t(sc["scales"]), rotations=t(sc["rotations"]))
    nine = np.concatenate([masks, masks[1:3] * masks[3]])
    assert len(nine) == 9
    out = contrib.contributions(st, masks=torch.from_numpy(nine > 0.5).to(DEV), **kw)          # bool masks: converted to float32
    hard = (nine > 0.5).astype(np.float32)
    single = np.zeros((P, 10))
    for k in range(9):
        a = _zeros(P, 2)
        _pass(sc, fwd, hard[k:k + 1], a, None, pixel=False)
        single[:, k] = _np(a)[:, 0]
        single[:, 9] = _np(a)[:, 1]
    assert out["acc"].shape == (P, 10)
    _bar(_np(out["acc"]), single, "nine masks in groups of seven")
    assert out["ids"].shape == (H, W) and out["wmax"] is None
    u8 = contrib.contributions(st, masks=torch.from_numpy((nine[:2] > 0.5).astype(np.uint8)).to(DEV), pixel_outputs=False, **kw)
    assert u8["alpha"] is None
    _bar(_np(u8["acc"]), single[:, [0, 1, 9]], "uint8 masks")


@pytest.mark.parametrize("name", ["chunks", "heavy_tail_round"])
def test_culled_and_reference_lists_agree(name, option, oracle_lib):
    r = _reference(name)
    sc, masks, P = r["scene"], r["masks"], r["P"]
    res = []
    for cull in (0, 1):
        option("tile_cull", cull)
        fwd = _forward(sc)
        acc, wmax = _zeros(P, 4), _zeros(P)
        pix = [_np(t) for t in _pass(sc, fwd, masks[:3], acc, wmax)]
        res.append((pix, _np(acc), _np(wmax)))
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(res[0][2], res[1][2])
    _bar(res[1][1], res[0][1].astype(np.float64), f"{name}: acc on the culled lists against the reference's lists")


def test_tile_bands(oracle_lib):
    from diff_gaussian_rasterization import _C
    r = _reference("chunks")
    sc, masks, W, H, P = r["scene"], r["masks"], r["W"], r["H"], r["P"]
    gy = (H + 15) // 16
    fwd = _forward(sc)
    acc_full, wmax_full = _zeros(P, 4), _zeros(P)
    full = [_np(t) for t in _pass(sc, fwd, masks[:3], acc_full, wmax_full)]
    acc_sum, wmax_band = np.zeros((P, 4)), _zeros(P)
    try:
        for r0, r1 in ((0, 2), (2, gy)):
            _C.set_tile_band(r0, r1)
            fb = _forward(sc)
            acc = _zeros(P, 4)
            pix = [_np(t) for t in _pass(sc, fb, masks[:3], acc, wmax_band)]
            y0, y1 = r0 * 16, min(H, r1 * 16)
            inside = np.zeros(H, bool)
            inside[y0:y1] = True
            for a, b in zip(pix, full):
                assert np.array_equal(a[inside], b[inside])
            alpha, median, ids, idw = pix
            assert not alpha[~inside].any() and (ids[~inside] == -1).all() and not idw[~inside].any() and not median[~inside].any()
            acc_sum += _np(acc)
    finally:
        _C.set_tile_band(0, 0)
    _bar(acc_sum, _np(acc_full).astype(np.float64), "the bands' acc against the whole view's")
    assert torch.equal(wmax_band, wmax_full)


# ---------------------------------------------------------------- MaskLifter: several views of one model

class _Model:
    def __init__(self, sc):
        t = lambda x: x.to(DEV).clone()
        self.active_sh_degree, self.max_sh_degree = sc["sh_degree"], 3
        self.get_xyz, self.get_opacity = t(sc["means3D"]), t(sc["opacities"])
        self.get_scaling, self.get_rotation = t(sc["scales"]), t(sc["rotations"])
        self.get_features = t(sc["shs"])
        self.get_semantic_feature = torch.zeros(sc["P"], 1, 0, device=DEV)


def _camera(cam):
    c = types.SimpleNamespace()
    c.FoVx, c.FoVy = 2 * math.atan(cam["tanfovx"]), 2 * math.atan(cam["tanfovy"])
    c.image_height, c.image_width = cam["image_height"], cam["image_width"]
    c.world_view_transform, c.full_proj_transform = cam["viewmatrix"].to(DEV), cam["projmatrix"].to(DEV)
    c.camera_center = cam["campos"].to(DEV)
    return c


# the dense scene here is the 3000-Gaussian one (100 x 70, lists of several chunks): at the 2500 large splats of 64 x 64 most
# Gaussians cover several cells of the checker and 7 % of the ratios lie within 2e-3 of 0.5 - by the judge alone
@pytest.mark.parametrize("name", ["opacity01", "chunks"])
def test_mask_lifter_over_three_views(name, oracle_lib):
    import contrib
    import edit
    from oracle.oracle import Oracle, scene_kwargs
    sc = CASES[name]()
    W, H, P = sc["image_width"], sc["image_height"], sc["P"]
    y, x = np.mgrid[0:H, 0:W]
    checker = ((x // 5 + y // 3) & 1).astype(np.float32)
    masks = np.stack([checker, 1 - checker])
    views = [dict(yaw=0.0, pitch=0.0, roll=0.0, campos=(0.0, 0.0, 0.0)), dict(yaw=6.0, pitch=-3.0, roll=10.0, campos=(0.3, -0.2, -0.5)),
             dict(yaw=-8.0, pitch=4.0, roll=-5.0, campos=(-0.4, 0.1, 0.4))]
    lifter = contrib.MaskLifter(P, 2, DEV)
    pc = _Model(sc)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = sc["bg"].to(DEV)
    judge = np.zeros((P, 3))
    for v in views:
        cam = general_camera(W, H, **v)
        for k in ("R", "t", "fovx", "fovy"):
            cam.pop(k)
        view = _camera(cam)
        out = lifter.add_view(view, pc, pipe, bg, torch.from_numpy(masks).to(DEV))
        assert out["alpha"] is None and out["render"].shape == (3, H, W)
        so = dict(sc, **cam)
        so["tanfovx"], so["tanfovy"] = math.tan(view.FoVx * 0.5), math.tan(view.FoVy * 0.5)      # as render() forms them
        o = Oracle()
        o.forward(**scene_kwargs(so))
        judge += co.walk(co.oracle_state(o), W, H, masks)["acc"]
    torch.cuda.synchronize()
    assert lifter.views == 3
    den = judge[:, 2]
    want = np.where(den[:, None] > 0, judge[:, :2] / np.maximum(den[:, None], 1e-300), 0.0)
    got = _np(lifter.ratios()).astype(np.float64)
    seen = den > 0
    assert np.array_equal(_np(lifter.seen()), seen) and seen.sum() > P // 4
    e = np.abs(got - want).max()
    print(f"{name}: worst |ratio - judge| = {e:.2e} over {int(seen.sum())} seen Gaussians")
    assert e <= 2e-3
    near = np.abs(want - 0.5) <= 2e-3
    n_near = int((near.any(1) & seen).sum())
    print(f"{name}: {n_near} Gaussians with a ratio within 2e-3 of 0.5")
    assert n_near <= 0.01 * seen.sum()
    sel = _np(lifter.select(0.5))
    assert sel.dtype == bool and sel.shape == (P, 2)
    assert np.array_equal(sel[~near], ((want >= 0.5) & seen[:, None])[~near])
    lab, top = _np(lifter.labels()), np.sort(judge[:, :2], 1)
    clear = seen & (top[:, 1] - top[:, 0] > 1e-3 * top[:, 1])
    assert lab.dtype == np.int64 and (lab[~seen] == -1).all() and np.array_equal(lab[clear], judge[:, :2].argmax(1)[clear])
    # select() drives the existing edit unchanged
    opacity, before = pc.get_opacity.clone(), pc.get_opacity.clone()
    edit.apply_edit(opacity, pc.get_features, lifter.select(0.5)[:, 0], {"deletion": True})
    gone = lifter.select(0.5)[:, 0]
    assert gone.any() and not opacity[gone].any() and torch.equal(opacity[~gone], before[~gone])
