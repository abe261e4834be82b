"""GPU parity under general cameras, focal ratios and SH widths (tests/util.py: general_view_scene).

Every other GPU test builds its camera with synth.make_camera: at the world origin, rotated about y only, fx == fy, and
hands the op sixteen SH coefficients.  Here the camera has an arbitrary rotation (no zero or unit entry), sits away from
the origin, has rectangular pixels in views B and C, and `shs` is (P, M, 3) for M in {1, 4, 5, 9, 16} - the generic SH
staging of csrc/preprocess.hip (whole float4 rows for 3 M % 4 == 0, the scalar path otherwise).  The product is held
against the C++ oracle (util._strict_compare) and against the reference's own strict and default builds
(test_gpu_vs_ref._compare) at their bars, unchanged.  Also: mark_visible at the near plane under such views, and tile
grids above 65,536 tiles (a third 8-bit digit of the tile sort, the one-launch sort with three digits).

Shapes: 3000 / 3001 Gaussians at 160 x 96 and 96 x 160 - several tile rows and columns, a ragged last block of the
64-row per-Gaussian backward, landscape and portrait.  Seeds were chosen on the CPU (with the oracle) so that every case
holds the input conditions asserted by util.assert_input_conditions."""
import ctypes
import os

import numpy as np
import pytest
import torch

import refutil as ru
from test_gpu_vs_ref import _compare, _lists_match
from util import ROOT, VIEWS, _strict_compare, assert_input_conditions, precompute_optionals, view_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAND, PORT = (160, 96), (96, 160)


def _scene(case):
    W, H = case["size"]
    sc = view_scene(case["view"], case["P"], case["C"], W, H, case["seed"], M=case.get("M", 16), sh_degree=case.get("D"),
                    with_depth_grad=case.get("depth", False), scale_lo=0.005, scale_hi=0.08, wide_scale=6.0)
    if "mod" in case:
        sc["scale_modifier"] = case["mod"]
    return precompute_optionals(sc)


# ---- a. product against the C++ oracle --------------------------------------------------------------------------------
ORACLE_CASES = [
    dict(id="A-C16", view="A", P=3000, C=16, size=LAND, seed=1),
    dict(id="B-C16", view="B", P=3001, C=16, size=PORT, seed=2),
    dict(id="C-C16", view="C", P=3001, C=16, size=LAND, seed=2),
    dict(id="D-C16", view="D", P=3000, C=16, size=PORT, seed=8),
    dict(id="B-C0", view="B", P=3000, C=0, size=LAND, seed=2),
    dict(id="C-precomp-color", view="C", P=3001, C=16, size=PORT, seed=4, pc=True),
    dict(id="C-precomp-cov", view="C", P=3000, C=16, size=LAND, seed=3, pv=True),
    dict(id="A-scale0.7", view="A", P=3001, C=16, size=PORT, seed=3, mod=0.7),
]
# ---- c. SH widths (M, D): view A at P = 3001, view E at (1, 0) ---------------------------------------------------------
SH_CASES = [dict(id=f"{v}-M{M}-D{D}", view=v, P=3001, C=16, size=size, seed=seed, M=M, D=D)
            for v, M, D, size, seed in (("A", 1, 0, LAND, 1), ("A", 4, 1, PORT, 3), ("A", 4, 0, LAND, 1), ("A", 9, 2, PORT, 4),
                                        ("A", 9, 1, LAND, 5), ("A", 5, 1, PORT, 5), ("A", 16, 3, LAND, 6), ("E", 1, 0, PORT, 2))]
# ---- b. product against the reference's strict and default builds -----------------------------------------------------
REF_CASES = [
    dict(id="A-C16", view="A", P=3001, C=16, size=PORT, seed=2),
    dict(id="B-C16", view="B", P=3000, C=16, size=LAND, seed=7),
    dict(id="C-C16", view="C", P=3000, C=16, size=PORT, seed=2),
    dict(id="D-C16", view="D", P=3001, C=16, size=LAND, seed=7),
    dict(id="C-C32-depthgrad", view="C", P=3001, C=32, size=LAND, seed=8, depth=True),
    dict(id="B-C0-in-C3", view="B", P=3001, C=0, Cref=3, size=PORT, seed=2),
]


def _check_dsh(case, dsh, radii):
    """dL_dsh is (P, M, 3), exactly zero in the coefficients above (D + 1)^2 and in every row of a culled Gaussian."""
    M, D = case.get("M", 16), case.get("D", 3)
    dsh, radii = np.asarray(dsh), np.asarray(radii)
    assert dsh.shape == (case["P"], M, 3), dsh.shape
    used = (D + 1) ** 2
    assert not dsh[:, used:].any(), f"gradient in SH coefficients {used}.. of degree {D}"
    assert not dsh[radii == 0].any(), "SH gradient in the row of a culled Gaussian"
    assert dsh[radii > 0][:, :used].any(axis=(0, 2)).all(), "an SH coefficient of the degree received no gradient at all"


@pytest.mark.parametrize("case", ORACLE_CASES + SH_CASES, ids=lambda c: c["id"])
def test_general_view_vs_oracle(case):
    scene = _scene(case)
    pc, pv = case.get("pc", False), case.get("pv", False)
    rep = {}
    nflip = _strict_compare(scene, pc, pv, report=rep)
    o = rep["oracle"]
    cond = assert_input_conditions(scene, rep["want"]["radii"], o.read("clamped"), case["view"], sh=not pc)
    print(case["id"], "flips", nflip, cond)
    if not pc:
        _check_dsh(case, rep["got_g"]["dL_dsh"], rep["got"]["radii"])


@pytest.mark.parametrize("case", REF_CASES + SH_CASES, ids=lambda c: c["id"])
def test_general_view_vs_reference(case, record_property):
    """Three-way comparison of tests/test_gpu_vs_ref.py (strict bars, projected state per Gaussian, fp64 adjudication of every
    pixel above a bar), every case as an input of the synthetic family: harsh = False, no allowance."""
    scene = _scene(case)
    C_ref = case.get("Cref", case["C"])
    st, g_ref, g_prod = _compare(scene, C_ref, check_state=True, harsh=False, return_grads=True)
    prod = ru.product_module()
    f = ru.raw_forward(prod, scene, ru.device_inputs(scene, case["C"], DEV))
    radii = f[4].cpu().numpy()
    clamped = ru.product_read("clamped", scene, f, np.uint8, 3 * case["P"])
    cond = assert_input_conditions(scene, radii, clamped, case["view"])
    _check_dsh(case, g_prod["dL_dsh"].cpu().numpy(), radii)
    assert g_ref["dL_dsh"].shape == g_prod["dL_dsh"].shape
    for k, v in st.items():
        record_property(k, str(v))
    print(case["id"], cond, st)


# ---- c. a degree the row does not hold ---------------------------------------------------------------------------------
def test_degree_above_the_sh_width_is_an_error():
    """D = 2 needs nine coefficients: with M = 4 the call must fail (F3DGS_ERR_INVALID_ARGUMENT) before anything is launched -
    through _C.rasterize_gaussians, through _C.rasterize_gaussians_backward (a state of a valid D = 1 call) and through the C
    ABI.  The SH tensor handed over is a view of a longer one, so that even a call that went ahead would stay inside it."""
    case = dict(view="A", P=200, C=4, size=(64, 48), seed=1, M=4, D=1)
    scene = _scene(case)
    P = case["P"]
    prod = ru.product_module()
    d = ru.device_inputs(scene, 4, DEV)
    room = torch.zeros(P + 8, 4, 3, device=DEV)
    room[:P] = d["shs"]
    d["shs"] = room[:P]
    fwd = ru.raw_forward(prod, scene, d)
    g = ru.raw_backward(prod, scene, d, fwd)
    assert g["dL_dsh"].shape == (P, 4, 3)
    bad = dict(scene, sh_degree=2)
    with pytest.raises(RuntimeError, match="SH degree 2 needs 9 coefficients, M = 4"):
        ru.raw_forward(prod, bad, d)
    with pytest.raises(RuntimeError, match="SH degree 2 needs 9 coefficients, M = 4"):
        ru.raw_backward(prod, bad, d, fwd)
    with pytest.raises(RuntimeError, match="SH degree 4 needs 25"):
        ru.raw_forward(prod, dict(scene, sh_degree=4), d)
    # the C ABI: every pointer valid, outputs pre-filled - the error comes back and nothing was written
    lib = ru._lib()
    hook_t = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
    held = []

    def resize(_ctx, nbytes):
        held.append(torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=DEV))
        return held[-1].data_ptr()
    hook = hook_t(resize)
    W, H = scene["image_width"], scene["image_height"]
    out_color = torch.full((3, H, W), -7.0, device=DEV)
    out_feat = torch.full((4, H, W), -7.0, device=DEV)
    out_depth = torch.full((1, H, W), -7.0, device=DEV)
    radii = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    n = ctypes.c_int(-1)
    vp, fl, it = ctypes.c_void_p, ctypes.c_float, ctypes.c_int
    lib.f3dgs_forward.restype = ctypes.c_int
    lib.f3dgs_forward.argtypes = ([hook_t, vp] * 3 + [it] * 4 + [vp, it, it] + [vp] * 6 + [fl] + [vp] * 5 + [fl, fl, it] + [vp] * 4
                                  + [it, vp, ctypes.POINTER(ctypes.c_int)])
    p = lambda t: t.data_ptr()
    torch.cuda.synchronize()

    def call(D):
        return lib.f3dgs_forward(hook, None, hook, None, hook, None, P, D, 4, 4, p(d["bg"]), W, H, p(d["means3D"]), p(d["shs"]), None,
                                 p(d["semantic_feature"]), p(d["opacities"]), p(d["scales"]), 1.0, p(d["rotations"]), None,
                                 p(d["viewmatrix"]), p(d["projmatrix"]), p(d["campos"]), scene["tanfovx"], scene["tanfovy"], 0,
                                 p(out_color), p(out_feat), p(out_depth), p(radii), 0, None, ctypes.byref(n))
    rc = call(2)
    torch.cuda.synchronize()
    assert rc == -1, rc                                           # F3DGS_ERR_INVALID_ARGUMENT (include/f3dgs.h)
    assert b"SH degree 2 needs 9 coefficients, M = 4" in lib.f3dgs_last_error()
    assert not held and n.value == 0
    assert bool((out_color == -7).all()) and bool((out_feat == -7).all()) and bool((out_depth == -7).all()) and bool((radii == -7).all())
    # the same call with the degree the row holds goes through (on the null stream) and gives the binding's image
    assert call(1) == 0, lib.f3dgs_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out_color, fwd[1]) and torch.equal(radii, fwd[4]) and n.value == int(fwd[0])


# ---- d. mark_visible ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["A", "C"])
def test_mark_visible_at_the_near_plane_under_general_views(view, oracle_lib):
    """50,000 points, 5 % of them within +-1e-3 of z_view = 0.2 (placed in fp64 in the camera frame, carried to the world frame,
    rounded to fp32): the product, the reference module and the oracle agree on every one."""
    P, W, H = 50000, 64, 64
    scene = view_scene(view, P, 16, W, H, seed=4)
    g = torch.Generator().manual_seed(99)
    n = P // 20
    view64 = scene["viewmatrix"].double().numpy()
    R, t = view64[:3, :3].T, view64[3, :3]
    cam = np.stack([(torch.rand(n, generator=g, dtype=torch.float64).numpy() - 0.5) * 0.4,
                    (torch.rand(n, generator=g, dtype=torch.float64).numpy() - 0.5) * 0.4,
                    0.2 + (torch.rand(n, generator=g, dtype=torch.float64).numpy() * 2 - 1) * 1e-3], 1)
    m = scene["means3D"].clone()
    idx = torch.randperm(P, generator=g)[:n]
    m[idx] = torch.from_numpy(((cam - t[None]) @ R).astype(np.float32))
    ref, prod = ru.load_ref(16), ru.product_module()
    md, v, p = m.to(DEV), scene["viewmatrix"].to(DEV), scene["projmatrix"].to(DEV)
    a, b = ref.mark_visible(md, v, p), prod.mark_visible(md, v, p)
    want = torch.from_numpy(oracle_lib.mark_visible(m, scene["viewmatrix"]))
    assert a.dtype == b.dtype == torch.bool
    assert torch.equal(a, b) and torch.equal(b.cpu(), want)
    near = b.cpu()[idx]
    assert 0.2 < float(near.float().mean()) < 0.8, "the points placed at the near plane fall on both sides of it"
    assert int((~b).sum()) > n // 5


# ---- e. tile grids above 65,536 tiles ----------------------------------------------------------------------------------
@pytest.mark.parametrize("P,short", [(3000, True), (30000, False)], ids=["one-launch-sort", "three-pass-sort"])
def test_tile_grid_above_65536_tiles(P, short, option):
    """8208 x 4112 pixels = 513 x 257 = 131,841 tiles: tile ids take a third 8-bit digit.  A list of at most 16,384 entries is
    sorted by the one-launch LDS sort with three digits, a longer one by three three-kernel passes; option sort_onesweep is
    refused for such a grid (the call takes the three-kernel flavour).  Instance list and tile ranges bit-identical to the
    reference's (C = 3 build, RGB-only scene); images and radii the same with sort_onesweep = 1 and with tile culling on."""
    from synth import make_scene
    W, H = 8208, 4112
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert gx * gy == 131841
    scene = make_scene(P=P, C=0, width=W, height=H, seed=11, scale_lo=1e-4, scale_hi=1e-3)
    option("tile_cull", 0)
    _lists_match(scene, P, W, H, 3)
    prod = ru.product_module()
    d = ru.device_inputs(scene, 0, DEV)
    f0 = ru.raw_forward(prod, scene, d)
    count = int(ru.product_read("counters", scene, f0, np.uint32, 16)[0])
    assert count == int(f0[0])                                    # culling off: our list is the reference's
    assert (count <= 16384) if short else (count > 16384), count
    rg = ru.product_read("ranges", scene, f0, np.uint32, 2 * gx * gy).reshape(-1, 2)
    high = rg[65536:]
    n_high = int((high[:, 1] > high[:, 0]).sum())
    assert n_high > 100, "no list entries in tiles with bit 16 of the id set"
    assert 0.3 < float((high[:, 1] - high[:, 0])[high[:, 1] > high[:, 0]].sum()) / count < 0.7
    keep = [f0[i].clone() for i in (1, 3, 4)]
    del f0
    for name, value in (("sort_onesweep", 1), ("tile_cull", 1)):
        option(name, value)
        f = ru.raw_forward(prod, scene, d)
        for a, i in zip(keep, (1, 3, 4)):
            assert torch.equal(a, f[i]), (name, i)
        del f
    torch.cuda.empty_cache()
