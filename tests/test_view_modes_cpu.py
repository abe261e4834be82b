"""CPU checks of the viewer's render modes: the float64 oracle (tests/view_modes_oracle.py) against what the reference's own
utils.image_utils returned (tests/golden/reference_view_modes.npz), the tap and padding quirks on hand-made inputs, the argument
errors of view_modes.py (raised before any device work) and the new symbols of the library and of `_C`."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import view_modes_oracle as O
from util import ROOT

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "reference_view_modes.npz"))


@pytest.mark.parametrize("name", list(O.DEPTH_CASES))
def test_oracle_against_the_reference_on_depth_cases(name):
    """the fixture's inputs are the generator's; the reference's float32 chain lies as far from the oracle as recorded, and its
    'Depth' frame and matplotlib's jet call index exactly as the oracle does (outside the rounding band)"""
    depth, proj, full = O.make_inputs(name)
    for key, a in (("depth", depth), ("projection_matrix", proj), ("full_proj_transform", full)):
        assert np.array_equal(GOLDEN[f"{name}/{key}"], a), key
    n, c = O.depth_to_normal(depth, proj, full), O.curvature(depth, proj, full)
    assert np.allclose(O.error_stats(GOLDEN[f"{name}/normals"], n, O.clean_footprint(depth, 0, 1)), GOLDEN[f"{name}/e_normals"], rtol=1e-6, atol=1e-12)
    assert np.allclose(O.error_stats(GOLDEN[f"{name}/curvature"], c, O.clean_footprint(depth, 1, 2)), GOLDEN[f"{name}/e_curvature"], rtol=1e-6, atol=1e-12)
    assert not n[-1, -1].any(), "the corner pixel's normal is 0"
    off = GOLDEN[f"{name}/idx_depth"].astype(np.int64) != O.colormap_index(depth)
    assert not (off & ~O.in_band(depth)).any()
    off = GOLDEN[f"{name}/idx_jet"].astype(np.int64) != O.max_index(depth)
    assert not (off & ~O.in_max_band(depth)).any()
    for key, field in (("band_depth", depth), ("band_curvature", c)):
        share = float(O.in_band(field).mean())
        assert share == float(GOLDEN[f"{name}/{key}"]) and share <= O.BAND_CAP


@pytest.mark.parametrize("name", list(O.IMAGE_CASES))
def test_oracle_against_the_reference_on_image_cases(name):
    img = O.make_inputs(name)
    assert np.array_equal(GOLDEN[f"{name}/image"], img)
    want = O.gradient_map(img)
    e = O.error_stats(GOLDEN[f"{name}/edge"], want)
    assert np.allclose(e, GOLDEN[f"{name}/e_edge"], rtol=1e-6, atol=1e-12) and e[2] <= 2e-7
    if f"{name}/idx_edge" in GOLDEN:
        off = GOLDEN[f"{name}/idx_edge"].astype(np.int64) != O.colormap_index(GOLDEN[f"{name}/edge"])
        assert not (off & ~O.in_band(GOLDEN[f"{name}/edge"])).any()


def test_the_fixture_has_both_tables():
    assert GOLDEN["turbo"].shape == GOLDEN["jet"].shape == (256, 3) and GOLDEN["turbo"].dtype == np.float32
    assert len(np.unique(GOLDEN["turbo"], axis=0)) == 256


def test_edge_taps_and_zero_padding_by_hand():
    # one bright pixel in the middle of 3 x 3: gx = taps mirrored, gy likewise
    a = np.zeros((1, 3, 3))
    a[0, 1, 1] = 4.0
    gx = np.array([[1, 0, -1], [2, 0, -2], [1, 0, -1]], float)
    gy = gx.T
    assert np.allclose(O.gradient_map(a), np.sqrt(gx ** 2 + gy ** 2), atol=0)
    # a constant 2 x 2 image: the zero padding makes every pixel a corner; |gx| = |gy| = (2 + 1) c / 4
    c = 0.8
    assert np.allclose(O.gradient_map(np.full((1, 2, 2), c)), np.sqrt(2) * 3 * c / 4)
    # channels add under the root
    assert np.allclose(O.gradient_map(np.full((4, 2, 2), c)), 2 * np.sqrt(2) * 3 * c / 4)
    # a horizontal ramp: gy = 0 inside, gx = (1 + 2 + 1) / 4 times the difference across two pixels = twice the slope
    r = np.tile(np.arange(5.0), (5, 1))[None]
    assert np.allclose(O.gradient_map(r)[1:-1, 1:-1], 2.0)


def test_normals_of_a_fronto_parallel_plane_and_the_padding():
    """identity view, constant depth: interior normals are +-z; the last row / column are computed against the zero vector
    and the corner is exactly 0"""
    P, full = O.make_camera("centred")
    d = np.full((3, 3), 2.0, np.float32)
    n = O.depth_to_normal(d, P, full)
    assert np.allclose(np.abs(n[:2, :2, 2]), 1.0, atol=1e-6) and np.allclose(n[:2, :2, :2], 0.0, atol=1e-6)
    assert not n[2, 2].any()
    pw = O.unproject_depth_map(d, P, full)
    assert np.allclose(pw[..., 2], 2.0, atol=1e-6)                       # the unprojection returns the depth it was given
    assert np.allclose(pw[0, 0, :2], -pw[2, 2, :2]) and pw[0, 0, 0] < 0     # pixel INDICES: the outermost pixels sit on the frustum's edge
    assert np.allclose(pw[2, 2, 0], 2.0 * np.tan(np.radians(30.0)), rtol=1e-5)
    want = np.cross(-pw[2, 0], pw[2, 1] - pw[2, 0])                       # last row: p2 is the zero vector
    assert np.allclose(n[2, 0], want / (np.linalg.norm(want) + 1e-8))
    # curvature pads the (n + 1) / 2 image with 0, not with 0.5: a flat wall still has a bright frame
    c = O.curvature(np.full((6, 6), 2.0, np.float32), P, full)
    assert c[2, 2] < 1e-6 and c[0, 2] > 0.3


def test_palette_rules_by_hand():
    f = np.array([[0.0, 1.0, 2.0, 255.0]])
    assert O.colormap_index(f).tolist() == [[0, 1, 2, 255]]
    assert O.colormap_index(np.array([[0.0, 0.5, 1.5, 2.5, 255.0]])).tolist() == [[0, 0, 2, 2, 255]]      # halves to even
    assert O.colormap_index(np.full((2, 2), 3.0)).tolist() == [[0, 0], [0, 0]]                             # max == min
    assert O.max_index(np.array([[0.0, 0.5, 0.999, 1.0, -0.1]]), L=256).tolist() == [[0, 128, 255, 255, 0]]
    lut = GOLDEN["jet"]
    img = O.palette(np.array([[0, 255]]), lut)
    assert img.shape == (3, 1, 2) and np.array_equal(img[:, 0, 1], lut[255])
    assert O.to_bytes(np.array([[[1.5]], [[-1.0]], [[0.5]]], np.float32)).tolist() == [[[255, 0, 127]]]


def test_argument_errors_are_raised_without_a_gpu():
    import view_modes as V
    cam = types.SimpleNamespace(projection_matrix=torch.eye(4), full_proj_transform=torch.eye(4))
    ok = torch.ones(1, 5, 6)
    for bad in (ok.double(), ok.half(), np.ones((5, 6), np.float32), None):
        with pytest.raises(ValueError, match="float32 expected"):
            V.depth_to_normal(bad, cam)
        with pytest.raises(ValueError, match="float32"):
            V.gradient_map(bad)
        with pytest.raises(ValueError, match="float32 expected"):
            V.colormap(bad, lut=torch.zeros(256, 3))
    with pytest.raises(ValueError, match=r"\(H, W\) or \(1, H, W\)"):
        V.depth_to_normal(torch.ones(3, 5, 6), cam)
    for shape in ((1, 1, 6), (5, 1), (1, 1)):
        with pytest.raises(ValueError, match="at least 2 rows and 2 columns"):
            V.depth_to_normal(torch.ones(*shape), cam)
    for bad_cam in (types.SimpleNamespace(projection_matrix=torch.eye(4)), types.SimpleNamespace(projection_matrix=torch.eye(3), full_proj_transform=torch.eye(4)),
                    types.SimpleNamespace(projection_matrix=np.eye(4), full_proj_transform=torch.eye(4))):
        with pytest.raises(ValueError, match=r"camera\.(projection_matrix|full_proj_transform)"):
            V.depth_to_normal(ok, bad_cam)
        with pytest.raises(ValueError, match=r"camera\."):
            V.render_net_image({"depth": ok}, list(V.RENDER_MODES), 4, bad_cam)
    with pytest.raises(ValueError, match="C >= 1"):
        V.gradient_map(torch.ones(5, 6))
    with pytest.raises(ValueError, match=r"\(L, 3\)"):
        V.colormap(ok, lut=torch.zeros(256, 4))
    for L in (1, V.MAX_PALETTE + 1):
        with pytest.raises(ValueError, match="entries"):
            V.colormap(ok, lut=torch.zeros(L, 3))
    with pytest.raises(ValueError, match="does not index"):
        V.render_net_image({"depth": ok}, list(V.RENDER_MODES), 9, cam)
    with pytest.raises(ValueError, match="float32 expected"):
        V.net_image_bytes({"depth": ok.double()}, list(V.RENDER_MODES), 1, cam)
    with pytest.raises(ValueError, match="float32 expected"):
        V.render_net_image({"feature_map": torch.zeros(8, 30)}, list(V.RENDER_MODES), 5, cam)
    assert V.RENDER_MODES == ("RGB", "Depth", "Edge", "Normal", "Curvature", "Feature Map")


def test_install_sets_the_reference_names():
    import view_modes as V
    m = types.ModuleType("utils.image_utils")
    assert V.install(m) is m
    for n in ("depth_to_normal", "gradient_map", "colormap", "render_net_image"):
        assert getattr(m, n) is getattr(V, n)


def test_the_limits_are_the_headers():
    import re
    import view_modes as V
    with open(os.path.join(ROOT, "include", "f3dgs.h")) as fh:
        h = fh.read()
    assert int(re.search(r"#define F3DGS_VIEW_PALETTE_MAX_ENTRIES (\d+)", h).group(1)) == V.MAX_PALETTE
    assert int(re.search(r"#define F3DGS_VIEW_TILE (\d+)", h).group(1)) == O.TILE


def test_new_symbols_and_refusals_before_any_launch():
    """fails on a library without the view modes"""
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    for n in ("f3dgs_view_normals", "f3dgs_view_gradient", "f3dgs_view_curvature", "f3dgs_view_minmax", "f3dgs_view_palette", "f3dgs_view_bytes"):
        assert hasattr(lib, n), n
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    P = ctypes.c_void_p
    lib.f3dgs_view_normals.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, P, ctypes.c_int, P]
    lib.f3dgs_view_gradient.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, P, P]
    lib.f3dgs_view_curvature.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, P, P, P]
    lib.f3dgs_view_minmax.argtypes = [ctypes.c_longlong, P, P, P]
    lib.f3dgs_view_palette.argtypes = [ctypes.c_longlong, P, P, P, ctypes.c_int, ctypes.c_int, P, P, P]
    lib.f3dgs_view_bytes.argtypes = [ctypes.c_longlong, P, P, P]
    UNSUPPORTED, INVALID = -4, -1
    for H, W in ((1 << 16, 1 << 15), (1, 8), (8, 1)):
        assert lib.f3dgs_view_normals(H, W, None, None, None, None, 0, None) == UNSUPPORTED, (H, W)
        assert lib.f3dgs_view_curvature(H, W, None, None, None, None, None, None) == UNSUPPORTED, (H, W)
    assert b"2 rows and 2 columns" in lib.f3dgs_last_error()
    assert lib.f3dgs_view_gradient(3, 1 << 16, 1 << 15, None, None, None, None) == UNSUPPORTED
    assert lib.f3dgs_view_gradient(3, 1, 8, None, None, None, None) == INVALID and b"null" in lib.f3dgs_last_error()     # 1 x 8 is served
    assert lib.f3dgs_view_gradient(0, 4, 4, None, None, None, None) == INVALID
    assert lib.f3dgs_view_normals(0, 8, None, None, None, None, 0, None) == 0                    # H * W == 0: a no-op
    assert lib.f3dgs_view_curvature(8, 0, None, None, None, None, None, None) == 0
    assert lib.f3dgs_view_gradient(3, 0, 8, None, None, None, None) == 0
    assert lib.f3dgs_view_minmax(0, None, None, None) == 0 and lib.f3dgs_view_bytes(0, None, None, None) == 0
    assert lib.f3dgs_view_normals(4, 4, None, None, None, None, 0, None) == INVALID
    assert lib.f3dgs_view_normals(4, 4, None, None, None, None, 8, None) == INVALID and b"flag" in lib.f3dgs_last_error()
    for L in (1, 0, 4097):
        assert lib.f3dgs_view_palette(16, None, None, None, L, 0, None, None, None) == UNSUPPORTED and b"entries" in lib.f3dgs_last_error()
    assert lib.f3dgs_view_palette((1 << 30) + 1, None, None, None, 256, 0, None, None, None) == UNSUPPORTED
    assert lib.f3dgs_view_palette(0, None, None, None, 256, 0, None, None, None) == 0
    assert lib.f3dgs_view_palette(16, None, None, None, 256, 2, None, None, None) == INVALID and b"mode" in lib.f3dgs_last_error()
    assert lib.f3dgs_view_palette(16, None, None, None, 256, 1, None, None, None) == INVALID
    assert lib.f3dgs_view_minmax((1 << 30) + 1, None, None, None) == UNSUPPORTED
    from diff_gaussian_rasterization import _C
    for n in ("view_normals", "view_gradient", "view_curvature", "view_minmax", "view_palette", "view_bytes"):
        assert hasattr(_C, n), n
    assert _C.VIEW_TILE == O.TILE and (_C.VIEW_PALETTE_MINMAX, _C.VIEW_PALETTE_MAX) == (0, 1) and _C.VIEW_PALETTE_MAX_ENTRIES == 4096
    with pytest.raises(RuntimeError, match="HIP device"):
        _C.view_gradient(torch.zeros(3, 4, 4))
