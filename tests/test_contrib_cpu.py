"""The contribution pass without a GPU: the float64 judge of tests/contrib_oracle.py pinned to the CPU oracle, the argument
errors of f3dgs_contributions (raised before any device work) and those of the Python wrapper."""
import ctypes
import os

import numpy as np
import pytest
import torch

import contrib_oracle as co
import refutil as ru
from util import ROOT, harsh_scene


def _masks(K, W, H, seed=0):
    """all ones, all zeros, the checker, a half plane cut at x = 21, uniform soft values - cycled to K masks"""
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(seed)
    kinds = [np.ones((H, W)), ((x // 5 + y // 3) & 1).astype(np.float64), (x < 21).astype(np.float64), rng.random((H, W)),
             np.zeros((H, W))]
    return np.stack([kinds[k % len(kinds)] for k in range(K)]).astype(np.float32)


@pytest.mark.parametrize("case", ["synth", "opacity01"])
def test_judge_is_pinned_to_the_oracle(oracle_lib, case):
    """(b) against the oracle itself: 1 - T within 1e-6 of 1 - final_T at every pixel, and the per-Gaussian sums inside the
    project's gradient bar of the oracle's backward (a) with C = K + 1 features, dL_dcolor = 0 and dL_dfeature = [masks; ones]."""
    from synth import make_scene
    from oracle.oracle import Oracle, scene_kwargs
    K = 3
    if case == "synth":
        W, H = 129, 64
        sc = make_scene(P=400, C=K + 1, width=W, height=H, seed=1)
    else:
        W, H = 70, 33
        sc = harsh_scene("opacity01", 1500, K + 1, W, H, seed=2)
    o = Oracle()
    o.forward(**scene_kwargs(sc))
    masks = _masks(K, W, H)
    j = co.walk(co.oracle_state(o), W, H, masks)
    final_T = o.read("final_T").reshape(H, W).astype(np.float64)
    err = np.abs(j["alpha"] - (1.0 - final_T)).max()
    print(f"{case}: max |alpha - (1 - final_T)| = {err:.2e}, borderline {int(j['borderline'].sum())} of {W * H}")
    assert err <= 1e-6
    up = np.concatenate([masks, np.ones((1, H, W), np.float32)])
    g = o.backward(np.zeros((3, H, W), np.float32), up, np.zeros((1, H, W), np.float32))["dL_dsemantic_feature"].reshape(-1, K + 1)
    assert np.abs(g).max() > 0
    mx, worst = ru.grad_errors(g, j["acc"])
    print(f"{case}: oracle backward against the judge: max err / max|g| = {mx:.2e}, worst element {worst:.2f} x the bar")
    assert mx <= 1e-3 and worst <= 1.0
    # the judge's own invariants
    assert (j["ids"] >= 0).sum() == (j["top1"] > 0).sum() and (j["top1"] >= j["top2"]).all()
    assert np.abs(j["acc"][:, K].sum() - j["alpha"].sum()) <= 1e-9 * W * H            # sum of w over a pixel = 1 - T
    assert np.abs(j["acc"][:, 0] - j["acc"][:, K]).max() <= 1e-12          # the all-ones mask
    assert (j["acc"][:, 1] <= j["acc"][:, K] + 1e-12).all()                  # the checker: a part of the total


def _lib():
    import diff_gaussian_rasterization  # noqa: F401  (its bundled HIP runtime must be the one the library binds to)
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    vp = ctypes.c_void_p
    lib.f3dgs_contributions.restype = ctypes.c_int
    lib.f3dgs_contributions.argtypes = [ctypes.c_int] * 4 + [vp] * 3 + [ctypes.c_int] + [vp] * 7 + [vp]
    return lib


def test_argument_errors_before_any_device_work():
    lib = _lib()
    A = 0x10000                 # a never dereferenced address
    call = lambda P, R, W, H, geom, binning, img, K, masks, acc, wmax, alpha, med, ids, idw: lib.f3dgs_contributions(
        P, R, W, H, geom, binning, img, K, masks, acc, wmax, alpha, med, ids, idw, None)
    assert call(-1, 0, 8, 8, A, A, A, 0, None, None, None, A, None, None, None) == -1 and b"P < 0" in lib.f3dgs_last_error()
    assert call(5, 3, 0, 8, A, A, A, 0, None, None, None, A, None, None, None) == -1 and b"sizes" in lib.f3dgs_last_error()
    for K in (-1, 8):
        assert call(5, 3, 8, 8, A, A, A, K, A, A, None, None, None, None, None) == -1 and b"masks" in lib.f3dgs_last_error()
    assert call(5, 3, 8, 8, A, A, A, 2, None, A, None, None, None, None, None) == -1 and b"masks is null" in lib.f3dgs_last_error()
    assert call(5, 3, 8, 8, A, A, A, 2, A, None, A, None, None, None, None) == -1 and b"acc is null" in lib.f3dgs_last_error()
    for geom, binning, img in ((None, A, A), (A, None, A), (A, A, None)):
        assert call(5, 3, 8, 8, geom, binning, img, 0, None, A, None, None, None, None, None) == -1
        assert b"null state buffer" in lib.f3dgs_last_error()
    assert call(5, 3, 8, 8, A, A, A, 0, None, None, None, None, None, None, None) == -1 and b"every output" in lib.f3dgs_last_error()
    assert call(0, 0, 8, 8, None, None, None, 0, None, None, None, None, None, None, None) == -1 and b"every output" in lib.f3dgs_last_error()
    # P = 0 with only per-Gaussian outputs: nothing to do, no device touched
    assert call(0, 0, 8, 8, None, None, None, 0, None, A, A, None, None, None, None) == 0
    lib.f3dgs_version.restype = ctypes.c_int
    assert lib.f3dgs_version() >= 31200


def _settings(sc):
    import diff_gaussian_rasterization as dgr
    return dgr.GaussianRasterizationSettings(sc["image_height"], sc["image_width"], sc["tanfovx"], sc["tanfovy"], sc["bg"], 1.0,
                                             sc["viewmatrix"], sc["projmatrix"], 3, sc["campos"], False, False)


def test_wrapper_errors_and_no_cpu_path():
    import contrib
    from synth import make_scene
    sc = make_scene(50, 0, 32, 24)
    st = _settings(sc)
    kw = dict(means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    with pytest.raises(ValueError, match="HIP device"):
        contrib.contributions(st, **kw)
    with pytest.raises(ValueError, match="HIP device"):
        contrib.MaskLifter(50, 2, "cpu")
    with pytest.raises(ValueError, match=r"\(50, 2\)"):
        contrib.contributions(st, **dict(kw, means3D=sc["means3D"][:, :2]))
    with pytest.raises(ValueError, match="exactly one of shs"):
        contrib.contributions(st, **dict(kw, colors_precomp=torch.zeros(50, 3)))
    with pytest.raises(ValueError, match="scales / rotations"):
        contrib.contributions(st, **dict(kw, cov3D_precomp=torch.zeros(50, 6)))
    with pytest.raises(ValueError, match=r"MaskLifter\(P=5, K=0\)"):
        contrib.MaskLifter(5, 0, "cuda")
    with pytest.raises(ValueError, match=r"\(3, 4\)"):
        contrib.MaskLifter.from_label_map(torch.zeros(3, 4), 2)
    onehot = contrib.MaskLifter.from_label_map(torch.tensor([[0, 1, 2], [1, 1, 5]]), 3)
    assert onehot.shape == (3, 2, 3) and onehot.dtype == torch.float32
    assert torch.equal(onehot.sum(0), torch.tensor([[1.0, 1.0, 1.0], [1.0, 1.0, 0.0]]))
    assert contrib.MAX_MASKS == 7


def test_mask_checks_name_the_shapes():
    """_check_masks / _check_acc answer before the device is touched: exercised directly, since contributions() refuses CPU
    Gaussians first."""
    import contrib
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match=r"masks \(K, 24, 32\) expected, got \(2, 24, 31\)"):
        contrib._check_masks(torch.zeros(2, 24, 31), 24, 32, cpu)
    with pytest.raises(ValueError, match="HIP device"):
        contrib._check_masks(torch.zeros(2, 24, 32), 24, 32, cpu)
    with pytest.raises(ValueError, match="HIP device"):
        contrib._check_acc(torch.zeros(50, 3), None, 50, 2, cpu)
    with pytest.raises(ValueError, match="HIP device"):
        contrib._check_acc(None, torch.zeros(50), 50, 2, cpu)
