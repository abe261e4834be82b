"""GPU tests of the PCA colour image (csrc/feature_pca.hip, feature_pca.py) against the float64 oracle on the host
(tests/feature_pca_oracle.py).  The judge is always that oracle, never the kernels' output.

The bar of every judged quantity is 8 x E, E being the largest error the reference's own float32 chain showed on that quantity
over the fixture cases (tests/golden/reference_feature_pca.npz: e_img for images, e_cov for the covariance over max |cov|,
e_mean for the mean): that chain's error is one realisation of float32 rounding under LAPACK's summation order, a blocked
MFMA order is another, and across cases of equal conditioning the chain's own error scatters by a factor of 7.  Only cases for
which scikit-learn runs an exact solver enter E of the image: for more than 500 channels it picks its randomized solver, whose
error (3e-5 on the fixture's image) is an approximation's, not rounding - leaving it out makes the bar tighter.

One case, c4_1x7, has exactly 3 samples: the covariance has rank 2, its third eigenvector is ANY unit vector of a
two-dimensional null space, and so is the third channel of the image wherever a pixel is not a sample.  The end-to-end test
judges what the samples determine there: channels 0 and 1 everywhere and channel 2 on the sampled pixels.
"""
import os
import types

import numpy as np
import pytest
import torch

import feature_pca_oracle as O
from util import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "reference_feature_pca.npz"))
E_IMG = max(float(GOLDEN[f"{n}/e_img"]) for n in O.FIXTURE_CASES if int(GOLDEN[f"{n}/exact"]))
E_COV = max(float(GOLDEN[f"{n}/e_cov"]) for n in O.FIXTURE_CASES)
E_MEAN = max(float(GOLDEN[f"{n}/e_mean"]) for n in O.FIXTURE_CASES)

# (case, stride)
CASES = [("c3_20x31", 3), ("c4_1x7", 3), ("c20_45x60", 3), ("c32_45x61", 3), ("c33_37x53", 3), ("c128_90x121", 3),
         ("c512_36x48", 3), ("c16_37x53_zeros", 3), ("c20_45x60", 1), ("c128_90x121", 1)]
IDS = [f"{n}-stride{s}" for n, s in CASES]
_cache = {}


def _case(name, stride):
    """(input on the host, input on the device, oracle result): computed once, shared, never modified"""
    if (name, stride) not in _cache:
        f = O.make_inputs(name, stride)
        _cache[(name, stride)] = (f, torch.from_numpy(f).to(DEV), O.oracle(f, stride))
    return _cache[(name, stride)]


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)   # (the oracle's eigenvalues are a reversed view)


@pytest.mark.parametrize("name,stride", CASES, ids=IDS)
def test_moments_against_the_oracle(name, stride):
    from diff_gaussian_rasterization import _C
    f, fd, want = _case(name, stride)
    mean, cov = _C.feature_pca_moments(fd, stride)
    C = f.shape[0]
    assert mean.shape == (C,) and cov.shape == (C, C) and mean.dtype == cov.dtype == torch.float64 and cov.device == fd.device
    cov, mean = cov.cpu().numpy(), mean.cpu().numpy()
    e_cov = np.abs(cov - want.cov).max() / np.abs(want.cov).max()
    e_mean = np.abs(mean - want.mean).max()
    print(f"{name} stride {stride}: e_cov {e_cov:.3e} (bar {8 * E_COV:.3e})  e_mean {e_mean:.3e} (bar {8 * E_MEAN:.3e})")
    assert np.array_equal(cov, cov.T)
    assert e_cov <= 8 * E_COV and e_mean <= 8 * E_MEAN


@pytest.mark.parametrize("name,stride", CASES, ids=IDS)
def test_projection_with_the_oracles_fit(name, stride):
    """apply_feature_pca fed the ORACLE's mean, components, lo and hi: the projection kernel alone"""
    from feature_pca import FeaturePCA, apply_feature_pca
    f, fd, want = _case(name, stride)
    before = fd.clone()
    fit = FeaturePCA(_t(want.mean), _t(want.components), _t(want.lo), _t(want.hi), _t(want.eigenvalues[:3]))
    img = apply_feature_pca(fd, fit)
    assert img.shape == (f.shape[1], f.shape[2], 3) and img.dtype == torch.float32 and img.device == fd.device
    assert torch.equal(fd, before), "the input was modified"
    # the oracle's projection with the fit as the kernel received it (rounded to float32)
    ref = O.project(f, fit.mean.cpu().numpy(), fit.components.cpu().numpy(), float(fit.lo), float(fit.hi))
    got = img.cpu().numpy().astype(np.float64)
    err, err_own = np.abs(got - want.image).max(), np.abs(got - ref).max()
    print(f"{name} stride {stride}: projection e_img {err:.3e} (bar {8 * E_IMG:.3e}), against the float32-rounded fit {err_own:.3e}")
    assert err <= 8 * E_IMG and err_own <= 8 * E_IMG
    assert float(img.min()) >= 0 and float(img.max()) <= 1


@pytest.mark.parametrize("name,stride", CASES, ids=IDS)
def test_feature_visualize_end_to_end(name, stride):
    from feature_pca import feature_visualize
    f, fd, want = _case(name, stride)
    before = fd.clone()
    img = feature_visualize(fd, stride)
    assert img.shape == (f.shape[1], f.shape[2], 3) and img.dtype == torch.float32 and img.device == fd.device
    assert torch.equal(fd, before), "the input was modified"
    assert float(img.min()) >= 0 and float(img.max()) <= 1
    diff = np.abs(img.cpu().numpy().astype(np.float64) - want.image)
    k = O.determined_components(f.shape[0], -(-f.shape[1] * f.shape[2] // stride))
    err = max(diff[..., :k].max(), diff.reshape(-1, 3)[::stride].max())
    print(f"{name} stride {stride}: end-to-end e_img {err:.3e} (bar {8 * E_IMG:.3e}), {k} determined components")
    assert err <= 8 * E_IMG


def test_non_contiguous_input():
    from feature_pca import feature_visualize
    f, fd, want = _case("c20_45x60", 3)
    view = fd.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert not view.is_contiguous()
    assert torch.equal(feature_visualize(view), feature_visualize(fd))


@pytest.mark.parametrize("name", ["c33_37x53", "c128_90x121"])
def test_two_calls_give_identical_bits(name):
    from feature_pca import apply_feature_pca, fit_feature_pca
    _, fd, _ = _case(name, 3)
    a, b = fit_feature_pca(fd), fit_feature_pca(fd)
    for field, x, y in zip(a._fields, a, b):
        assert torch.equal(x, y), field
    assert a.lo.dim() == 0 and a.hi.dim() == 0 and a.lo.device == fd.device and a.mean.dtype == a.components.dtype == torch.float32
    assert a.components.shape == (3, fd.shape[0]) and a.explained_variance.shape == (3,)
    assert torch.equal(apply_feature_pca(fd, a), apply_feature_pca(fd, a))


def test_one_fit_applied_to_a_second_view():
    """fit on one map, apply to a second map of the same family: the oracle's projection of the second map with the first
    map's (oracle) fit"""
    from feature_pca import apply_feature_pca, fit_feature_pca
    f1, fd1, want1 = _case("c20_45x60", 3)
    f2, fd2, _ = _case("c20_45x60_second_view", 3)
    fit = fit_feature_pca(fd1)
    img = apply_feature_pca(fd2, fit)
    ref = O.project(f2, want1.mean, want1.components, want1.lo, want1.hi)
    err = np.abs(img.cpu().numpy().astype(np.float64) - ref).max()
    print(f"second view: e_img {err:.3e} (bar {8 * E_IMG:.3e}); clamped share {float(((ref == 0) | (ref == 1)).mean()):.3f}")
    assert err <= 8 * E_IMG
    ev = fit.explained_variance.cpu().numpy()
    assert np.abs(ev - want1.eigenvalues[:3]).max() <= 8 * E_COV * np.abs(want1.cov).max() * f1.shape[0]


def test_drop_in_name_returns_a_cpu_tensor():
    import feature_pca as P
    f, fd, want = _case("c16_37x53_zeros", 3)
    img = P.feature_visualize_saving(fd)
    assert img.device.type == "cpu" and img.dtype == torch.float32 and img.shape == (37, 53, 3)
    assert np.abs(img.numpy().astype(np.float64) - want.image).max() <= 8 * E_IMG
    from diff_gaussian_rasterization import _C
    assert _C.FEATURE_PCA_MAX_CHANNELS == P.MAX_CHANNELS
    m = types.ModuleType("render")
    P.install(m)
    assert m.feature_visualize_saving is P.feature_visualize_saving


def test_the_map_is_never_copied():
    """128 x 180 x 240: the peak extra allocation during feature_visualize is at most a quarter of the map's bytes - any
    normalised or permuted copy of the map would be four quarters"""
    from feature_pca import feature_visualize
    f, fd, want = _case("c128_180x240", 3)
    feature_visualize(fd)                        # (first-call allocations of the runtime and of the solver)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    img = feature_visualize(fd)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak rise {rise} bytes, the map {fd.numel() * 4}")
    assert rise <= fd.numel() * 4 // 4
    assert np.abs(img.cpu().numpy().astype(np.float64) - want.image).max() <= 8 * E_IMG
