"""CPU checks of the PCA colour image: the float64 oracle (tests/feature_pca_oracle.py) against the images the reference's own
feature_visualize_saving returned (tests/golden/reference_feature_pca.npz), the sign rule, a live scikit-learn where there is
one, and the argument errors of feature_pca.py, which are raised before any device work."""
import os
import types

import numpy as np
import pytest
import torch

import feature_pca_oracle as O
from util import ROOT

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "reference_feature_pca.npz"))


@pytest.mark.parametrize("name", O.FIXTURE_CASES)
def test_oracle_reproduces_the_reference_image(name):
    """within 4 x the error recorded when the fixture was made: the oracle is float64, what remains is the reference's own
    rounding (and, for the 512-channel case, its randomized solver)"""
    f = GOLDEN[f"{name}/feature"]
    assert np.array_equal(f, O.make_inputs(name)), "the fixture's input is not the generator's"
    err = np.abs(O.oracle(f, 3).image - GOLDEN[f"{name}/image"].astype(np.float64)).max()
    print(name, "max |oracle - reference|", err, "recorded", float(GOLDEN[f"{name}/e_img"]))
    assert err <= 4 * float(GOLDEN[f"{name}/e_img"])


@pytest.mark.parametrize("name", ["c3_20x31", "c4_1x7", "c20_45x60", "c33_37x53", "c512_12x16"])
def test_components_are_unit_signed_and_ordered(name):
    r = O.oracle(O.make_inputs(name), 3)
    assert np.allclose(np.linalg.norm(r.components, axis=1), 1.0, atol=1e-12)
    for c in r.components:
        assert c[np.argmax(np.abs(c))] > 0
    assert np.all(np.diff(r.eigenvalues) <= 1e-18)
    assert np.allclose(r.cov, r.cov.T, atol=0) and r.lo < r.hi
    assert r.image.min() >= 0 and r.image.max() <= 1


@pytest.mark.parametrize("name", ["c3_20x31", "c16_37x53_zeros", "c20_45x60", "c128_12x16"])
def test_components_match_a_live_scikit_learn(name):
    skd = pytest.importorskip("sklearn.decomposition")
    f = O.make_inputs(name)
    s = O.normalized_pixels(f)[::3]
    pca = skd.PCA(3, random_state=42).fit(s)
    r = O.oracle(f, 3)
    assert np.abs(pca.components_ - r.components).max() <= 1e-5
    assert np.abs(pca.mean_ - r.mean).max() <= 1e-12


def test_zero_pixels_stay_zero_and_the_family_has_them():
    f = O.make_inputs("c16_37x53_zeros")
    flat = f.reshape(16, -1)
    assert all(not flat[:, i].any() for i in O.ZERO_PIXELS)
    assert any(i % 3 == 0 for i in O.ZERO_PIXELS) and any(i % 3 for i in O.ZERO_PIXELS)
    assert not O.normalized_pixels(f)[list(O.ZERO_PIXELS)].any()


def test_argument_errors_are_raised_without_a_gpu():
    import feature_pca as P
    ok = torch.zeros(8, 5, 6)
    fit = P.FeaturePCA(torch.zeros(8), torch.zeros(3, 8), torch.tensor(0.0), torch.tensor(1.0), torch.zeros(3))
    for bad in (torch.zeros(8, 30), torch.zeros(1, 8, 5, 6), ok.double(), ok.half(), np.zeros((8, 5, 6), np.float32)):
        for call in (lambda m: P.fit_feature_pca(m), lambda m: P.apply_feature_pca(m, fit), P.feature_visualize,
                     P.feature_visualize_saving):
            with pytest.raises(ValueError, match="float32 expected"):
                call(bad)
    with pytest.raises(ValueError, match="at least 3"):
        P.fit_feature_pca(torch.zeros(2, 5, 6))
    with pytest.raises(ValueError, match="at least 3"):
        P.apply_feature_pca(torch.zeros(2, 5, 6), fit)
    with pytest.raises(ValueError, match="2 samples"):
        P.fit_feature_pca(torch.zeros(8, 2, 3))                # 6 pixels, stride 3
    with pytest.raises(ValueError, match="2 samples"):
        P.fit_feature_pca(torch.zeros(8, 1, 2), stride=1)
    for stride in (0, -3, 1.5):
        with pytest.raises(ValueError, match="stride"):
            P.fit_feature_pca(ok, stride=stride)
    with pytest.raises(ValueError, match="the map 9 channels"):
        P.apply_feature_pca(torch.zeros(9, 5, 6), fit)
    with pytest.raises(ValueError, match="beyond the limit"):
        P.fit_feature_pca(torch.zeros(P.MAX_CHANNELS + 1, 1, 3), stride=1)


def test_install_sets_the_reference_name():
    import feature_pca as P
    m = types.ModuleType("render")
    assert P.install(m) is m and m.feature_visualize_saving is P.feature_visualize_saving


def test_c_abi_refuses_unsupported_shapes_before_any_launch():
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_feature_pca_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_feature_pca_scratch_bytes.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_int]
    lib.f3dgs_feature_pca_moments.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_int] + [ctypes.c_void_p] * 5
    lib.f3dgs_feature_pca_project.argtypes = [ctypes.c_int, ctypes.c_longlong] + [ctypes.c_void_p] * 7
    UNSUPPORTED, INVALID = -4, -1
    assert lib.f3dgs_feature_pca_moments(2, 100, 3, *([None] * 5)) == UNSUPPORTED and b"at least 3 channels" in lib.f3dgs_last_error()
    assert lib.f3dgs_feature_pca_moments(8, 100, 0, *([None] * 5)) == UNSUPPORTED and b"stride" in lib.f3dgs_last_error()
    assert lib.f3dgs_feature_pca_moments(8, 6, 3, *([None] * 5)) == UNSUPPORTED and b"2 samples" in lib.f3dgs_last_error()
    assert lib.f3dgs_feature_pca_moments(8, 0, 3, *([None] * 5)) == 0                       # HW == 0: a no-op
    assert lib.f3dgs_feature_pca_moments(8, 100, 3, *([None] * 5)) == INVALID and b"null" in lib.f3dgs_last_error()
    assert lib.f3dgs_feature_pca_project(2, 100, *([None] * 7)) == UNSUPPORTED
    assert lib.f3dgs_feature_pca_project(8, 0, *([None] * 7)) == 0
    assert lib.f3dgs_feature_pca_project(8, 100, *([None] * 7)) == INVALID
    # the scratch: the per-sample norms, the partial sums and the float64 partial Gram blocks - far below the map
    for C, HW in ((128, 180 * 240), (512, 360 * 480), (128, 1080 * 1920)):
        b = lib.f3dgs_feature_pca_scratch_bytes(C, HW, 3)
        assert 0 < b <= 0.1 * 4 * C * HW, (C, HW, b)
    assert lib.f3dgs_feature_pca_scratch_bytes(2, 100, 3) == 0
    # the documented bound (include/f3dgs.h), small maps of many channels and the largest supported shape included; 1 KB is
    # the alignment of the five parts
    for C, HW, stride in ((512, 36 * 48, 3), (4096, 9, 1), (4096, 1 << 30, 1), (3, 1 << 30, 1), (128, 90 * 121, 1)):
        n, nb = -(-HW // stride), -(-C // 64)
        pairs = nb * (nb + 1) // 2
        bound = 4 * n + 8 * C * -(-n // 16384) + 12 * C + min(-(-n // 1024), max(1, 1024 // pairs)) * pairs * 32768 + 1024
        assert 0 < lib.f3dgs_feature_pca_scratch_bytes(C, HW, stride) <= bound, (C, HW, stride)


def test_the_channel_limit_is_the_headers():
    import re
    import feature_pca as P
    with open(os.path.join(ROOT, "include", "f3dgs.h")) as fh:
        assert int(re.search(r"#define F3DGS_FEATURE_PCA_MAX_CHANNELS (\d+)", fh.read()).group(1)) == P.MAX_CHANNELS
