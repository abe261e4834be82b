"""CPU checks of the image metrics: the fp64 oracle (tests/image_metrics_oracle.py) against the reference's own `ssim`,
`l1_loss`, `mse` and `psnr` (tests/golden/reference_image_metrics.npz), its integer quantiser against torch's tensor chain,
the kernel's division-free v / 255 in exact arithmetic, and the argument errors of the C ABI and of the Python surface (no device
work)."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import image_metrics_oracle as O
from util import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_image_metrics.npz")
CASES = ("float", "png", "special", "identical")


def _oracle_of(z, name, route="float"):
    img, gt = torch.from_numpy(z[f"{name}/image"]), torch.from_numpy(z[f"{name}/gt"])
    if name == "png":
        if route == "u8":
            return O.metrics(torch.from_numpy(z["png/image_u8"]), torch.from_numpy(z["png/gt_u8"]), channels_last=(True, True))
        return O.metrics(img, gt, quantize=(True, True))
    if name == "special":
        if route == "u8":
            return O.metrics(torch.from_numpy(z["special/image_u8"]), gt, channels_last=(True, False))
        return O.metrics(img, gt, quantize=(True, False))
    return O.metrics(img, gt)


@pytest.mark.parametrize("name,route", [("float", "float"), ("png", "float"), ("png", "u8"), ("special", "float"), ("special", "u8"),
                                        ("identical", "float")])
def test_oracle_matches_the_reference_fixture(name, route):
    """l1, mse, ssim: fp64 against fp64, 1e-9 relative.  psnr: the oracle rounds the mse to fp32 first (relative 2^-24 = 6e-8,
    i.e. 10 log10(1 + 6e-8) = 2.6e-7 dB) - 1e-6 dB against the reference's fp64 value; the reference's fp32 value adds its own fp32
    sum, sqrt, division and log10, a few ulp of a value below 64 (3.8e-6 each): 2e-5 dB."""
    z = np.load(GOLDEN)
    r = _oracle_of(z, name, route)
    for k in ("l1", "mse", "ssim"):
        want = z[f"{name}/{k}"]
        assert r[k].shape == want.shape
        assert np.all(np.abs(r[k].numpy() - want) <= 1e-9 * np.abs(want) + 1e-300), (k, r[k], want)
    got = r["psnr"].numpy()
    if name == "identical":
        assert np.all(np.isposinf(got)) and np.all(np.isposinf(z[f"{name}/psnr"])) and np.all(np.isposinf(z[f"{name}/psnr_fp32"]))
        assert np.all(r["l1"].numpy() == 0) and np.all(r["mse"].numpy() == 0)
    else:
        assert np.all(np.abs(got - z[f"{name}/psnr"]) <= 1e-6), (got, z[f"{name}/psnr"])
        assert np.all(np.abs(got - z[f"{name}/psnr_fp32"].astype(np.float64)) <= 2e-5), (got, z[f"{name}/psnr_fp32"])


def test_fixture_pins_the_round_trip_and_the_nan_cast():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 64 * 1024
    for k in z.files:
        assert z[k].nbytes <= 8 * 1024, (k, z[k].nbytes)
    assert z["png/image_u8"].shape == (2, 14, 19, 3) and z["png/image_u8"].dtype == np.uint8          # as PIL hands it over
    assert int(z["nan_byte"]) == O.NAN_BYTE
    special = z["special/image"].reshape(-1)
    assert np.isnan(special).sum() == 2 and np.isinf(special).sum() == 2 and (special < 0).any() and (special > 1).any()
    # the oracle's integer quantiser reproduces the bytes of the PNG files and of torch's cast, NaN and infinities included
    for name in ("png", "special"):
        got = O.quantize_u8(torch.from_numpy(z[f"{name}/image"])).permute(0, 2, 3, 1).numpy()
        assert np.array_equal(got, z[f"{name}/image_u8"]), name
    assert np.array_equal(O.quantize_u8(torch.from_numpy(z["png/gt"])).permute(0, 2, 3, 1).numpy(), z["png/gt_u8"])
    assert z["float/psnr_chw_fp32"].shape == (3,)


def _neighbours(v, steps=(-2, -1, 0, 1, 2)):
    v = np.asarray(v, np.float32)
    out = []
    for s in steps:
        w = v.copy()
        for _ in range(abs(s)):
            w = np.nextafter(w, np.float32(np.inf if s > 0 else -np.inf), dtype=np.float32)
        out.append(w)
    return np.concatenate(out)


def test_quantiser_matches_the_tensor_chain():
    """quantize_u8 against `mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)` on every k / 255, on (k +- 0.5) / 255 - where the
    byte changes - with their fp32 neighbours, on negatives and on values above 1."""
    k = np.arange(256, dtype=np.float64)
    exact = (k / 255).astype(np.float32)
    lo, hi = ((k - 0.5) / 255).astype(np.float32), ((k + 0.5) / 255).astype(np.float32)
    fp32_quotient = (torch.arange(256, dtype=torch.float32) / 255).numpy()
    extra = np.array([-1e-3, -0.5 / 255, -0.49 / 255, -1.0, -300.0, 1.0, 1.0001, 1.5, 2.0, 255.0, 1e6, 2 ** -10, 2 ** -11, 1e-30,
                      -1e-30, 3.4e38, -3.4e38, np.inf, -np.inf], np.float32)
    rng = np.random.default_rng(5)
    v = np.concatenate([_neighbours(exact), _neighbours(lo), _neighbours(hi), _neighbours(fp32_quotient), _neighbours(extra[:-2]),
                        extra, rng.uniform(-0.2, 1.2, 4096).astype(np.float32),
                        (rng.integers(0, 512, 4096) / 510).astype(np.float32)])
    t = torch.from_numpy(v)
    want = t.clone().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
    got = O.quantize_u8(t)
    bad = (got != want).nonzero().reshape(-1)
    assert bad.numel() == 0, [(float(v[i]), int(got[i]), int(want[i])) for i in bad[:8]]
    assert got.min() == 0 and got.max() == 255 and len(set(got.tolist())) == 256
    # every byte survives the round trip: quantising k / 255 gives k back
    assert torch.equal(O.quantize_u8(torch.from_numpy(fp32_quotient)), torch.arange(256, dtype=torch.uint8))


def _fp32(fr: Fraction) -> Fraction:
    """fr rounded to fp32 (nearest, ties to even) in exact arithmetic; normal range"""
    if fr == 0:
        return fr
    sign, fr, e = (-1 if fr < 0 else 1), abs(fr), 0
    while fr >= 1 << 24:
        fr, e = fr / 2, e + 1
    while fr < 1 << 23:
        fr, e = fr * 2, e - 1
    n, rem = divmod(fr.numerator, fr.denominator)
    if 2 * rem > fr.denominator or (2 * rem == fr.denominator and n & 1):
        n += 1
    return sign * Fraction(n) * Fraction(2) ** e


def test_division_free_byte_to_unit_is_the_fp32_quotient():
    """csrc/image_metrics.hip widens a byte with q = fl(b r), e = fma(-q, 255, b), fma(e, r, q), r = fl(1 / 255), instead of a
    division per tap.  In exact arithmetic: that is torch's fp32 `b / 255` for all 256 bytes, though the bare product is not."""
    r = _fp32(Fraction(1, 255))
    want = torch.arange(256, dtype=torch.float32).div(255).to(torch.float64).tolist()
    plain_wrong = 0
    for b in range(256):
        q = _fp32(b * r)
        e = _fp32(b - q * 255)
        got = _fp32(q + e * r)
        assert got == Fraction(want[b]), b
        assert got == _fp32(Fraction(b, 255))
        plain_wrong += q != got
    assert plain_wrong > 0


def _lib():
    so = os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(so)
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_image_metrics_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_image_metrics_scratch_bytes.argtypes = [ctypes.c_int] * 4
    lib.f3dgs_image_metrics.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + \
        [ctypes.c_void_p] * 6
    return lib


def test_c_abi_image_metrics_rejects_bad_arguments():
    """Everything here returns before a launch: the addresses are host memory that is never dereferenced."""
    lib = _lib()
    dummy = (ctypes.c_float * 64)()
    p = ctypes.addressof(dummy)
    F32, U8P, U8I = 0, 1, 2
    # three partial sums per 64 x 16 tile
    assert lib.f3dgs_image_metrics_scratch_bytes(1, 3, 8, 8) >= 3 * 3 * 4
    assert lib.f3dgs_image_metrics_scratch_bytes(2, 3, 17, 65) >= 2 * 3 * 2 * 2 * 3 * 4
    assert lib.f3dgs_image_metrics_scratch_bytes(2, 3, 17, 65) < 2 * 3 * 17 * 65          # no per-pixel maps
    for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1), (-1, 3, 8, 8)):
        assert lib.f3dgs_image_metrics_scratch_bytes(*dims) == 0
    call = lambda dims, fx=F32, fy=F32, flags=0, img=p, gt=p, scratch=p: \
        lib.f3dgs_image_metrics(*dims, img, fx, gt, fy, flags, p, p, p, p, scratch, None)
    for dims in ((1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1), (-1, 3, 8, 8), (1, 1 << 20, 1 << 20, 1 << 20)):
        assert call(dims) == -1 and b"bad sizes" in lib.f3dgs_last_error()
    assert call((0, 3, 8, 8)) == 0                                          # N = 0: a no-op
    assert lib.f3dgs_image_metrics(0, 3, 8, 8, None, F32, None, F32, 0, None, None, None, None, None, None) == 0
    for fx, fy in ((3, F32), (F32, -1), (7, 7)):
        assert call((1, 3, 8, 8), fx, fy) == -1 and b"unknown format" in lib.f3dgs_last_error()
    for fx, fy, flags in ((U8P, F32, 1), (F32, U8I, 2), (U8I, U8P, 3), (U8P, F32, 3)):
        assert call((1, 3, 8, 8), fx, fy, flags) == -1 and b"quantize" in lib.f3dgs_last_error()
    assert call((1, 3, 8, 8), flags=4) == -1 and b"unknown flags" in lib.f3dgs_last_error()
    for kw in (dict(img=None), dict(gt=None), dict(scratch=None)):
        assert call((1, 3, 8, 8), **kw) == -1 and b"null" in lib.f3dgs_last_error()
    # no output asked for: nothing to do
    assert lib.f3dgs_image_metrics(1, 3, 8, 8, p, F32, p, F32, 0, None, None, None, None, p, None) == 0
    lib.f3dgs_version.restype = ctypes.c_int
    assert lib.f3dgs_version() >= 31100


def test_python_surface_raises_value_errors_before_any_device_work():
    import image_metrics as M
    a, b = torch.rand(2, 3, 8, 9), torch.rand(2, 3, 8, 9)
    a8, b8 = (a * 255).to(torch.uint8), (b * 255).to(torch.uint8)
    with pytest.raises(ValueError, match="shapes differ"):
        M.image_metrics(a, b[:, :, :, :8])
    with pytest.raises(ValueError, match="shapes differ"):
        M.image_metrics(a8, b8.permute(0, 2, 3, 1))                       # interleaved bytes not declared as such
    with pytest.raises(ValueError, match="float32 or uint8"):
        M.image_metrics(a.double(), b.double())
    with pytest.raises(ValueError, match="float32 or uint8"):
        M.image_metrics(a.half(), b)
    with pytest.raises(ValueError, match="quantize applies to a float32"):
        M.image_metrics(a8, b, quantize=True)
    with pytest.raises(ValueError, match="quantize applies to a float32"):
        M.image_metrics(a, b8, quantize=(False, True))
    with pytest.raises(ValueError, match="channels_last is the layout of a uint8"):
        M.image_metrics(a, b8, channels_last=True)
    with pytest.raises(ValueError, match=r"\(C,H,W\) or \(N,C,H,W\)"):
        M.image_metrics(a[0, 0], b[0, 0])
    with pytest.raises(ValueError, match="pair"):
        M.image_metrics(a, b, quantize=(True, False, True))
    with pytest.raises(ValueError, match="a tensor expected"):
        M.image_metrics(a.numpy(), b)
    # well-formed arguments that live on the host: refused, no CPU path
    for args, kw in (((a, b), {}), ((a, b), dict(quantize=True)), ((a8, b8), {}), ((a8.permute(0, 2, 3, 1), b), dict(channels_last=(True, False)))):
        with pytest.raises(ValueError, match="HIP device"):
            M.image_metrics(*args, **kw)
    with pytest.raises(ValueError, match="HIP device"):
        M.psnr(a, b)
    with pytest.raises(ValueError, match="HIP device"):
        M.ssim(a, b)
    with pytest.raises(ValueError, match="window_size"):
        M.ssim(a, b, window_size=7)
    with pytest.raises(ValueError, match="size_average=False"):
        M.ssim(a[0], b[0], size_average=False)
    with pytest.raises(ValueError, match="2 renders and 1 ground-truth"):
        M.evaluate_views([a[0], a[1]], [b[0]])
    with pytest.raises(ValueError, match="one image per list entry"):
        M.evaluate_views([a], [b])
    with pytest.raises(ValueError, match="HIP device"):
        M.evaluate_views([a[0], a[1]], [b[0], b[1]])
    assert M.evaluate_views([], [])["per_view"] == {"SSIM": [], "PSNR": [], "L1": []}


def test_install_rebinds_only_what_the_module_has():
    import types
    import image_metrics as M
    image_utils, loss_utils = types.ModuleType("utils.image_utils"), types.ModuleType("utils.loss_utils")
    image_utils.psnr = image_utils.mse = lambda a, b: None
    loss_utils.ssim = loss_utils.l1_loss = lambda a, b: None
    keep = loss_utils.l1_loss
    assert M.install(image_utils) is image_utils and image_utils.psnr is M.psnr and not hasattr(image_utils, "ssim")
    assert M.install(loss_utils) is loss_utils and loss_utils.ssim is M.ssim and loss_utils.l1_loss is keep
    assert not hasattr(loss_utils, "psnr")
    with pytest.raises(AttributeError, match="neither psnr nor ssim"):
        M.install(types.ModuleType("something_else"))
