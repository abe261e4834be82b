"""CPU checks of the fused image loss: the fp64 oracle of the kernels' decomposition (tests/image_loss_oracle.py) against
the reference's own `ssim` / `l1_loss` + autograd (tests/golden/reference_ssim.npz), and the C-ABI entry points' argument
validation (no device work)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import image_loss_oracle as O
from util import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_ssim.npz")


def _cases():
    z = np.load(GOLDEN)
    return sorted({k.split("/")[0] for k in z.files if "/" in k})


@pytest.mark.parametrize("name", _cases())
def test_oracle_matches_the_reference_fixture(name):
    z = np.load(GOLDEN)
    lam = float(z["lambda_dssim"])
    img, gt = torch.from_numpy(z[f"{name}/image"]), torch.from_numpy(z[f"{name}/gt"])
    per_image = f"{name}/ssim_per_image" in z.files
    r = O.image_loss(img, gt, lam, z["upstream_per_image"] if per_image else None)
    for k in ("loss", "l1", "ssim"):
        want = float(z[f"{name}/{k}"])
        assert abs(float(r[k]) - want) <= 1e-9 * abs(want) + 1e-300, (k, float(r[k]), want)
    n = img.numel()
    for k in ("grad_loss", "grad_ssim", "ssim_per_image", "grad_ssim_per_image"):
        if f"{name}/{k}" not in z.files:
            continue
        want = z[f"{name}/{k}"]
        # relative to the largest element; where the gradient vanishes (identical images) relative to the loss's natural
        # gradient scale 1/n instead
        scale = max(np.abs(want).max(), 1.0 / n if k.startswith("grad") else 0.0)
        err = np.abs(r[k].numpy() - want).max()
        assert err <= 1e-9 * scale, (k, err, scale)


def test_fixture_covers_the_issue_shapes():
    z = np.load(GOLDEN)
    shapes = {tuple(z[f"{c}/image"].shape) for c in _cases()}
    assert {(1, 3, 37, 53), (2, 3, 8, 6), (1, 1, 1, 1), (1, 3, 4, 7), (3, 20, 30)} <= shapes
    assert "batch_2x3x8x6/grad_ssim_per_image" in z.files
    assert os.path.getsize(GOLDEN) < 256 * 1024


def _lib():
    so = os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(so)
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_image_loss_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_image_loss_scratch_bytes.argtypes = [ctypes.c_int] * 5
    lib.f3dgs_image_loss_forward.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2 + [ctypes.c_float, ctypes.c_int] + \
        [ctypes.c_void_p] * 6
    lib.f3dgs_image_loss_backward.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2 + [ctypes.c_float, ctypes.c_int] + \
        [ctypes.c_void_p] * 4
    return lib


def test_c_abi_image_loss_rejects_bad_arguments():
    lib = _lib()
    dummy = (ctypes.c_float * 64)()
    p = ctypes.addressof(dummy)
    # scratch: partial sums, plus three maps with want_grad
    assert lib.f3dgs_image_loss_scratch_bytes(1, 3, 8, 8, 1) >= 3 * 3 * 64 * 4 + 2 * 4
    assert lib.f3dgs_image_loss_scratch_bytes(1, 3, 8, 8, 0) < lib.f3dgs_image_loss_scratch_bytes(1, 3, 8, 8, 1)
    assert lib.f3dgs_image_loss_scratch_bytes(0, 3, 8, 8, 1) == 0
    for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1)):
        assert lib.f3dgs_image_loss_forward(*dims, p, p, 0.2, 1, p, p, p, None, p, None) < 0
        assert b"bad sizes" in lib.f3dgs_last_error()
        assert lib.f3dgs_image_loss_backward(*dims, p, p, 0.2, 0, p, p, p, None) < 0
        assert b"bad sizes" in lib.f3dgs_last_error()
    for k in range(6):          # image, gt, loss, l1, ssim, scratch
        args = [p] * 6
        args[k] = None
        assert lib.f3dgs_image_loss_forward(1, 3, 8, 8, args[0], args[1], 0.2, 1, args[2], args[3], args[4], None, args[5],
                                            None) < 0
        assert b"null" in lib.f3dgs_last_error()
    for k in range(5):          # image, gt, upstream, scratch, d_image
        args = [p] * 5
        args[k] = None
        assert lib.f3dgs_image_loss_backward(1, 3, 8, 8, args[0], args[1], 0.2, 0, args[2], args[3], args[4], None) < 0
        assert b"null" in lib.f3dgs_last_error()
    assert lib.f3dgs_image_loss_backward(1, 3, 8, 8, p, p, 0.2, 7, p, p, p, None) < 0
    assert b"unknown mode" in lib.f3dgs_last_error()


def test_public_surface_refuses_what_it_does_not_build():
    """Argument errors raised before any device work."""
    from image_loss import fused_l1_dssim, fused_ssim
    a, b = torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8)
    with pytest.raises(ValueError, match="window_size"):
        fused_ssim(a, b, window_size=7)
    with pytest.raises(ValueError, match="ground-truth"):
        fused_l1_dssim(a, b.requires_grad_(True))
    with pytest.raises(ValueError, match="size_average=False"):
        fused_ssim(a[0], b[0].detach(), size_average=False)
    with pytest.raises(RuntimeError, match="HIP device"):
        fused_l1_dssim(a, b.detach())
