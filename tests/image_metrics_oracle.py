"""fp64 oracle of the image metrics (feature-3dgs_amd/image_metrics.py, csrc/image_metrics.hip): per image of an (N,C,H,W)
batch the mean |x - y|, the mean (x - y)^2, the mean SSIM and PSNR.

The SSIM map is the one of tests/image_loss_oracle.py (`window2d`, `maps`: the reference's fp32 window widened to fp64, the
11x11 stencil as 121 shifted multiply-adds).  PSNR is formed from the fp32-ROUNDED mse, as the kernel and the reference
(utils/image_utils.py:23-25 on fp32 tensors) form it, but evaluated in fp64: 20 log10(1 / sqrt(float32(mse))).

The quantiser - what `mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)` of torchvision's save_image makes of an fp32 value -
is restated in exact integer arithmetic on the bits of the fp32 value: the product with 255 and the sum with 0.5 are formed
exactly as integers (in units of 2^-40) and each is rounded to 24 significant bits, ties to even, as the two fp32 operations
round.  A NaN gives `NAN_BYTE`, the value tests/golden/reference_image_metrics.npz pins for torch's cast on the CPU."""
import numpy as np
import torch

from image_loss_oracle import maps, window2d

NAN_BYTE = 0            # pinned by the fixture (key "nan_byte"); tests/test_image_metrics_cpu.py compares the two
_SCALE = 40             # integers below are in units of 2^-40


def _round24(p: np.ndarray) -> np.ndarray:
    """Non-negative int64 values rounded to 24 significant bits, ties to even."""
    length = np.frexp(p.astype(np.float64))[1].astype(np.int64)          # bit length (p < 2^53: exact in fp64); 0 for p == 0
    d = np.maximum(length - 24, 0)
    q = p >> d
    rem = p - (q << d)
    half = (np.int64(1) << d) >> 1
    up = (d > 0) & ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    return (q + up.astype(np.int64)) << d


def quantize_u8(v: torch.Tensor) -> torch.Tensor:
    """uint8 tensor of floor(clamp(fl(fl(v * 255) + 0.5), 0, 255)) for an fp32 tensor v, in integer arithmetic."""
    a = v.detach().cpu().contiguous().numpy().astype(np.float32)
    bits = a.view(np.uint32).astype(np.int64)
    neg = (bits >> 31) == 1
    expo = (bits >> 23) & 0xFF
    frac = bits & 0x7FFFFF
    out = np.zeros(a.shape, np.int64)
    nan = (expo == 255) & (frac != 0)
    # |v| >= 2 (infinities included): the clamp decides.  |v| < 2^-10: v * 255 + 0.5 lies in (0.25, 0.75).
    big = (expo >= 128) & ~nan
    out[big & ~neg] = 255
    mid = (expo >= 117) & (expo < 128)
    m = (frac[mid] | 0x800000)                                # 24-bit significand; v = m 2^(expo - 150)
    val = m << (expo[mid] - 150 + _SCALE)                     # shift 7 .. 17: below 2^41
    prod = _round24(val * 255)                                # fl(v * 255), below 2^49
    s = np.where(neg[mid], -prod, prod) + (np.int64(1) << (_SCALE - 1))
    s = _round24(np.maximum(s, 0))                            # fl(. + 0.5); a negative sum clamps to 0 either way
    s = np.minimum(s, np.int64(255) << _SCALE)
    out[mid] = s >> _SCALE
    out[nan] = NAN_BYTE
    return torch.from_numpy(out.astype(np.uint8))


def side_values(t: torch.Tensor, quantize: bool = False, channels_last: bool = False) -> torch.Tensor:
    """The (N,C,H,W) fp64 values the kernel reads of one side: the fp32 quotient v / 255 of an 8-bit value."""
    t = t.detach().cpu()
    if t.dim() == 3:
        t = t[None]
    if t.dtype == torch.uint8:
        assert not quantize
        if channels_last:
            t = t.permute(0, 3, 1, 2)
        return t.to(torch.float32).div(255).to(torch.float64)
    assert t.dtype == torch.float32 and not channels_last
    if quantize:
        return quantize_u8(t).to(torch.float32).div(255).to(torch.float64)
    return t.to(torch.float64)


def psnr_of_mse(mse: torch.Tensor) -> torch.Tensor:
    m32 = mse.to(torch.float32).to(torch.float64)
    return 20.0 * torch.log10(1.0 / torch.sqrt(m32))


def metrics(image, gt, quantize=(False, False), channels_last=(False, False)) -> dict:
    """fp64 per-image results: dict of (N,) tensors l1, mse, psnr, ssim."""
    x = side_values(image, quantize[0], channels_last[0])
    y = side_values(gt, quantize[1], channels_last[1])
    assert x.shape == y.shape
    S = maps(x, y, window2d())[0]
    d = x - y
    mse = (d * d).mean(dim=(1, 2, 3))
    return dict(l1=d.abs().mean(dim=(1, 2, 3)), mse=mse, psnr=psnr_of_mse(mse), ssim=S.mean(dim=(1, 2, 3)))
