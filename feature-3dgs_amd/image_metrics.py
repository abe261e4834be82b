"""Image-quality metrics of rendered views in one pass: L1, MSE, PSNR and SSIM of N view pairs, on the device.

Replaces the image half of the reference's evaluation - metrics.py:71-74

    ssims.append(ssim(renders[idx], gts[idx]))
    psnrs.append(psnr(renders[idx], gts[idx]))

and training_report (train.py:210-239)

    l1_test += l1_loss(image, gt_image).mean().double()
    psnr_test += psnr(image, gt_image).mean().double()

which per view pair run five depthwise 11x11 convolutions, a squared-error pass and a host read, with

    m = image_metrics(renders, gts, quantize=True)        # ImageMetrics(l1, psnr, ssim, mse): (N,) device tensors, no host read
    report = evaluate_views(renders, gts)                 # the SSIM / PSNR / L1 means and per-view lists, one host read
    import utils.image_utils, utils.loss_utils, image_metrics
    image_metrics.install(utils.image_utils); image_metrics.install(utils.loss_utils)    # or: the reference's scripts, fused

Two kernels per call (csrc/image_metrics.hip behind include/f3dgs.h: f3dgs_image_metrics): the windowed moments, SSIM,
|d| and d^2 of every 64 x 16 tile, and a fixed-order fp64 reduction per image that also forms PSNR.  Forward only; the
training loss stays image_loss.py.

metrics.py does not score the float render but the PNG render.py wrote of it.  `quantize=True` applies what that round trip
does to a float value, `floor(clamp(v * 255 + 0.5, 0, 255)) / 255` in torch's fp32 order, as the tile is read, so the
reference's reported numbers come out without the disk.  uint8 tensors - planar (N,C,H,W), or (N,H,W,C) as PIL hands an image
over with `channels_last=True` - are read as they are, value v / 255.  The two sides choose their form independently:
`quantize` and `channels_last` are one bool for both sides or an (image, gt) pair.

LPIPS (metrics.py:74) is lpips_vgg.py's: this repository holds no VGG weights, `evaluate_views(..., lpips_weights=...)` takes the
caller's (lpips_vgg.LpipsWeights) and adds the third number.
HIP only; no CPU fallback; argument errors are raised as ValueError before any device work.
"""
from __future__ import annotations

from collections import namedtuple

import torch

ImageMetrics = namedtuple("ImageMetrics", ["l1", "psnr", "ssim", "mse"])


def _C():
    from diff_gaussian_rasterization import _C as ext
    return ext


def _pair(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what}: one bool, or an (image, gt) pair, expected; got {v!r}")
        return bool(v[0]), bool(v[1])
    return bool(v), bool(v)


def _side(t, name, quantize, channels_last):
    """(4-D tensor in its stored layout, format name, logical (N,C,H,W)) of one side; every check before device work."""
    if not torch.is_tensor(t):
        raise ValueError(f"{name}: a tensor expected, got {type(t).__name__}")
    if t.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{name}: float32 or uint8 expected, got {t.dtype}")
    if t.dim() not in (3, 4):
        raise ValueError(f"{name}: (C,H,W) or (N,C,H,W) expected ((H,W,C) or (N,H,W,C) with channels_last), got {tuple(t.shape)}")
    if t.dtype == torch.uint8 and quantize:
        raise ValueError(f"{name}: quantize applies to a float32 image; a uint8 image holds the 8-bit values already")
    if t.dtype == torch.float32 and channels_last:
        raise ValueError(f"{name}: channels_last is the layout of a uint8 image; a float32 image is (N,C,H,W)")
    t = t.detach()
    if t.dim() == 3:
        t = t[None]
    n, a, b, c = t.shape
    logical = (n, c, a, b) if channels_last else (n, a, b, c)
    if n and min(logical[1:]) < 1:
        raise ValueError(f"{name}: empty image {tuple(t.shape)}")
    fmt = "IMAGE_F32" if t.dtype == torch.float32 else ("IMAGE_U8_INTERLEAVED" if channels_last else "IMAGE_U8_PLANAR")
    return t, fmt, logical


def _prepare(image, gt, quantize, channels_last):
    q, cl = _pair(quantize, "quantize"), _pair(channels_last, "channels_last")
    x, fx, sx = _side(image, "image", q[0], cl[0])
    y, fy, sy = _side(gt, "gt", q[1], cl[1])
    if sx != sy:
        raise ValueError(f"image (N,C,H,W) = {sx} and gt (N,C,H,W) = {sy} shapes differ")
    for name, t in (("image", x), ("gt", y)):          # last, so that every other error can be met without a device
        if t.device.type != "cuda":
            raise ValueError(f"{name} lives on {t.device}: the metrics run on a HIP device only (no CPU path)")
    if x.device != y.device:
        raise ValueError(f"image is on {x.device}, gt on {y.device}")
    return x, fx, y, fy, q


def _run(image, gt, quantize, channels_last, want_ssim):
    x, fx, y, fy, q = _prepare(image, gt, quantize, channels_last)
    C = _C()
    flags = (C.METRICS_QUANTIZE_IMAGE if q[0] else 0) | (C.METRICS_QUANTIZE_GT if q[1] else 0)
    return C.image_metrics(x, y, getattr(C, fx), getattr(C, fy), flags, want_ssim)


@torch.no_grad()
def image_metrics(image, gt, quantize=False, channels_last=False) -> ImageMetrics:
    """ImageMetrics(l1, psnr, ssim, mse), each an (N,) float32 device tensor with one value per view pair.
    image, gt: float32 (N,C,H,W) or (C,H,W), or uint8 in the same layout or, with channels_last, (N,H,W,C) / (H,W,C).
    quantize: a float32 side is read as the 8-bit image a saved PNG holds of it.  Both take one bool or an (image, gt) pair."""
    l1, mse, psnr_, ssim_ = _run(image, gt, quantize, channels_last, True)
    return ImageMetrics(l1=l1, psnr=psnr_, ssim=ssim_, mse=mse)


@torch.no_grad()
def psnr(img1, img2):
    """Drop-in for utils/image_utils.py `psnr`: 20 log10(1 / sqrt(mse)) with the mse over everything behind the first axis,
    (N, 1) float32.  A (C,H,W) input gives one value per channel, (C, 1), as the reference's `view(img1.shape[0], -1)` does."""
    img1, img2 = (t[:, None] if torch.is_tensor(t) and t.dim() == 3 else t for t in (img1, img2))
    return _run(img1, img2, False, False, False)[2][:, None]


@torch.no_grad()
def ssim(img1, img2, window_size=11, size_average=True):
    """Drop-in for utils/loss_utils.py `ssim` where no gradient is wanted (evaluation): the mean SSIM as a 0-dim tensor, or one
    mean per image with size_average=False.  Training needs image_loss.fused_ssim, which is differentiable."""
    if window_size != 11:
        raise ValueError(f"window_size {window_size}: the fused SSIM implements the reference's default window of 11 only")
    if not size_average and (not torch.is_tensor(img1) or img1.dim() != 4):
        raise ValueError("size_average=False needs an (N,C,H,W) input (the reference's per-image mean does too)")
    per_image = _run(img1, img2, False, False, True)[3]
    return per_image.mean() if size_average else per_image


def evaluate_views(renders, gts, quantize=True, channels_last=False, lpips_weights=None) -> dict:
    """The image metrics of a test set as metrics.py:81-86 reports them: {"SSIM", "PSNR", "L1"} - the means over the views, formed
    as metrics.py forms them (`torch.tensor(values).mean().item()`) - and {"per_view": {"SSIM": [...], "PSNR": [...], "L1": [...]}}
    in the order of `renders`.  renders, gts: lists of (3,H,W) (any C) tensors of possibly different sizes; every run of
    equal-sized, equally typed views goes to the device in one call, and the host reads the results once, at the end.
    quantize (default True: the PNG round trip of metrics.py) applies to the float32 tensors only and channels_last to the
    uint8 ones only.  lpips_weights (lpips_vgg.LpipsWeights): the result also carries "LPIPS" and per_view "LPIPS"
    (lpips_vgg.evaluate_views, metrics.py:74; a second host read); None: exactly the three."""
    if len(renders) != len(gts):
        raise ValueError(f"{len(renders)} renders and {len(gts)} ground-truth images")
    cl = _pair(channels_last, "channels_last")
    q = _pair(quantize, "quantize")

    def key(i):
        return tuple((tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t) for t in (renders[i], gts[i]))

    def is_float(t):
        return torch.is_tensor(t) and t.dtype == torch.float32

    # argument errors of every view before any device work
    runs, i = [], 0
    while i < len(renders):
        j = i + 1
        while j < len(renders) and key(j) == key(i):
            j += 1
        qq = (q[0] and is_float(renders[i]), q[1] and is_float(gts[i]))
        cc = (cl[0] and not is_float(renders[i]), cl[1] and not is_float(gts[i]))
        for k in range(i, j):
            if torch.is_tensor(renders[k]) and renders[k].dim() == 4 and renders[k].shape[0] != 1:
                raise ValueError(f"view {k}: one image per list entry expected, got a batch of {renders[k].shape[0]}")
            _prepare(renders[k], gts[k], qq, cc)
        runs.append((i, j, qq, cc))
        i = j
    perceptual = None
    if lpips_weights is not None:
        import lpips_vgg

        def planar(t, last):                                  # an interleaved uint8 view, read in place through its strides
            return t.movedim(-1, -3) if last and torch.is_tensor(t) and t.dtype == torch.uint8 else t
        perceptual = lpips_vgg.evaluate_views([planar(t, cl[0]) for t in renders], [planar(t, cl[1]) for t in gts], lpips_weights, q)
    if not runs:
        empty = {"SSIM": float("nan"), "PSNR": float("nan"), "L1": float("nan"), "per_view": {"SSIM": [], "PSNR": [], "L1": []}}
        if perceptual is not None:
            empty["LPIPS"], empty["per_view"]["LPIPS"] = perceptual["LPIPS"], perceptual["per_view"]["LPIPS"]
        return empty
    parts = []
    for i, j, qq, cc in runs:
        m = image_metrics(torch.stack([t if t.dim() == 3 else t[0] for t in renders[i:j]]),
                          torch.stack([t if t.dim() == 3 else t[0] for t in gts[i:j]]), qq, cc)
        parts.append(torch.stack([m.ssim, m.psnr, m.l1]))
    table = torch.cat(parts, dim=1).cpu()                     # the one host read
    out = {"per_view": {}}
    for row, name in enumerate(("SSIM", "PSNR", "L1")):
        values = table[row].tolist()
        out[name] = torch.tensor(values).mean().item()
        out["per_view"][name] = values
    if perceptual is not None:
        out["LPIPS"], out["per_view"]["LPIPS"] = perceptual["LPIPS"], perceptual["per_view"]["LPIPS"]
    return out


def install(module):
    """Sets `psnr` in an imported `utils.image_utils` and `ssim` in an imported `utils.loss_utils` (whichever of the two names the
    module has), so that the reference's metrics.py and training_report score their views with the fused kernels.  Only for
    evaluation: a script that also trains through `ssim` must keep the differentiable one (image_loss.fused_ssim).
    Returns the module."""
    found = [name for name in ("psnr", "ssim") if hasattr(module, name)]
    if not found:
        raise AttributeError(f"{module.__name__} has neither psnr nor ssim: not the reference's utils.image_utils or utils.loss_utils")
    for name in found:
        setattr(module, name, globals()[name])
    return module
