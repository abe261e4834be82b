"""Fused L1 + D-SSIM image loss: the image half of the reference's training loss, forward and backward in HIP.

Replaces these lines of the reference's training loop (train.py:99-105; utils/loss_utils.py:17-18, :33-63)

    Ll1 = l1_loss(image, gt_image)
    loss = (1.0 - opt.lambda_dssim) * Ll1 + opt.lambda_dssim * (1.0 - ssim(image, gt_image))

with

    loss, Ll1, _ssim = fused_l1_dssim(image, gt_image, opt.lambda_dssim, return_parts=True)

The five 11x11 depthwise convolutions, the elementwise kernels and their autograd backward become two kernels forward (the
windowed moments, SSIM and three per-pixel derivative maps; a fixed-order reduction) and one backward (the transposed
window over the maps).  No host round trip and no host-built window: the call may sit inside `graph_step.CapturedStep`.
HIP only (csrc/image_loss.hip behind include/f3dgs.h); no CPU fallback.  Only the rendered image's gradient is built.
"""
from __future__ import annotations

import torch

from diff_gaussian_rasterization import _C


def _check(img1: torch.Tensor, img2: torch.Tensor, window_size: int) -> None:
    if window_size != 11:
        raise ValueError(f"window_size {window_size}: the fused SSIM implements the reference's default window of 11 only")
    if img2.requires_grad:
        raise ValueError("the ground-truth image requires a gradient: the fused loss builds the gradient of the rendered image "
                         "only (detach the ground truth)")


class _FusedImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, lambda_dssim, mode):
        image, gt = image.contiguous(), gt.contiguous()
        per_image = mode == _C.IMAGE_LOSS_SSIM_PER_IMAGE
        loss, l1, ssim, ssim_img, scratch = _C.image_loss_forward(image, gt, float(lambda_dssim), True, per_image)
        ctx.save_for_backward(image, gt, scratch)
        ctx.lambda_dssim, ctx.mode = float(lambda_dssim), mode
        out = {_C.IMAGE_LOSS_L1_DSSIM: loss, _C.IMAGE_LOSS_SSIM: ssim, _C.IMAGE_LOSS_SSIM_PER_IMAGE: ssim_img}[mode]
        parts = (l1, ssim) if mode == _C.IMAGE_LOSS_L1_DSSIM else (l1, loss)
        ctx.mark_non_differentiable(*parts)
        return out, parts[0], parts[1]

    @staticmethod
    def backward(ctx, g, _g1, _g2):
        image, gt, scratch = ctx.saved_tensors
        u = g.detach().to(torch.float32).contiguous()
        d = _C.image_loss_backward(image, gt, scratch, u, ctx.lambda_dssim, ctx.mode)
        return d, None, None, None


def _run(image, gt, lambda_dssim, mode):
    """(output, l1, ssim): the output differentiable in `image` where autograd records, else computed without the maps."""
    if torch.is_grad_enabled() and image.requires_grad:
        out, a, b = _FusedImageLoss.apply(image, gt, lambda_dssim, mode)
        return (out, a, b) if mode == _C.IMAGE_LOSS_L1_DSSIM else (out, a, out)
    per_image = mode == _C.IMAGE_LOSS_SSIM_PER_IMAGE
    loss, l1, ssim, ssim_img, _ = _C.image_loss_forward(image.detach(), gt.detach(), float(lambda_dssim), False, per_image)
    return {_C.IMAGE_LOSS_L1_DSSIM: loss, _C.IMAGE_LOSS_SSIM: ssim, _C.IMAGE_LOSS_SSIM_PER_IMAGE: ssim_img}[mode], l1, ssim


def fused_l1_dssim(image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2, return_parts: bool = False):
    """(1 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt)) as one differentiable scalar.
    image, gt: (C,H,W) or (N,C,H,W) float32 on the GPU.  return_parts=True: (loss, l1, ssim), the last two detached scalars
    (train.py logs l1 as Ll1)."""
    _check(image, gt, 11)
    loss, l1, ssim = _run(image, gt, lambda_dssim, _C.IMAGE_LOSS_L1_DSSIM)
    return (loss, l1, ssim) if return_parts else loss


def fused_ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """Drop-in for utils/loss_utils.py `ssim`: the mean SSIM (size_average=True) or one mean per image (size_average=False,
    (N,C,H,W) input only, as in the reference), differentiable in img1."""
    _check(img1, img2, window_size)
    if not size_average and img1.dim() != 4:
        raise ValueError("size_average=False needs an (N,C,H,W) input (the reference's per-image mean does too)")
    return _run(img1, img2, 0.0, _C.IMAGE_LOSS_SSIM if size_average else _C.IMAGE_LOSS_SSIM_PER_IMAGE)[0]
