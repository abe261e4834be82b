"""fp64 torch oracle of the fused image loss (feature-3dgs_amd/image_loss.py, csrc/image_loss.hip) - the decomposition the
kernels use, restated with plain tensor ops so that it runs on the CPU and, for the large cases, on the GPU in fp64.

The window is built as the reference builds it (utils/loss_utils.py:20-31): Gaussian weights rounded to fp32 and
normalised in fp32, the 2-D window their fp32 outer product, then widened to fp64.  The 11x11 stencil is applied as 121
shifted multiply-adds over a zero-padded copy (no convolution library, fp64 on any device).  The gradient is

    d/dx sum S = G*g_mu + 2 x G*g_11 + y G*g_12,   g_mu = dS/dmu1, g_11 = dS/dE[x^2], g_12 = dS/dE[xy] (total derivatives)

with G symmetric, so its transpose is the same stencil."""
from math import exp

import torch

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window2d(device="cpu") -> torch.Tensor:
    g = torch.tensor([exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = g / g.sum()
    return (g[:, None] @ g[None, :]).to(torch.float64).to(device)


def stencil(t: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Zero-padded 11x11 correlation of every (..., H, W) plane with w."""
    H, W = t.shape[-2:]
    p = torch.nn.functional.pad(t, (5, 5, 5, 5))
    out = torch.zeros_like(t)
    for i in range(11):
        for j in range(11):
            out += w[i, j] * p[..., i:i + H, j:j + W]
    return out


def maps(x: torch.Tensor, y: torch.Tensor, w: torch.Tensor):
    """S and the three derivative maps, fp64."""
    mu1, mu2 = stencil(x, w), stencil(y, w)
    e11, e22, e12 = stencil(x * x, w), stencil(y * y, w), stencil(x * y, w)
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    A1, A2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    D = B1 * B2
    S = A1 * A2 / D
    g_mu = 2 * (mu2 * (A2 - A1) + mu1 * S * (B1 - B2)) / D
    return S, g_mu, -S / B2, 2 * A1 / D


def image_loss(image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2, upstream_ssim=None):
    """fp64 results for (C,H,W) or (N,C,H,W) inputs: dict with loss, l1, ssim, ssim_per_image (4-D input), grad_loss
    (d loss / d image), grad_ssim (d mean ssim / d image) and, given `upstream_ssim` (N values), grad_ssim_per_image
    (d sum_n upstream_n ssim_n / d image)."""
    x, y = image.to(torch.float64), gt.to(torch.float64)
    w = window2d(x.device)
    S, g_mu, g_11, g_12 = maps(x, y, w)
    n = x.numel()
    dsum = stencil(g_mu, w) + 2 * x * stencil(g_11, w) + y * stencil(g_12, w)      # d sum(S) / dx
    sign = torch.sign(x - y)
    l1 = (x - y).abs().mean()
    ssim = S.mean()
    out = dict(l1=l1, ssim=ssim, loss=(1 - lambda_dssim) * l1 + lambda_dssim * (1 - ssim),
               grad_loss=-lambda_dssim / n * dsum + (1 - lambda_dssim) / n * sign, grad_ssim=dsum / n)
    if x.dim() == 4:
        out["ssim_per_image"] = S.mean(dim=(1, 2, 3))
        if upstream_ssim is not None:
            u = torch.as_tensor(upstream_ssim, dtype=torch.float64, device=x.device).reshape(-1, 1, 1, 1)
            out["grad_ssim_per_image"] = u * dsum / (n // x.shape[0])
    return out
