"""Development aid (GPU): time of the fused L1 + D-SSIM image loss (image_loss.py) against the reference's torch ops
(utils/loss_utils.py restated: five depthwise 11x11 conv2d, the elementwise SSIM, autograd), forward + backward, at
3 x 1080 x 1920 and 3 x 2160 x 3840.  Device events around 20 calls after 5 warm-up calls, in one process.

Algorithmic bytes of the fused call: forward reads image and gt and writes three fp32 maps (5 planes), backward reads the
three maps, image and gt and writes the gradient (6 planes): 11 x 4 x 3 H W bytes.  At 1080p (75 MB of maps) everything fits
in the 256 MiB Infinity Cache, so the byte rate there is not an HBM figure; at 4K (300 MB of maps) it is."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import torch.nn.functional as F

from image_loss import fused_l1_dssim
import image_loss_oracle as O

dev = "cuda:0"
LAM = 0.2
WIN = O.window2d(dev).to(torch.float32).expand(3, 1, 11, 11).contiguous()


def torch_ops(img, gt):
    conv = lambda t: F.conv2d(t, WIN, padding=5, groups=3)
    mu1, mu2 = conv(img), conv(gt)
    s1, s2, s12 = conv(img * img) - mu1 ** 2, conv(gt * gt) - mu2 ** 2, conv(img * gt) - mu1 * mu2
    S = ((2 * mu1 * mu2 + O.C1) * (2 * s12 + O.C2)) / ((mu1 ** 2 + mu2 ** 2 + O.C1) * (s1 + s2 + O.C2))
    return (1 - LAM) * (img - gt).abs().mean() + LAM * (1 - S.mean())


for H, W in ((1080, 1920), (2160, 3840)):
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(3, H, W, generator=g).to(dev)
    img = (gt + 0.2 * torch.randn(3, H, W, generator=g).to(dev)).clamp(0, 1).requires_grad_(True)
    res = {}
    for name, fn in (("torch ops", lambda: torch_ops(img, gt)), ("fused", lambda: fused_l1_dssim(img, gt, LAM))):
        def call():
            fn().backward()
            img.grad = None
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            call()
        e1.record()
        torch.cuda.synchronize()
        res[name] = e0.elapsed_time(e1) / 20
    nbytes = 11 * 4 * 3 * H * W
    print(f"{W}x{H}x3  torch ops {res['torch ops']:8.3f} ms   fused {res['fused']:8.3f} ms   "
          f"speed-up {res['torch ops'] / res['fused']:6.1f}x   fused: {nbytes / 1e6:6.1f} MB algorithmic, "
          f"{nbytes / res['fused'] / 1e9:6.2f} TB/s", flush=True)
