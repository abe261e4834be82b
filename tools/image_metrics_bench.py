"""Development aid (GPU): time of the fused image metrics (image_metrics.py: L1, MSE, PSNR and SSIM of N view pairs in two
launches) against the reference's torch ops on the same device (utils/loss_utils.py `ssim` and `l1_loss`, utils/image_utils.py
`psnr` restated: five depthwise 11x11 conv2d, the elementwise SSIM, a squared-error pass; one call per view pair, as metrics.py
loops), at 3 x 1080 x 1920 for N = 1 and N = 8.  Device events around every call, median of 50 after 5 warm-up calls, in one
process.  The torch chain gets the 8-bit values as fp32 tensors (what to_tensor hands metrics.py); the fused call is timed on
three of its input forms.

Algorithmic bytes of the fused call: both views are read once - 2 x 4 x 3 H W as fp32, 2 x 3 H W as uint8 - and nothing of
image size is written.  At 1080p everything fits in the 256 MiB Infinity Cache: the byte rate is not an HBM figure."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import torch.nn.functional as F

from image_metrics import image_metrics
import image_loss_oracle as O

dev = "cuda:0"
H, W = 1080, 1920
WIN = O.window2d(dev).to(torch.float32).expand(3, 1, 11, 11).contiguous()


def torch_ops(img, gt):
    """metrics.py:72-73 and train.py:227 for one (1,3,H,W) pair: ssim, psnr, l1"""
    conv = lambda t: F.conv2d(t, WIN, padding=5, groups=3)
    mu1, mu2 = conv(img), conv(gt)
    s1, s2, s12 = conv(img * img) - mu1 ** 2, conv(gt * gt) - mu2 ** 2, conv(img * gt) - mu1 * mu2
    S = ((2 * mu1 * mu2 + O.C1) * (2 * s12 + O.C2)) / ((mu1 ** 2 + mu2 ** 2 + O.C1) * (s1 + s2 + O.C2))
    mse = ((img - gt) ** 2).view(img.shape[0], -1).mean(1, keepdim=True)
    return S.mean(), 20 * torch.log10(1.0 / torch.sqrt(mse)), torch.abs(img - gt).mean()


def median_ms(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times)


for N in (1, 8):
    g = torch.Generator().manual_seed(N)
    gt = torch.rand(N, 3, H, W, generator=g).to(dev)
    img = (gt + 0.1 * torch.randn(N, 3, H, W, generator=g).to(dev)).clamp(0, 1)
    i8, g8 = (img * 255 + 0.5).to(torch.uint8), (gt * 255 + 0.5).to(torch.uint8)
    iq, gq = i8.float() / 255, g8.float() / 255
    i8l, g8l = i8.permute(0, 2, 3, 1).contiguous(), g8.permute(0, 2, 3, 1).contiguous()
    with torch.no_grad():
        rows = [("torch ops, one pair at a time", lambda: [torch_ops(iq[n:n + 1], gq[n:n + 1]) for n in range(N)], None),
                ("fused, fp32 quantised as read", lambda: image_metrics(img, gt, quantize=True), 2 * 4),
                ("fused, fp32 as they are", lambda: image_metrics(img, gt), 2 * 4),
                ("fused, uint8 planar", lambda: image_metrics(i8, g8), 2),
                ("fused, uint8 interleaved", lambda: image_metrics(i8l, g8l, channels_last=True), 2)]
        base = None
        for name, fn, bytes_per_element in rows:
            med, best = median_ms(fn)
            base = base or med
            line = f"N={N} {W}x{H}x3  {name:32s} median {med:8.3f} ms  min {best:8.3f} ms  per pair {med / N * 1e3:8.1f} us"
            if bytes_per_element:
                nbytes = bytes_per_element * 3 * H * W * N
                line += f"  speed-up {base / med:6.1f}x  {nbytes / 1e6:6.1f} MB algorithmic, {nbytes / med / 1e9:5.2f} TB/s"
            print(line, flush=True)
        ref, got = torch_ops(iq[:1], gq[:1]), image_metrics(i8, g8)
        print(f"      check, pair 0: ssim {float(ref[0]):.6f} / {float(got.ssim[0]):.6f}   psnr {float(ref[1]):.4f} / "
              f"{float(got.psnr[0]):.4f}   l1 {float(ref[2]):.6f} / {float(got.l1[0]):.6f}", flush=True)
