"""Generates tests/golden/reference_ssim.npz by IMPORTING the reference's own loss code (utils/loss_utils.py).

For every case, in fp64 on seeded inputs, it evaluates the reference's `ssim` and the training loss of train.py:99-105,
(1 - lambda) * l1_loss + lambda * (1 - ssim), and takes their gradients with respect to the image by autograd.  The
reference builds its window in fp32 (`create_window`) and `type_as` widens it: the fixture carries that rounding, which the
fp64 oracle of tests/image_loss_oracle.py restates.  Run it here, where the reference exists (GPU tests read only the npz):

    python tests/golden/make_reference_ssim_vectors.py
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
LAMBDA = 0.2

# name: (shape, kind); 4-D shapes are batches, 3-D shapes unbatched images
CASES = {
    "rand_1x3x37x53": ((1, 3, 37, 53), "random"),
    "batch_2x3x8x6": ((2, 3, 8, 6), "random"),          # also size_average=False
    "tiny_1x1x1x1": ((1, 1, 1, 1), "random"),
    "small_1x3x4x7": ((1, 3, 4, 7), "random"),
    "unbatched_3x20x30": ((3, 20, 30), "random"),
    "identical_1x3x16x16": ((1, 3, 16, 16), "identical"),
    "constant_1x3x12x12": ((1, 3, 12, 12), "constant"),
}
UPSTREAM = np.array([0.7, -1.3])     # per-image upstream gradient of the size_average=False case


def main():
    sys.path.insert(0, REF)
    from utils.loss_utils import l1_loss, ssim  # noqa: E402  (reference code)

    g = torch.Generator().manual_seed(4321)
    out = {"lambda_dssim": np.float64(LAMBDA), "upstream_per_image": UPSTREAM}
    for name, (shape, kind) in CASES.items():
        # inputs are fp32 values (what the kernels take), widened to fp64 for the reference's arithmetic
        gt = torch.rand(shape, generator=g).to(torch.float64)
        if kind == "identical":
            img = gt.clone()
        elif kind == "constant":
            img = torch.full(shape, 0.5, dtype=torch.float64)
        else:
            # the rendering: the target plus noise, clamped to [0, 1] as the rasterizer's colours are
            img = (gt + 0.2 * torch.randn(shape, generator=g)).clamp(0, 1).to(torch.float32).to(torch.float64)
        x = img.clone().requires_grad_(True)
        s = ssim(x, gt)
        l1 = l1_loss(x, gt)
        loss = (1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - s)
        gl, = torch.autograd.grad(loss, x, retain_graph=True)
        gs, = torch.autograd.grad(s, x)
        out[f"{name}/image"], out[f"{name}/gt"] = img.to(torch.float32).numpy(), gt.to(torch.float32).numpy()
        out[f"{name}/loss"], out[f"{name}/l1"], out[f"{name}/ssim"] = loss.item(), l1.item(), s.item()
        out[f"{name}/grad_loss"] = gl.numpy()
        if img.numel() <= 1024:        # (the size bound of the file: the larger cases carry the loss's gradient only)
            out[f"{name}/grad_ssim"] = gs.numpy()
        if len(shape) == 4 and shape[0] > 1:
            x = img.clone().requires_grad_(True)
            v = ssim(x, gt, size_average=False)
            gv, = torch.autograd.grad((v * torch.as_tensor(UPSTREAM)).sum(), x)
            out[f"{name}/ssim_per_image"], out[f"{name}/grad_ssim_per_image"] = v.detach().numpy(), gv.numpy()
    path = os.path.join(HERE, "reference_ssim.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(CASES)} cases)")


if __name__ == "__main__":
    main()
