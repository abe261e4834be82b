"""Generates tests/golden/reference_image_metrics.npz by running the reference's own metric code on the CPU:
utils/loss_utils.py `ssim` and `l1_loss`, utils/image_utils.py `psnr` and `mse` - what metrics.py:71-74 and training_report
(train.py:210-239) call.

Per case and per image: `ssim` (size_average=False), `l1_loss`, `mse` and `psnr` in fp64 on the values the views hold (the fp64
oracle of tests/image_metrics_oracle.py is held to these), and `psnr_fp32`: the reference's psnr on the fp32 tensors, which is
what a user of the reference sees.  The cases:

  float        fp32 render and ground truth scored as they are (training_report); `psnr_chw_fp32` of the first image pins what
               the reference's psnr makes of an unbatched (C,H,W) input: one value per channel
  png          metrics.py's route: the fp32 views go through torchvision's save_image arithmetic
               (`mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8)`), a true PNG file written and read
               back with PIL, and to_tensor's arithmetic (`.permute(2, 0, 1).to(float32).div(255)`); the decoded (H,W,C) bytes are
               stored as PIL hands them over.  torchvision is not installed where this runs, so its two one-line conversions are
               restated here; the PNG encode / decode is PIL's own.
  special      the quantiser's edge inputs - NaN, +-inf, negatives, values above 1, exact halves - through the same tensor chain
               on the CPU: `nan_byte` and `special/image_u8` PIN what torch's cast does with them there; nothing here decides it.
  identical    the same image twice: psnr = +inf

utils/image_utils.py imports matplotlib and sklearn at module level for its viewer helpers.  Where that import fails, the two
metric functions are taken from the file's syntax tree and compiled alone, with `torch` as their only global.

Run it where the reference exists (the tests read only the npz):

    python tests/golden/make_reference_image_metrics_vectors.py
"""
import ast
import io
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def load_psnr():
    try:
        from utils.image_utils import mse, psnr  # noqa: E402  (reference code)
        return mse, psnr, "imported"
    except ImportError:
        path = os.path.join(REF, "utils", "image_utils.py")
        tree = ast.parse(open(path).read(), path)
        tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("mse", "psnr")]
        ns = {"torch": torch}
        exec(compile(tree, path, "exec"), ns)
        return ns["mse"], ns["psnr"], "functions compiled without the module-level imports"


def save_image_bytes(t):
    """(H,W,C) uint8 of a (C,H,W) float tensor: torchvision.utils.save_image's conversion"""
    return t.clone().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def png_round_trip(hwc):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(hwc).save(buf, format="PNG")
    buf.seek(0)
    back = np.array(Image.open(buf))
    assert back.dtype == np.uint8 and back.shape == hwc.shape
    return back


def to_tensor(hwc):
    """torchvision.transforms.functional.to_tensor of a uint8 image"""
    return torch.from_numpy(hwc).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def views(shape, g, noise=0.1):
    gt = torch.rand(shape, generator=g)
    img = (gt + noise * torch.randn(shape, generator=g)).clamp(0, 1)
    return img, gt


def main():
    sys.path.insert(0, REF)
    from utils.loss_utils import l1_loss, ssim  # noqa: E402  (reference code)
    mse, psnr, how = load_psnr()
    print("utils.image_utils:", how)
    g = torch.Generator().manual_seed(97531)
    out = {}

    def score(name, x32, y32):
        """x32, y32: (N,C,H,W) fp32 values the reference scores"""
        x, y = x32.to(torch.float64), y32.to(torch.float64)
        out[f"{name}/ssim"] = ssim(x, y, size_average=False).numpy()
        out[f"{name}/l1"] = np.array([l1_loss(x[i], y[i]).item() for i in range(x.shape[0])])
        out[f"{name}/mse"] = mse(x, y)[:, 0].numpy()
        out[f"{name}/psnr"] = psnr(x, y)[:, 0].numpy()
        out[f"{name}/psnr_fp32"] = psnr(x32, y32)[:, 0].numpy()
        out[f"{name}/ssim_fp32"] = np.array([ssim(x32[i:i + 1], y32[i:i + 1]).item() for i in range(x.shape[0])], np.float32)

    # training_report: the float views as they are; three images of different content and error level
    img, gt = views((3, 3, 12, 18), g)
    img[1] = (gt[1] + 0.3 * torch.randn(gt[1].shape, generator=g)).clamp(0, 1)
    img[2] = 0.5 * gt[2]
    out["float/image"], out["float/gt"] = img.numpy(), gt.numpy()
    score("float", img, gt)
    out["float/psnr_chw_fp32"] = psnr(img[0], gt[0])[:, 0].numpy()

    # metrics.py: both views through a PNG file
    img, gt = views((2, 3, 14, 19), g)
    img = img + 0.05 * torch.randn(img.shape, generator=g)           # an unclamped render: some values leave [0, 1]
    i8 = np.stack([png_round_trip(save_image_bytes(t)) for t in img])
    g8 = np.stack([png_round_trip(save_image_bytes(t)) for t in gt])
    out["png/image"], out["png/gt"] = img.numpy(), gt.numpy()
    out["png/image_u8"], out["png/gt_u8"] = i8, g8          # (N,H,W,C)
    score("png", torch.stack([to_tensor(a) for a in i8]), torch.stack([to_tensor(a) for a in g8]))

    # the quantiser's edge inputs, through the tensor chain on the CPU
    nan, inf = float("nan"), float("inf")
    edge = torch.tensor([nan, inf, -inf, -0.25, -1e-3, -0.0, 0.0, 1.0, 1.0 + 1e-6, 1.7, 300.0, 0.5, 0.5 / 255, 1.5 / 255, 2.5 / 255,
                         254.5 / 255, 253.5 / 255, 0.0019607844, 0.001960784, 1e-30, nan, 0.9980392, 0.99803925, 0.7],
                        dtype=torch.float32)
    img = torch.rand(1, 1, 6, 8, generator=g)
    img.view(-1)[:edge.numel()] = edge
    gt = torch.rand(1, 1, 6, 8, generator=g)
    i8 = save_image_bytes(img[0])[None]                               # (1,H,W,1)
    nan_bytes = save_image_bytes(torch.full((1, 5, 7), nan)).reshape(-1)
    assert len(set(nan_bytes.tolist())) == 1
    out["nan_byte"] = nan_bytes[0]
    out["special/image"], out["special/gt"], out["special/image_u8"] = img.numpy(), gt.numpy(), i8
    score("special", to_tensor(i8[0])[None], gt)                      # render quantised, ground truth as it is

    img, _ = views((1, 3, 16, 16), g)
    out["identical/image"], out["identical/gt"] = img.numpy(), img.numpy().copy()
    score("identical", img, img.clone())

    path = os.path.join(HERE, "reference_image_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for k in sorted(out):
        if "/" in k and out[k].size <= 3:
            print(k, out[k])
    print("nan_byte", out["nan_byte"])


if __name__ == "__main__":
    main()
