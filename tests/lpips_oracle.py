"""LPIPS with VGG16 in plain torch ops, the dtype a parameter: written from the definition (z-score with zero padding behind it,
13 convolutions 3x3 with bias and ReLU, 2x2 max-pools between the blocks, taps behind relu1_2 .. relu5_3, n(t) = t / (|t| + 1e-10),
d_l = mean over pixels of sum_c w_l[c] (n(tx) - n(ty))^2, the sum over l), not from the reference's text.  Weights: {name: array}
under lpips_vgg.parameter_table()'s names."""
import numpy as np
import torch
import torch.nn.functional as F

CONV_LAYERS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
POOL_BEFORE = (5, 10, 17, 24)
TAP_AFTER = (2, 7, 14, 21, 28)
MEAN, STD = (-.030, -.088, -.188), (.458, .448, .450)


def _t(v, dtype):
    return (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(dtype)


@torch.no_grad()
def taps(weights, x, dtype=torch.float64):
    """the five un-normalised taps of x (N,3,H,W), as `dtype` tensors (the constants are the float32 ones the reference holds)"""
    t = _t(x, dtype)
    mean = torch.tensor(MEAN, dtype=torch.float32).to(t.device, dtype)[None, :, None, None]
    std = torch.tensor(STD, dtype=torch.float32).to(t.device, dtype)[None, :, None, None]
    t = (t - mean) / std
    out = []
    for n in CONV_LAYERS:
        if n in POOL_BEFORE:
            t = F.max_pool2d(t, 2, 2)
        t = F.relu(F.conv2d(t, _t(weights[f"features.{n}.weight"], dtype), _t(weights[f"features.{n}.bias"], dtype), padding=1))
        if n in TAP_AFTER:
            out.append(t)
    return out


def _normalize(t):
    return t / (torch.sqrt((t * t).sum(1, keepdim=True)) + 1e-10)


@torch.no_grad()
def layer_terms(weights, x, y, dtype=torch.float64):
    """((N, 5) layer terms, (N,) totals) as `dtype` tensors"""
    terms = []
    for l, (tx, ty) in enumerate(zip(taps(weights, x, dtype), taps(weights, y, dtype))):
        d = (_normalize(tx) - _normalize(ty)) ** 2
        w = _t(weights[f"lin.{l}.weight"], dtype).reshape(1, -1, 1, 1)
        terms.append((d * w).sum(1).mean((1, 2)))
    terms = torch.stack(terms, 1)
    return terms, terms.sum(1)


@torch.no_grad()
def lpips(weights, x, y, dtype=torch.float64):
    """the drop-in's value: (1,1,1,1), summed over the batch as the reference's forward does"""
    return layer_terms(weights, x, y, dtype)[1].sum().reshape(1, 1, 1, 1)
