"""LPIPS (VGG16, version 0.1) of rendered views on the device: the third number of the reference's evaluation.

Replaces metrics.py:74

    lpipss.append(lpips(renders[idx], gts[idx], net_type='vgg'))

- whose lpipsPyTorch imports torchvision at module level and downloads the linear heads at construction - with

    weights = LpipsWeights.load("vgg16-397923af.pth", "vgg.pth")         # local files; or from_state_dicts(vgg_sd, lin_sd)
    d = lpips_views(renders, gts, weights, quantize=True)                # (N,) float32 on the device, no host read
    terms = layer_terms(renders, gts, weights)                           # (N, 5): the five layer terms
    taps = vgg_taps(weights, images)                                     # relu1_2 .. relu5_3, un-normalised
    report = evaluate_views(renders, gts, weights)                       # {"LPIPS", "per_view"}, one host read
    import metrics, lpips_vgg;  lpips_vgg.install(metrics, weights)      # or: the reference's script, fused

csrc/lpips.hip behind include/f3dgs.h (f3dgs_lpips_*).  Exactly the reference's network for net_type 'vgg': z-score (values as
given, metrics.py passes [0, 1]), torchvision's vgg16().features[0:30], taps behind relu1_2 .. relu5_3, channel-normalised with
eps 1e-10, squared differences weighted by the non-negative heads, mean over pixels, sum over layers.  AlexNet and SqueezeNet
raise NotImplementedError.  fp32 throughout, the convolutions on the exact-fp32 matrix instructions in one fixed summation
order: two calls give the same bits, and a pair's value is the same bits at every batch size and position in the batch.

This repository holds no checkpoint: the weights are any state dict with the reference's names (`canonical_names`).  Neither
torchvision nor lpipsPyTorch is imported, nothing is downloaded.  HIP only; no CPU fallback; argument errors are raised before
any device work.
"""
from __future__ import annotations

import re

import torch

CONV_LAYERS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)          # torchvision's vgg16().features
CONV_WIDTHS = ((64, 3), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256), (512, 512), (512, 512),
               (512, 512), (512, 512), (512, 512))                       # (Cout, Cin)
TAP_CHANNELS = (64, 128, 256, 512, 512)
MIN_SIZE = 16                                                            # below it torch's fifth block is empty
_OTHER_HEADS = {(64, 192, 384, 256, 256): "AlexNet", (64, 128, 256, 384, 384, 512, 512): "SqueezeNet"}

_default_weights = None


def parameter_table():
    """[(name, shape)]: the parameters in the order f3dgs_lpips_pack_weights takes them (include/f3dgs.h): 13 convolution
    weights, their 13 biases, the five heads."""
    t = [(f"features.{n}.weight", (co, ci, 3, 3)) for n, (co, ci) in zip(CONV_LAYERS, CONV_WIDTHS)]
    t += [(f"features.{n}.bias", (co,)) for n, (co, _) in zip(CONV_LAYERS, CONV_WIDTHS)]
    t += [(f"lin.{i}.weight", (1, c, 1, 1)) for i, c in enumerate(TAP_CHANNELS)]
    return t


_CONV_SPELLINGS = (re.compile(r"^features\.(\d+)\.(weight|bias)$"), re.compile(r"^net\.layers\.(\d+)\.(weight|bias)$"),
                   re.compile(r"^(\d+)\.(weight|bias)$"))
_HEAD_SPELLINGS = (re.compile(r"^lin(\d+)\.model\.1\.weight$"), re.compile(r"^lin\.(\d+)\.1\.weight$"), re.compile(r"^lin\.(\d+)\.weight$"),
                   re.compile(r"^(\d+)\.1\.weight$"))


def _canonical(key):
    for pat in _HEAD_SPELLINGS:
        m = pat.match(key)
        if m:
            return f"lin.{int(m.group(1))}.weight"
    for pat in _CONV_SPELLINGS:
        m = pat.match(key)
        if m:
            return f"features.{int(m.group(1))}.{m.group(2)}"
    return None


def canonical_names(sd) -> dict:
    """{canonical name: value} of parameter_table()'s 31 names out of a state dict (or two merged ones) in any accepted spelling:
    a convolution as `features.N.*` (a torchvision checkpoint), `N.*` or `net.layers.N.*` (the reference's LPIPS.state_dict()); a
    head as `lin{i}.model.1.weight` (the upstream file), `{i}.1.weight` (the reference's renamed keys), `lin.{i}.1.weight` or
    `lin.{i}.weight`.  Other entries (a classifier, buffers) are ignored.  A missing name raises KeyError, a wrong shape
    ValueError, the heads or widths of AlexNet / SqueezeNet NotImplementedError; each names the parameter.  Pure Python."""
    found, spelled = {}, {}
    for key, value in sd.items():
        name = _canonical(str(key))
        if name is not None:
            found[name], spelled[name] = value, key
    heads = tuple(int(found[f"lin.{i}.weight"].shape[1]) for i in range(8)
                  if f"lin.{i}.weight" in found and len(found[f"lin.{i}.weight"].shape) == 4)
    if heads in _OTHER_HEADS:
        raise NotImplementedError(f"{spelled['lin.0.weight']}: heads of {heads} channels are {_OTHER_HEADS[heads]}'s; only net_type 'vgg' is built")
    out = {}
    for name, shape in parameter_table():
        if name not in found:
            raise KeyError(f"{name}: not in the state dict (in any accepted spelling)")
        got = tuple(found[name].shape)
        if got != shape:
            if name == "features.0.weight" and len(got) == 4 and got[2:] != (3, 3):
                raise NotImplementedError(f"{spelled[name]}: shape {got} is not VGG16's {shape} (AlexNet and SqueezeNet are not built)")
            raise ValueError(f"{spelled[name]}: shape {got}, {shape} expected")
        out[name] = found[name]
    return out


def _C():
    from diff_gaussian_rasterization import _C as ext
    return ext


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("lpips_vgg needs a HIP device: there is no CPU path")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"lpips_vgg needs a HIP device, got {device}: there is no CPU path")
    return device


class LpipsWeights:
    """The packed VGG16 convolutions and the five heads on one device (59 MB)."""

    def __init__(self, packed):
        self.packed = packed

    @property
    def device(self):
        return self.packed.device

    @classmethod
    def from_state_dicts(cls, vgg_sd, lin_sd=None, device=None):
        """vgg_sd: the convolutions (and, with lin_sd None, the heads too: one merged dict); lin_sd: the heads.  Names as
        canonical_names accepts them; its errors first, then the refusal without a HIP device."""
        merged = dict(vgg_sd)
        if lin_sd is not None:
            merged.update(lin_sd)
        named = canonical_names(merged)
        tensors = []
        for name, _ in parameter_table():
            t = torch.as_tensor(named[name])
            if not t.dtype.is_floating_point:
                raise ValueError(f"{name}: a floating-point tensor expected, got {t.dtype}")
            tensors.append(t)
        device = _device(device)
        return cls(_C().lpips_pack([t.detach().to(device=device, dtype=torch.float32).contiguous() for t in tensors]))

    @classmethod
    def load(cls, vgg_path, lin_path, device=None):
        """torch.load of two local files: torchvision's vgg16 checkpoint and the heads (`vgg.pth` of LPIPS v0.1)."""
        return cls.from_state_dicts(torch.load(vgg_path, map_location="cpu"), torch.load(lin_path, map_location="cpu"), device)


def _pair(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what}: one bool, or an (x, y) pair, expected; got {v!r}")
        return bool(v[0]), bool(v[1])
    return bool(v), bool(v)


def _image(t, name, quantize):
    """the (N,3,H,W) view of one side, checked; no copy"""
    if not torch.is_tensor(t):
        raise ValueError(f"{name}: a tensor expected, got {type(t).__name__}")
    if t.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{name}: float32 or uint8 expected, got {t.dtype}")
    if t.dim() not in (3, 4):
        raise ValueError(f"{name}: (3,H,W) or (N,3,H,W) expected, got {tuple(t.shape)}")
    if t.dtype == torch.uint8 and quantize:
        raise ValueError(f"{name}: quantize applies to a float32 image; a uint8 image holds the 8-bit values already")
    t = t.detach()
    if t.dim() == 3:
        t = t[None]
    if t.shape[1] != 3:
        raise ValueError(f"{name}: 3 channels expected, got {tuple(t.shape)}")
    if t.shape[2] < MIN_SIZE or t.shape[3] < MIN_SIZE:
        raise ValueError(f"{name}: {t.shape[2]} x {t.shape[3]} pixels: below {MIN_SIZE} x {MIN_SIZE} the fifth block of VGG16 is empty")
    if any(s < 0 for s in t.stride()):
        raise ValueError(f"{name}: a negative stride")
    return t


def _weights(weights):
    if weights is None:
        weights = _default_weights
    if weights is None:
        raise ValueError("weights: LpipsWeights expected (LpipsWeights.from_state_dicts / load, or set_default_weights)")
    if not isinstance(weights, LpipsWeights):
        raise ValueError("weights: LpipsWeights expected (LpipsWeights.from_state_dicts / load)")
    return weights


def _prepare(x, y, weights, quantize):
    q = _pair(quantize, "quantize")
    if weights is not None and not isinstance(weights, LpipsWeights):
        raise ValueError("weights: LpipsWeights expected (LpipsWeights.from_state_dicts / load)")
    x, y = _image(x, "x", q[0]), _image(y, "y", q[1])
    if x.shape != y.shape:
        raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} shapes differ")
    for name, t in (("x", x), ("y", y)):                  # last, so that every other error can be met without a device
        if t.device.type != "cuda":
            raise ValueError(f"{name} lives on {t.device}: LPIPS runs on a HIP device only (no CPU path)")
    weights = _weights(weights)
    if x.device != y.device or x.device != weights.device:
        raise ValueError(f"x is on {x.device}, y on {y.device}, the weights on {weights.device}")
    return x, y, weights, q


def _forward(x, y, weights, quantize):
    x, y, weights, q = _prepare(x, y, weights, quantize)
    C = _C()
    flags = (C.LPIPS_QUANTIZE_X if q[0] else 0) | (C.LPIPS_QUANTIZE_Y if q[1] else 0)
    return C.lpips_forward(weights.packed, x, y, flags)


@torch.no_grad()
def lpips_views(x, y, weights=None, quantize=False):
    """(N,) float32 on the device: LPIPS of every pair.  x, y: float32 or uint8 (value / 255), (N,3,H,W) or (3,H,W), H, W >= 16,
    any non-negative strides, read in place.  quantize (one bool or an (x, y) pair): a float32 side is read as the 8-bit image a
    saved PNG holds of it, as in image_metrics."""
    return _forward(x, y, weights, quantize)[1]


@torch.no_grad()
def layer_terms(x, y, weights=None, quantize=False):
    """(N, 5) float32: the five layer terms d_l, whose sum is lpips_views."""
    return _forward(x, y, weights, quantize)[0]


@torch.no_grad()
def vgg_taps(weights, x, quantize=False):
    """The five un-normalised taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 of x: (N, C_l, H_l, W_l) float32."""
    if not isinstance(weights, LpipsWeights):
        raise ValueError("weights: LpipsWeights expected (LpipsWeights.from_state_dicts / load)")
    x = _image(x, "x", bool(quantize))
    if x.device.type != "cuda":
        raise ValueError(f"x lives on {x.device}: LPIPS runs on a HIP device only (no CPU path)")
    if x.device != weights.device:
        raise ValueError(f"x is on {x.device}, the weights on {weights.device}")
    return _C().lpips_taps(weights.packed, x, bool(quantize))


def set_default_weights(weights):
    """The weights `lpips` uses where none are given; None clears them."""
    global _default_weights
    if weights is not None and not isinstance(weights, LpipsWeights):
        raise ValueError("weights: LpipsWeights or None expected")
    _default_weights = weights


@torch.no_grad()
def lpips(x, y, net_type="vgg", version="0.1", weights=None):
    """Drop-in for lpipsPyTorch.lpips with net_type='vgg': a (1,1,1,1) tensor, summed over the layers and - as the reference's
    `torch.sum(torch.cat(res, 0), 0, True)` does - over the batch too."""
    if net_type != "vgg":
        raise NotImplementedError(f"net_type {net_type!r}: only 'vgg' is built (AlexNet and SqueezeNet are not)")
    if version != "0.1":
        raise NotImplementedError(f"version {version!r}: v0.1 is only supported")
    return _forward(x, y, weights, False)[1].sum().reshape(1, 1, 1, 1)


def install(module, weights):
    """Sets `lpips` in an imported module that has the name - metrics.py's namespace, or lpipsPyTorch (or a stub of it) - to the
    fused one and makes `weights` the default.  Returns the module."""
    if not hasattr(module, "lpips"):
        raise AttributeError(f"{module.__name__} has no lpips: not the reference's metrics or lpipsPyTorch")
    set_default_weights(weights)
    module.lpips = lpips
    return module


def evaluate_views(renders, gts, weights=None, quantize=True, max_workspace_bytes=4 << 30) -> dict:
    """LPIPS of a test set as metrics.py:83 reports it: {"LPIPS": the mean over the views, formed as metrics.py forms it
    (`torch.tensor(values).mean().item()`), "per_view": {"LPIPS": [...]}} in the order of `renders`.  renders, gts: lists of
    (3,H,W) tensors of possibly different sizes; a run of equal-sized, equally typed views shares a call, split so that the
    workspace of a call stays under max_workspace_bytes (a single view takes what it takes); one host read, at the end.
    quantize (default True: the PNG round trip of metrics.py) applies to the float32 tensors only."""
    if len(renders) != len(gts):
        raise ValueError(f"{len(renders)} renders and {len(gts)} ground-truth images")
    q = _pair(quantize, "quantize")

    def key(i):
        return tuple((tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t) for t in (renders[i], gts[i]))

    def is_float(t):
        return torch.is_tensor(t) and t.dtype == torch.float32

    runs, i = [], 0
    while i < len(renders):                                 # argument errors of every view before any device work
        j = i + 1
        while j < len(renders) and key(j) == key(i):
            j += 1
        qq = (q[0] and is_float(renders[i]), q[1] and is_float(gts[i]))
        for k in range(i, j):
            if torch.is_tensor(renders[k]) and renders[k].dim() == 4 and renders[k].shape[0] != 1:
                raise ValueError(f"view {k}: one image per list entry expected, got a batch of {renders[k].shape[0]}")
            _prepare(renders[k], gts[k], weights, qq)
        runs.append((i, j, qq))
        i = j
    if not runs:
        return {"LPIPS": float("nan"), "per_view": {"LPIPS": []}}
    weights = _weights(weights)
    C = _C()
    parts = []
    for i, j, qq in runs:
        H, W = int(renders[i].shape[-2]), int(renders[i].shape[-1])
        per_pair = C.lpips_workspace_bytes(1, H, W)
        step = max(1, int(max_workspace_bytes) // max(1, per_pair))
        for a in range(i, j, step):
            b = min(j, a + step)
            parts.append(lpips_views(torch.stack([t if t.dim() == 3 else t[0] for t in renders[a:b]]),
                                     torch.stack([t if t.dim() == 3 else t[0] for t in gts[a:b]]), weights, qq))
    values = torch.cat(parts).cpu().tolist()               # the one host read
    return {"LPIPS": torch.tensor(values).mean().item(), "per_view": {"LPIPS": values}}
