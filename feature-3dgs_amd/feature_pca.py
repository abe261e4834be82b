"""PCA colour image of a feature map: the picture that shows what a feature field has learned.

The reference's `feature_visualize_saving` (render.py:38-53) L2-normalises the (C, H, W) map, permutes it to (HW, C), copies
every third pixel to the host, fits `sklearn.decomposition.PCA(3)` there, copies mean and components back, multiplies
another permuted copy of the whole map by them, takes the 1st and 99th percentile of the samples' projection and clamps:
about three transient copies of the map - 354 MB each at 360 x 480 x 512 - and a host PCA per view.  Here the map is read by
HIP kernels only (csrc/feature_pca.hip behind include/f3dgs.h: f3dgs_feature_pca_moments, f3dgs_feature_pca_project) and
nothing of its size is allocated: the kernels produce the samples' mean and C x C covariance and the three-channel
projection; what remains is small and plain torch on the map's device - `torch.linalg.eigh` of the C x C matrix in float64
and two order statistics of the samples' 3 n projected values.

    image = feature_visualize(render_pkg["feature_map"])                 # (H, W, 3) float32 in [0, 1], on the GPU
    pca = fit_feature_pca(first_view_map);  frames = [apply_feature_pca(m, pca) for m in maps]     # one basis for a video
    import feature_pca, render; feature_pca.install(render)              # or: the reference's own script, fused

The components are the eigenvectors of the covariance for its three largest eigenvalues, each signed so that its entry of
largest magnitude is positive: the rule of scikit-learn 1.5 and later (`svd_flip(u_based_decision=False)`).  Older releases
decided the sign by U and can give mirrored colours for the same map.

HIP only; no CPU fallback.  `fit_feature_pca` reads nothing back to the host.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

MAX_CHANNELS = 4096             # F3DGS_FEATURE_PCA_MAX_CHANNELS


class FeaturePCA(NamedTuple):
    mean: torch.Tensor                  # (C,) float32: the mean of the normalised samples
    components: torch.Tensor            # (3, C) float32, unit rows
    lo: torch.Tensor                    # 0-dim float32 on the device: the 1st percentile of the samples' projection
    hi: torch.Tensor                    # 0-dim float32: the 99th
    explained_variance: torch.Tensor    # (3,) float32: the three largest eigenvalues of the covariance


def _check(feature_map, stride=1, pca=None):
    """Argument errors, raised before any device work."""
    if not torch.is_tensor(feature_map) or feature_map.dim() != 3 or feature_map.dtype != torch.float32:
        what = (tuple(feature_map.shape), feature_map.dtype) if torch.is_tensor(feature_map) else type(feature_map).__name__
        raise ValueError(f"feature_map (C, H, W) float32 expected, got {what}")
    if int(stride) != stride or stride < 1:
        raise ValueError(f"stride {stride!r}: a positive integer is needed")
    C, H, W = feature_map.shape
    if C < 3:
        raise ValueError(f"{C} channels: at least 3 are needed for 3 components")
    if C > MAX_CHANNELS:
        raise ValueError(f"{C} channels: beyond the limit of {MAX_CHANNELS}")
    if pca is None:
        n = (H * W + int(stride) - 1) // int(stride)
        if n < 3:
            raise ValueError(f"{n} samples ({H} x {W} pixels, stride {stride}): at least 3 are needed")
    else:
        if pca.mean.shape != (C,) or pca.components.shape != (3, C):
            raise ValueError(f"the fit has mean {tuple(pca.mean.shape)} and components {tuple(pca.components.shape)}, the map "
                             f"{C} channels")


def _percentiles(values: torch.Tensor, qs):
    """numpy.percentile(values, qs) with linear interpolation, by one sort on the values' device; 0-dim results."""
    v = values.reshape(-1).sort().values
    out = []
    for q in qs:
        pos = q / 100.0 * (v.numel() - 1)
        i = int(pos)
        j = min(i + 1, v.numel() - 1)
        out.append(torch.lerp(v[i], v[j], pos - i))
    return out


@torch.no_grad()
def fit_feature_pca(feature_map: torch.Tensor, stride: int = 3) -> FeaturePCA:
    """The reference's fit: PCA(3) of every `stride`-th pixel (row-major over H * W) of the L2-normalised map, and the 1st
    and 99th percentile of those samples' projection.  feature_map (C, H, W) float32 on the GPU, C >= 3, at least 3 samples;
    never modified.  Two calls on the same map give the same bits."""
    _check(feature_map, stride)
    from diff_gaussian_rasterization import _C
    fm = feature_map.detach().contiguous()
    mean64, cov = _C.feature_pca_moments(fm, int(stride))
    w, v = torch.linalg.eigh(cov)                               # ascending, float64, on the map's device
    comp = v[:, -3:].flip(1).t()                                # (3, C): the largest first
    big = comp.gather(1, comp.abs().argmax(dim=1, keepdim=True))
    comp = comp * torch.where(big < 0, -1.0, 1.0)
    mean, comp = mean64.to(torch.float32), comp.to(torch.float32).contiguous()
    t = _C.feature_pca_project(fm, mean, comp)                  # raw projection of every pixel
    lo, hi = _percentiles(t.reshape(-1, 3)[::int(stride)], (1.0, 99.0))
    return FeaturePCA(mean, comp, lo, hi, w[-3:].flip(0).to(torch.float32))


@torch.no_grad()
def apply_feature_pca(feature_map: torch.Tensor, pca: FeaturePCA) -> torch.Tensor:
    """(H, W, 3) float32 on the map's device: clamp(((x / ||x|| - mean) . components - lo) / (hi - lo), 0, 1) per pixel, one
    pass over the map.  One fit applied to any view gives a consistent basis and range."""
    _check(feature_map, pca=pca)
    from diff_gaussian_rasterization import _C
    return _C.feature_pca_project(feature_map.detach(), pca.mean, pca.components, pca.lo, pca.hi)


def feature_visualize(feature_map: torch.Tensor, stride: int = 3) -> torch.Tensor:
    """The reference's picture, on the GPU: apply_feature_pca(feature_map, fit_feature_pca(feature_map))."""
    return apply_feature_pca(feature_map, fit_feature_pca(feature_map, stride))


def feature_visualize_saving(feature: torch.Tensor) -> torch.Tensor:
    """Drop-in for the reference's function: the (H, W, 3) float32 image as a CPU tensor."""
    return feature_visualize(feature).cpu()


def install(module):
    """Sets `feature_visualize_saving` in an imported `render` module, so that the reference's own script draws its PCA images
    with the fused kernels.  Returns the module."""
    module.feature_visualize_saving = feature_visualize_saving
    return module
