"""The contribution pass: from a region of a rendered view back to the Gaussians behind it.

The rasterizer's forward call leaves, in its three state buffers, everything needed to ask "which Gaussians did this pixel
blend, and with which weight?".  One more walk over those tile lists (csrc/contrib.hip behind include/f3dgs.h:
f3dgs_contributions) reproduces the forward's blend weights w = alpha * T bit for bit and gives

    per pixel      alpha, the median depth (where T crosses 0.5), the dominant Gaussian's index and its weight
    per Gaussian   acc[g, k] += sum over pixels of w * masks[k, pixel], acc[g, K] += sum of w, wmax[g] = max(wmax[g], w)

without a backward pass, autograd leaves or fake feature channels.  It is the missing path from a 2D mask - of a SAM-distilled
model, of this package's own `segment()`, of a click in the viewer - to the `mask` argument of `edit.apply_edit`:

    lifter = MaskLifter(P, K, device)
    for cam in cameras:
        lifter.add_view(cam, gaussians, pipe, bg, masks_of(cam))        # (K, H, W) bool / uint8 / float
    edit.apply_edit(opacity, shs, lifter.select(0.5)[:, k], {"deletion": True})

A label map - one class per pixel, as segment() or sam_masks.instance_map() give it - is lifted in ONE walk per view however many
classes it has (f3dgs_label_votes), without the (L, H, W) one-hot stack:

    lifter = LabelLifter(P, 150, device)
    for cam in cameras:
        lifter.add_view(cam, gaussians, pipe, bg, label_map_of(cam))    # (H, W) uint8 / int32 / int64
    edit.apply_edit(opacity, shs, lifter.select(cls), {"deletion": True});  picture = lifter.label_image(ids)

Instance maps whose ids are NOT consistent between views (SAM's) go through instances.InstanceLifter, a LabelLifter that
associates every view's masks with the 3D instances built so far before it adds them.

HIP only; no CPU fallback.  Nothing is read back to the host.
"""
from __future__ import annotations

import math

import torch

from diff_gaussian_rasterization import _C, GaussianRasterizationSettings

MAX_MASKS = 7           # F3DGS_CONTRIB_MAX_MASKS: mask columns one walk carries (more are taken in groups)
MAX_LABELS = 65536      # F3DGS_LABEL_VOTES_MAX_LABELS: classes of a label vote
LABEL_DTYPES = (torch.uint8, torch.int32, torch.int64)


def _need_device(t, name):
    if not t.is_cuda:
        raise ValueError(f"{name} must live on a HIP device (got {t.device}): the contribution pass has no CPU path")


def _check_masks(masks, H, W, dev):
    if masks is None:
        return None
    if masks.dim() == 2:
        masks = masks[None]
    if masks.dim() != 3 or tuple(masks.shape[1:]) != (H, W):
        raise ValueError(f"masks (K, {H}, {W}) expected, got {tuple(masks.shape)}")
    _need_device(masks, "masks")
    if masks.device != dev:
        raise ValueError(f"masks on {masks.device}, the Gaussians on {dev}")
    if masks.dtype in (torch.bool, torch.uint8):
        masks = masks.to(torch.float32)
    if masks.dtype != torch.float32:
        raise ValueError(f"masks must be bool, uint8 or float32, got {masks.dtype}")
    return masks.contiguous()


def _check_acc(acc, wmax, P, K, dev):
    if acc is not None:
        _need_device(acc, "acc")
        if acc.dtype != torch.float32 or not acc.is_contiguous() or tuple(acc.shape) != (P, K + 1) or acc.device != dev:
            raise ValueError(f"acc must be a contiguous float32 ({P}, {K + 1}) tensor on {dev} (one column per mask and the "
                             f"weight total), got {acc.dtype} {tuple(acc.shape)} on {acc.device}")
    if wmax is not None:
        _need_device(wmax, "wmax")
        if wmax.dtype != torch.float32 or not wmax.is_contiguous() or tuple(wmax.shape) != (P,) or wmax.device != dev:
            raise ValueError(f"wmax must be a contiguous float32 ({P},) tensor on {dev}, got {wmax.dtype} {tuple(wmax.shape)} "
                             f"on {wmax.device}")


def _check_gaussians(means3D, shs, colors_precomp, scales, rotations, cov3D_precomp):
    """The argument rules of the rasterizer's forward call; returns (P, device)."""
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise ValueError(f"means3D (P, 3) expected, got {tuple(means3D.shape)}")
    if (shs is None) == (colors_precomp is None):
        raise ValueError("provide exactly one of shs and colors_precomp")
    if (scales is None or rotations is None) == (cov3D_precomp is None) or ((scales is None) != (rotations is None)):
        raise ValueError("provide exactly one of the scales / rotations pair and cov3D_precomp")
    _need_device(means3D, "means3D")
    return means3D.shape[0], means3D.device


def _forward(rs, means3D, opacities, shs, colors_precomp, semantic_feature, scales, rotations, cov3D_precomp):
    """One forward call of the rasterizer (the caller holds no_grad): render, feature_map, depth, radii and the state tuple
    (geom, binning, img, P, num_rendered, H, W) the passes take."""
    P, H, W = means3D.shape[0], int(rs.image_height), int(rs.image_width)
    empty = torch.Tensor([])
    opt = lambda t: empty if t is None else t.detach()
    feat = means3D.new_zeros((P, 1, 0)) if semantic_feature is None else semantic_feature.detach()
    (num_rendered, color, feature_map, depth, radii, geom, binning, img) = _C.rasterize_gaussians(
        rs.bg, means3D.detach(), opt(colors_precomp), feat, opacities.detach(), opt(scales), opt(rotations), rs.scale_modifier,
        opt(cov3D_precomp), rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, opt(shs), rs.sh_degree, rs.campos,
        rs.prefiltered, rs.debug)
    return color, feature_map, depth, radii, (geom, binning, img, P, num_rendered, H, W)


def contributions(raster_settings, *, means3D, opacities, shs=None, colors_precomp=None, semantic_feature=None, scales=None,
                  rotations=None, cov3D_precomp=None, masks=None, acc=None, wmax=None, pixel_outputs=True) -> dict:
    """One forward call of the rasterizer and the contribution pass over its state, under no_grad.

    masks: (K, H, W) or (H, W), bool / uint8 / float32 (soft values allowed), any K - more than seven are taken in groups of
    seven over the same forward state (only the pass is repeated).  acc: (P, K + 1) float32, ADDED to (column K: the weight
    total, added once); made of zeros when masks are given without it.  wmax: (P,) float32 of non-negative values, MAX-ed into,
    or None.  pixel_outputs: alpha, median_depth, ids (int32, -1: nothing blended), id_weight, each (H, W).
    Returns render, feature_map, depth, radii and alpha, median_depth, ids, id_weight, acc, wmax (None where not asked for)."""
    rs = raster_settings
    H, W = int(rs.image_height), int(rs.image_width)
    P, dev = _check_gaussians(means3D, shs, colors_precomp, scales, rotations, cov3D_precomp)
    masks = _check_masks(masks, H, W, dev)
    K = 0 if masks is None else masks.shape[0]
    if acc is None and masks is not None:
        acc = torch.zeros(P, K + 1, device=dev, dtype=torch.float32)
    _check_acc(acc, wmax, P, K, dev)
    if acc is None and wmax is None and not pixel_outputs:
        raise ValueError("nothing asked for: no masks, no acc, no wmax and pixel_outputs=False")

    with torch.no_grad():
        color, feature_map, depth, radii, state = _forward(rs, means3D, opacities, shs, colors_precomp, semantic_feature, scales,
                                                           rotations, cov3D_precomp)
        pix = (None, None, None, None)
        if K <= MAX_MASKS:
            pix = _C.contributions(*state, masks if K else None, acc, wmax, bool(pixel_outputs))
        else:
            # groups of seven: each walk adds its columns into a (P, k + 1) block; the weight total of the first one is kept
            for k0 in range(0, K, MAX_MASKS):
                k1 = min(K, k0 + MAX_MASKS)
                first = k0 == 0
                part = torch.zeros(P, k1 - k0 + 1, device=dev, dtype=torch.float32)
                out = _C.contributions(*state, masks[k0:k1], part, wmax if first else None, bool(pixel_outputs) and first)
                acc[:, k0:k1] += part[:, :-1]
                if first:
                    acc[:, K] += part[:, -1]
                    pix = out
    return {"render": color, "feature_map": feature_map, "depth": depth, "radii": radii, "alpha": pix[0], "median_depth": pix[1],
            "ids": pix[2], "id_weight": pix[3], "acc": acc, "wmax": wmax}


def _render_inputs(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color):
    """The raster settings and the Gaussian arguments of the reference's render() (gaussian_renderer/__init__.py:173)."""
    raster_settings = GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5), bg=bg_color,
        scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=pc.active_sh_degree, campos=viewpoint_camera.camera_center,
        prefiltered=False, debug=pipe.debug)
    scales = rotations = cov3D_precomp = None
    if pipe.compute_cov3D_python:
        cov3D_precomp = pc.get_covariance(scaling_modifier)
    else:
        scales, rotations = pc.get_scaling, pc.get_rotation
    shs = colors_precomp = None
    if override_color is None:
        if pipe.convert_SHs_python:
            from utils.sh_utils import eval_sh          # the caller's own module, as in the reference
            shs_view = pc.get_features.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
            dir_pp = pc.get_xyz - viewpoint_camera.camera_center.repeat(pc.get_features.shape[0], 1)
            sh2rgb = eval_sh(pc.active_sh_degree, shs_view, dir_pp / dir_pp.norm(dim=1, keepdim=True))
            colors_precomp = torch.clamp_min(sh2rgb + 0.5, 0.0)
        else:
            shs = pc.get_features
    else:
        colors_precomp = override_color
    return raster_settings, dict(means3D=pc.get_xyz, opacities=pc.get_opacity, shs=shs, colors_precomp=colors_precomp,
                                 semantic_feature=pc.get_semantic_feature, scales=scales, rotations=rotations,
                                 cov3D_precomp=cov3D_precomp)


def render_contributions(viewpoint_camera, pc, pipe, bg_color, masks=None, acc=None, wmax=None, pixel_outputs=True,
                         scaling_modifier=1.0, override_color=None) -> dict:
    """`contributions` with the argument conventions of the reference's render() (gaussian_renderer/__init__.py:173):
    camera, Gaussian model, pipeline flags, background."""
    raster_settings, kw = _render_inputs(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color)
    return contributions(raster_settings, masks=masks, acc=acc, wmax=wmax, pixel_outputs=pixel_outputs, **kw)


def _check_labels(labels, H, W, dev):
    if not torch.is_tensor(labels) or labels.dtype not in LABEL_DTYPES or tuple(labels.shape) != (H, W):
        got = f"{labels.dtype} {tuple(labels.shape)}" if torch.is_tensor(labels) else type(labels).__name__
        raise ValueError(f"labels: a uint8, int32 or int64 ({H}, {W}) tensor expected (a map of another size is the caller's to "
                         f"resize), got {got}")
    _need_device(labels, "labels")
    if labels.device != dev:
        raise ValueError(f"labels on {labels.device}, the Gaussians on {dev}")
    return labels.detach().contiguous()


def _check_votes(acc, P, L, dev):
    _need_device(acc, "acc")
    if acc.dtype != torch.float32 or not acc.is_contiguous() or tuple(acc.shape) != (P, L + 1) or acc.device != dev:
        raise ValueError(f"acc must be a contiguous float32 ({P}, {L + 1}) tensor on {dev} (one column per class and the weight "
                         f"total), got {acc.dtype} {tuple(acc.shape)} on {acc.device}")


def label_votes(raster_settings, *, means3D, opacities, shs=None, colors_precomp=None, semantic_feature=None, scales=None,
                rotations=None, cov3D_precomp=None, labels, num_classes, acc=None) -> dict:
    """One forward call of the rasterizer and the label vote over its state, under no_grad: what `contributions` gives for
    masks=MaskLifter.from_label_map(labels, num_classes), in ONE walk whatever num_classes is and without the one-hot stack.

    labels: (H, W) uint8 / int32 / int64 on the Gaussians' device, e.g. the map of segment() (at the view's size: a map of
    another size is the caller's to resize) or sam_masks.instance_map(); a label outside [0, num_classes) belongs to no class
    but counts in the weight total.  acc: (P, num_classes + 1) float32, ADDED to (the last column: the weight total); made of
    zeros when not given.  Returns render, feature_map, depth, radii and acc."""
    rs = raster_settings
    H, W = int(rs.image_height), int(rs.image_width)
    P, dev = _check_gaussians(means3D, shs, colors_precomp, scales, rotations, cov3D_precomp)
    L = int(num_classes)
    if not 1 <= L <= MAX_LABELS:
        raise ValueError(f"num_classes = {num_classes}: 1 .. {MAX_LABELS} expected")
    labels = _check_labels(labels, H, W, dev)
    if acc is None:
        acc = torch.zeros(P, L + 1, device=dev, dtype=torch.float32)
    _check_votes(acc, P, L, dev)
    with torch.no_grad():
        color, feature_map, depth, radii, state = _forward(rs, means3D, opacities, shs, colors_precomp, semantic_feature, scales,
                                                           rotations, cov3D_precomp)
        _C.label_votes(*state, labels, L, acc)
    return {"render": color, "feature_map": feature_map, "depth": depth, "radii": radii, "acc": acc}


def render_label_votes(viewpoint_camera, pc, pipe, bg_color, labels, num_classes, acc=None, scaling_modifier=1.0,
                       override_color=None) -> dict:
    """`label_votes` with the argument conventions of the reference's render(), as render_contributions."""
    raster_settings, kw = _render_inputs(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color)
    return label_votes(raster_settings, labels=labels, num_classes=num_classes, acc=acc, **kw)


class MaskLifter:
    """Lifts K 2D masks, seen in any number of views, to the P Gaussians: per Gaussian the share of its blend weight that fell
    inside each mask, summed over the views."""

    def __init__(self, P: int, K: int, device):
        if P < 0 or K < 1:
            raise ValueError(f"MaskLifter(P={P}, K={K}): P >= 0 and K >= 1 expected")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"MaskLifter needs a HIP device (got {device}): the contribution pass has no CPU path")
        self.P, self.K = int(P), int(K)
        self.acc = torch.zeros(self.P, self.K + 1, device=device, dtype=torch.float32)
        self.wmax = torch.zeros(self.P, device=device, dtype=torch.float32)
        self.views = 0

    def add_view(self, viewpoint_camera, pc, pipe, bg_color, masks, scaling_modifier=1.0, override_color=None) -> dict:
        """Accumulates one view's masks (K, H, W).  Returns the view's render dictionary (no per-pixel outputs)."""
        if masks is None or (masks.dim() == 3 and masks.shape[0] != self.K) or (masks.dim() == 2 and self.K != 1) or masks.dim() not in (2, 3):
            raise ValueError(f"masks ({self.K}, H, W) expected, got {None if masks is None else tuple(masks.shape)}")
        out = render_contributions(viewpoint_camera, pc, pipe, bg_color, masks=masks, acc=self.acc, wmax=self.wmax,
                                   pixel_outputs=False, scaling_modifier=scaling_modifier, override_color=override_color)
        self.views += 1
        return out

    def seen(self, min_weight: float = 0.0) -> torch.Tensor:
        """(P,) bool: the Gaussians whose weight total over the views exceeds min_weight."""
        return self.acc[:, self.K] > min_weight

    def ratios(self) -> torch.Tensor:
        """(P, K): weight inside mask k over the weight total; 0 where a Gaussian was never seen."""
        den = self.acc[:, self.K:]
        return torch.where(den > 0, self.acc[:, :self.K] / den.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(den))

    def select(self, threshold: float = 0.5, min_weight: float = 0.0) -> torch.Tensor:
        """(P, K) bool: seen Gaussians with at least `threshold` of their weight inside mask k.  A column is a `mask` of
        edit.apply_edit."""
        return (self.ratios() >= threshold) & self.seen(min_weight)[:, None]

    def labels(self) -> torch.Tensor:
        """(P,) int64: the mask that holds most of the Gaussian's weight (torch.argmax of the sums), -1 where unseen."""
        lab = self.acc[:, :self.K].argmax(dim=1)
        return torch.where(self.seen(), lab, torch.full_like(lab, -1))

    @staticmethod
    def from_label_map(label_map: torch.Tensor, num_classes: int) -> torch.Tensor:
        """(num_classes, H, W) float32 one-hot masks of an (H, W) integer label map, e.g. the labels of segment(); labels
        outside [0, num_classes) belong to no mask."""
        if label_map.dim() != 2 or label_map.dtype.is_floating_point or label_map.dtype == torch.bool:
            raise ValueError(f"label_map: an (H, W) integer tensor expected, got {label_map.dtype} {tuple(label_map.shape)}")
        if num_classes < 1:
            raise ValueError(f"num_classes = {num_classes}")
        classes = torch.arange(num_classes, device=label_map.device, dtype=label_map.dtype)
        return (label_map[None] == classes[:, None, None]).to(torch.float32)


class LabelLifter:
    """Labels the P Gaussians in 3D from label maps of L classes seen in any number of views: per Gaussian the blend weight that
    fell on each class, summed over the views - one walk per view (f3dgs_label_votes), whatever L is."""

    def __init__(self, P: int, L: int, device):
        if P < 0 or not 1 <= L <= MAX_LABELS:
            raise ValueError(f"LabelLifter(P={P}, L={L}): P >= 0 and 1 <= L <= {MAX_LABELS} expected")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"LabelLifter needs a HIP device (got {device}): the label vote has no CPU path")
        self.P, self.L = int(P), int(L)
        self.acc = torch.zeros(self.P, self.L + 1, device=device, dtype=torch.float32)
        self.views = 0

    def add_view(self, viewpoint_camera, pc, pipe, bg_color, label_map, scaling_modifier=1.0, override_color=None) -> dict:
        """Accumulates one view's (H, W) label map.  Returns the view's render dictionary."""
        out = render_label_votes(viewpoint_camera, pc, pipe, bg_color, label_map, self.L, acc=self.acc,
                                 scaling_modifier=scaling_modifier, override_color=override_color)
        self.views += 1
        return out

    def seen(self, min_weight: float = 0.0) -> torch.Tensor:
        """(P,) bool: the Gaussians whose weight total over the views exceeds min_weight."""
        return self.acc[:, self.L] > min_weight

    def _share(self, column: torch.Tensor) -> torch.Tensor:
        den = self.acc[:, self.L]
        return torch.where(den > 0, column / den.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(den))

    def labels(self) -> torch.Tensor:
        """(P,) int64: the class that holds most of the Gaussian's weight (torch.argmax of the sums), -1 where the Gaussian was
        never seen - or seen only under labels outside [0, L)."""
        top, lab = self.acc[:, :self.L].max(dim=1)
        return torch.where(top > 0, lab, torch.full_like(lab, -1))

    def confidence(self) -> torch.Tensor:
        """(P,) float32: the winning class's weight over the weight total; 0 where unseen."""
        return self._share(self.acc[:, :self.L].max(dim=1)[0])

    def ratios(self) -> torch.Tensor:
        """(P, L): weight on class l over the weight total; 0 where a Gaussian was never seen."""
        den = self.acc[:, self.L:]
        return torch.where(den > 0, self.acc[:, :self.L] / den.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(den))

    def select(self, cls: int, threshold: float = 0.5, min_weight: float = 0.0) -> torch.Tensor:
        """(P,) bool, a `mask` of edit.apply_edit: the seen Gaussians with at least `threshold` of their weight on class `cls` -
        column `cls` of ratios() >= threshold, formed from that column alone."""
        if not 0 <= int(cls) < self.L:
            raise ValueError(f"cls = {cls}: 0 .. {self.L - 1} expected")
        return (self._share(self.acc[:, int(cls)]) >= threshold) & self.seen(min_weight)

    def label_image(self, ids: torch.Tensor) -> torch.Tensor:
        """labels()[ids], -1 where ids == -1: the 3D labels seen from the view whose `ids` (the dominant Gaussian per pixel) came
        from contributions()."""
        if not torch.is_tensor(ids) or ids.dtype not in (torch.int32, torch.int64):
            raise ValueError("ids: an int32 or int64 tensor of Gaussian indices expected")
        lab = self.labels()
        if self.P == 0:
            return torch.full(ids.shape, -1, dtype=torch.int64, device=ids.device)
        return torch.where(ids >= 0, lab[ids.clamp_min(0).long()], torch.full((), -1, dtype=torch.int64, device=ids.device))


__all__ = ["MAX_MASKS", "MAX_LABELS", "contributions", "render_contributions", "MaskLifter", "label_votes", "render_label_votes",
           "LabelLifter"]
