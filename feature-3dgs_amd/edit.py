"""Language-guided editing: delete, extract or recolour the Gaussians whose semantic feature matches a text prompt.

The reference's `render_edit` (gaussian_renderer/__init__.py:58-170) scores every Gaussian against K text embeddings with
about ten PyTorch ops over the whole (P, C) feature table per frame (calculate_selection_score and
calculate_selection_score_delete, :21-55).  Here that is ONE HIP kernel (csrc/edit.hip behind include/f3dgs.h:
f3dgs_edit_select): one pass over the table, in the reference's number formats - the fp16 roundings of its half GEMM and
half softmax decide which side of the threshold a Gaussian falls on, so they are reproduced, not improved on.

    from edit import render_edit                     # the reference's signature and result dictionary
    import edit, gaussian_renderer; edit.install(gaussian_renderer)     # or: the reference's own render_edit, fused

HIP only; no CPU fallback.  The call reads nothing back to the host: it may be captured in a graph.
"""
from __future__ import annotations

import math

import torch

from diff_gaussian_rasterization import _C, GaussianRasterizationSettings, GaussianRasterizer

MAX_TEXTS = 64                  # F3DGS_EDIT_MAX_TEXTS
MAX_TEXT_ELEMENTS = 32768       # F3DGS_EDIT_MAX_TEXT_ELEMENTS: the fp16 text block lives in 64 KB of LDS


def _check(features, text_features, score_threshold, positive_ids, variant):
    """Argument errors, raised before any device work.  Returns (features as (P, C), positive mask, first positive)."""
    if variant not in ("select", "delete"):
        raise ValueError(f"variant {variant!r}: 'select' or 'delete'")
    if features.dim() == 3 and features.shape[1] == 1:
        features = features[:, 0, :]
    if features.dim() != 2 or text_features.dim() != 2 or features.shape[1] != text_features.shape[1]:
        raise ValueError(f"features (P, C) or (P, 1, C) and text_features (K, C) expected, got {tuple(features.shape)} and "
                         f"{tuple(text_features.shape)}")
    K, C = text_features.shape
    if K < 1 or C < 1:
        raise ValueError("empty text_features")
    if K > MAX_TEXTS or K * C > MAX_TEXT_ELEMENTS:
        raise ValueError(f"{K} text embeddings of {C} channels: beyond the limit of {MAX_TEXTS} embeddings and K * C <= "
                         f"{MAX_TEXT_ELEMENTS}")
    ids = [int(i) for i in positive_ids]
    if not ids:
        raise ValueError("positive_ids is empty")
    if len(set(ids)) != len(ids):
        raise ValueError(f"positive_ids {ids} holds a duplicate")
    if any(i < 0 or i >= K for i in ids):
        raise ValueError(f"positive_ids {ids} out of range for {K} text embeddings")
    if K == 1 and score_threshold is None:
        raise ValueError("a single text embedding needs a score_threshold")
    return features, sum(1 << i for i in ids), ids[0]


def _run(features, text, score_threshold, positive_ids, variant, inplace, text_normalized, want_score, opacity, fill_unselected):
    f2, pmask, first = _check(features, text, score_threshold, positive_ids, variant)
    flags = (_C.EDIT_DELETE if variant == "delete" else _C.EDIT_SELECT) | (_C.EDIT_TEXT_NORMALIZED if text_normalized else 0) | \
        (_C.EDIT_FILL_UNSELECTED if fill_unselected else 0)
    thr = None if score_threshold is None else float(score_threshold)
    work = f2
    if inplace and not (f2.is_contiguous() and f2.data_ptr() % 16 == 0):
        work = f2.contiguous().clone()          # an odd view: compute on an aligned copy and copy the rows back
    mask, score, op_out = _C.edit_select(work, text, pmask, first, flags, thr, inplace, want_score, opacity)
    if work is not f2:
        f2.copy_(work)
    return mask, score, op_out


def selection_mask(features, text_features, score_threshold=None, positive_ids=(0,), variant="select", normalize_inplace=False,
                   return_score=False, opacity=None, fill_unselected=False):
    """The (P,) float32 0/1 mask of the Gaussians that match: variant "select" is the reference's calculate_selection_score,
    "delete" its calculate_selection_score_delete (include/f3dgs.h lists the branches).  features: (P, C) or (P, 1, C)
    float32 on the GPU, left untouched unless normalize_inplace (then each row is divided by its norm, as the reference
    does); text_features (K, C), never modified.  return_score: also the (P,) decided quantity (s_0, q or q2) as float32.
    opacity (P,) or (P, 1): also a copy of it with the selected Gaussians (fill_unselected: the others) zeroed, written by
    the same kernel.  Returns the mask, or a tuple (mask[, score][, filled opacity])."""
    mask, score, filled = _run(features, text_features, score_threshold, positive_ids, variant, normalize_inplace, False,
                               return_score, opacity, fill_unselected)
    out = (mask,) + ((score,) if return_score else ()) + ((filled,) if opacity is not None else ())
    return out if len(out) > 1 else mask


def _drop_in(features, query_features, score_threshold, positive_ids, variant):
    _check(features, query_features, score_threshold, positive_ids, variant)
    query_features /= query_features.norm(dim=-1, keepdim=True)          # the reference's side effect, by the same op
    mask, _, _ = _run(features, query_features, score_threshold, positive_ids, variant, True, True, False, None, False)
    return mask


def calculate_selection_score(features, query_features, score_threshold=None, positive_ids=[0]):
    """Drop-in for the reference's function: same result, and `features` and `query_features` come back normalised in place."""
    return _drop_in(features, query_features, score_threshold, positive_ids, "select")


def calculate_selection_score_delete(features, query_features, score_threshold=None, positive_ids=[0]):
    """Drop-in for the reference's function; without a threshold and with several texts it returns a bool mask, as there."""
    mask = _drop_in(features, query_features, score_threshold, positive_ids, "delete")
    if query_features.shape[0] > 1 and score_threshold is None:
        return mask.bool()
    return mask


def apply_edit(opacity, shs, mask, op_dict):
    """render_edit's three operations for one mask (:136-148), in place like the reference: "deletion" zeroes the opacity
    of the selected Gaussians, "extraction" that of the others, "color_func" blends the DC colour `shs[:, 0, :]` towards
    op_dict["color_func"](shs[:, 0, :]).  `mask`: (P,) 0/1 (float or bool), or a dict with one mask per operation.
    Returns (opacity, shs)."""
    of = lambda op: (mask[op] if isinstance(mask, dict) else mask).to(torch.float32)
    if "deletion" in op_dict:
        opacity.masked_fill_(of("deletion")[:, None] >= 0.5, 0)
    if "extraction" in op_dict:
        opacity.masked_fill_(of("extraction")[:, None] <= 0.5, 0)
    if "color_func" in op_dict:
        s = of("color_func")
        shs[:, 0, :] = shs[:, 0, :] * (1 - s[:, None]) + op_dict["color_func"](shs[:, 0, :]) * s[:, None]
    return opacity, shs


def render_edit(viewpoint_camera, pc, pipe, bg_color, text_feature, edit_dict, scaling_modifier=1.0, override_color=None):
    """The reference's render_edit on this package's rasterizer and the fused selection: same arguments, same result
    dictionary, same side effects (the semantic features and text_feature are normalised in place, opacity and the DC
    colours are edited in place).  With only one of "deletion" / "extraction" asked, the opacity fill rides in the
    selection kernel."""
    screenspace_points = torch.zeros_like(pc.get_xyz, dtype=pc.get_xyz.dtype, requires_grad=True, device="cuda") + 0
    try:
        screenspace_points.retain_grad()
    except Exception:
        pass
    raster_settings = GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5), bg=bg_color,
        scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=pc.active_sh_degree, campos=viewpoint_camera.camera_center,
        prefiltered=False, debug=pipe.debug)
    rasterizer = GaussianRasterizer(raster_settings=raster_settings)
    means3D, opacity = pc.get_xyz, pc.get_opacity
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
    semantic_feature = pc.get_semantic_feature
    positive_ids, thr, op_dict = edit_dict["positive_ids"], edit_dict["score_threshold"], edit_dict["operations"]
    feats = semantic_feature[:, 0, :]

    fills = [op for op in ("deletion", "extraction") if op in op_dict]
    if len(fills) == 1:
        # one fill: fused.  The kernel writes the filled opacity; it is copied into the model's tensor as masked_fill_ would
        _check(feats, text_feature, thr, positive_ids, "select")
        text_feature /= text_feature.norm(dim=-1, keepdim=True)
        variant = "delete" if fills[0] == "deletion" else "select"
        _, _, filled = _run(feats, text_feature, thr, positive_ids, variant, True, True, False, opacity.detach(),
                            fills[0] == "extraction")
        with torch.no_grad():
            opacity.copy_(filled.view_as(opacity))
    else:
        if "deletion" in op_dict:
            m = calculate_selection_score_delete(feats, text_feature, score_threshold=thr, positive_ids=positive_ids)
            apply_edit(opacity, shs, m, {"deletion": True})
        if "extraction" in op_dict:
            m = calculate_selection_score(feats, text_feature, score_threshold=thr, positive_ids=positive_ids)
            apply_edit(opacity, shs, m, {"extraction": True})
    if "color_func" in op_dict:
        m = calculate_selection_score(feats, text_feature, score_threshold=thr, positive_ids=positive_ids)
        apply_edit(opacity, shs, m, {"color_func": op_dict["color_func"]})

    rendered_image, feature_map, radii, depth = rasterizer(
        means3D=means3D, means2D=screenspace_points, shs=shs, colors_precomp=colors_precomp, semantic_feature=semantic_feature,
        opacities=opacity, scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp)
    return {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii,
            "feature_map": feature_map, "depth": depth}


def install(module):
    """Rebinds calculate_selection_score and calculate_selection_score_delete in an imported `gaussian_renderer` module, so
    that the reference's own render_edit runs unmodified on the fused kernel.  Returns the module."""
    for name in ("calculate_selection_score", "calculate_selection_score_delete"):
        if not hasattr(module, name):
            raise AttributeError(f"{module.__name__} has no {name}: not the reference's gaussian_renderer")
    module.calculate_selection_score = calculate_selection_score
    module.calculate_selection_score_delete = calculate_selection_score_delete
    return module
