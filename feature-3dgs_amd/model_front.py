"""The model's front end: what stands between a GaussianModel's raw parameters and the op, and the bookkeeping behind it.

Every `render()` of the reference runs the model's getters (scene/gaussian_model.py:98-127): `exp` of the scaling,
`F.normalize` of the rotation (a norm, a clamp and a divide), `sigmoid` of the opacity, `cat` of the two SH tensors, and a
`zeros_like(...) + 0` for the screen-space points; autograd mirrors each on the way back, and the cat's gradient becomes two
strided slices that are cloned to contiguous.  After the op, train.py:132-133 keeps the densification statistics with
boolean-mask indexing - every mask index is a `nonzero` and a host read, so the iteration cannot be captured in a graph.

Here that is three HIP kernels (csrc/model_front.hip behind include/f3dgs.h: f3dgs_activate_forward, f3dgs_activate_backward,
f3dgs_densify_stats), one launch each, none of which reads anything back to the host:

    from model_front import render                   # the reference's signature and result dictionary
    import model_front, gaussian_renderer; model_front.install(gaussian_renderer)     # or: rebind the reference's own name
    model_front.add_densification_stats(gaussians, render_pkg)                        # train.py:132-133 in one launch

The SH pack moves the bytes `torch.cat` moves: what is saved is launches, host reads and the copies of the activation
results that autograd keeps beside the ones handed to the op - not bandwidth.  HIP only; no CPU fallback.
"""
from __future__ import annotations

import math

import torch

from diff_gaussian_rasterization import _C, GaussianRasterizationSettings, GaussianRasterizer


class _Activate(torch.autograd.Function):
    """All four getters as one launch, their gradients as one launch.  Saved for the backward: the raw rotation and this
    function's own `scales` and `opacities` outputs - nothing else."""

    @staticmethod
    def forward(ctx, scaling, rotation, opacity, features_dc, features_rest):
        scales, rotations, opacities, shs = _C.activate_forward(scaling, rotation, opacity, features_dc, features_rest)
        first = next(t for t in (scaling, rotation, opacity, features_dc) if t is not None)
        ctx.P = first.shape[0]
        ctx.M = 1 if shs is None else shs.shape[1]
        ctx.has = tuple(t is not None for t in (scaling, rotation, opacity, features_dc, features_rest))
        ctx.set_materialize_grads(False)        # an unused output arrives as None: the kernel takes NULL as zeros
        need = ctx.needs_input_grad
        ctx.mark_non_differentiable(*[out for out, n in zip((scales, rotations, opacities, shs), (need[0], need[1], need[2], need[3] or need[4]))
                                      if out is not None and not n])
        ctx.save_for_backward(rotation, scales, opacities)
        return scales, rotations, opacities, shs

    @staticmethod
    def backward(ctx, g_scales, g_rotations, g_opacities, g_shs):
        raw_rotation, scales, opacities = ctx.saved_tensors
        want = [bool(h and n) for h, n in zip(ctx.has, ctx.needs_input_grad)]
        if not any(want):
            return None, None, None, None, None
        like = next(t for t in (scales, raw_rotation, opacities, g_shs, g_scales, g_rotations, g_opacities) if t is not None)
        return _C.activate_backward(ctx.P, ctx.M, scales, raw_rotation, opacities, g_scales, g_rotations, g_opacities, g_shs,
                                    want, like)


def activate(scaling, rotation, opacity, features_dc, features_rest):
    """(scales, rotations, opacities, shs) = (exp(scaling), F.normalize(rotation), sigmoid(opacity), cat(features_dc,
    features_rest)) in one launch, differentiable with one launch.  Any argument may be None to skip its group (its result is
    then None); `features_rest` may also be None or empty with `features_dc` given (degree 0).  Raw parameters as the
    reference holds them: (P, 3), (P, 4), (P, 1), (P, 1, 3), (P, M - 1, 3) float32 on the GPU; `opacities` comes back in the
    shape of `opacity`, as get_opacity returns it."""
    if features_dc is None and features_rest is not None:
        raise ValueError("features_rest without features_dc")
    if all(t is None for t in (scaling, rotation, opacity, features_dc)):
        return None, None, None, None
    return _Activate.apply(scaling, rotation, opacity, features_dc, features_rest)


def render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0, override_color=None):
    """The reference's render (gaussian_renderer/__init__.py:173-261) with the fused front end: same arguments, same result
    dictionary.  The activations come from `activate` on `pc`'s raw parameters; with pipe.compute_cov3D_python or
    pipe.convert_SHs_python the group concerned goes through the model's getters, as in the reference."""
    xyz = pc.get_xyz
    # a leaf: it receives .grad like the reference's retained `zeros + 0`, without the add
    screenspace_points = torch.zeros_like(xyz, dtype=xyz.dtype, requires_grad=True, device=xyz.device)
    raster_settings = GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5), bg=bg_color,
        scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=pc.active_sh_degree, campos=viewpoint_camera.camera_center,
        prefiltered=False, debug=pipe.debug)
    rasterizer = GaussianRasterizer(raster_settings=raster_settings)

    cov_python = bool(pipe.compute_cov3D_python)
    sh_in_op = override_color is None and not pipe.convert_SHs_python
    scales, rotations, opacity, shs = activate(
        None if cov_python else pc._scaling, None if cov_python else pc._rotation, pc._opacity,
        pc._features_dc if sh_in_op else None, pc._features_rest if sh_in_op else None)
    cov3D_precomp = pc.get_covariance(scaling_modifier) if cov_python else None
    colors_precomp = None
    if override_color is not None:
        colors_precomp = override_color
    elif pipe.convert_SHs_python:
        from utils.sh_utils import eval_sh          # the caller's own module, as in the reference
        features = pc.get_features
        shs_view = features.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
        dir_pp = xyz - viewpoint_camera.camera_center.repeat(features.shape[0], 1)
        sh2rgb = eval_sh(pc.active_sh_degree, shs_view, dir_pp / dir_pp.norm(dim=1, keepdim=True))
        colors_precomp = torch.clamp_min(sh2rgb + 0.5, 0.0)

    rendered_image, feature_map, radii, depth = rasterizer(
        means3D=xyz, means2D=screenspace_points, shs=shs, colors_precomp=colors_precomp,
        semantic_feature=pc.get_semantic_feature, opacities=opacity, scales=scales, rotations=rotations,
        cov3D_precomp=cov3D_precomp)
    return {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii,
            "feature_map": feature_map, "depth": depth}


def install(module):
    """Rebinds `render` in an imported `gaussian_renderer` module, so that the reference's train.py and render.py run on the
    fused front end unmodified.  Returns the module."""
    for name in ("render", "GaussianRasterizer"):
        if not hasattr(module, name):
            raise AttributeError(f"{module.__name__} has no {name}: not the reference's gaussian_renderer")
    module.render = render
    return module


def densification_stats(viewspace_grad, radii, xyz_gradient_accum, denom, max_radii2D):
    """For every Gaussian with radii > 0: xyz_gradient_accum += |viewspace_grad[:, :2]|, denom += 1, max_radii2D = max(
    max_radii2D, radii); the others are untouched.  In place, one launch, nothing read back.  viewspace_grad (P, 3) or None
    (zero gradients: the other two still update), radii (P,) int32; each accumulator a contiguous float32 tensor of P
    elements, or None.  On zeroed buffers the call gives one view's deltas."""
    _C.densify_stats(viewspace_grad, radii, xyz_gradient_accum, denom, max_radii2D)


def reset_opacity_(model, cap=0.01):
    """The reference's reset_opacity (scene/gaussian_model.py:231-234) IN PLACE, one launch: `model._opacity` becomes
    inverse_sigmoid(min(sigmoid(_opacity), cap)) and the Adam moments of its optimizer group become zero; the step count stays.
    The reference registers a new Parameter; here `model._opacity` keeps its identity and its address, so a captured iteration
    (train_step.CapturedTrainer) stays valid.  Works with either mode of FusedAdam, and without an optimizer."""
    p = model._opacity
    opt = getattr(model, "optimizer", None)
    st = opt.state.get(p, {}) if opt is not None else {}
    with torch.no_grad():
        _C.reset_opacity(p.detach(), st.get("exp_avg"), st.get("exp_avg_sq"), float(cap))


def add_densification_stats(model, render_pkg):
    """train.py:132-133 in one launch:  max_radii2D[vis] = max(max_radii2D[vis], radii[vis])  and
    add_densification_stats(viewspace_points, vis)  (scene/gaussian_model.py:436-438) for a render_pkg after its backward."""
    with torch.no_grad():
        densification_stats(render_pkg["viewspace_points"].grad, render_pkg["radii"], model.xyz_gradient_accum, model.denom,
                            model.max_radii2D)
