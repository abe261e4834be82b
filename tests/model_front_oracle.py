"""fp64 oracle of the model front end (include/f3dgs.h: f3dgs_activate_forward, f3dgs_activate_backward,
f3dgs_densify_stats), straight from the formulas of the contract.  torch on the CPU; every input is taken as it is (fp32 values
are widened exactly) and every result is float64.  `None` stands for a NULL pointer."""
import torch

EPS = 1e-12


def _d(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def activate_forward(scaling, rotation, opacity, features_dc, features_rest):
    """-> (scales, rotations, opacities, shs); a group whose input is None gives None."""
    scaling, rotation, opacity, dc, rest = map(_d, (scaling, rotation, opacity, features_dc, features_rest))
    scales = None if scaling is None else torch.exp(scaling)
    rotations = None
    if rotation is not None:
        n = torch.sqrt((rotation * rotation).sum(-1, keepdim=True))
        rotations = rotation / torch.clamp_min(n, EPS)
    opacities = None if opacity is None else 1.0 / (1.0 + torch.exp(-opacity))
    shs = None
    if dc is not None:
        shs = dc.clone() if rest is None or rest.numel() == 0 else torch.cat((dc, rest), dim=1)
    return scales, rotations, opacities, shs


def activate_backward(scales, raw_rotation, opacities, dL_dscale, dL_drot, dL_dopacity, dL_dsh, P, M):
    """-> (d_raw_scaling, d_raw_rotation, d_raw_opacity, d_features_dc, d_features_rest); a None upstream counts as zeros.
    scales / opacities: the forward's outputs (whatever precision they were computed in), raw_rotation: its input."""
    scales, q, o, gs, gr, go, gsh = map(_d, (scales, raw_rotation, opacities, dL_dscale, dL_drot, dL_dopacity, dL_dsh))
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    d_scaling = z(P, 3) if gs is None else gs.reshape(P, 3) * scales.reshape(P, 3)
    if go is None:
        d_opacity = z(P, 1)
    else:
        o = o.reshape(P, 1)
        d_opacity = go.reshape(P, 1) * o * (1.0 - o)
    if gr is None:
        d_rotation = z(P, 4)
    else:
        g = gr.reshape(P, 4)
        n = torch.sqrt((q * q).sum(-1, keepdim=True))
        safe = torch.where(n >= EPS, n, torch.ones_like(n))
        h = q / safe
        d_rotation = torch.where(n >= EPS, (g - h * (h * g).sum(-1, keepdim=True)) / safe, g / EPS)
    if gsh is None:
        d_dc, d_rest = z(P, 1, 3), z(P, M - 1, 3)
    else:
        gsh = gsh.reshape(P, M, 3)
        d_dc, d_rest = gsh[:, :1].clone(), gsh[:, 1:].clone()
    return d_scaling, d_rotation, d_opacity, d_dc, d_rest


def densify_stats(dL_dmean2D, radii, xyz_gradient_accum, denom, max_radii2D):
    """-> the three accumulators after the call (float64, flat); None in, None out."""
    g, acc, den, mr = map(_d, (dL_dmean2D, xyz_gradient_accum, denom, max_radii2D))
    r = radii.detach().to("cpu", torch.int64).reshape(-1)
    vis = r > 0
    P = r.numel()
    norm = torch.zeros(P, dtype=torch.float64) if g is None else torch.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2)
    out_acc = None if acc is None else torch.where(vis, acc.reshape(-1) + norm, acc.reshape(-1))
    out_den = None if den is None else torch.where(vis, den.reshape(-1) + 1.0, den.reshape(-1))
    out_mr = None if mr is None else torch.where(vis, torch.maximum(mr.reshape(-1), r.to(torch.float64)), mr.reshape(-1))
    return out_acc, out_den, out_mr
