"""Helpers shared by the parity tests: run a synth scene through the HIP op / the oracle and compare."""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

def set_option(name: str, value: int) -> int:
    """Change a process-wide option of the product library (include/f3dgs.h); returns the previous value."""
    from diff_gaussian_rasterization import _C
    old = _C.get_option(name)
    _C.set_option(name, int(value))
    return old


GRAD_NAMES = ["dL_dmeans3D", "dL_dmeans2D", "dL_dsh", "dL_dcolors", "dL_dsemantic_feature", "dL_dopacity",
              "dL_dscales", "dL_drotations", "dL_dcov3D"]


def precompute_optionals(scene: dict) -> dict:
    """Add colors_precomp / cov3D_precomp variants (plain torch fp32, same formulas the reference's Python
    fall-backs use: gaussian_renderer/__init__.py:218-238)."""
    from oracle.torch_oracle import _quat_to_rot, _sh_to_rgb
    sc = dict(scene)
    d = scene["means3D"] - scene["campos"][None]
    d = d / d.norm(dim=1, keepdim=True)
    sc["colors_precomp"] = torch.clamp_min(_sh_to_rgb(scene["sh_degree"], scene["shs"], d) + 0.5, 0.0).contiguous()
    R = _quat_to_rot(scene["rotations"])
    L = R * (scene["scale_modifier"] * scene["scales"])[:, None, :]
    S = L @ L.transpose(1, 2)
    sc["cov3D_precomp"] = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()
    return sc


# ---- general cameras: arbitrary rotation and position, fx != fy, any SH width ---------------------------------------
# Views A-D have no zero or unit entry in the view rotation and a camera away from the origin; B and C have rectangular
# pixels (fy / fx = 1 / pix_aspect).  E is the family of synth.make_camera (used with SH widths other than 16 only).
VIEWS = {
    "A": dict(yaw=17.0, pitch=-11.0, roll=23.0, campos=(0.7, -0.4, -1.3), fovx_deg=60.0, pix_aspect=1.0, znear=0.01, zfar=100.0),
    "B": dict(yaw=-31.0, pitch=8.0, roll=-140.0, campos=(-2.0, 1.5, 0.6), fovx_deg=35.0, pix_aspect=2.0, znear=0.01, zfar=100.0),
    "C": dict(yaw=5.0, pitch=29.0, roll=90.0, campos=(3.0, 0.2, -0.8), fovx_deg=100.0, pix_aspect=0.5, znear=0.5, zfar=20.0),
    "D": dict(yaw=12.0, pitch=-3.0, roll=7.0, campos=(0.1, 0.1, 0.1), fovx_deg=60.0, pix_aspect=1.0, znear=0.01, zfar=100.0),
    "E": dict(yaw=0.0, pitch=0.0, roll=0.0, campos=(0.0, 0.0, 0.0), fovx_deg=60.0, pix_aspect=1.0, znear=0.01, zfar=100.0),
}
DEGREE_OF_M = {1: 0, 4: 1, 5: 1, 9: 2, 16: 3}         # the largest SH degree M coefficients hold


def view_rotation(yaw: float, pitch: float, roll: float) -> np.ndarray:
    """World-to-camera rotation R = Rz(roll) Rx(pitch) Ry(yaw), fp64, angles in degrees; Ry as synth.make_camera writes it
    (the camera looks along (sin yaw, 0, cos yaw))."""
    import math
    a, b, c = (math.radians(v) for v in (yaw, pitch, roll))
    Ry = np.array([[math.cos(a), 0.0, -math.sin(a)], [0.0, 1.0, 0.0], [math.sin(a), 0.0, math.cos(a)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(b), -math.sin(b)], [0.0, math.sin(b), math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0.0], [math.sin(c), math.cos(c), 0.0], [0.0, 0.0, 1.0]])
    return Rz @ Rx @ Ry


def general_camera(width: int, height: int, yaw=0.0, pitch=0.0, roll=0.0, campos=(0.0, 0.0, 0.0), fovx_deg=60.0,
                   pix_aspect=1.0, znear=0.01, zfar=100.0) -> dict:
    """The camera entries of a scene dict for a camera at `campos` (world) with world-to-camera rotation view_rotation(...),
    composed as the reference's Camera composes them (scene/cameras.py:55-58): viewmatrix = W2C^T, projmatrix = view P^T,
    campos = view^-1 [3, :3].  tanfovy = tanfovx H / W pix_aspect, so fy / fx = 1 / pix_aspect.  Also R, t (fp64)."""
    import math
    from synth import projection_matrix
    fovx = math.radians(fovx_deg)
    tanfovx = math.tan(fovx / 2)
    tanfovy = tanfovx * height / width * pix_aspect
    fovy = 2 * math.atan(tanfovy)
    R = view_rotation(yaw, pitch, roll)
    t = -R @ np.asarray(campos, np.float64)
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, t
    view_t = torch.from_numpy(w2c.astype(np.float32)).t()      # a transposed view of W2C, as the reference's Camera holds it:
    campos = view_t.inverse()[3, :3].contiguous()              # the fp32 inverse rounds differently on a contiguous copy
    view = view_t.contiguous()
    proj = projection_matrix(znear, zfar, fovx, fovy).t().contiguous()
    full = (view.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0).contiguous()
    return dict(image_width=width, image_height=height, tanfovx=tanfovx, tanfovy=tanfovy, viewmatrix=view, projmatrix=full,
                campos=campos, R=R, t=t, fovx=fovx, fovy=fovy)


def general_view_scene(P: int, C: int, width: int, height: int, seed: int = 0, *, yaw=0.0, pitch=0.0, roll=0.0,
                       campos=(0.0, 0.0, 0.0), fovx_deg=60.0, pix_aspect=1.0, znear=0.01, zfar=100.0, M=16, sh_degree=None,
                       with_depth_grad=False, scale_lo=0.003, scale_hi=0.03, wide_scale=1.0) -> dict:
    """synth.make_scene seen by a general camera.  make_scene's positions are camera-frame positions (its camera is the
    identity): x and y are rescaled to the new frustum - which keeps the recipe's 2 % of splats beyond the frustum and 1 %
    at the near plane -, carried to the world frame in fp64 (R^T (m - t)) and rounded to fp32.  `shs` keeps its first M
    coefficients; sh_degree defaults to the largest M holds.  wide_scale multiplies the scales of the beyond-frustum
    splats (the first 2 %): only a splat whose 3 sigma reach back into the image is visible with the 1.3x clamp active."""
    import math
    from synth import make_scene
    if sh_degree is None:
        sh_degree = DEGREE_OF_M[M]
    sc = make_scene(P=P, C=C, width=width, height=height, seed=seed, sh_degree=sh_degree, with_depth_grad=with_depth_grad,
                    scale_lo=scale_lo, scale_hi=scale_hi)
    cam = general_camera(width, height, yaw, pitch, roll, campos, fovx_deg, pix_aspect, znear, zfar)
    R, t = cam.pop("R"), cam.pop("t")
    cam.pop("fovx"), cam.pop("fovy")
    m = sc["means3D"].double().numpy().copy()
    m[:, 0] *= cam["tanfovx"] / sc["tanfovx"]
    m[:, 1] *= cam["tanfovy"] / sc["tanfovy"]
    sc["means3D"] = torch.from_numpy(((m - t[None, :]) @ R).astype(np.float32)).contiguous()      # rows: R^T (m - t)
    n_wide = int(0.02 * P)
    if wide_scale != 1.0:
        s = sc["scales"].clone()
        s[:n_wide] *= wide_scale
        sc["scales"] = s.contiguous()
    sc["shs"] = sc["shs"][:, :M, :].contiguous()
    sc["M"] = M
    sc.update(cam)
    return sc


def view_scene(view: str, P: int, C: int, width: int, height: int, seed: int = 0, **kw) -> dict:
    return general_view_scene(P, C, width, height, seed, **VIEWS[view], **kw)


def input_conditions(scene: dict, radii, clamped) -> dict:
    """What a general-view case must hold to be worth running (fp64 restatement of the view transform): visible Gaussians
    with the 1.3x frustum clamp active in x / in y, Gaussians culled at the near plane, clamped SH colour channels."""
    m = scene["means3D"].double().numpy()
    pv = np.concatenate([m, np.ones((len(m), 1))], 1) @ scene["viewmatrix"].double().numpy()
    z = pv[:, 2]
    vis = np.asarray(radii).reshape(-1) > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        rx, ry = np.abs(pv[:, 0] / z), np.abs(pv[:, 1] / z)
    return dict(clamp_x=int((vis & (rx > 1.3 * scene["tanfovx"])).sum()), clamp_y=int((vis & (ry > 1.3 * scene["tanfovy"])).sum()),
                near_culled=int((z <= 0.2).sum()), sh_clamped=int((np.asarray(clamped).reshape(-1, 3)[vis] != 0).sum()))


def assert_input_conditions(scene: dict, radii, clamped, view: str = None, sh: bool = True):
    c = input_conditions(scene, radii, clamped)
    assert c["clamp_x"] >= 1 and c["clamp_y"] >= 1, f"no visible Gaussian with the frustum clamp active in x and in y: {c}"
    assert c["near_culled"] >= 10, c
    if sh:
        assert c["sh_clamped"] >= 1, c
    if view is not None and view != "E":
        Rv = scene["viewmatrix"][:3, :3].numpy()
        assert float(scene["campos"].norm()) > 0 and float(np.abs(scene["viewmatrix"][3, :3].numpy()).min()) > 0
        assert (Rv != 0).all() and (np.abs(Rv) != 1).all()
        fx = scene["image_width"] / (2 * scene["tanfovx"])
        fy = scene["image_height"] / (2 * scene["tanfovy"])
        if view in ("B", "C"):
            assert abs(fx / fy - 1) > 0.1, (fx, fy)
    return c


def run_oracle(scene: dict, use_precomp_color=False, use_precomp_cov=False, backward=True):
    from oracle.oracle import Oracle, scene_kwargs
    o = Oracle()
    out = o.forward(**scene_kwargs(scene, use_precomp_color, use_precomp_cov))
    grads = o.backward(scene["dL_dcolor"], scene["dL_dfeature"], scene["dL_ddepth"]) if backward else None
    return o, out, grads


def run_hip(scene: dict, use_precomp_color=False, use_precomp_cov=False, backward=True, device="cuda:0",
            debug=False):
    """Run through the reference-compatible Python surface (-> _C -> C ABI -> HIP kernels)."""
    import diff_gaussian_rasterization as dgr
    dev = torch.device(device)
    t = lambda x: x.to(dev)
    P = scene["means3D"].shape[0]
    settings = dgr.GaussianRasterizationSettings(
        image_height=scene["image_height"], image_width=scene["image_width"], tanfovx=scene["tanfovx"],
        tanfovy=scene["tanfovy"], bg=t(scene["bg"]), scale_modifier=scene["scale_modifier"],
        viewmatrix=t(scene["viewmatrix"]), projmatrix=t(scene["projmatrix"]), sh_degree=scene["sh_degree"],
        campos=t(scene["campos"]), prefiltered=False, debug=debug)
    leaf = lambda x: t(x).clone().requires_grad_(backward)
    L = dict(means3D=leaf(scene["means3D"]), means2D=leaf(torch.zeros(P, 3)), opacities=leaf(scene["opacities"]),
             semantic_feature=leaf(scene["semantic_feature"]))
    if use_precomp_color:
        L["colors_precomp"] = leaf(scene["colors_precomp"])
    else:
        L["shs"] = leaf(scene["shs"])
    if use_precomp_cov:
        L["cov3D_precomp"] = leaf(scene["cov3D_precomp"])
    else:
        L["scales"], L["rotations"] = leaf(scene["scales"]), leaf(scene["rotations"])
    color, feat, radii, depth = dgr.GaussianRasterizer(settings)(**L)
    out = dict(color=color.detach().cpu().numpy(), feature_map=feat.detach().cpu().numpy(),
               depth=depth.detach().cpu().numpy(), radii=radii.cpu().numpy())
    grads = None
    if backward:
        loss = (color * t(scene["dL_dcolor"])).sum() + (depth * t(scene["dL_ddepth"])).sum()
        if scene["C"]:
            loss = loss + (feat * t(scene["dL_dfeature"])).sum()
        loss.backward()
        g = lambda k: (L[k].grad.detach().cpu().numpy() if k in L and L[k].grad is not None else None)
        grads = dict(dL_dmeans3D=g("means3D"), dL_dmeans2D=g("means2D"), dL_dsh=g("shs"),
                     dL_dcolors=g("colors_precomp"), dL_dsemantic_feature=g("semantic_feature"),
                     dL_dopacity=g("opacities"), dL_dscales=g("scales"), dL_drotations=g("rotations"),
                     dL_dcov3D=g("cov3D_precomp"))
    torch.cuda.synchronize()
    return out, grads


def grad_report(name, got, want, rel=1e-3):
    """Error of `got` against `want` relative to the tensor's max magnitude; returns (max_rel, frac_bad)."""
    want = np.asarray(want, np.float64).reshape(-1)
    got = np.asarray(got, np.float64).reshape(-1)
    scale = np.abs(want).max() + 1e-30
    err = np.abs(got - want)
    bad = err > rel * np.abs(want) + rel * 1e-2 * scale
    return float(err.max() / scale), float(bad.mean())


def _strict_compare(scene, pc=False, pv=False, channel_scale=None, report=None):
    """HIP path vs the C++ oracle with the north-star bars: outputs <= 1e-4 abs, gradients <= 1e-3 rel
    (`|err| <= 1e-3 |g| + 1e-5 max|g|` for EVERY element and max err <= 1e-3 max|g|), after the pixels PROVEN to be
    threshold flips (refutil.flip_pixels: n_contrib / final-T evidence from both implementations) have been
    counted, bounded and removed exactly by zeroing their upstream gradients on both sides.

    channel_scale (opt-in, one positive number s_c per feature channel): on top of those bars, feature-map channel c within
    1e-4 s_c at every non-flip pixel, and column c of dL_dsemantic_feature held to the gradient bars on its own - a channel
    whose values are small next to the others' cannot hide an error in the whole-tensor maxima.

    report (opt-in, a dict): receives both sides' outputs and gradients and the oracle, for further assertions of the caller."""
    import refutil as ru
    W, H = scene["image_width"], scene["image_height"]
    npix = W * H
    o, want, _ = run_oracle(scene, pc, pv, backward=False)
    old = set_option("tile_cull", 0)      # n_contrib is a list position: comparable only on the reference's lists
    try:
        d = ru.device_inputs(scene, scene["C"], "cuda:0", pc, pv)
        f0 = ru.raw_forward(ru.product_module(), scene, d)
        img_prod = ru.product_image_state(scene, f0)
    finally:
        set_option("tile_cull", old)
    flips = ru.flip_pixels(dict(n_contrib=o.read("n_contrib"), final_T=o.read("final_T")), img_prod)
    nflip = int(flips.sum())
    assert nflip <= max(2, npix // 10000), f"{nflip} threshold-flip pixels"
    ok = ~flips
    masked = dict(scene)
    keep = torch.from_numpy(ok.reshape(1, H, W))
    for k in ("dL_dcolor", "dL_dfeature", "dL_ddepth"):
        masked[k] = scene[k] * keep
    got, got_g = run_hip(masked, pc, pv)
    want_g = o.backward(masked["dL_dcolor"], masked["dL_dfeature"], masked["dL_ddepth"])
    assert np.array_equal(got["radii"], want["radii"])
    for k in ("color", "feature_map", "depth"):
        if want[k].size == 0:
            assert got[k].shape == want[k].shape
            continue
        err = np.abs(got[k] - want[k]).reshape(want[k].shape[0], -1).max(0)
        assert err[ok].max() <= 1e-4, f"{k}: max abs err {err[ok].max():.3e} outside the {nflip} flip pixels"
    if channel_scale is not None:
        s = np.asarray(channel_scale, np.float64)
        assert s.shape == (scene["C"],)
        if scene["C"]:
            err = np.abs(got["feature_map"] - want["feature_map"]).reshape(scene["C"], -1)[:, ok].max(1)
            c = int(np.argmax(err / s))
            assert err[c] <= 1e-4 * s[c], f"feature_map channel {c}: max abs err {err[c]:.3e} above 1e-4 x {s[c]:g}"
    names = {"dL_dmeans3D", "dL_dmeans2D", "dL_dsemantic_feature", "dL_dopacity"}
    names |= {"dL_dcolors"} if pc else {"dL_dsh"}
    names |= {"dL_dcov3D"} if pv else {"dL_dscales", "dL_drotations"}
    for k in sorted(names):
        w = want_g[k]
        if w.size == 0:
            continue
        mx, worst = ru.grad_errors(got_g[k], w)
        assert mx <= 1e-3, f"{k}: max err / max|g| = {mx:.2e}"
        assert worst <= 1.0, f"{k}: worst element {worst:.2f}x outside 1e-3*|g| + 1e-5*max|g|"
    if channel_scale is not None and scene["C"]:
        C = scene["C"]
        g_, w_ = got_g["dL_dsemantic_feature"].reshape(-1, C), want_g["dL_dsemantic_feature"].reshape(-1, C)
        for c in range(C):
            mx, worst = ru.grad_errors(g_[:, c], w_[:, c])
            assert mx <= 1e-3, f"dL_dsemantic_feature channel {c}: max err / max|g| = {mx:.2e}"
            assert worst <= 1.0, f"dL_dsemantic_feature channel {c}: worst element {worst:.2f}x outside 1e-3*|g| + 1e-5*max|g|"
    if report is not None:
        report.update(got=got, got_g=got_g, want=want, want_g=want_g, oracle=o, nflip=nflip)
    return nflip


def harsh_scene(kind: str, P: int, C: int, width: int, height: int, seed: int, with_depth_grad: bool = False) -> dict:
    """Scenes OUTSIDE the synthetic family of SURVEY.md 8(d) (uniform depth, log-uniform scales), for the comparison against
    the reference-compiled checker:

      heavy_tail  log-normal scales, independent per axis (median 0.04, sigma_log 1.3, up to 4 world units: splats larger than
                  the image AND needles with axis ratios of 1 : 300, for which the fp32 cov2D / cov3D backward formulas of
                  either implementation are ill-conditioned), half of the Gaussians nearly transparent (opacity 0.004 .. 0.03:
                  just above the 1/255 cut, so that pixels do NOT saturate early and the deep tile lists are actually walked)
      heavy_tail_round  the same size distribution with axis ratios of at most 2 : 1 (one log-normal size per Gaussian):
                  splats larger than the image and tile lists of tens of thousands of entries at 1080p without the needles -
                  the stress on the BLEND kernels alone
      opacity01   a third of the opacities exactly 0, a third exactly 1 (the 0.99 clamp, Q1; alpha = 0 < 1/255)
      zero_scales scales exactly 0 on all three axes (cov2D = the 0.3 low-pass alone), on one axis (flat splats), denormal
                  scales, and a few all-zero quaternions (the kernels do not normalise: R = I)
    """
    import math
    from synth import make_scene
    sc = make_scene(P=P, C=C, width=width, height=height, seed=seed, with_depth_grad=with_depth_grad)
    g = torch.Generator().manual_seed(seed * 7919 + 13)
    if kind in ("heavy_tail", "heavy_tail_round"):
        if kind == "heavy_tail":
            sc["scales"] = torch.exp(math.log(0.04) + 1.3 * torch.randn(P, 3, generator=g)).clamp(1e-5, 4.0).contiguous()
        else:
            size = torch.exp(math.log(0.04) + 1.3 * torch.randn(P, 1, generator=g))
            sc["scales"] = (size * (1.0 + torch.rand(P, 3, generator=g))).clamp(1e-5, 4.0).contiguous()
        low = torch.rand(P, generator=g) < 0.5
        faint = 0.004 + 0.026 * torch.rand(P, 1, generator=g)
        sc["opacities"] = torch.where(low[:, None], faint, sc["opacities"]).contiguous()
    elif kind == "opacity01":
        r = torch.rand(P, generator=g)
        op = sc["opacities"].clone()
        op[r < 1 / 3] = 0.0
        op[r > 2 / 3] = 1.0
        sc["opacities"] = op.contiguous()
    elif kind == "zero_scales":
        r = torch.rand(P, generator=g)
        s = sc["scales"].clone()
        s[r < 0.10] = 0.0
        flat = (r >= 0.10) & (r < 0.20)
        axis = torch.randint(0, 3, (P,), generator=g)
        s[flat, axis[flat]] = 0.0
        s[(r >= 0.20) & (r < 0.25)] = 1e-40           # denormal
        sc["scales"] = s.contiguous()
        q = sc["rotations"].clone()
        q[(r >= 0.25) & (r < 0.27)] = 0.0
        sc["rotations"] = q.contiguous()
    elif kind == "nonfinite_means":
        # 2 % of the Gaussians with a NaN / +inf / -inf coordinate: projected to NaN pixel coordinates, their tile rectangle
        # is empty on either implementation (forward.cu:232-238: the int conversions of NaN give an empty rectangle) - they
        # must vanish without a trace: no hang, no NaN anywhere in the images or in any other Gaussian's gradient
        r = torch.rand(P, generator=g)
        m = sc["means3D"].clone()
        axis = torch.randint(0, 3, (P,), generator=g)
        for lo_, hi_, val in ((0.0, 0.007, float("nan")), (0.007, 0.014, float("inf")), (0.014, 0.02, float("-inf"))):
            sel = (r >= lo_) & (r < hi_)
            m[sel, axis[sel]] = val
        sc["means3D"] = m.contiguous()
    else:
        raise ValueError(kind)
    return sc
