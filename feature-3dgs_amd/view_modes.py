"""The viewer's render modes of a rendered view: 'Depth', 'Edge', 'Normal', 'Curvature' and 'Feature Map' as fused kernels.

The reference's `render_net_image` (utils/image_utils.py:141-161; callers view.py:25 and the training GUI, train.py:164) turns
the rasterizer's `render` and `depth` into the frame the viewer shows with a chain of torch ops: for 'Curvature' a meshgrid,
three stacks, an (HW, 4) x (4, 4) matmul with `full_proj_transform.inverse()`, a zero-padded copy, a cross product, six conv2d
calls, a min, a max and a LUT gather - dozens of launches and about twenty full-frame temporaries per frame.  Here each mode is
one or two HIP kernels (csrc/view_modes.hip behind include/f3dgs.h: f3dgs_view_*):

    image = render_net_image(render_pkg, render_items, render_mode, camera)      # (3, H, W) float32, the reference's signature
    frame = net_image_bytes(render_pkg, render_items, render_mode, camera)       # (H, W, 3) uint8: what view.py:26 sends
    import utils.image_utils, view_modes; view_modes.install(utils.image_utils)  # or: the reference's own scripts, fused

Normals are NOT a transliteration of the reference's float32 chain, which loses the surface to rounding at a fraction of a per
cent of the pixels (errors of order 1 on a unit normal): the unprojection - the reference's formula, with the
inverse of `full_proj_transform` taken in float64 by `torch.linalg.inv` on the map's device - and the two point differences
are float64 in the kernel, everything after them float32.  The judge is the reference's function evaluated in float64.

`colormap`: the reference's 0/0 for a constant map (max == min) is defined here: every index is 0.  The library ships no
palette: without `lut` the table is taken once per device from matplotlib.

'Feature Map' delegates to feature_pca.py: the basis comes from the first frame and is kept at module level (as the reference
keeps `pca_mean` and `top_vector`; `reset_feature_basis()` clears it).  That mode is NOT parity-pinned to the reference's
`feature_map`: the sign rule and the percentile method of feature_pca.py apply (largest entry positive, numpy's linear
interpolation, range from the first frame as well).

`camera` needs only `projection_matrix` and `full_proj_transform`.  HIP only; no CPU fallback; argument errors are raised before
any device work.
"""
from __future__ import annotations

import torch

RENDER_MODES = ("RGB", "Depth", "Edge", "Normal", "Curvature", "Feature Map")      # arguments/__init__.py:59
MAX_PALETTE = 4096              # F3DGS_VIEW_PALETTE_MAX_ENTRIES
MAX_PIXELS = 1 << 30

_luts = {}                      # (cmap, device) -> (L, 3) float32
_feature_basis = None           # feature_pca.FeaturePCA of the first 'Feature Map' frame


def _C():
    from diff_gaussian_rasterization import _C as ext
    return ext


def _is_f32(t):
    return torch.is_tensor(t) and t.dtype == torch.float32


def _describe(t):
    return (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__


def _check_depth(depth_map):
    """(H, W) or (1, H, W) as they are; anything else is squeezed, as the reference does, and must leave two axes."""
    if not _is_f32(depth_map):
        raise ValueError(f"depth_map float32 expected, got {_describe(depth_map)}")
    d = depth_map[0] if depth_map.dim() == 3 and depth_map.shape[0] == 1 else depth_map if depth_map.dim() == 2 else depth_map.squeeze()
    if d.dim() != 2:
        raise ValueError(f"depth_map (H, W) or (1, H, W) expected, got {tuple(depth_map.shape)}")
    H, W = d.shape
    if H < 2 or W < 2:
        raise ValueError(f"depth_map {H} x {W}: at least 2 rows and 2 columns are needed (the reference divides by H - 1 and W - 1)")
    if H * W > MAX_PIXELS:
        raise ValueError(f"depth_map {H} x {W}: beyond the limit of 2^30 pixels")
    return d


def _check_camera(camera):
    for name in ("projection_matrix", "full_proj_transform"):
        m = getattr(camera, name, None)
        if not torch.is_tensor(m) or tuple(m.shape) != (4, 4) or not m.dtype.is_floating_point:
            raise ValueError(f"camera.{name}: a (4, 4) floating-point tensor is needed, got {_describe(m)}")


def _check_image(image):
    if not _is_f32(image) or image.dim() != 3 or image.shape[0] < 1:
        raise ValueError(f"image (C, H, W) float32 with C >= 1 expected, got {_describe(image)}")
    if image.shape[1] * image.shape[2] > MAX_PIXELS:
        raise ValueError(f"image {image.shape[1]} x {image.shape[2]}: beyond the limit of 2^30 pixels")


def _check_map(map):
    if not _is_f32(map):
        raise ValueError(f"map float32 expected, got {_describe(map)}")
    m = map[0] if map.dim() == 3 and map.shape[0] == 1 else map if map.dim() == 2 else map.squeeze()
    if m.dim() != 2:
        raise ValueError(f"map (1, H, W) or (H, W) expected, got {tuple(map.shape)}")
    if m.numel() > MAX_PIXELS:
        raise ValueError(f"map {m.shape[0]} x {m.shape[1]}: beyond the limit of 2^30 pixels")
    return m


def _check_lut(lut):
    if not _is_f32(lut) or lut.dim() != 2 or lut.shape[1] != 3:
        raise ValueError(f"lut (L, 3) float32 expected, got {_describe(lut)}")
    if not 2 <= lut.shape[0] <= MAX_PALETTE:
        raise ValueError(f"lut of {lut.shape[0]} entries: 2 to {MAX_PALETTE} are supported")


def _camera_matrices(camera, device):
    """projection_matrix as float32 and the float64 inverse of full_proj_transform, both on `device`; no host read."""
    proj = camera.projection_matrix.to(device=device, dtype=torch.float32)
    inv = torch.linalg.inv(camera.full_proj_transform.to(device=device, dtype=torch.float64))
    return proj, inv


def matplotlib_lut(cmap="turbo", device="cpu"):
    """The (L, 3) float32 table of a listed matplotlib colormap (`.colors`, as the reference's `colormap` reads it), or the
    256 sampled entries of any other one.  Taken once per (name, device)."""
    key = (cmap, str(device))
    if key not in _luts:
        try:
            import matplotlib
        except ImportError as exc:
            raise RuntimeError("colormap() without `lut` takes its palette from matplotlib, which is not installed: "
                               "pass lut=(L, 3) float32") from exc
        if hasattr(matplotlib, "colormaps"):
            cm = matplotlib.colormaps[cmap]
        else:
            import matplotlib.pyplot as plt
            cm = plt.cm.get_cmap(cmap)
        colors = cm.colors if hasattr(cm, "colors") else cm(range(256))
        _luts[key] = torch.tensor(colors, dtype=torch.float32)[:, :3].contiguous().to(device)
    return _luts[key]


@torch.no_grad()
def depth_to_normal(depth_map, camera):
    """(H, W, 3) float32: the reference's depth_to_normal, its unprojection and point differences in float64.  The last row and
    column are computed against the reference's zero padding; the corner pixel is 0."""
    d = _check_depth(depth_map)
    _check_camera(camera)
    proj, inv = _camera_matrices(camera, d.device)
    return _C().view_normals(d.detach(), proj, inv, False, False)


@torch.no_grad()
def gradient_map(image):
    """(1, H, W) float32: sqrt(sum over channels of gx^2 + gy^2), taps [[-1,0,1],[-2,0,2],[-1,0,1]] / 4 and their transpose,
    zeros outside the image."""
    _check_image(image)
    return _C().view_gradient(image.detach())[0][None]


@torch.no_grad()
def colormap(map, cmap="turbo", lut=None):
    """(3, H, W) float32: lut[rint((map - min) / (max - min) * (L - 1))], halves to even; a constant map gets lut[0]."""
    m = _check_map(map)
    if lut is not None:
        _check_lut(lut)
    else:
        lut = matplotlib_lut(cmap, m.device)
    C = _C()
    m = m.detach()
    return C.view_palette(m, C.view_minmax(m), lut.to(m.device), C.VIEW_PALETTE_MINMAX, True, False)[0]


def reset_feature_basis():
    """Forgets the PCA basis of the 'Feature Map' mode: the next frame fits a new one."""
    global _feature_basis
    _feature_basis = None


def _feature_image(feature_map):
    global _feature_basis
    import feature_pca
    if _feature_basis is None or _feature_basis.mean.shape[0] != feature_map.shape[0] or _feature_basis.mean.device != feature_map.device:
        _feature_basis = feature_pca.fit_feature_pca(feature_map)
    return feature_pca.apply_feature_pca(feature_map, _feature_basis).permute(2, 0, 1)


def _mode_of(render_items, render_mode):
    try:
        return render_items[render_mode].lower()
    except (IndexError, KeyError, TypeError, AttributeError) as exc:
        raise ValueError(f"render_mode {render_mode!r} does not index render_items {render_items!r}") from exc


def _net(render_pkg, render_items, render_mode, camera, want_float, want_u8):
    """(float image or None, uint8 frame or None) of one mode"""
    output = _mode_of(render_items, render_mode)
    C = _C
    field = minmax = None
    if output == "depth":
        net = render_pkg["depth"]
        if net.shape[0] == 1:
            field = _check_map(net).detach()
            minmax = C().view_minmax(field)
    elif output == "edge":
        _check_image(render_pkg["render"])
        field, minmax = C().view_gradient(render_pkg["render"].detach())
    elif output in ("normal", "curvature"):
        d = _check_depth(render_pkg["depth"])
        _check_camera(camera)
        proj, inv = _camera_matrices(camera, d.device)
        if output == "normal":
            net = C().view_normals(d.detach(), proj, inv, True, True)
        else:
            field, minmax = C().view_curvature(d.detach(), proj, inv)
    elif output == "feature map":
        import feature_pca
        feature_pca._check(render_pkg["feature_map"])
        net = _feature_image(render_pkg["feature_map"])
    else:
        net = render_pkg["render"]
    if field is not None:
        lut = matplotlib_lut("turbo", field.device)
        return C().view_palette(field, minmax, lut, C().VIEW_PALETTE_MINMAX, want_float, want_u8)
    if net.dim() == 3 and net.shape[0] == 1:            # a one-channel `render`: the reference colours whatever has one channel
        return _net({"depth": net}, ["depth"], 0, camera, want_float, want_u8)
    frame = None
    if want_u8:
        if not _is_f32(net) or net.dim() != 3 or net.shape[0] != 3:
            raise ValueError(f"a (3, H, W) float32 image is needed for the frame, got {_describe(net)}")
        frame = C().view_bytes(net.detach())
    return (net if want_float else None), frame


@torch.no_grad()
def render_net_image(render_pkg, render_items, render_mode, camera):
    """The reference's render_net_image: (3, H, W) float32 of mode `render_items[render_mode]` (RENDER_MODES; any other name is
    'RGB').  One-channel results are coloured with matplotlib's turbo table."""
    return _net(render_pkg, render_items, render_mode, camera, True, False)[0]


@torch.no_grad()
def net_image_bytes(render_pkg, render_items, render_mode, camera):
    """(H, W, 3) uint8 on the device: (clamp(render_net_image(...), 0, 1) * 255).byte().permute(1, 2, 0) of view.py:26, for the
    palette modes written by the palette kernel itself (the float image is never formed)."""
    return _net(render_pkg, render_items, render_mode, camera, False, True)[1]


def install(module):
    """Sets depth_to_normal, gradient_map, colormap and render_net_image in an imported `utils.image_utils`, so that the
    reference's viewer and training GUI draw their frames with the fused kernels.  Returns the module."""
    module.depth_to_normal = depth_to_normal
    module.gradient_map = gradient_map
    module.colormap = colormap
    module.render_net_image = render_net_image
    return module
