"""Float64 restatement of the reference's viewer modes (utils/image_utils.py:60-161: unproject_depth_map, depth_to_normal,
gradient_map, colormap; render.py:155-161 for the `max` palette mode) and the seeded inputs of their tests.  numpy only.

Quirks kept from the reference:
  - pixel INDICES, not centres: X = x / (W - 1) * 2 - 1, Y = y / (H - 1) * 2 - 1
  - sdepth = (f1 d + f2) / (d + 1e-8), f1 = projection_matrix[2][2], f2 = projection_matrix[3][2] (the transposed matrix)
  - the world points are zero-padded to (H + 1, W + 1): the last row's p2 and the last column's p3 are the zero vector, and
    the corner pixel's normal is 0 / (0 + 1e-8) = 0
  - the edge operator pads the image it is GIVEN with zeros: for curvature that is the (n + 1) / 2 image, 0 outside, not 0.5
  - colormap rounds halves to even (torch.round); a constant map (0 / 0 in the reference) is defined as index 0 everywhere
"""
import numpy as np

TILE = 16                                   # F3DGS_VIEW_TILE: the shapes below are T-1, T, T+1, 2T+1 and their like
BAND = 255.0 * 2.0 ** -22                   # float32 rounding of the scaled value s = (v - min) / (max - min) * 255 <= 255:
#                                             the subtraction, the division and the product each round once, 3 * 2^-24 * 255
BAND_CAP = 0.01                             # at most this share of a case's pixels may lie inside the band


# ---- the four functions ------------------------------------------------------------------------------------------------------
def unproject_depth_map(depth, projection_matrix, full_proj_transform):
    d = np.asarray(depth, np.float64)
    H, W = d.shape
    P = np.asarray(projection_matrix, np.float64)
    Y, X = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    Xn, Yn = X / (W - 1) * 2 - 1, Y / (H - 1) * 2 - 1
    sd = (P[2, 2] * d + P[3, 2]) / (d + 1e-8)
    pts = np.stack([Xn, Yn, sd, np.ones_like(sd)], axis=-1) @ np.linalg.inv(np.asarray(full_proj_transform, np.float64))
    return pts[..., :3] / pts[..., 3:]


def depth_to_normal(depth, projection_matrix, full_proj_transform):
    """(H, W, 3) float64"""
    H, W = np.asarray(depth).shape
    pw = np.zeros((H + 1, W + 1, 3))
    pw[:H, :W] = unproject_depth_map(depth, projection_matrix, full_proj_transform)
    p1, p2, p3 = pw[:-1, :-1], pw[1:, :-1], pw[:-1, 1:]
    n = np.cross(p2 - p1, p3 - p1)
    return n / (np.linalg.norm(n, axis=-1, keepdims=True) + 1e-8)


def gradient_map(image):
    """(H, W) float64 of a (C, H, W) image"""
    a = np.pad(np.asarray(image, np.float64), ((0, 0), (1, 1), (1, 1)))
    H, W = a.shape[1] - 2, a.shape[2] - 2
    s = lambda dy, dx: a[:, dy:dy + H, dx:dx + W]
    gx = (-s(0, 0) + s(0, 2) - 2 * s(1, 0) + 2 * s(1, 2) - s(2, 0) + s(2, 2)) / 4
    gy = (-s(0, 0) - 2 * s(0, 1) - s(0, 2) + s(2, 0) + 2 * s(2, 1) + s(2, 2)) / 4
    return np.sqrt((gx ** 2 + gy ** 2).sum(axis=0))


def normal_image(depth, projection_matrix, full_proj_transform):
    """the (3, H, W) image of the 'Normal' mode"""
    return (depth_to_normal(depth, projection_matrix, full_proj_transform).transpose(2, 0, 1) + 1) / 2


def curvature(depth, projection_matrix, full_proj_transform):
    return gradient_map(normal_image(depth, projection_matrix, full_proj_transform))


def scaled(field, lo=None, hi=None, L=256):
    """s = (v - min) / (max - min) * (L - 1) in float64; None where max == min"""
    v = np.asarray(field, np.float64)
    lo = v.min() if lo is None else float(lo)
    hi = v.max() if hi is None else float(hi)
    if hi == lo:
        return None
    return (v - lo) / (hi - lo) * (L - 1)


def colormap_index(field, lo=None, hi=None, L=256):
    s = scaled(field, lo, hi, L)
    if s is None:
        return np.zeros(np.shape(field), np.int64)
    return np.clip(np.rint(s), 0, L - 1).astype(np.int64)          # np.rint: halves to even


def in_band(field, lo=None, hi=None, L=256, widen=0.0):
    """True where the scaled value lies within BAND + widen of a half-integer: there the rounded index may differ by 1"""
    s = scaled(field, lo, hi, L)
    if s is None:
        return np.zeros(np.shape(field), bool)
    return np.abs(s - (np.floor(s) + 0.5)) <= BAND + widen


def max_index(field, hi=None, L=256):
    """render.py:155-161: matplotlib's float call, min(int(v / max * L), L - 1); negative values take the first entry"""
    v = np.asarray(field, np.float64)
    hi = v.max() if hi is None else float(hi)
    if hi == 0:
        return np.zeros(v.shape, np.int64)
    return np.clip(np.trunc(v / hi * L), 0, L - 1).astype(np.int64)


def in_max_band(field, hi=None, L=256):
    """True where v / max * L lies within L * 2^-22 of an integer (the truncation's edge)"""
    v = np.asarray(field, np.float64)
    hi = v.max() if hi is None else float(hi)
    if hi == 0:
        return np.zeros(v.shape, bool)
    s = v / hi * L
    return (np.abs(s - np.rint(s)) <= L * 2.0 ** -22) & (v != hi) & (v != 0)      # v / max = 1 and 0 are exact in any precision


def palette(idx, lut):
    """(3, H, W) float32 colours of an (H, W) index map"""
    return np.asarray(lut, np.float32)[idx].transpose(2, 0, 1)


def to_bytes(image):
    """view.py:26 on a (3, H, W) float32 image: (clamp(c, 0, 1) * 255) truncated to a byte, in float32 as there, (H, W, 3)"""
    c = np.clip(np.asarray(image, np.float32), np.float32(0), np.float32(1)) * np.float32(255)
    return c.astype(np.uint8).transpose(1, 2, 0)


def error_stats(got, want, mask=None):
    """median, 99th percentile and maximum of |got - want| over the pixels of `mask` (H, W); vectors count by their largest
    component"""
    e = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    if e.ndim == 3:
        e = e.max(axis=-1)
    if mask is not None:
        e = e[mask]
    return np.array([np.median(e), np.percentile(e, 99), e.max()])


def clean_footprint(depth, before, after):
    """(H, W) bool: True where no depth of rows y - before .. y + after, columns x - before .. x + after (inside the image) is
    exactly 0.  Normals read (0, 1), curvature (1, 2)."""
    z = np.asarray(depth) == 0
    H, W = z.shape
    zp = np.pad(z, ((before, after), (before, after)))
    bad = np.zeros((H, W), bool)
    for dy in range(before + after + 1):
        for dx in range(before + after + 1):
            bad |= zp[dy:dy + H, dx:dx + W]
    return ~bad


# ---- cameras (the construction of the reference's utils/graphics_utils.py, float32 matrices as its Camera holds them) -------
class Camera:
    def __init__(self, projection_matrix, full_proj_transform):
        self.projection_matrix, self.full_proj_transform = projection_matrix, full_proj_transform


def _projection(znear, zfar, tanx, tany, cx=0.0, cy=0.0):
    """the transposed projection matrix; (cx, cy) shifts the principal point by that share of the half-frame"""
    top, right = tany * znear, tanx * znear
    l, r, b, t = -right + cx * right, right + cx * right, -top + cy * top, top + cy * top
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 2 * znear / (r - l), 2 * znear / (t - b)
    P[0, 2], P[1, 2] = (r + l) / (r - l), (t + b) / (t - b)
    P[3, 2] = 1.0
    P[2, 2], P[2, 3] = zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    return P.T


def _world_view(angles, t):
    ax, ay, az = angles
    cx_, sx_, cy_, sy_, cz_, sz_ = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx_], [0, sx_, cx_]])
    Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
    Rz = np.array([[cz_, -sz_, 0], [sz_, cz_, 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = Rz @ Ry @ Rx
    M[:3, 3] = t
    return M.T


T60 = float(np.tan(np.radians(30.0)))
CAMERAS = {
    "centred": dict(angles=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0), tanx=T60, tany=T60),
    "posed": dict(angles=(0.3, -0.5, 0.2), t=(0.7, -1.1, 2.3), tanx=T60, tany=T60),
    "aniso": dict(angles=(-0.2, 0.4, 0.0), t=(-0.4, 0.3, 0.5), tanx=0.9, tany=0.45),
    "offcentre": dict(angles=(0.1, 0.25, -0.3), t=(0.2, 0.6, -0.8), tanx=T60, tany=0.5, cx=0.3, cy=-0.2),
}


def make_camera(kind):
    """(projection_matrix, full_proj_transform) float32, znear 0.01, zfar 100"""
    c = CAMERAS[kind]
    P = _projection(0.01, 100.0, c["tanx"], c["tany"], c.get("cx", 0.0), c.get("cy", 0.0)).astype(np.float32)
    V = _world_view(c["angles"], c["t"]).astype(np.float32)
    return P, (V.astype(np.float64) @ P.astype(np.float64)).astype(np.float32)


# ---- depth fields and images --------------------------------------------------------------------------------------------------
def _grid(H, W):
    return np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")


def smooth_depth(H, W):
    """z between 2.5 and 6"""
    v, u = _grid(H, W)
    return 4.25 + 1.1 * np.sin(2.1 * u + 0.4) * np.cos(1.7 * v - 0.3) + 0.6 * np.sin(3.3 * v + 1.1 * u)


def hole_of(H, W):
    """rows and columns of the rectangle of zeros: it crosses the first tile boundary wherever the frame has one"""
    y0, y1 = (TILE - 3, min(TILE + 4, H)) if H > TILE else (H // 2, H // 2 + 1)
    x0, x1 = (TILE - 2, min(TILE + 6, W)) if W > TILE else (W // 2, W // 2 + 1)
    return y0, y1, x0, x1


def make_depth(kind, H, W):
    v, u = _grid(H, W)
    if kind == "plane":
        d = 4.0 + 0.9137 * u - 0.6211 * v
    elif kind == "smooth":
        d = smooth_depth(H, W)
    elif kind == "hole":
        d = smooth_depth(H, W)
        y0, y1, x0, x1 = hole_of(H, W)
        d[y0:y1, x0:x1] = 0.0
    elif kind == "step":
        d = smooth_depth(H, W) + 1.5 * (u + 0.35 * v > 0.1)
    else:
        raise KeyError(kind)
    return d.astype(np.float32)


def make_image(kind, Cn, H, W, seed):
    """(Cn, H, W) float32 of order 1"""
    if kind == "constant":
        return np.full((Cn, H, W), 0.37, np.float32)
    r = np.random.default_rng(seed)
    v, u = _grid(H, W)
    img = np.stack([0.5 + 0.4 * np.sin((2 + c) * u + 0.7 * c) * np.cos((1.5 + 0.5 * c) * v) for c in range(Cn)])
    return (img + 0.05 * r.standard_normal((Cn, H, W))).astype(np.float32)


SHAPES = ((2, 2), (2, 9), (9, 2), (15, 15), (16, 16), (17, 17), (17, 23), (33, 70), (64, 129))

# depth cases: name -> (H, W, camera, field).  Every camera and every field at several shapes, every shape twice (64 x 129,
# the largest, once); the holes and steps at the shapes that have a tile boundary to cross.
DEPTH_CASES = {
    "2x2_posed_smooth": (2, 2, "posed", "smooth"), "2x2_centred_plane": (2, 2, "centred", "plane"),
    "2x9_aniso_step": (2, 9, "aniso", "step"), "2x9_offcentre_hole": (2, 9, "offcentre", "hole"),
    "9x2_offcentre_smooth": (9, 2, "offcentre", "smooth"), "9x2_posed_hole": (9, 2, "posed", "hole"),
    "15x15_centred_smooth": (15, 15, "centred", "smooth"), "15x15_aniso_plane": (15, 15, "aniso", "plane"),
    "16x16_posed_step": (16, 16, "posed", "step"), "16x16_offcentre_plane": (16, 16, "offcentre", "plane"),
    "17x17_aniso_smooth": (17, 17, "aniso", "smooth"), "17x17_centred_hole": (17, 17, "centred", "hole"),
    "17x23_posed_smooth": (17, 23, "posed", "smooth"), "17x23_offcentre_step": (17, 23, "offcentre", "step"),
    "33x70_aniso_hole": (33, 70, "aniso", "hole"), "33x70_centred_step": (33, 70, "centred", "step"),
    "64x129_posed_hole": (64, 129, "posed", "hole"),
}
# image cases of the edge operator: name -> (Cn, H, W, kind, seed)
IMAGE_CASES = {
    "c1_2x2": (1, 2, 2, "smooth", 11), "c3_2x9": (3, 2, 9, "smooth", 12), "c5_9x2": (5, 9, 2, "smooth", 13),
    "c3_15x15": (3, 15, 15, "smooth", 14), "c1_16x16": (1, 16, 16, "smooth", 15), "c5_17x17": (5, 17, 17, "smooth", 16),
    "c3_17x23_constant": (3, 17, 23, "constant", 0), "c1_17x23": (1, 17, 23, "smooth", 17), "c5_33x70": (5, 33, 70, "smooth", 18),
    "c3_64x129": (3, 64, 129, "smooth", 19), "c1_33x70_constant": (1, 33, 70, "constant", 0),
}
FIXTURE_CASES = tuple(DEPTH_CASES) + tuple(IMAGE_CASES)


def make_inputs(name):
    """depth cases: (depth (H, W), projection_matrix, full_proj_transform); image cases: the (Cn, H, W) image.  float32."""
    if name in DEPTH_CASES:
        H, W, cam, field = DEPTH_CASES[name]
        return (make_depth(field, H, W),) + make_camera(cam)
    Cn, H, W, kind, seed = IMAGE_CASES[name]
    return make_image(kind, Cn, H, W, seed)
