"""Object transforms: move, rotate and scale groups of Gaussians.

groups.group_stats ends in knowledge about an object ("instance 17 is the chair, it is here and this big"); edit.apply_edit can
delete it, extract it or recolour it.  This module moves it, turns it, resizes it or puts a second one beside it
(csrc/transform.hip behind include/f3dgs.h: f3dgs_transform_gaussians): every group by its own similarity transform
x' = s R (x - p) + p + t in ONE launch - positions, the model's un-normalised quaternions, log-scales, precomputed covariances,
and the 45 higher-order SH coefficients rotated band by band in the rasterizer's own basis, so that a turned object keeps its
view-dependent colour on its own surface.

    st = groups.lifter_stats(instance_lifter, gaussians.get_xyz)
    tr = Transforms.about_centroid(st, quat=Transforms.from_axis_angle((0, 0, 1), angles).quat, translation=shift)
    transform_model(gaussians, instance_lifter.labels(), tr)                      # in place
    new = transform_model(gaussians, instance_lifter.labels(), tr, rows=rows_of_17)   # a moved copy, as new rows

HIP only; no CPU fallback.  Nothing is read back to the host.
"""
from __future__ import annotations

import collections

import torch

from simple_knn import _C
from groups import MAX_GROUPS, _group_ids
from neighbors import _describe, _need_device

BAD_QUAT, ZERO_QUAT, BAD_SCALE, NONPOSITIVE_SCALE, BAD_TRANSLATION, BAD_PIVOT = 1, 2, 3, 4, 5, 6      # F3DGS_TRANSFORM_*

Transformed = collections.namedtuple("Transformed", ["xyz", "rotations", "scales", "cov3d", "sh_rest", "status"])


def _rows_of(value, G, width, device, name, default):
    """a (G, width) float32 tensor on `device` from a tensor, a sequence or None (`default` per row); width 0: (G,)"""
    shape = (G,) if width == 0 else (G, width)
    if value is None:
        value = default
    t = torch.as_tensor(value, dtype=torch.float32, device=device)
    try:
        return t.expand(shape).contiguous()
    except RuntimeError:
        raise ValueError(f"{name}: a float32 tensor that broadcasts to {shape} expected, got {_describe(t)}") from None


class Transforms(collections.namedtuple("Transforms", ["quat", "scale", "translation", "pivot"])):
    """The per-group table, on the device: quat (G, 4) in the model's order (w, x, y, z) - any length but 0, it is normalised in
    fp64 by the kernel -, scale (G,) > 0, translation (G, 3), pivot (G, 3) or None (the origin).  Group g maps
    x -> scale R(quat) (x - pivot) + pivot + translation.  No constructor reads the device."""
    __slots__ = ()

    @property
    def num_groups(self):
        return self.scale.shape[0]

    @classmethod
    def identity(cls, G, device):
        return cls.from_parts(G, device)

    @classmethod
    def from_parts(cls, G, device, quat=None, scale=None, translation=None, pivot=None):
        """Every part a tensor or a sequence that broadcasts over the G rows, or None (no rotation, 1, no shift, the origin)."""
        if not isinstance(G, int) or isinstance(G, bool) or not 1 <= G <= MAX_GROUPS:
            raise ValueError(f"G = {G!r}: an integer in 1 .. {MAX_GROUPS} expected")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"device = {device}: a HIP device expected, the object transforms have no CPU path")
        return cls(_rows_of(quat, G, 4, device, "quat", (1.0, 0.0, 0.0, 0.0)), _rows_of(scale, G, 0, device, "scale", 1.0),
                   _rows_of(translation, G, 3, device, "translation", 0.0),
                   None if pivot is None else _rows_of(pivot, G, 3, device, "pivot", 0.0))

    @classmethod
    def from_axis_angle(cls, axis, angle, device=None, scale=None, translation=None, pivot=None):
        """axis (3,) or (G, 3) - any length but 0 -, angle (G,) or a number, in radians: right-handed turns about the axis."""
        angle = torch.as_tensor(angle, dtype=torch.float64, device=device).reshape(-1)
        device = angle.device
        axis = torch.as_tensor(axis, dtype=torch.float64, device=device)
        if axis.shape[-1:] != (3,) or axis.dim() > 2:
            raise ValueError(f"axis: (3,) or (G, 3) expected, got {_describe(axis)}")
        G = max(angle.shape[0], axis.shape[0] if axis.dim() == 2 else 1)
        axis = axis.expand(G, 3)
        axis = axis / axis.norm(dim=1, keepdim=True)
        half = 0.5 * angle.expand(G)
        quat = torch.cat([torch.cos(half)[:, None], torch.sin(half)[:, None] * axis], dim=1).float()
        return cls.from_parts(G, device, quat, scale, translation, pivot)

    @classmethod
    def from_matrix(cls, R, device=None, scale=None, translation=None, pivot=None):
        """R: (3, 3) or (G, 3, 3) proper rotations.  Shepperd's method without a branch: of the four candidates (w, x, y or z
        largest) each row takes the one with the largest divisor, chosen by a gather."""
        R = torch.as_tensor(R, dtype=torch.float64, device=device)
        if R.shape[-2:] != (3, 3) or R.dim() not in (2, 3):
            raise ValueError(f"R: (3, 3) or (G, 3, 3) expected, got {_describe(R)}")
        R = R.reshape(-1, 3, 3)
        m = lambda a, b: R[:, a, b]
        tr = m(0, 0) + m(1, 1) + m(2, 2)
        four = torch.stack([1 + tr, 1 + 2 * m(0, 0) - tr, 1 + 2 * m(1, 1) - tr, 1 + 2 * m(2, 2) - tr], dim=1)      # 4 w^2, 4 x^2, ...
        cand = torch.stack([
            torch.stack([four[:, 0], m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)], dim=1),
            torch.stack([m(2, 1) - m(1, 2), four[:, 1], m(0, 1) + m(1, 0), m(0, 2) + m(2, 0)], dim=1),
            torch.stack([m(0, 2) - m(2, 0), m(0, 1) + m(1, 0), four[:, 2], m(1, 2) + m(2, 1)], dim=1),
            torch.stack([m(1, 0) - m(0, 1), m(0, 2) + m(2, 0), m(1, 2) + m(2, 1), four[:, 3]], dim=1)], dim=1)   # (G, 4, 4)
        best = four.argmax(dim=1)
        quat = cand.gather(1, best[:, None, None].expand(-1, 1, 4))[:, 0, :]
        quat = quat / quat.norm(dim=1, keepdim=True)
        return cls.from_parts(R.shape[0], R.device, quat.float(), scale, translation, pivot)

    @classmethod
    def about_centroid(cls, stats, quat=None, scale=None, translation=None):
        """Every group about its own centroid: pivot = stats.centroid (groups.GroupStats), on the device.  An empty group has the
        centroid 0 and nobody to move."""
        c = getattr(stats, "centroid", None)
        if not torch.is_tensor(c) or c.dim() != 2 or c.shape[1] != 3 or c.dtype != torch.float32:
            raise ValueError(f"stats: groups.GroupStats with a float32 (G, 3) centroid expected, got {_describe(c)}")
        _need_device(c, "stats.centroid")
        return cls.from_parts(c.shape[0], c.device, quat, scale, translation, c.detach())


def _check_table(transforms, dev):
    if not isinstance(transforms, Transforms):
        raise ValueError(f"transforms: a Transforms expected, got {type(transforms).__name__}")
    G = transforms.scale.shape[0] if torch.is_tensor(transforms.scale) and transforms.scale.dim() == 1 else -1
    for name, t, shape in (("quat", transforms.quat, (G, 4)), ("scale", transforms.scale, (G,)), ("translation", transforms.translation, (G, 3)),
                           ("pivot", transforms.pivot, (G, 3))):
        if t is None and name == "pivot":
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != dev or not 1 <= G <= MAX_GROUPS:
            raise ValueError(f"transforms.{name}: a float32 {shape} tensor on {dev} with 1 <= G <= {MAX_GROUPS} expected, got {_describe(t)}")
    return G


def transform_gaussians(groups, transforms, xyz=None, rotations=None, scales=None, log_scales=True, cov3d=None, sh_rest=None, rows=None,
                        out=None):
    """Transforms the Gaussians of every group by the group's row of `transforms`.

    groups: (P,) int32 or int64 on the device - any integers, an id outside [0, G) belongs to no group - or a bool `mask` of
    edit.apply_edit (selected = group 0, a table of one row).  Per-Gaussian tensors, float32 on the device, each optional, at
    least one: xyz (P, 3); rotations (P, 4), the model's un-normalised (w, x, y, z); scales (P, 3) - the model's raw _scaling
    with log_scales=True (+ ln s), activated scales with log_scales=False (* s); cov3d (P, 6) as cov3D_precomp; sh_rest
    (P, n_rest, 3), n_rest in {0, 3, 8, 15}: the model's _features_rest, or the view shs[:, 1:, :] of a (P, 16, 3) tensor, read
    in place.  Gaussian i is transformed iff its id is in range and the table's row is valid (Transformed.status: 0, or which
    part of the row was wrong); every other row comes back unchanged, bit for bit.

    out=None: new tensors.  out="inplace": written into the inputs (contiguous, but for the row stride of sh_rest); the rows that
    are not transformed are not written at all.  rows: (M,) int32 or int64 on the device - the GATHER form: output row j is the
    transform of input row rows[j] (a row of zeros for an index outside [0, P)), into new (M, ...) tensors; not with
    out="inplace".  Returns Transformed(xyz, rotations, scales, cov3d, sh_rest, status): None where nothing was given, status (G,)
    int32.  Every output element is accumulated in fp64 and rounded once.  DC colour, opacity and semantic features do not change
    under a similarity transform and are not taken."""
    _need_device(groups, "groups")
    num_groups = _check_table(transforms, groups.device)
    if groups.dtype == torch.bool and num_groups != 1:
        raise ValueError(f"transforms: a bool mask is one group (selected = group 0), a table of one row expected, got {num_groups} rows")
    g32, _ = _group_ids(groups, None if groups.dtype == torch.bool else num_groups, MAX_GROUPS)
    P, dev = g32.shape[0], g32.device
    if out not in (None, "inplace"):
        raise ValueError(f"out = {out!r}: None or \"inplace\" expected")
    inplace = out == "inplace"
    if inplace and rows is not None:
        raise ValueError("out=\"inplace\" with rows: the gather form writes new rows")
    r32 = None
    if rows is not None:
        _need_device(rows, "rows")
        if rows.dim() != 1 or rows.dtype not in (torch.int32, torch.int64) or rows.device != dev:
            raise ValueError(f"rows: an int32 or int64 (M,) tensor on {dev} expected, got {_describe(rows)}")
        r32 = rows.detach()
        if r32.dtype == torch.int64:
            r32 = torch.where((r32 >= 0) & (r32 < P), r32, torch.full((), -1, dtype=torch.int64, device=dev)).to(torch.int32)
        r32 = r32.contiguous()
    given = {}
    for name, t, width in (("xyz", xyz, 3), ("rotations", rotations, 4), ("scales", scales, 3), ("cov3d", cov3d, 6)):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (P, width) or t.device != dev:
            raise ValueError(f"{name}: a float32 ({P}, {width}) tensor on {dev} expected, got {_describe(t)}")
        if inplace and not t.is_contiguous():
            raise ValueError(f"{name}: out=\"inplace\" needs a contiguous tensor, got strides {tuple(t.stride())}")
        given[name] = t.detach() if inplace else t.detach().contiguous()
    empty_sh = None
    if sh_rest is not None:
        if not torch.is_tensor(sh_rest) or sh_rest.dtype != torch.float32 or sh_rest.dim() != 3 or sh_rest.shape[0] != P \
                or sh_rest.shape[2] != 3 or sh_rest.shape[1] not in (0, 3, 8, 15) or sh_rest.device != dev:
            raise ValueError(f"sh_rest: a float32 ({P}, n_rest, 3) tensor on {dev} with n_rest in (0, 3, 8, 15) expected, got "
                             f"{_describe(sh_rest)}")
        s = sh_rest.detach()
        n_rest = s.shape[1]
        if n_rest == 0:                                       # degree 0: nothing turns
            empty_sh = s if inplace else s.new_empty((P if rows is None else rows.shape[0], 0, 3))
        else:
            rows_ok = P == 0 or (s.stride(2) == 1 and s.stride(1) == 3 and (P == 1 or s.stride(0) >= 3 * n_rest))
            if not rows_ok:
                if inplace:
                    raise ValueError(f"sh_rest: out=\"inplace\" needs rows of n_rest x 3 contiguous floats (any row stride), got strides "
                                     f"{tuple(s.stride())}")
                s = s.contiguous()
            given["sh_rest"] = s
    if not given and empty_sh is None:
        raise ValueError("no per-Gaussian tensor given: xyz, rotations, scales, cov3d or sh_rest expected")
    with torch.no_grad():
        if given:
            res = _C.transform_gaussians(g32, transforms.quat, transforms.scale, transforms.translation, transforms.pivot, given.get("xyz"),
                                         given.get("rotations"), given.get("scales"), not log_scales, given.get("cov3d"),
                                         given.get("sh_rest"), r32, inplace)
        else:                                                 # only an empty sh_rest: the status of the table all the same
            dummy = torch.zeros(0, 3, dtype=torch.float32, device=dev)
            res = [None] * 5 + [_C.transform_gaussians(g32[:0], transforms.quat, transforms.scale, transforms.translation, transforms.pivot,
                                                       dummy, None, None, False, None, None, None, False)[5]]
    return Transformed(res[0], res[1], res[2], res[3], res[4] if empty_sh is None else empty_sh, res[5])


def transform_model(gaussians, groups, transforms, rows=None):
    """transform_gaussians on a GaussianModel-like object: its _xyz, _rotation, _scaling (log) and _features_rest, under
    torch.no_grad().

    rows=None: in place, into the parameters' storage; returns the status (G,) int32.  rows (M,): returns a dict of NEW rows for
    every per-Gaussian tensor of the model, keyed as the optimizer's groups ("xyz", "f_dc", "f_rest", "opacity", "scaling",
    "rotation", "semantic_feature") - the transformed copies of rows `rows`, the invariant tensors by index_select - and
    "status": what the model's densification_postfix, or densify.py's buffers, take.

    The optimizer state is NOT edited: Adam's moments of a moved parameter stay as they were (for the position and the
    quaternion they point the old way until they decay), and new rows have none until the caller appends them as the
    densification does."""
    names = ("_xyz", "_rotation", "_scaling", "_features_rest")
    for name in names:
        if not torch.is_tensor(getattr(gaussians, name, None)):
            raise ValueError(f"gaussians: an object with the tensors {', '.join(names)} expected, {name} is missing")
    with torch.no_grad():
        if rows is None:
            res = transform_gaussians(groups, transforms, xyz=gaussians._xyz, rotations=gaussians._rotation, scales=gaussians._scaling,
                                      log_scales=True, sh_rest=gaussians._features_rest, out="inplace")
            return res.status
        res = transform_gaussians(groups, transforms, xyz=gaussians._xyz, rotations=gaussians._rotation, scales=gaussians._scaling,
                                  log_scales=True, sh_rest=gaussians._features_rest, rows=rows)
        new = {"xyz": res.xyz, "rotation": res.rotations, "scaling": res.scales, "f_rest": res.sh_rest, "status": res.status}
        at = rows.detach().long()
        for key, name in (("f_dc", "_features_dc"), ("opacity", "_opacity"), ("semantic_feature", "_semantic_feature")):
            t = getattr(gaussians, name, None)
            if torch.is_tensor(t):
                new[key] = t.detach().index_select(0, at)
        return new


def transform_camera(world_view_transform, full_proj_transform, camera_center, quat, scale, translation, pivot=None):
    """The camera under which the transformed scene looks as the scene did: (world_view_transform, full_proj_transform,
    camera_center) in the reference's transposed convention (a point is the ROW vector [x, 1] in front of the matrix), computed in
    fp64 on the tensors' device and returned in their dtype.

    One transform: quat (4,), scale a number or a 0-dim tensor, translation (3,), pivot (3,) or None.  With T the map
    x -> A x + b, A = s R, b = p + t - A p: view' = T^-1 view diag(s, s, s, 1) - a rigid view matrix again, view-space lengths
    (the depth map) times s -, proj' = T^-1 proj - the same clip coordinates for every moved point -, centre' = T(centre)."""
    W = torch.as_tensor(world_view_transform)
    dev, dtype = W.device, W.dtype
    f64 = lambda a, shape: torch.as_tensor(a, device=dev).to(torch.float64).reshape(shape)
    W64, F64, c64 = f64(W, (4, 4)), f64(full_proj_transform, (4, 4)), f64(camera_center, (3,))
    q = f64(quat, (4,))
    s = f64(scale, ())
    t = f64(translation, (3,))
    p = torch.zeros(3, dtype=torch.float64, device=dev) if pivot is None else f64(pivot, (3,))
    r, x, y, z = (q / q.norm()).unbind(0)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]).reshape(3, 3)
    b = p + t - s * (R @ p)
    inv = torch.zeros(4, 4, dtype=torch.float64, device=dev)            # [x', 1] inv = [x, 1]: x = R^T (x' - b) / s
    inv[:3, :3] = R / s
    inv[3, :3] = -(R.t() @ b) / s
    inv[3, 3] = 1.0
    grow = torch.cat([s.expand(3), torch.ones(1, dtype=torch.float64, device=dev)])
    view = (inv @ W64) * grow[None, :]
    proj = inv @ F64
    center = s * (R @ c64) + b
    like = lambda v, ref: v.to(torch.as_tensor(ref).dtype) if torch.as_tensor(ref).is_floating_point() else v
    return like(view, W), like(proj, full_proj_transform), like(center, camera_center)


__all__ = ["Transforms", "Transformed", "transform_gaussians", "transform_model", "transform_camera", "BAD_QUAT", "ZERO_QUAT",
           "BAD_SCALE", "NONPOSITIVE_SCALE", "BAD_TRANSLATION", "BAD_PIVOT"]
