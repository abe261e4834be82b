"""GPU tests of the object transforms (csrc/transform.hip; transform.py) against tests/transform_oracle.py: every float output within
the judge's derived bound, status exact, the rows that are not transformed bit-identical to the input - over sizes, table sizes,
SH widths, layouts and both forms -, exact cases, chains of transforms, and the test of record: a transformed scene looks the same
from the correspondingly transformed camera."""
import math
import types

import numpy as np
import pytest
import torch

import transform_oracle as to
from test_gpu_contrib import _Model, _camera

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF, NAN = np.inf, np.nan
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _table(G, seed, invalid=True):
    """quat (any length), scale, translation, pivot as float32 arrays; with `invalid`: one row of every kind where G allows it"""
    g = np.random.default_rng(1000 + seed)
    quat = (g.normal(0, 1, (G, 4)) * g.uniform(0.2, 5.0, (G, 1))).astype(np.float32)
    scale = np.exp(g.uniform(-1.0, 1.0, G)).astype(np.float32)
    trans = g.normal(0, 2, (G, 3)).astype(np.float32)
    pivot = g.normal(0, 3, (G, 3)).astype(np.float32)
    if G > 0:
        quat[0], scale[0], trans[0], pivot[0] = (1, 0, 0, 0), 1, 0, 0          # (an identity row among them)
    if invalid and G >= 300:
        quat[7, 2] = NAN
        quat[8] = 0
        scale[9] = INF
        scale[10] = 0
        scale[11] = -2
        trans[12, 0] = -INF
        pivot[13, 1] = NAN
        quat[14], scale[14] = (NAN, 0, 0, 0), -1                                # (the first that applies: the quaternion)
    elif invalid and G >= 3:
        kind = seed % 3
        if kind == 0:
            trans[1, 2] = NAN
        elif kind == 1:
            quat[1] = 0
        else:
            scale[1] = -1
    return quat, scale, trans, pivot


def _data(P, n_rest, seed, offset=(0.0, 0.0, 0.0)):
    g = np.random.default_rng(seed)
    A = g.normal(0, 0.3, (P, 3, 3))
    S = A @ A.transpose(0, 2, 1)
    return dict(xyz=(g.normal(0, 2, (P, 3)) + np.asarray(offset)).astype(np.float32), rotations=g.normal(0, 1, (P, 4)).astype(np.float32),
                scales=g.uniform(-5, 0, (P, 3)).astype(np.float32),
                cov3d=np.stack([S[:, a, b] for a, b in to.COV_PAIRS], 1).astype(np.float32).reshape(P, 6),
                sh_rest=(0.3 * g.normal(0, 1, (P, n_rest, 3))).astype(np.float32))


def _ids(P, G, seed, coherent=False):
    g = np.random.default_rng(2000 + seed)
    ids = (np.arange(P) * G // max(P, 1)) if coherent else g.integers(0, G, P)
    bad = g.random(P) < 0.1                                                  # 10 % outside [0, G)
    ids = np.where(bad, g.choice(np.array([-1, G, G + 5, I32_MIN, I32_MAX, -7]), P), ids)
    return ids.astype(np.int64)


def _run(ids, table, data, log_scales=True, rows=None, out=None, dtype=torch.int64, tensors=None):
    import transform
    quat, scale, trans, pivot = table
    tr = transform.Transforms(_t(quat), _t(scale), _t(trans), None if pivot is None else _t(pivot))
    tensors = tensors if tensors is not None else {k: _t(v) for k, v in data.items()}
    rows_t = None if rows is None else _t(rows, torch.int32 if np.asarray(rows).dtype == np.int32 else torch.int64)
    res = transform.transform_gaussians(_t(ids, dtype), tr, log_scales=log_scales, rows=rows_t, out=out, **tensors)
    torch.cuda.synchronize()
    return res


def _check(res, ids, table, data, what, log_scales=True, rows=None, factor=1.0):
    """every given field against the judge: moved rows within `factor` x the bound, the others the input's bits (or zeros)"""
    want = to.transform(ids, *table, log_scales=log_scales, rows=rows, **data)
    assert res.status.dtype == torch.int32 and np.array_equal(_np(res.status), want["status"]), what
    moved, src = want["moved"], want["src"]
    worst = 0.0
    for name in to.FIELDS:
        got = getattr(res, name)
        if name not in data:
            assert got is None, (what, name)
            continue
        got = _np(got)
        assert got.dtype == np.float32 and got.shape == want[name].shape, (what, name, got.shape)
        if got.size == 0:
            continue
        ok = to.within(got, want[name], factor * want[name + "_bar"])
        if not ok[moved].all():
            bad = np.argwhere(~ok & moved.reshape((-1,) + (1,) * (got.ndim - 1)))[0]
            raise AssertionError(f"{what}: {name}{tuple(bad)} = {got[tuple(bad)]!r}, the judge has {want[name][tuple(bad)]!r} +- "
                                 f"{want[name + '_bar'][tuple(bad)]:.3e}")
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.abs(got.astype(np.float64) - want[name]) / want[name + "_bar"]
        if moved.any():
            worst = max(worst, float(np.nanmax(np.where(np.isfinite(ratio), ratio, 0.0)[moved])))
        same = ~moved
        ref = np.where((src >= 0).reshape((-1,) + (1,) * (got.ndim - 1)), data[name][np.maximum(src, 0)], np.float32(0)) if len(data[name]) \
            else np.zeros_like(got)
        assert np.array_equal(_bits(got[same]), _bits(ref[same])), (what, name, "rows that are not transformed changed")
    return want, worst


# ---- the sweep ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 257, 2049])
def test_sweep(P):
    worst = 0.0
    for G in (1, 3, 300):
        for n_rest in (0, 3, 8, 15):
            seed = P + 7 * G + n_rest
            table, data, ids = _table(G, seed), _data(P, n_rest, seed), _ids(P, G, seed, coherent=n_rest == 8)
            what = f"P = {P}, G = {G}, n_rest = {n_rest}"
            res = _run(ids, table, data)
            want, w = _check(res, ids, table, data, what)
            worst = max(worst, w)
            if G == 300:
                assert sorted(set(want["status"].tolist())) == [0, 1, 2, 3, 4, 5, 6]
            if P >= 63:
                assert 0 < want["moved"].sum() < P or G == 1
            # in place: the same bits as out of place, in the caller's own tensors
            tensors = {k: _t(v) for k, v in data.items()}
            ptr = {k: v.data_ptr() for k, v in tensors.items()}
            res2 = _run(ids, table, data, out="inplace", tensors=tensors)
            for name in to.FIELDS:
                a, b = getattr(res, name), getattr(res2, name)
                assert b.data_ptr() == ptr[name] and b is not None
                assert np.array_equal(_bits(_np(a)), _bits(_np(b))) and np.array_equal(_bits(_np(tensors[name])), _bits(_np(a))), (what, name)
            assert torch.equal(res.status, res2.status)
    print(f"P = {P}: worst |got - judge| / bound = {worst:.3f}")


def test_in_place_writes_nothing_to_the_rows_that_stay():
    """a NaN with a payload in a row that is not transformed survives bit for bit, in place and out of place (a copy through a
    float register keeps it; an arithmetic pass would quieten or replace it)"""
    P, G = 300, 3
    table, data, ids = _table(G, 1, invalid=False), _data(P, 15, 5), _ids(P, G, 5)
    stay = np.flatnonzero((ids < 0) | (ids >= G))
    assert len(stay) > 10
    payload = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x00000001, 0x80000000], np.uint32).view(np.float32)
    for name in data:
        flat = data[name].reshape(P, -1)
        flat[stay[:5], 0] = payload
    for out in (None, "inplace"):
        res = _run(ids, table, data, out=out)
        for name in data:
            got = _np(getattr(res, name)).reshape(P, -1)
            assert np.array_equal(_bits(got[stay]), _bits(data[name].reshape(P, -1)[stay])), (name, out)


def test_identity_table_returns_the_inputs():
    import transform
    P, G = 1000, 5
    data, ids = _data(P, 15, 3, offset=(100.0, -50.0, 7.0)), _ids(P, G, 3)
    ident = transform.Transforms.identity(G, DEV)
    assert ident.pivot is None and ident.quat.shape == (G, 4) and ident.num_groups == G
    for log_scales in (True, False):
        res = transform.transform_gaussians(_t(ids, torch.int64), ident, log_scales=log_scales, **{k: _t(v) for k, v in data.items()})
        torch.cuda.synchronize()
        assert _np(res.status).tolist() == [0] * G
        for name in to.FIELDS:
            assert (_np(getattr(res, name)) == data[name]).all(), name
    with_pivot = transform.Transforms.from_parts(G, DEV, pivot=[3.0, -2.0, 0.5])
    res = transform.transform_gaussians(_t(ids, torch.int64), with_pivot, xyz=_t(data["xyz"]))
    want = to.transform(ids, *[_np(a) for a in with_pivot], xyz=data["xyz"])
    assert to.within(_np(res.xyz), want["xyz"], want["xyz_bar"]).all()


def test_quarter_turns_are_exact():
    """Rotations of the cube and scales that are powers of two: every product is exact, the kernel's float32 equals the judge's
    fp64 value rounded once.  The first table has unit quaternions with exact entries (every field); the second the quarter turns
    (1, 0, 0, +-1) / sqrt 2 and their like, whose matrices carry 2^-52 where a 0 belongs - every field but the quaternions, whose
    products with sqrt(1/2) are not exact."""
    P = 500
    data = _data(P, 15, 9)
    data["scales"] = np.exp(data["scales"]).astype(np.float32)
    exact = np.array([[0.5, 0.5, 0.5, 0.5], [0, 1, 0, 0], [0, 0, 0, 1], [0.5, -0.5, 0.5, -0.5], [0, 0, 1, 0], [-0.5, 0.5, 0.5, 0.5]], np.float32)
    turns = np.array([[1, 0, 0, 1], [1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, -1], [3, -3, 0, 0], [2, 0, -2, 0]], np.float32)
    scale = np.array([1, 2, 0.5, 4, 1, 0.25], np.float32)
    zero = np.zeros((6, 3), np.float32)
    ids = _ids(P, 6, 9)
    for name, quat in (("exact", exact), ("turns", turns)):
        use = {k: v for k, v in data.items() if not (name == "turns" and k == "rotations")}
        res = _run(ids, (quat, scale, zero, None), use, log_scales=False)
        want, _ = _check(res, ids, (quat, scale, zero, None), use, name, log_scales=False)
        for field in use:
            got, w = _np(getattr(res, field)), want[field].astype(np.float32)
            assert np.array_equal(got, w), (name, field, np.abs(got - w).max())
            assert not np.array_equal(got, use[field])


def test_composition_and_inverse():
    """T1 then T2 against T2 o T1 in one call, and T then T^-1 against the input.  The tables are chosen so that the composite
    and the inverse are float32 tables themselves: quaternions with small integer entries (the kernel normalises), scales that are
    powers of two, one pivot for both steps and no shift in the first.  Then every route approximates the same exact map, and a
    vector that the second step rotates (a position, a quaternion, the coefficients of a band; a covariance, with the square of
    the scale) is off by at most the second step's bound plus the first step's bound carried through the second map - which keeps
    its Euclidean length up to the scale: |error| <= |bar_2| + k |bar_1| in the Euclidean norm of that vector, twice the bound
    where the two steps' magnitudes agree.  (k = s_2 for a position, 1 for a quaternion, a band and - added, not turned - a
    log-scale, sqrt 2 s_2^2 for the six covariance entries: the map keeps the Frobenius norm, which counts the off-diagonal
    entries twice.)"""
    P, G = 700, 4
    g = np.random.default_rng(17)
    data, ids = _data(P, 15, 17), _ids(P, G, 17, coherent=True)
    q1 = g.integers(-3, 4, (G, 4)).astype(np.float32)
    q2 = g.integers(-3, 4, (G, 4)).astype(np.float32)
    q1[:, 0] += 4
    q2[:, 0] -= 4
    s1, s2 = np.array([2, 0.5, 1, 4], np.float32), np.array([0.5, 0.25, 2, 1], np.float32)
    pivot = g.integers(-4, 5, (G, 3)).astype(np.float32) * 0.5
    t2 = g.integers(-8, 9, (G, 3)).astype(np.float32) * 0.25
    zero = np.zeros((G, 3), np.float32)
    T1, T2 = (q1, s1, zero, pivot), (q2, s2, t2, pivot)
    T12 = (to.quat_mul(q2, q1).astype(np.float32), s1 * s2, t2, pivot)
    assert np.array_equal(T12[0].astype(np.float64), to.quat_mul(q2, q1))                     # (the composite table is exact)
    Tinv = (q1 * np.array([1, -1, -1, -1], np.float32), 1 / s1, -zero, pivot)

    def chain(first, second, want_fp64, k_of):
        r1 = _run(ids, first, data)
        mid = {k: _np(getattr(r1, k)) for k in data}
        w1, _ = _check(r1, ids, first, data, "first step")
        r2 = _run(ids, second, mid)
        w2, _ = _check(r2, ids, second, mid, "second step")
        worst = 0.0
        for name in data:
            got = _np(getattr(r2, name)).astype(np.float64)
            k = k_of[name]
            if name == "sh_rest":                                    # a band of one colour turns together
                parts = [(slice(None), slice(a - 1, b - 1), c) for a, b in to.BANDS for c in range(3)]
            elif name == "scales":                                   # nothing turns: element by element
                parts = [(slice(None), slice(c, c + 1)) for c in range(3)]
            else:
                parts = [(slice(None), slice(None))]
            for part in parts:
                norm = lambda a: np.sqrt((a[part].reshape(P, -1) ** 2).sum(1))
                err, bar = norm(got - want_fp64[name]), norm(w2[name + "_bar"]) + k * norm(w1[name + "_bar"])
                assert (err <= bar).all(), (name, part, float((err / bar).max()))
                worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
        return worst

    gid = np.where((ids >= 0) & (ids < G), ids, 0)
    k12 = dict(xyz=s2[gid], rotations=1.0, scales=1.0, cov3d=math.sqrt(2) * (s2 * s2)[gid], sh_rest=1.0)
    one = to.transform(ids, *T12, **data)
    w = chain(T1, T2, one, k12)
    r12 = _run(ids, T12, data)
    _check(r12, ids, T12, data, "T2 o T1 in one call")
    print(f"T1 then T2 against T2 o T1: worst |error| / (|bar_2| + k |bar_1|) = {w:.3f}")
    kinv = dict(xyz=(1 / s1)[gid], rotations=1.0, scales=1.0, cov3d=math.sqrt(2) * (1 / (s1 * s1))[gid], sh_rest=1.0)
    back = {k: v.astype(np.float64) for k, v in data.items()}
    w = chain(T1, Tinv, back, kinv)
    print(f"T then T^-1 against the input: worst |error| / (|bar_2| + k |bar_1|) = {w:.3f}")


def test_conditioning_far_from_the_origin():
    """A group centred at (500, -200, 70), 0.1 wide, turned about its centroid: the fp64 chain on x - p stays within the
    one-rounding bound; float32 s R x + t', t' = p + t - s R p folded beforehand, does not."""
    P = 4000
    g = np.random.default_rng(23)
    centre = np.array([500.0, -200.0, 70.0])
    xyz = (centre + g.normal(0, 0.1, (P, 3))).astype(np.float32)
    table = (np.array([[0.3, 0.5, -0.4, 0.7]], np.float32), np.array([1.3], np.float32), np.array([[0.25, 0.5, -0.125]], np.float32),
             centre.astype(np.float32)[None])
    ids = np.zeros(P, np.int64)
    res = _run(ids, table, dict(xyz=xyz))
    want, worst = _check(res, ids, table, dict(xyz=xyz), "far from the origin")
    assert worst <= 1.0
    A32 = (1.3 * to.quat_to_rot(table[0][0])).astype(np.float32)
    b32 = (centre + table[2][0] - (1.3 * to.quat_to_rot(table[0][0])) @ centre).astype(np.float32)
    folded = (xyz @ A32.T + b32).astype(np.float32)                          # the float32 route
    ratio = np.abs(folded.astype(np.float64) - want["xyz"]) / want["xyz_bar"]
    print(f"far from the origin: kernel within {worst:.3f} of the bound; float32 s R x + t' up to {ratio.max():.1f} bounds off")
    assert ratio.max() > 2


def test_layouts_ids_and_single_inputs():
    import transform
    P, G = 777, 3
    table, data, ids = _table(G, 4, invalid=False), _data(P, 15, 31), _ids(P, G, 31)
    # sh_rest as shs[:, 1:, :] of a (P, 16, 3) tensor: read and written in place, the DC term untouched
    shs = np.concatenate([np.full((P, 1, 3), 0.25, np.float32), data["sh_rest"]], 1)
    t_shs = _t(shs)
    view = t_shs[:, 1:, :]
    assert not view.is_contiguous() and view.data_ptr() % 16 != 0
    res = _run(ids, table, None, tensors=dict(sh_rest=view))
    _check(res, ids, table, dict(sh_rest=data["sh_rest"]), "a view of shs")
    assert res.sh_rest.is_contiguous() and torch.equal(t_shs, _t(shs))
    res = _run(ids, table, None, tensors=dict(sh_rest=view), out="inplace")
    _check(res, ids, table, dict(sh_rest=data["sh_rest"]), "a view of shs, in place")
    assert res.sh_rest.data_ptr() == view.data_ptr() and (_np(t_shs[:, 0, :]) == 0.25).all()
    # degree 1 and 2 of the same tensor, and a transposed layout (copied first; refused in place)
    for n in (3, 8):
        res = _run(ids, table, None, tensors=dict(sh_rest=_t(shs)[:, 1:1 + n, :]))
        _check(res, ids, table, dict(sh_rest=data["sh_rest"][:, :n]), f"shs[:, 1:{1 + n}]")
    odd = _t(np.ascontiguousarray(data["sh_rest"].transpose(0, 2, 1))).transpose(1, 2)
    _check(_run(ids, table, None, tensors=dict(sh_rest=odd)), ids, table, dict(sh_rest=data["sh_rest"]), "a transposed sh_rest")
    with pytest.raises(ValueError, match="inplace"):
        _run(ids, table, None, tensors=dict(sh_rest=odd), out="inplace")
    # a base pointer that is only 4-byte aligned, for every tensor
    for name, v in data.items():
        flat = torch.zeros(v.size + 1, device=DEV)
        flat[1:] = _t(v).reshape(-1)
        shifted = flat[1:].view(v.shape)
        assert shifted.data_ptr() % 8 == 4
        _check(_run(ids, table, None, tensors={name: shifted}), ids, table, {name: v}, f"{name} alone, misaligned")
    # cov3d in the place of scales and rotations; activated scales; no pivot; empty sh_rest
    _check(_run(ids, table, dict(xyz=data["xyz"], cov3d=data["cov3d"])), ids, table, dict(xyz=data["xyz"], cov3d=data["cov3d"]), "cov3d")
    lin = dict(scales=np.exp(data["scales"]).astype(np.float32))
    _check(_run(ids, table, lin, log_scales=False), ids, table, lin, "activated scales", log_scales=False)
    no_pivot = table[:3] + (None,)
    _check(_run(ids, no_pivot, dict(xyz=data["xyz"])), ids, no_pivot, dict(xyz=data["xyz"]), "no pivot")
    res = _run(ids, table, dict(xyz=data["xyz"], sh_rest=data["sh_rest"][:, :0]))
    assert res.sh_rest.shape == (P, 0, 3)
    res = _run(ids, table, dict(sh_rest=data["sh_rest"][:, :0]))
    assert res.sh_rest.shape == (P, 0, 3) and res.xyz is None and _np(res.status).tolist() == [0] * G
    # int32 ids, and a bool mask as the one group of a table of one row
    _check(_run(ids.clip(I32_MIN, I32_MAX), table, dict(xyz=data["xyz"]), dtype=torch.int32), ids, table, dict(xyz=data["xyz"]), "int32 ids")
    one = tuple(a[2:3] for a in table)
    mask = ids == 1
    res = transform.transform_gaussians(_t(mask, torch.bool), transform.Transforms(*[_t(a) for a in one]), xyz=_t(data["xyz"]))
    _check(res, np.where(mask, 0, -1), one, dict(xyz=data["xyz"]), "a bool mask")
    # the constructors: axis and angle, a matrix (every branch of Shepperd's method), about the centroid
    axis = np.array([[0, 0, 1], [1, 1, 0], [0, -2, 0], [1, 2, 3]], np.float64)
    angle = np.array([0.5 * math.pi, 3.1, -2.0, 1e-3])
    aa = transform.Transforms.from_axis_angle(_t(axis, torch.float64), _t(angle, torch.float64))
    for k in range(4):
        u = axis[k] / np.linalg.norm(axis[k])
        Kx = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
        R = np.eye(3) + math.sin(angle[k]) * Kx + (1 - math.cos(angle[k])) * Kx @ Kx
        assert np.abs(to.quat_to_rot(_np(aa.quat)[k]) - R).max() < 1e-6
    Rs = np.stack([to.quat_to_rot(q) for q in np.array([[1, 0.1, 0, 0.2], [0.1, 1, 0.2, 0], [0, 0.1, 1, 0.1], [0.05, 0, 0.1, 1], [0, 0, 0, 1],
                                                          [1, 1, 1, 1]], np.float64)])
    fm = transform.Transforms.from_matrix(_t(Rs, torch.float64), scale=2.0, translation=[1.0, 2.0, 3.0])
    for k in range(len(Rs)):
        assert np.abs(to.quat_to_rot(_np(fm.quat)[k]) - Rs[k]).max() < 1e-6
    assert _np(fm.scale).tolist() == [2.0] * 6 and _np(fm.translation)[3].tolist() == [1.0, 2.0, 3.0] and fm.pivot is None


def test_gather():
    P, G = 500, 3
    table, data = _table(G, 1), _data(P, 15, 41)
    ids = _ids(P, G, 41)
    g = np.random.default_rng(41)
    rows = np.concatenate([g.permutation(P), g.integers(0, P, 300), [-1, P, P + 7, I32_MIN, I32_MAX, 2**40, -2**40], np.full(9, 17)])
    assert len(rows) > P
    res = _run(ids, table, data, rows=rows)
    want, _ = _check(res, ids, table, data, "gather, M > P", rows=rows)
    assert (want["src"] < 0).sum() == 7 and res.xyz.shape == (len(rows), 3)
    res32 = _run(ids, table, dict(xyz=data["xyz"]), rows=rows.clip(I32_MIN, I32_MAX).astype(np.int32))
    assert torch.equal(res32.xyz, res.xyz)
    for M in (0, 1):
        r = _run(ids, table, data, rows=rows[:M])
        _check(r, ids, table, data, f"M = {M}", rows=rows[:M])
    empty = _run(np.zeros(0, np.int64), table, _data(0, 15, 1), rows=np.zeros(0, np.int64))
    assert empty.xyz.shape == (0, 3) and np.array_equal(_np(empty.status), want["status"])
    # "a second instance over there": 100 000 rows of one group in one call (several hundred workgroups)
    M = 100_000
    one = tuple(a[:1] for a in _table(1, 3))
    one[0][0], one[1][0], one[2][0], one[3][0] = (0.6, -0.2, 0.7, 0.1), 1.25, (4.0, 0.0, -1.0), (0.5, 0.5, 2.0)
    big_rows = g.integers(0, P, M)
    res = _run(np.zeros(P, np.int64), one, data, rows=big_rows)
    _check(res, np.zeros(P, np.int64), one, data, "100 000 rows", rows=big_rows)


# ---- the test of record: the render invariant ---------------------------------------------------------------------------------

def _scene(P, W, H, seed, split=False):
    from test_transform_cpu import _tiny_scene
    sc = _tiny_scene(P, W, H, seed)
    sc["P"] = P
    if split:                                                # two instances, well apart: the left and the right of the image
        half = P // 2
        sc["means3D"][:half, 0] = -0.75 * sc["tanfovx"] * sc["means3D"][:half, 2] + 0.05 * sc["means3D"][:half, 0]
        sc["means3D"][half:, 0] = 0.75 * sc["tanfovx"] * sc["means3D"][half:, 2] + 0.05 * sc["means3D"][half:, 0]
        sc["scales"] *= 0.3
    return sc


def _render(sc, pc, cam=None):
    import contrib
    from diff_gaussian_rasterization import GaussianRasterizer
    view = _camera(sc)
    if cam is not None:
        view.world_view_transform, view.full_proj_transform, view.camera_center = cam
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    settings, args = contrib._render_inputs(view, pc, pipe, sc["bg"].to(DEV), 1.0, None)
    with torch.no_grad():
        color, fmap, radii, depth = GaussianRasterizer(settings)(means2D=torch.zeros_like(pc.get_xyz), **args)
    torch.cuda.synchronize()
    return dict(color=color, feature_map=fmap, depth=depth, radii=radii)


def _model(sc):
    pc = _Model(sc)
    pc.get_semantic_feature = sc["semantic_feature"].to(DEV).clone()
    pc.get_rotation = torch.nn.functional.normalize(pc.get_rotation)        # the model's activation
    return pc


def test_render_invariant_whole_scene():
    """The scene as one group under a similarity transform, the camera under transform_camera: colour, feature map and depth / s
    against the untransformed render.  The bar is the same difference with the JUDGE's fp64-transformed parameters (rounded to
    float32) in the kernel's place: float32 parameters and a float32 rasterizer on both sides, so the kernel may take twice that,
    and never needs to be under the project's image bar of 1e-4."""
    import transform
    P, W, H = 400, 64, 48
    sc = _scene(P, W, H, 6)
    pc = _model(sc)
    base = _render(sc, pc)
    assert int((base["radii"] > 0).sum()) == P
    quat, s, t, p = np.array([0.8, 0.3, -0.4, 0.2], np.float32), np.float32(1.6), np.array([0.5, -2.0, 3.0], np.float32), \
        np.array([0.1, 0.0, 5.0], np.float32)
    tr = transform.Transforms.from_parts(1, DEV, quat, float(s), t, p)
    ids = torch.zeros(P, dtype=torch.int64, device=DEV)
    shs = pc.get_features.clone()
    res = transform.transform_gaussians(ids, tr, xyz=pc.get_xyz, rotations=pc.get_rotation, scales=pc.get_scaling, log_scales=False,
                                        sh_rest=shs[:, 1:, :])
    cam = transform.transform_camera(sc["viewmatrix"].to(DEV), sc["projmatrix"].to(DEV), sc["campos"].to(DEV), quat, s, t, p)
    assert all(c.dtype == torch.float32 and c.device.type == "cuda" for c in cam)
    want = to.transform(np.zeros(P, np.int64), quat[None], [s], t[None], p[None], xyz=_np(pc.get_xyz), rotations=_np(pc.get_rotation),
                        scales=_np(pc.get_scaling), log_scales=False, sh_rest=_np(shs[:, 1:, :]))

    def moved_model(xyz, rot, scales, rest):
        m = _model(sc)
        m.get_xyz, m.get_rotation, m.get_scaling = xyz, torch.nn.functional.normalize(rot), scales
        m.get_features = torch.cat([shs[:, :1, :], rest], 1).contiguous()
        return m

    outs = {"kernel": _render(sc, moved_model(res.xyz, res.rotations, res.scales, res.sh_rest), cam),
            "judge": _render(sc, moved_model(*[_t(want[k].astype(np.float32)) for k in ("xyz", "rotations", "scales", "sh_rest")]), cam)}
    diff = {}
    for who, out in outs.items():
        assert int((out["radii"] > 0).sum()) == P
        diff[who] = {k: float((out[k] / d - base[k]).abs().max()) for k, d in (("color", 1.0), ("feature_map", 1.0), ("depth", float(s)))}
        print(f"render invariant, {who}'s parameters: max |moved - base| colour {diff[who]['color']:.3e}, feature map "
              f"{diff[who]['feature_map']:.3e}, depth / s {diff[who]['depth']:.3e}")
    for k in ("color", "feature_map", "depth"):
        assert diff["kernel"][k] <= max(2 * diff["judge"][k], 1e-4), (k, diff)
    assert float((outs["kernel"]["color"] - base["color"]).abs().max()) < 1e-2 < float(base["color"].abs().max())


def test_render_invariant_one_of_two_instances():
    """Only the left instance moves (in place, through transform_model): the tiles that the right instance alone covers keep
    their bits."""
    import transform
    P, W, H = 300, 64, 48
    sc = _scene(P, W, H, 8, split=True)
    half = P // 2
    pc = _model(sc)
    log_scaling = torch.log(pc.get_scaling)
    pc.get_scaling = torch.exp(log_scaling)                  # the model's activation of ITS parameter: the same bits on both sides
    base = _render(sc, pc)
    gm = types.SimpleNamespace(_xyz=pc.get_xyz.clone(), _rotation=pc.get_rotation.clone(), _scaling=log_scaling.clone(),
                               _features_rest=pc.get_features[:, 1:, :].clone())
    ids = torch.where(torch.arange(P, device=DEV) < half, 0, 1)
    tr = transform.Transforms.from_parts(2, DEV, quat=[[0.95, 0.05, 0.05, 0.3], [1.0, 0, 0, 0]], scale=[0.8, 1.0],
                                         translation=[[0.0, 0.3, 0.5], [0, 0, 0]], pivot=[[-2.0, 0.0, 5.0], [0, 0, 0]])
    tr = transform.Transforms(tr.quat, torch.tensor([0.8, float("nan")], device=DEV), tr.translation, tr.pivot)      # group 1: invalid, stays
    status = transform.transform_model(gm, ids, tr)
    torch.cuda.synchronize()
    assert _np(status).tolist() == [0, transform.BAD_SCALE]
    assert torch.equal(gm._xyz[half:], pc.get_xyz[half:]) and not torch.equal(gm._xyz[:half], pc.get_xyz[:half])
    moved = _model(sc)
    # (the product of two unit quaternions, used as it is: a second normalisation could move the last bit of the rows that stayed)
    moved.get_xyz, moved.get_rotation, moved.get_scaling = gm._xyz, gm._rotation, torch.exp(gm._scaling)
    moved.get_features = torch.cat([pc.get_features[:, :1, :], gm._features_rest], 1).contiguous()
    out = _render(sc, moved)
    # the tiles of the right instance alone: columns of tiles that no Gaussian of the left one reaches, before or after
    rad = torch.maximum(base["radii"], out["radii"])[:half].float()
    assert float((out["color"] - base["color"]).abs().max()) > 0.05
    left_reach = 0.0
    for m in (pc, moved):
        px = ((m.get_xyz[:half, 0] / m.get_xyz[:half, 2]) / sc["tanfovx"] * 0.5 + 0.5) * W
        left_reach = max(left_reach, float((px + rad + 1).max()))
    first = (int(left_reach) // 16 + 1) * 16
    assert first < W, "the left instance reaches every column of tiles: choose another scene"
    for k in ("color", "feature_map", "depth"):
        assert torch.equal(out[k][..., first:], base[k][..., first:]), k
    assert float(base["color"][..., first:].sub(sc["bg"].to(DEV)[:, None, None]).abs().max()) > 0.05


# ---- end to end, capture, errors ------------------------------------------------------------------------------------------------

def test_instance_lifter_to_transform_model():
    """InstanceLifter labels -> group_stats -> Transforms.about_centroid -> transform_model, nothing read in between; then the
    judge on the read-back labels and centroids.  And the gather form: moved copies of one instance as new rows."""
    import groups
    import instances as ins
    import transform
    from synth import make_scene
    P, L = 2000, 12
    sc = make_scene(P=P, C=4, width=64, height=64, seed=21, scale_lo=0.01, scale_hi=0.1)
    y, x = np.mgrid[0:64, 0:64]
    lifter = ins.InstanceLifter(P, L, 16, DEV)
    pc = _Model(sc)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    lifter.add_view(_camera(sc), pc, pipe, sc["bg"].to(DEV), torch.from_numpy(((x // 16) + 4 * (y // 32)).astype(np.int64)).to(DEV))
    gm = types.SimpleNamespace(_xyz=pc.get_xyz.clone(), _rotation=pc.get_rotation.clone() * 1.5, _scaling=torch.log(pc.get_scaling),
                               _features_rest=pc.get_features[:, 1:, :].clone(), _features_dc=pc.get_features[:, :1, :].clone(),
                               _opacity=pc.get_opacity.clone(), _semantic_feature=sc["semantic_feature"].to(DEV))
    before = {k: _np(v).copy() for k, v in vars(gm).items()}
    labels = groups.lifter_labels(lifter, 0.05)
    st = groups.group_stats(labels, gm._xyz, L)
    angles = torch.linspace(0.2, 2.4, L, device=DEV)
    tr = transform.Transforms.about_centroid(st, quat=transform.Transforms.from_axis_angle([0.0, 1.0, 0.2], angles).quat,
                                             scale=torch.linspace(0.5, 1.5, L, device=DEV), translation=[0.0, 0.1, 0.0])
    rows = torch.nonzero(labels == labels[labels >= 0][0])[:, 0]            # (the caller's host read, before the chain under test)
    new = transform.transform_model(gm, labels, tr, rows=rows)
    status = transform.transform_model(gm, labels, tr)
    torch.cuda.synchronize()
    lab = _np(labels)
    assert 0.2 < (lab >= 0).mean() and len(np.unique(lab[lab >= 0])) >= 4 and _np(status).tolist() == [0] * L
    table = tuple(_np(a) for a in tr)
    data = dict(xyz=before["_xyz"], rotations=before["_rotation"], scales=before["_scaling"], sh_rest=before["_features_rest"])
    got = transform.Transformed(gm._xyz, gm._rotation, gm._scaling, None, gm._features_rest, status)
    _check(got, lab, table, data, "transform_model in place")
    got = transform.Transformed(new["xyz"], new["rotation"], new["scaling"], None, new["f_rest"], new["status"])
    _check(got, lab, table, data, "transform_model, new rows", rows=_np(rows))
    at = _np(rows)
    assert len(at) > 5 and set(new) == {"xyz", "rotation", "scaling", "f_rest", "status", "f_dc", "opacity", "semantic_feature"}
    for key, name in (("f_dc", "_features_dc"), ("opacity", "_opacity"), ("semantic_feature", "_semantic_feature")):
        assert np.array_equal(_np(new[key]), before[name][at]) and np.array_equal(_np(getattr(gm, name)), before[name])


def test_capture_and_replay():
    """group_stats followed by transform_gaussians about the centroids, captured as one linear graph on one stream and replayed
    on new data behind the same pointers."""
    import groups
    import transform
    P, G = 3000, 20
    sets = []
    for seed in (1, 2):
        d = _data(P, 15, 50 + seed, offset=(3.0 * seed, 0.0, -2.0))
        sets.append((_ids(P, G, seed, coherent=seed == 2), d, _table(G, seed)))
    t_ids = _t(sets[0][0], torch.int64)
    t_data = {k: _t(v) for k, v in sets[0][1].items()}
    t_quat, t_scale, t_trans = [_t(a) for a in sets[0][2][:3]]

    def run():
        st = groups.group_stats(t_ids, t_data["xyz"], G, cov=False)
        tr = transform.Transforms(t_quat, t_scale, t_trans, st.centroid)
        return st, transform.transform_gaussians(t_ids, tr, **t_data)

    def load(which):
        ids, d, table = sets[which]
        t_ids.copy_(_t(ids, torch.int64))
        for k, v in d.items():
            t_data[k].copy_(_t(v))
        for t, a in zip((t_quat, t_scale, t_trans), table[:3]):
            t.copy_(_t(a))

    def check(which, res):
        ids, d, table = sets[which]
        st, out = res
        _check(out, ids, table[:3] + (_np(st.centroid),), d, f"data {which}")

    for which in (0, 1):
        load(which)
        res = run()
        torch.cuda.synchronize()
        check(which, res)
    load(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # one stream, no parallel branches
        captured = run()
    for which in (1, 0):
        load(which)
        graph.replay()
        torch.cuda.synchronize()
        check(which, captured)


def test_errors():
    import transform
    from simple_knn import _C
    P, G = 10, 4
    ids = torch.zeros(P, device=DEV, dtype=torch.int64)
    xyz, rot, sh = torch.zeros(P, 3, device=DEV), torch.ones(P, 4, device=DEV), torch.zeros(P, 15, 3, device=DEV)
    tr = transform.Transforms.identity(G, DEV)
    bad_tables = (None, (tr.quat, tr.scale, tr.translation, None), transform.Transforms(tr.quat.cpu(), tr.scale, tr.translation, None),
                  transform.Transforms(tr.quat[:3], tr.scale, tr.translation, None), transform.Transforms(tr.quat.double(), tr.scale, tr.translation, None),
                  transform.Transforms(tr.quat, tr.scale[:, None], tr.translation, None), transform.Transforms(tr.quat, tr.scale, tr.translation, tr.quat))
    for table in bad_tables:
        with pytest.raises(ValueError, match="expected"):
            transform.transform_gaussians(ids, table, xyz=xyz)
    for args, kw in (((ids.cpu(), tr), dict(xyz=xyz)), ((ids.float(), tr), dict(xyz=xyz)), ((ids[None], tr), dict(xyz=xyz)), ((ids > 0, tr), dict(xyz=xyz)),
                     ((ids, tr), {}), ((ids, tr), dict(xyz=xyz.cpu())), ((ids, tr), dict(xyz=xyz[:9])), ((ids, tr), dict(xyz=xyz.double())),
                     ((ids, tr), dict(rotations=xyz)), ((ids, tr), dict(scales=rot)), ((ids, tr), dict(cov3d=xyz)),
                     ((ids, tr), dict(sh_rest=sh[:, :4])), ((ids, tr), dict(sh_rest=sh.half())), ((ids, tr), dict(sh_rest=sh.reshape(P, 45))),
                     ((ids, tr), dict(sh_rest=sh.cpu())), ((ids, tr), dict(xyz=xyz, out="in place")),
                     ((ids, tr), dict(xyz=xyz, out="inplace", rows=ids)), ((ids, tr), dict(xyz=xyz.t().contiguous().t(), out="inplace")),
                     ((ids, tr), dict(xyz=xyz, rows=ids.float())), ((ids, tr), dict(xyz=xyz, rows=ids.cpu())), ((ids, tr), dict(xyz=xyz, rows=ids[None]))):
        with pytest.raises(ValueError, match="expected|HIP device|one group|inplace"):
            transform.transform_gaussians(*args, **kw)
    with pytest.raises(ValueError, match=r"torch.float64 \(10, 3\) on cuda:0"):      # dtype, shape and device are named
        transform.transform_gaussians(ids, tr, xyz=xyz.double())
    with pytest.raises(ValueError, match="broadcasts"):
        transform.Transforms.from_parts(G, DEV, quat=[1.0, 0.0, 0.0])
    # the binding's own checks
    g32 = ids.int()
    for args in ((g32, tr.quat, tr.scale, tr.translation, None, None, None, None, False, None, None, None, False),
                 (ids, tr.quat, tr.scale, tr.translation, None, xyz, None, None, False, None, None, None, False),
                 (g32, tr.quat[:3], tr.scale, tr.translation, None, xyz, None, None, False, None, None, None, False),
                 (g32, tr.quat, tr.scale, tr.translation, None, xyz, None, None, False, None, sh[:, :4], None, False),
                 (g32, tr.quat, tr.scale, tr.translation, None, xyz, None, None, False, None, None, g32, True),
                 (g32, tr.quat, tr.scale, tr.translation, None, xyz, None, None, False, None, None, ids, False),
                 (g32.cpu(), tr.quat, tr.scale, tr.translation, None, xyz, None, None, False, None, None, None, False)):
        with pytest.raises(RuntimeError, match="expected|given|taken|exclude|HIP device"):
            _C.transform_gaussians(*args)
