"""TEST INFRASTRUCTURE - numpy fp64 restatement of the object transforms (csrc/transform.hip; include/f3dgs.h:
f3dgs_transform_gaussians): the contract as array expressions, and for every float output the BOUND the GPU test uses - derived,
not measured.

The rotation matrices D_l of the SH bands come from a route that shares nothing with the kernel's recursion: a least-squares fit
of the rasterizer's own real basis (oracle/torch_oracle.py: _sh_to_rgb, restated in `basis`) on N_DIRS fixed unit directions,
band by band: basis(R d) = D_l basis(d).

The bound of an output that is a sum of n terms t_k, accumulated in fp64 and rounded once to float32:
    bar = ulp32(want) / 2 + 4 n 2^-53 sum|t_k|
Two fp64 evaluations of such a sum - the kernel's fused chain and numpy's - each lie within about n 2^-53 sum|t_k| of the true value
(the factors of a term come from two fp64 tables that agree to a few 2^-53); the factor 4 covers both and the tables; the rounding
to float32 adds half an ulp."""
import numpy as np

U = 2.0 ** -53
C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435]
BANDS = ((1, 4), (4, 9), (9, 16))            # columns of `basis` per band l = 1, 2, 3
N_DIRS = 200
COV_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
OK, BAD_QUAT, ZERO_QUAT, BAD_SCALE, NONPOSITIVE_SCALE, BAD_TRANSLATION, BAD_PIVOT = range(7)


def ulp32(v):
    """the spacing of float32 at |v| (fp64 array); 0 where v is not finite"""
    a = np.abs(np.asarray(v, np.float64)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.spacing(a).astype(np.float64)
    return np.where(np.isfinite(s), s, 0.0)


def basis(d):
    """(N, 3) unit directions -> (N, 16): the functions whose coefficients the rasterizer sums (signs and constants included)"""
    d = np.asarray(d, np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return np.stack([np.full_like(x, C0), -C1 * y, C1 * z, -C1 * x,
                     C2[0] * xy, C2[1] * yz, C2[2] * (2.0 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
                     C3[0] * y * (3.0 * xx - yy), C3[1] * xy * z, C3[2] * y * (4.0 * zz - xx - yy),
                     C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), C3[4] * x * (4.0 * zz - xx - yy), C3[5] * z * (xx - yy),
                     C3[6] * x * (xx - 3.0 * yy)], axis=1)


def _fixed_directions(n):
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


DIRS = _fixed_directions(N_DIRS)
_B = basis(DIRS)


def quat_to_rot(q):
    """R(q / |q|), (w, x, y, z), by oracle/torch_oracle.py's _quat_to_rot"""
    q = np.asarray(q, np.float64)
    r, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


_FITS = {}


def sh_matrices(R, full=False):
    """[D_1 (3, 3), D_2 (5, 5), D_3 (7, 7)] with basis(R d) = D_l basis(d) on the band; full=True: the (16, 16) fit over all
    bands at once (block-diagonal iff the bands do not mix)"""
    R = np.asarray(R, np.float64)
    rotated = basis(DIRS @ R.T)
    if full:
        return np.linalg.lstsq(_B, rotated, rcond=None)[0].T
    key = R.tobytes()
    if key not in _FITS:                                             # (the tests use a table many times over)
        _FITS[key] = [np.linalg.lstsq(_B[:, a:b], rotated[:, a:b], rcond=None)[0].T for a, b in BANDS]
    return [D.copy() for D in _FITS[key]]


def quat_mul(a, b):
    """Hamilton product a (x) b, (w, x, y, z), over the last axis"""
    aw, ax, ay, az = np.moveaxis(np.asarray(a, np.float64), -1, 0)
    bw, bx, by, bz = np.moveaxis(np.asarray(b, np.float64), -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


# the four products (component of a, component of b) summed into each component of a (x) b
QUAT_TERMS = (((0, 0), (1, 1), (2, 2), (3, 3)), ((0, 1), (1, 0), (2, 3), (3, 2)), ((0, 2), (1, 3), (2, 0), (3, 1)),
              ((0, 3), (1, 2), (2, 1), (3, 0)))


def table_status(quat, scale, translation, pivot=None):
    """(G,) int32: 0, or which input of the row was wrong - the first that applies"""
    q = np.asarray(quat, np.float32).reshape(-1, 4).astype(np.float64)
    s = np.asarray(scale, np.float32).reshape(-1).astype(np.float64)
    t = np.asarray(translation, np.float32).reshape(-1, 3)
    G = len(s)
    p = np.zeros((G, 3), np.float32) if pivot is None else np.asarray(pivot, np.float32).reshape(-1, 3)
    st = np.zeros(G, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        norm = np.sqrt((q * q).sum(1))
        rules = ((BAD_PIVOT, ~np.isfinite(p).all(1)), (BAD_TRANSLATION, ~np.isfinite(t).all(1)), (NONPOSITIVE_SCALE, ~(s > 0)),
                 (BAD_SCALE, ~np.isfinite(s)), (ZERO_QUAT, ~(norm > 0) | ~np.isfinite(norm)), (BAD_QUAT, ~np.isfinite(q).all(1)))
    for code, bad in rules:                                        # (the last written wins: the first of the order)
        st[bad] = code
    return st


def _bar(want, n, terms_abs):
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(want), 0.5 * ulp32(want) + 4 * n * U * terms_abs, 0.0)


def transform(groups, quat, scale, translation, pivot=None, xyz=None, rotations=None, scales=None, log_scales=True, cov3d=None,
              sh_rest=None, rows=None, dtype=np.float32):
    """The judge.  Per-Gaussian inputs as float32 arrays (sh_rest (P, n_rest, 3)); rows: None or (M,) integers (the gather form).
    Returns a dict: status (G,) int32; moved (rows,) bool - the output rows that are transformed; src (rows,) int64 - the input row
    of every output row, -1 for a row of zeros (dtype: what the table and the inputs are rounded to first - float32 as the kernel
    takes them; float64 judges a chain of maps on unrounded values); and per given input `name`: name (fp64: the value before the one rounding; the
    input itself on the rows that are not moved, 0 on the rows of zeros), name + "_bar" (fp64)."""
    g = np.asarray(groups).astype(np.int64)
    P = len(g)
    q = np.asarray(quat, dtype).reshape(-1, 4).astype(np.float64)
    s = np.asarray(scale, dtype).reshape(-1).astype(np.float64)
    t = np.asarray(translation, dtype).reshape(-1, 3).astype(np.float64)
    G = len(s)
    p = np.zeros((G, 3)) if pivot is None else np.asarray(pivot, dtype).reshape(-1, 3).astype(np.float64)
    status = table_status(quat, scale, translation, pivot)
    if rows is None:
        src = np.arange(P, dtype=np.int64)
    else:
        src = np.asarray(rows).astype(np.int64)
        src = np.where((src >= 0) & (src < P), src, -1)
    at = np.maximum(src, 0)
    gid = g[at] if P else np.zeros(len(src), np.int64)
    inside = (src >= 0) & (gid >= 0) & (gid < G)
    moved = inside & (status[np.where(inside, gid, 0)] == 0)
    out = dict(status=status, moved=moved, src=src)
    used = np.unique(gid[moved])
    R = {k: quat_to_rot(q[k]) for k in used}
    qn = {k: q[k] / np.sqrt((q[k] * q[k]).sum()) for k in used}

    def start(a, tail):
        a32 = np.asarray(a, dtype).reshape((P,) + tail)
        v = np.where((src >= 0).reshape((-1,) + (1,) * len(tail)), a32[at].astype(np.float64), 0.0) if P else np.zeros((len(src),) + tail)
        return v, np.zeros_like(v)

    with np.errstate(invalid="ignore", over="ignore"):
        if xyz is not None:
            v, bar = start(xyz, (3,))
            for k in used:
                sel = moved & (gid == k)
                d = v[sel] - p[k]
                terms = (s[k] * R[k])[None, :, :] * d[:, None, :]                        # (n, 3 out, 3 in)
                want = terms.sum(2) + p[k] + t[k]
                bar[sel] = _bar(want, 5, np.abs(terms).sum(2) + np.abs(p[k]) + np.abs(t[k]))
                v[sel] = want
            out["xyz"], out["xyz_bar"] = v, bar
        if rotations is not None:
            v, bar = start(rotations, (4,))
            for k in used:
                sel = moved & (gid == k)
                want = quat_mul(qn[k][None, :], v[sel])
                bar[sel] = _bar(want, 4, np.stack([sum(abs(qn[k][i]) * np.abs(v[sel][:, j]) for i, j in pairs) for pairs in QUAT_TERMS], 1))
                v[sel] = want
            out["rotations"], out["rotations_bar"] = v, bar
        if scales is not None:
            v, bar = start(scales, (3,))
            for k in used:
                sel = moved & (gid == k)
                if log_scales:
                    want = v[sel] + np.log(s[k])
                    bar[sel] = _bar(want, 2, np.abs(v[sel]) + abs(np.log(s[k])))
                else:
                    want = v[sel] * s[k]
                    bar[sel] = _bar(want, 1, np.abs(want))
                v[sel] = want
            out["scales"], out["scales_bar"] = v, bar
        if cov3d is not None:
            v, bar = start(cov3d, (6,))
            full = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
            for k in used:
                sel = moved & (gid == k)
                M = s[k] * R[k]
                S = v[sel][:, full]                                                     # (n, 3, 3)
                want = np.einsum("aj,njk,bk->nab", M, S, M)
                mag = np.einsum("aj,njk,bk->nab", np.abs(M), np.abs(S), np.abs(M))
                w6 = np.stack([want[:, a, b] for a, b in COV_PAIRS], 1)
                m6 = np.stack([mag[:, a, b] for a, b in COV_PAIRS], 1)
                bar[sel] = _bar(w6, 9, m6)
                v[sel] = w6
            out["cov3d"], out["cov3d_bar"] = v, bar
        if sh_rest is not None:
            n_rest = np.asarray(sh_rest).shape[1]
            assert n_rest in (0, 3, 8, 15)
            v, bar = start(sh_rest, (n_rest, 3))
            for k in used:
                sel = moved & (gid == k)
                D = sh_matrices(R[k])
                for l, (a, b) in enumerate(BANDS, start=1):
                    if b - 1 > n_rest:
                        break
                    c = v[sel][:, a - 1:b - 1, :]                                       # (n, 2l + 1, 3)
                    want = np.einsum("mk,nkc->nmc", D[l - 1], c)
                    mag = np.einsum("mk,nkc->nmc", np.abs(D[l - 1]), np.abs(c))
                    bb = _bar(want, 2 * l + 1, mag)
                    idx = np.flatnonzero(sel)
                    v[idx, a - 1:b - 1, :] = want
                    bar[idx, a - 1:b - 1, :] = bb
            out["sh_rest"], out["sh_rest_bar"] = v, bar
    return out


FIELDS = ("xyz", "rotations", "scales", "cov3d", "sh_rest")


def within(got, want, bar):
    """elementwise: |got - want| <= bar in fp64; a non-finite `want` needs the same value (NaN matches NaN)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        near = np.abs(got - want) <= bar
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    return np.where(np.isfinite(want), near, same)


def compose(first, second):
    """(quat, scale, translation) with pivot 0 of `second` after `first`, each (quat (4,), scale, translation (3,), pivot (3,)),
    fp64: x -> s2 R2 (s1 R1 (x - p1) + p1 + t1 - p2) + p2 + t2"""
    q1, s1, t1, p1 = [np.asarray(a, np.float64) for a in first]
    q2, s2, t2, p2 = [np.asarray(a, np.float64) for a in second]
    R1, R2 = quat_to_rot(q1), quat_to_rot(q2)
    b1 = p1 + t1 - s1 * R1 @ p1
    b2 = p2 + t2 - s2 * R2 @ p2
    q = quat_mul(q2 / np.sqrt((q2 * q2).sum()), q1 / np.sqrt((q1 * q1).sum()))
    return q, s1 * s2, s2 * R2 @ b1 + b2


def inverse(tr):
    """(quat, scale, translation) with pivot 0 of the inverse of (quat, scale, translation, pivot), fp64"""
    q, s, t, p = [np.asarray(a, np.float64) for a in tr]
    R = quat_to_rot(q)
    b = p + t - s * R @ p
    return q * np.array([1.0, -1.0, -1.0, -1.0]), 1.0 / s, -(R.T @ b) / s
