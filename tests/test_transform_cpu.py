"""The judge of the object transforms (tests/transform_oracle.py) judged itself, without a GPU: the fitted SH rotation matrices
against the properties of a rotation and against hand cases, the quaternion and covariance rules against the rasterizer's own
formulas, transform.transform_camera against the fp64 rasterizer (oracle/torch_oracle.py), and the argument checks of the C ABI
(include/f3dgs.h: f3dgs_transform_gaussians) and of transform.py that answer before any device work."""
import ctypes
import os

import numpy as np
import pytest
import torch

import transform_oracle as to
from oracle import torch_oracle
from util import ROOT


def _quats(n, seed):
    q = np.random.default_rng(seed).normal(0, 1, (n, 4))
    return q / np.sqrt((q * q).sum(1, keepdims=True))


def _dirs(n, seed):
    d = np.random.default_rng(seed).normal(0, 1, (n, 3))
    return d / np.sqrt((d * d).sum(1, keepdims=True))


QUARTER_Z = np.array([np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)])        # x -> y -> -x


def test_basis_is_the_rasterizers():
    d = _dirs(40, 1)
    sh = np.random.default_rng(2).normal(0, 1, (40, 16, 3))
    for deg in range(4):
        want = torch_oracle._sh_to_rgb(deg, torch.from_numpy(sh), torch.from_numpy(d)).numpy()
        n = (deg + 1) ** 2
        got = np.einsum("nk,nkc->nc", to.basis(d)[:, :n], sh[:, :n])
        assert np.abs(got - want).max() < 1e-14, deg


def test_sh_matrices_compose_are_orthogonal_and_block_diagonal():
    q = _quats(6, 3)
    for a in range(0, 6, 2):
        R1, R2 = to.quat_to_rot(q[a]), to.quat_to_rot(q[a + 1])
        D1, D2, D12 = to.sh_matrices(R1), to.sh_matrices(R2), to.sh_matrices(R1 @ R2)
        for l in range(3):
            n = 2 * l + 3
            assert np.abs(D12[l] - D1[l] @ D2[l]).max() < 2e-14
            assert np.abs(D1[l] @ D1[l].T - np.eye(n)).max() < 2e-14
            assert abs(np.linalg.det(D1[l]) - 1) < 1e-13
        full = to.sh_matrices(R1, full=True)
        assert abs(full[0, 0] - 1) < 1e-14
        for l, (a0, b0) in enumerate(to.BANDS):
            assert np.abs(full[a0:b0, a0:b0] - D1[l]).max() < 2e-14
            full[a0:b0, a0:b0] = 0
        full[0, 0] = 0
        assert np.abs(full).max() < 2e-14                            # the bands do not mix
    for l, D in enumerate(to.sh_matrices(np.eye(3))):
        assert np.abs(D - np.eye(2 * l + 3)).max() < 1e-14


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_rotated_coefficients_give_the_same_colour_in_the_rotated_direction(deg):
    """_sh_to_rgb(deg, D c, R d) == _sh_to_rgb(deg, c, d) on fresh directions"""
    g = np.random.default_rng(10 + deg)
    R = to.quat_to_rot(_quats(1, 20 + deg)[0])
    d = _dirs(64, 30 + deg)
    n = (deg + 1) ** 2
    sh = g.normal(0, 1, (64, n, 3))
    groups = np.zeros(64, np.int64)
    rest = sh[:, 1:, :].astype(np.float32)
    sh[:, 1:, :] = rest
    out = to.transform(groups, _quat32(R), [1.0], [[0, 0, 0]], sh_rest=rest)
    turned = np.concatenate([sh[:, :1, :], out["sh_rest"]], axis=1)
    Rq = to.quat_to_rot(_quat32(R)[0].astype(np.float64))            # the rotation of the float32 quaternion the judge was given
    want = torch_oracle._sh_to_rgb(deg, torch.from_numpy(sh), torch.from_numpy(d)).numpy()
    got = torch_oracle._sh_to_rgb(deg, torch.from_numpy(turned), torch.from_numpy(d @ Rq.T)).numpy()
    assert np.abs(got - want).max() < 1e-13
    if deg:
        assert np.abs(turned[:, 1:] - sh[:, 1:]).max() > 0.1         # (and something turned)


def _quat32(R):
    """a float32 (1, 4) quaternion of the rotation matrix R (numpy; the w-largest branch, |w| is never small in these tests)"""
    w = 0.5 * np.sqrt(1 + np.trace(R))
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    return q.astype(np.float32)[None, :]


def test_quarter_turn_about_z_by_hand():
    R = to.quat_to_rot(QUARTER_Z)
    assert np.abs(R - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])).max() < 1e-15
    D1, D2, D3 = to.sh_matrices(R)
    c = np.arange(1.0, 16.0)
    # band 1, the functions -y, z, -x: c'_1 = c_3, c'_2 = c_2, c'_3 = -c_1
    assert np.abs(D1 @ c[:3] - np.array([c[2], c[1], -c[0]])).max() < 1e-14
    # band 2, the functions xy, -yz, 2zz - xx - yy, -xz, xx - yy at R d = (-y, x, z): -(xy), (-xz), the same, -(-yz), -(xx - yy)
    want2 = np.array([[-1, 0, 0, 0, 0], [0, 0, 0, 1, 0], [0, 0, 1, 0, 0], [0, -1, 0, 0, 0], [0, 0, 0, 0, -1]], np.float64)
    # band 3: -y(3xx - yy), xyz, -y(4zz - xx - yy), z(..), -x(4zz - xx - yy), z(xx - yy), -x(xx - 3yy) under the same substitution
    want3 = np.zeros((7, 7))
    for m, (n, sign) in enumerate(((6, -1), (1, -1), (4, 1), (3, 1), (2, -1), (5, -1), (0, 1))):
        want3[m, n] = sign
    for D, want in ((D2, want2), (D3, want3)):
        assert np.abs(np.abs(D) - np.abs(want)).max() < 1e-14        # a signed permutation ...
        B = to.basis(_dirs(8, 5))
        a, b = (4, 9) if D is D2 else (9, 16)
        assert np.abs(to.basis(_dirs(8, 5) @ R.T)[:, a:b] - B[:, a:b] @ D.T).max() < 1e-14      # ... that maps the basis
        assert np.abs(D - want).max() < 1e-14, D.round(3)            # ... and the one worked out by hand


def test_quaternion_product_is_the_product_of_the_rotations():
    q = _quats(8, 7)
    for a, b in zip(q[:4], q[4:]):
        assert np.abs(to.quat_to_rot(to.quat_mul(a, b)) - to.quat_to_rot(a) @ to.quat_to_rot(b)).max() < 1e-14
    # the judge's rotations: q_T normalised, q as it is
    raw = (q[4:] * np.array([[0.5], [2.0], [1.0], [3.0]])).astype(np.float32)
    out = to.transform(np.zeros(4, np.int64), (q[:1] * 7).astype(np.float32), [2.0], [[1, 2, 3]], rotations=raw)
    qt = (q[:1] * 7).astype(np.float32).astype(np.float64)[0]
    assert np.abs(out["rotations"] - to.quat_mul(qt / np.linalg.norm(qt), raw.astype(np.float64))).max() < 1e-15
    assert (out["rotations_bar"] > 0).all() and (out["rotations_bar"] < 1e-6).all()


def test_covariance_of_the_transformed_scales_and_rotations():
    """R' S'^2 R'^T of the transformed (q, log s) equals the transformed cov3d = s^2 R Sigma R^T"""
    g = np.random.default_rng(8)
    P = 16
    q = _quats(P, 9).astype(np.float32)                                    # (normalised to float32 rounding)
    ls = g.uniform(-3, 0, (P, 3)).astype(np.float32)
    qd = q.astype(np.float64)
    Rg = np.stack([to.quat_to_rot(v) for v in qd])
    S2 = np.exp(2 * ls.astype(np.float64))
    Sigma = np.einsum("nab,nb,ncb->nac", Rg, S2, Rg)
    cov6 = np.stack([Sigma[:, a, b] for a, b in to.COV_PAIRS], 1).astype(np.float32)
    tq, ts = _quats(1, 11).astype(np.float32), 1.7
    out = to.transform(np.zeros(P, np.int64), tq, [ts], [[0.5, -1, 2]], rotations=q, scales=ls, cov3d=cov6)
    R2 = np.stack([to.quat_to_rot(v) for v in out["rotations"]])
    S22 = np.exp(2 * out["scales"])
    Sigma2 = np.einsum("nab,nb,ncb->nac", R2, S22, R2)
    got6 = np.stack([Sigma2[:, a, b] for a, b in to.COV_PAIRS], 1)
    assert np.abs(got6 - out["cov3d"]).max() < 2e-7 * np.abs(out["cov3d"]).max()      # (cov6 was rounded to float32)
    lin = to.transform(np.zeros(P, np.int64), tq, [ts], [[0, 0, 0]], scales=np.exp(ls), log_scales=False)
    assert np.abs(lin["scales"] - np.exp(ls).astype(np.float64) * np.float32(ts)).max() == 0


def test_members_validity_and_gather_rules():
    nan, inf = np.nan, np.inf
    quat = np.array([[1, 0, 0, 0], [nan, 0, 0, 1], [0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0],
                     [inf, 0, 0, 0]], np.float32)
    scale = np.array([2, 1, 1, inf, 0, -1, 1, 1, nan], np.float32)
    trans = np.zeros((9, 3), np.float32)
    trans[6, 1] = nan
    pivot = np.zeros((9, 3), np.float32)
    pivot[7, 2] = -inf
    st = to.table_status(quat, scale, trans, pivot)
    assert st.tolist() == [to.OK, to.BAD_QUAT, to.ZERO_QUAT, to.BAD_SCALE, to.NONPOSITIVE_SCALE, to.NONPOSITIVE_SCALE,
                           to.BAD_TRANSLATION, to.BAD_PIVOT, to.BAD_QUAT]
    assert to.table_status(quat, scale, trans).tolist()[7] == to.OK
    ids = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, -1, 9, 0])
    xyz = np.arange(36, dtype=np.float32).reshape(12, 3)
    out = to.transform(ids, quat, scale, trans, pivot, xyz=xyz)
    assert out["moved"].tolist() == [True] + [False] * 10 + [True]
    assert np.array_equal(out["xyz"][1:11], xyz[1:11]) and np.array_equal(out["xyz"][[0, 11]], 2.0 * xyz[[0, 11]])
    assert (out["xyz_bar"][1:11] == 0).all() and (out["xyz_bar"][0] > 0).all()
    rows = np.array([11, 11, -1, 12, 3, 0])
    got = to.transform(ids, quat, scale, trans, pivot, xyz=xyz, rows=rows)
    assert got["src"].tolist() == [11, 11, -1, -1, 3, 0] and got["moved"].tolist() == [True, True, False, False, False, True]
    assert np.array_equal(got["xyz"], np.stack([2 * xyz[11], 2 * xyz[11], [0, 0, 0], [0, 0, 0], xyz[3], 2 * xyz[0]]))
    # x' = s R (x - p) + p + t by hand: a quarter turn about z, about the pivot (1, 0, 0), twice the size, then one up
    one = to.transform([0], QUARTER_Z.astype(np.float32)[None], [2.0], [[0, 0, 1]], [[1, 0, 0]], xyz=np.array([[2, 0, 0]], np.float32))
    assert np.abs(one["xyz"][0] - np.array([1, 2, 1])).max() < 1e-7
    assert one["xyz_bar"][0, 1] == 0.5 * to.ulp32(one["xyz"][0, 1]) + 4 * 5 * 2.0 ** -53 * (
        np.abs(2 * to.quat_to_rot(QUARTER_Z.astype(np.float32))[1] * np.array([1.0, 0, 0])).sum() + 0 + 0)
    # compose and inverse of the judge's helpers
    a = (_quats(1, 1)[0], 1.5, np.array([1.0, 2, 3]), np.array([0.5, 0, -1]))
    b = (_quats(1, 2)[0], 0.7, np.array([-1.0, 0, 2]), np.array([2.0, 2, 2]))
    x = np.array([0.3, -0.2, 0.9])
    f = lambda tr, v: tr[1] * to.quat_to_rot(tr[0]) @ (v - tr[3]) + tr[3] + tr[2]
    q, s, t = to.compose(a, b)
    assert np.abs(s * to.quat_to_rot(q) @ x + t - f(b, f(a, x))).max() < 1e-14
    q, s, t = to.inverse(a)
    assert np.abs(s * to.quat_to_rot(q) @ f(a, x) + t - x).max() < 1e-14


def _tiny_scene(P, W, H, seed):
    g = torch.Generator().manual_seed(seed)
    from synth import make_camera
    cam = make_camera(W, H)
    U = lambda *shape, lo=0.0, hi=1.0: torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo
    z = U(P, lo=3.0, hi=8.0)
    means = torch.stack([U(P, lo=-0.6, hi=0.6) * cam["tanfovx"] * z, U(P, lo=-0.6, hi=0.6) * cam["tanfovy"] * z, z], 1)
    rot = torch.randn(P, 4, generator=g, dtype=torch.float64)
    sc = dict(means3D=means.float(), scales=torch.exp(U(P, 3, lo=-3.0, hi=-1.2)).float(), rotations=(rot / rot.norm(dim=1, keepdim=True)).float(),
              opacities=torch.sigmoid(torch.randn(P, 1, generator=g)).float(), shs=(0.3 * torch.randn(P, 16, 3, generator=g)).float(),
              semantic_feature=torch.randn(P, 1, 4, generator=g).float(), bg=torch.tensor([0.1, 0.2, 0.3]), sh_degree=3)
    sc["shs"][:, 0, :] += 0.8
    sc.update(cam)
    return sc


def _raster(sc, **over):
    kw = dict(bg=sc["bg"], means3D=sc["means3D"], means2D=None, opacities=sc["opacities"], semantic_feature=sc["semantic_feature"],
              viewmatrix=sc["viewmatrix"], projmatrix=sc["projmatrix"], campos=sc["campos"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"],
              image_height=sc["image_height"], image_width=sc["image_width"], sh_degree=3, shs=sc["shs"], scales=sc["scales"],
              rotations=sc["rotations"])
    kw.update(over)
    if kw["rotations"] is not None:                          # the model's get_rotation: the rasterizer itself does not normalise, and
        q = kw["rotations"].double()                         # |q|^2 R + (1 - |q|^2) I does not turn with R (include/f3dgs.h)
        kw["rotations"] = q / q.norm(dim=1, keepdim=True)
    with torch.no_grad():
        return torch_oracle.rasterize(**kw)


def test_transform_camera_keeps_the_image_of_the_transformed_scene():
    import transform
    P, W, H = 50, 32, 32
    sc = _tiny_scene(P, W, H, 4)
    base = _raster(sc)
    assert (base["radii"] > 0).all() and float(base["color"].sub(sc["bg"].double()[:, None, None]).abs().max()) > 0.1
    quat = _quats(1, 12)[0].astype(np.float32)
    s, t, p = np.float32(1.7), np.array([0.4, -1.0, 2.5], np.float32), np.array([0.2, 0.1, 5.0], np.float32)
    out = to.transform(np.zeros(P, np.int64), quat[None], [s], t[None], p[None], xyz=sc["means3D"].numpy(),
                       rotations=sc["rotations"].numpy(), scales=sc["scales"].numpy(), log_scales=False,
                       sh_rest=sc["shs"][:, 1:, :].numpy())
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    shs = torch.cat([sc["shs"][:, :1, :].double(), f64(out["sh_rest"])], 1)
    view, proj, center = transform.transform_camera(sc["viewmatrix"].double(), sc["projmatrix"].double(), sc["campos"].double(), quat, s, t, p)
    assert view.dtype == torch.float64
    Rv = view[:3, :3]
    assert float((Rv @ Rv.t() - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-14        # a rigid view matrix again
    assert float((torch.linalg.inv(view)[3, :3] - center).abs().max()) < 1e-13               # whose centre is the moved centre
    moved = _raster(sc, means3D=f64(out["xyz"]), rotations=f64(out["rotations"]), scales=f64(out["scales"]), shs=shs, viewmatrix=view,
                    projmatrix=proj, campos=center)
    assert np.array_equal(moved["radii"].numpy(), base["radii"].numpy())
    for key, k in (("color", 1.0), ("feature_map", 1.0), ("depth", float(s))):
        e = float((moved[key] / k - base[key]).abs().max())
        assert e <= 1e-9, (key, e)
    # the covariance route: s^2 R Sigma R^T in the place of scales and rotations
    R0 = torch_oracle._quat_to_rot(sc["rotations"].double() / sc["rotations"].double().norm(dim=1, keepdim=True))
    RS = R0 * sc["scales"].double()[:, None, :]
    Sigma = RS @ RS.transpose(1, 2)
    c6 = torch.stack([Sigma[:, a, b] for a, b in to.COV_PAIRS], 1).float()
    base6 = _raster(sc, scales=None, rotations=None, cov3D_precomp=c6)
    out6 = to.transform(np.zeros(P, np.int64), quat[None], [s], t[None], p[None], cov3d=c6.numpy())
    moved6 = _raster(sc, means3D=f64(out["xyz"]), scales=None, rotations=None, cov3D_precomp=f64(out6["cov3d"]), shs=shs, viewmatrix=view,
                     projmatrix=proj, campos=center)
    assert float((moved6["color"] - base6["color"]).abs().max()) <= 1e-9
    # float32 camera tensors come back as float32
    v32 = transform.transform_camera(sc["viewmatrix"], sc["projmatrix"], sc["campos"], quat, s, t)
    assert all(a.dtype == torch.float32 for a in v32)


# ---- the C ABI: what is refused before any device work ---------------------------------------------------------------------

def _lib():
    so = os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(so)
    vp, ci, sz, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int64
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_version.restype = ci
    lib.f3dgs_transform_gaussians_scratch_bytes.restype = sz
    lib.f3dgs_transform_gaussians_scratch_bytes.argtypes = [ci]
    lib.f3dgs_transform_gaussians.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, ci, i64, vp, vp, vp, vp, vp, i64, vp,
                                              vp, sz, vp]
    return lib


def test_c_abi_refuses_bad_arguments_without_gpu():
    lib = _lib()
    assert lib.f3dgs_version() >= 32100
    Q, S, T, PV, GR, ST, SC = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000      # never dereferenced addresses
    X, XO, R, RO, SH, SHO, ROWS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000
    INV, UNS = -1, -4
    err = lib.f3dgs_last_error
    BIG = 1 << 40

    def call(P=10, G=4, quat=Q, scale=S, trans=T, pivot=PV, groups=GR, rows=None, M=0, xyz=X, rot=None, scales=None, mode=0, cov=None, sh=None,
             n_rest=0, stride=0, xyz_out=XO, rot_out=None, scales_out=None, cov_out=None, sh_out=None, ostride=0, status=ST, scratch=SC,
             nbytes=BIG):
        return lib.f3dgs_transform_gaussians(P, G, quat, scale, trans, pivot, groups, rows, M, xyz, rot, scales, mode, cov, sh, n_rest, stride,
                                             xyz_out, rot_out, scales_out, cov_out, sh_out, ostride, status, scratch, nbytes, None)

    need = lib.f3dgs_transform_gaussians_scratch_bytes(300)
    assert need >= 300 * (18 + 83) * 8 and lib.f3dgs_transform_gaussians_scratch_bytes(65536) >= 65536 * 101 * 8
    assert call(P=-1) == INV and b"P < 0" in err()
    for G in (0, -1, 65537):
        assert call(G=G) == INV and b"1 .. 65536" in err()
    for kw in (dict(quat=None), dict(scale=None), dict(trans=None), dict(status=None), dict(groups=None)):
        assert call(**kw) == INV and b"null" in err(), kw
    assert call(P=(1 << 30) + 1) == UNS
    assert call(rows=ROWS, M=-1) == INV and b"M < 0" in err()
    for n in (-1, 1, 4, 16):
        assert call(sh=SH, sh_out=SHO, n_rest=n, stride=48, ostride=48) == INV and b"n_rest" in err()
    assert call(mode=2) == INV and b"scale_mode" in err()
    assert call(sh=SH, sh_out=SHO, n_rest=0) == INV and b"do not agree" in err()
    assert call(n_rest=15) == INV and b"do not agree" in err()
    assert call(xyz=None, xyz_out=None) == INV and b"every input" in err()
    for kw in (dict(xyz_out=None), dict(rot_out=RO), dict(rot=R), dict(sh=SH, n_rest=3, stride=9)):
        assert call(**kw) == INV and b"without its" in err(), kw
    for kw in (dict(stride=44, ostride=45), dict(stride=45, ostride=44)):
        assert call(sh=SH, sh_out=SHO, n_rest=15, **kw) == INV and b"below 3 n_rest" in err()
    # overlap: in place is the same array without src_rows, and nothing else
    assert call(sh=SH, sh_out=SH, n_rest=15, stride=48, ostride=45) == INV and b"strides" in err()
    assert call(xyz_out=X + 12) == INV and b"overlaps" in err()
    assert call(rot=R, rot_out=X + 8) == INV and b"overlaps" in err()
    assert call(rows=ROWS, M=5, xyz_out=X) == INV and b"overlaps" in err()
    assert call(rows=ROWS, M=5, xyz_out=X + 12 * 9) == INV and b"overlaps" in err()
    assert call(scratch=None) == INV and b"scratch" in err()
    assert call(nbytes=lib.f3dgs_transform_gaussians_scratch_bytes(4) - 1) == INV and b"scratch" in err()
    assert call(scratch=SC + 4) == INV and b"8-byte" in err()


def test_python_surface_refuses_without_a_device_read():
    import transform
    ids = torch.zeros(10, dtype=torch.int64)
    xyz = torch.zeros(10, 3)
    with pytest.raises(ValueError, match="HIP device"):
        transform.Transforms.identity(2, "cpu")
    with pytest.raises(ValueError, match="1 .. 65536"):
        transform.Transforms.identity(0, "cuda:0")
    with pytest.raises(ValueError, match="1 .. 65536"):
        transform.Transforms.identity(65537, "cuda:0")
    table = transform.Transforms(torch.zeros(2, 4), torch.ones(2), torch.zeros(2, 3), None)      # (a table on the CPU, built by hand)
    with pytest.raises(ValueError, match="HIP device.*int64.*10.*cpu"):
        transform.transform_gaussians(ids, table, xyz=xyz)
    with pytest.raises(ValueError, match="GroupStats"):
        transform.Transforms.about_centroid(object())
    with pytest.raises(ValueError, match=r"\(3, 3\)"):
        transform.Transforms.from_matrix(torch.zeros(2, 2))
    with pytest.raises(ValueError, match=r"\(3,\) or \(G, 3\)"):
        transform.Transforms.from_axis_angle(torch.zeros(4), 0.1)
    with pytest.raises(ValueError, match="_xyz"):
        transform.transform_model(object(), ids, table)
    assert transform.Transforms._fields == ("quat", "scale", "translation", "pivot")
    assert transform.Transformed._fields == ("xyz", "rotations", "scales", "cov3d", "sh_rest", "status")
    assert {"Transforms", "transform_gaussians", "transform_model", "transform_camera"} <= set(transform.__all__)
    assert (transform.BAD_QUAT, transform.ZERO_QUAT, transform.BAD_SCALE, transform.NONPOSITIVE_SCALE, transform.BAD_TRANSLATION,
            transform.BAD_PIVOT) == (to.BAD_QUAT, to.ZERO_QUAT, to.BAD_SCALE, to.NONPOSITIVE_SCALE, to.BAD_TRANSLATION, to.BAD_PIVOT)
