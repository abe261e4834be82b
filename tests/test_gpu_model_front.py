"""The model front end on the GPU (csrc/model_front.hip, model_front.py): the fused activations and SH pack against torch's
own chain and the fp64 oracle, the densification statistics against the torch route, `model_front.render` against the product
rasterizer and against the reference's glue, the training loop with the fused bookkeeping, and the whole iteration captured
in a graph.

Shapes: P one either side of a wave (63, 65), of a workgroup's 256 rows (257) and over several workgroups (1025), and a
single row; M = 1, 4, 9, 16 puts the seam between `features_dc` and `features_rest` at every position of the pack's 16-byte
stores and gives LDS tiles of 256, 256, 112 and 64 rows.
"""
import ctypes
import math
import os
import types

import pytest
import torch
import torch.nn.functional as F

import model_front_oracle as mo
import refutil as ru
from test_gpu_dropin import reference_render  # noqa: F401  (fixture)
from util import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PS = [1, 63, 65, 257, 1025]
MS = [1, 4, 9, 16]
M_OF_P = {1: 16, 63: 1, 65: 4, 257: 9, 1025: 16}
K_SPECIAL = 8           # the first rows of every input hold the specials
SENTINEL = -777.25


def _offset_view(t):
    """The same values in a view at a storage offset of one float (4-byte aligned, never 16)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(t.shape)
    assert (t.numel() == 0 or v.data_ptr() % 16 == 4) and v.is_contiguous()
    return v


def _raw(P, M, seed=0):
    """Raw parameters from a normal distribution, with the block of specials in the first rows (as many as P holds)."""
    g = torch.Generator().manual_seed(1000 * P + M + seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    s, q, o, dc, rest = r(P, 3), r(P, 4), r(P, 1) * 3.0, r(P, 1, 3), r(P, M - 1, 3)
    nan, inf = float("nan"), float("inf")
    s_sp = torch.tensor([[88.8, -88.8, 104.0], [-104.0, nan, 0.5], [88.8, 1.0, -1.0]])
    o_sp = torch.tensor([17.0, -17.0, 90.0, -90.0, inf, -inf])
    e = torch.tensor([0.6, 0.0, -0.8, 0.0])
    q_sp = torch.stack([torch.zeros(4), 1e-13 * e, torch.full((4,), 1e-20), torch.full((4,), 1e19),
                        torch.tensor([1e19, 0.0, 0.0, 0.0]), torch.tensor([1e-40, -3e-41, 0.0, 2e-45]), 2e-12 * e,
                        torch.tensor([5e18, -5e18, 5e18, 5e18])])
    for t, sp in ((s, s_sp), (o, o_sp.reshape(-1, 1)), (q, q_sp)):
        n = min(P, sp.shape[0], K_SPECIAL)
        t[:n] = sp[:n]
    return [t.to(DEV) for t in (s, q, o, dc, rest)]


def _torch_chain(s, q, o, dc, rest):
    """The getters of scene/gaussian_model.py:98-127 in torch's own fp32 kernels."""
    return torch.exp(s), F.normalize(q), torch.sigmoid(o), torch.cat((dc, rest), dim=1)


def _ulps(x, oracle):
    """|x - oracle| in ulps of the oracle rounded to fp32 (fp64 tensors on the CPU)."""
    r = oracle.float()
    ulp = (torch.nextafter(r.abs(), torch.full_like(r, float("inf"))) - r.abs()).double()
    return (x.double().cpu() - oracle).abs() / ulp


# ---- 1. the copies ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("P", PS)
def test_sh_pack_and_its_gradients_are_copies(P, M):
    import model_front
    _s, _q, _o, dc, rest = _raw(P, M)
    want = torch.cat((dc, rest), dim=1)
    g = torch.randn(P, M, 3, generator=torch.Generator().manual_seed(P + M)).to(DEV)
    variants = [(dc, rest, g), (_offset_view(dc), _offset_view(rest), _offset_view(g))]
    if M == 1:
        variants += [(dc, None, g), (dc, torch.empty(P, 0, 3, device=DEV), g)]
    for a, b, up in variants:
        a = a.detach().requires_grad_(True)
        b = None if b is None else b.detach().requires_grad_(True)
        _, _, _, shs = model_front.activate(None, None, None, a, b)
        assert shs.shape == (P, M, 3) and shs.data_ptr() % 16 == 0
        assert torch.equal(shs, want)
        shs.backward(up)
        assert a.grad.shape == (P, 1, 3) and torch.equal(a.grad, g[:, :1])
        if b is not None:
            assert b.grad.shape == (P, M - 1, 3) and torch.equal(b.grad, g[:, 1:])


def test_empty_model_through_the_python_surface():
    import model_front
    raw = [torch.zeros(0, *s, device=DEV, requires_grad=True) for s in ((3,), (4,), (1,), (1, 3), (15, 3))]
    outs = model_front.activate(*raw)
    assert [tuple(t.shape) for t in outs] == [(0, 3), (0, 4), (0, 1), (0, 16, 3)]
    sum(t.sum() for t in outs).backward()
    assert all(p.grad is not None and p.grad.shape == p.shape for p in raw)
    acc = torch.zeros(0, 1, device=DEV)
    model_front.densification_stats(torch.zeros(0, 3, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), acc, acc.clone(),
                                    torch.zeros(0, device=DEV))
    assert model_front.activate(None, None, None, None, None) == (None, None, None, None)


# ---- 2. activations forward -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("P", PS)
def test_activations_forward_in_ulps_of_the_oracle(P, offset):
    """Per tensor, the kernel's largest error over the plain rows is at most that of torch's own fp32 chain plus one ulp; on the
    specials the two agree on NaN, inf, exact zeros and exact ones.  (The measured maxima: profiles/model_front_bench.md.)"""
    import model_front
    raw = _raw(P, M_OF_P[P])
    if offset:
        raw = [_offset_view(t) for t in raw]
    got = model_front.activate(*raw)
    ref = _torch_chain(*raw)
    want = mo.activate_forward(*raw)
    assert got[2].shape == (P, 1) and got[1].data_ptr() % 16 == 0
    for name, k, t, o in zip(("scales", "rotations", "opacities"), got, ref, want):
        k, t = k.cpu(), t.cpu()
        plain = torch.zeros_like(o, dtype=torch.bool)
        plain[K_SPECIAL:] = True
        plain &= torch.isfinite(o)
        e_k = float(_ulps(k, o)[plain].max()) if plain.any() else 0.0
        e_t = float(_ulps(t, o)[plain].max()) if plain.any() else 0.0
        print(f"P={P} offset={offset} {name}: kernel {e_k:.3f} ulp, torch chain {e_t:.3f} ulp")
        assert e_k <= e_t + 1.0, (name, e_k, e_t)
        sp_k, sp_t = k[:K_SPECIAL], t[:K_SPECIAL]
        assert torch.equal(torch.isnan(sp_k), torch.isnan(sp_t)), name
        assert torch.equal(torch.isinf(sp_k), torch.isinf(sp_t)) and torch.equal(sp_k[torch.isinf(sp_k)], sp_t[torch.isinf(sp_t)]), name
        assert torch.equal(sp_k == 0, sp_t == 0) and torch.equal(sp_k == 1, sp_t == 1), name
    assert torch.equal(got[3], ref[3])


# ---- 3. activations backward ----------------------------------------------------------------------------------------------

def _normalised_error(x, o, e_row):
    """max |x - o| / (|o| + e_row) over the elements whose oracle value is finite; a value that is not finite there counts as
    an infinite error.  Where the oracle is not finite (an upstream times an infinite scale) the classes must agree."""
    x = x.double().cpu()
    fin = torch.isfinite(o)
    bad = fin & ~torch.isfinite(x)
    err = ((x - o).abs() / (o.abs() + e_row + 1e-300))[fin & ~bad]
    worst = float("inf") if bad.any() else (float(err.max()) if err.numel() else 0.0)
    return worst, torch.equal(torch.isnan(x[~fin]), torch.isnan(o[~fin])) and torch.equal(x[~fin][torch.isinf(x[~fin])], o[~fin][torch.isinf(o[~fin])])


@pytest.mark.parametrize("P", PS)
def test_activations_backward_against_the_oracle(P):
    """The kernel's largest normalised error is at most that of torch's fp32 autograd plus 2^-22."""
    import model_front
    M = M_OF_P[P]
    raw = [t.requires_grad_(True) for t in _raw(P, M)]
    outs = model_front.activate(*raw)
    g = torch.Generator().manual_seed(31 + P)
    ups = [torch.randn(t.shape, generator=g).to(DEV) for t in outs]
    torch.autograd.backward(outs, ups)
    got = [p.grad for p in raw]
    # torch's fp32 autograd through its own chain, same inputs and upstream gradients
    raw_t = [p.detach().clone().requires_grad_(True) for p in raw]
    torch.autograd.backward(_torch_chain(*raw_t), ups)
    ref = [p.grad for p in raw_t]
    # the fp64 oracle fed the kernel's own fp32 forward outputs
    want = mo.activate_backward(outs[0], raw[1], outs[2], *ups, P, M)
    q64 = raw[1].detach().double().cpu()
    n = torch.sqrt((q64 * q64).sum(-1, keepdim=True)).clamp_min(1e-12)
    e_rot = ups[1].double().cpu().abs().amax(dim=-1, keepdim=True) / n
    for name, k, t, o, e_row in zip(("scaling", "rotation", "opacity"), got, ref, want, (0.0, e_rot, 0.0)):
        assert k.shape == o.shape
        e_k, classes_ok = _normalised_error(k, o, e_row)
        e_t, _ = _normalised_error(t, o, e_row)
        print(f"P={P} d_{name}: kernel {e_k:.3e}, torch autograd {e_t:.3e}")
        assert classes_ok, name
        assert e_k <= e_t + 2.0 ** -22, (name, e_k, e_t)
    assert torch.equal(got[3], ups[3][:, :1]) and torch.equal(got[4], ups[3][:, 1:])


@pytest.mark.parametrize("P", [65, 1025])
def test_unused_outputs_give_exact_zeros(P):
    import model_front
    M = 16
    raw = [t.requires_grad_(True) for t in _raw(P, M)]
    scales, rotations, opacities, shs = model_front.activate(*raw)
    (rotations * 2.0).sum().backward()                  # three of the four results are never used
    assert float(raw[1].grad.abs().max()) > 0
    for i in (0, 2, 3, 4):
        assert raw[i].grad is not None and raw[i].grad.shape == raw[i].shape
        assert torch.equal(raw[i].grad, torch.zeros_like(raw[i])), i
    # a parameter that does not require a gradient gets none; a skipped group returns None
    s = raw[0].detach()
    out = model_front.activate(s, None, raw[2].detach().requires_grad_(True), None, None)
    assert out[1] is None and out[3] is None and not out[0].requires_grad and out[2].requires_grad


def _lib():
    import diff_gaussian_rasterization  # noqa: F401  (loads the HIP runtime the library links against)
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    vp = ctypes.c_void_p
    lib.f3dgs_activate_forward.argtypes = [ctypes.c_int] * 2 + [vp] * 10
    lib.f3dgs_activate_backward.argtypes = [ctypes.c_int] * 2 + [vp] * 13
    return lib


@pytest.mark.parametrize("P,M", [(65, 9), (257, 16), (1025, 4), (63, 1)])
def test_skipped_groups_write_nothing(P, M):
    """Through the C ABI on caller-owned buffers: a group whose output is NULL is skipped, and no call writes outside the rows
    it was given - every output is allocated with a guard of 64 floats behind it, filled with a sentinel."""
    lib = _lib()
    raw = _raw(P, M)
    sizes_fw = [P * 3, P * 4, P, P * M * 3]
    sizes_bw = [P * 3, P * 4, P, P * 3, P * (M - 1) * 3]
    GUARD = 64
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    ref_fw = [t.reshape(-1) for t in _torch_chain(*raw)]
    g = torch.Generator().manual_seed(9)
    ups = [torch.randn(n, generator=g).to(DEV) for n in sizes_fw]
    full_fw = None
    for mask in (0b1111, 0b0001, 0b0010, 0b0100, 0b1000, 0b0110):
        outs = [torch.full((n + GUARD,), SENTINEL, device=DEV) for n in sizes_fw]
        use = [bool(mask >> i & 1) for i in range(4)]
        ins = [raw[0] if use[0] else None, raw[1] if use[1] else None, raw[2] if use[2] else None,
               raw[3] if use[3] else None, raw[4] if use[3] else None]
        rc = lib.f3dgs_activate_forward(P, M, *[ptr(t) for t in ins], *[ptr(o) if u else None for o, u in zip(outs, use)], stream)
        assert rc == 0, lib.f3dgs_last_error()
        torch.cuda.synchronize()
        if mask == 0b1111:
            full_fw = [o[:n].clone() for o, n in zip(outs, sizes_fw)]
        for i, (o, n) in enumerate(zip(outs, sizes_fw)):
            assert torch.equal(o[n:], torch.full((GUARD,), SENTINEL, device=DEV)), (mask, i)
            if use[i]:
                assert torch.equal(torch.nan_to_num(o[:n], nan=123.0), torch.nan_to_num(full_fw[i], nan=123.0)), (mask, i)
            else:
                assert torch.equal(o[:n], torch.full((n,), SENTINEL, device=DEV)), (mask, i)
    assert torch.equal(full_fw[3], ref_fw[3])
    # backward: outputs (d_scaling, d_rotation, d_opacity, d_dc, d_rest)
    scales, opac = full_fw[0], full_fw[2]
    for mask in (0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b10000, 0b11000):
        outs = [torch.full((n + GUARD,), SENTINEL, device=DEV) for n in sizes_bw]
        use = [bool(mask >> i & 1) for i in range(5)]
        rc = lib.f3dgs_activate_backward(P, M, ptr(scales), ptr(raw[1]), ptr(opac), ptr(ups[0]), ptr(ups[1]), ptr(ups[2]), ptr(ups[3]),
                                         *[ptr(o) if u else None for o, u in zip(outs, use)], stream)
        assert rc == 0, lib.f3dgs_last_error()
        torch.cuda.synchronize()
        for i, (o, n) in enumerate(zip(outs, sizes_bw)):
            assert torch.equal(o[n:], torch.full((GUARD,), SENTINEL, device=DEV)), (mask, i)
            if not use[i]:
                assert torch.equal(o[:n], torch.full((n,), SENTINEL, device=DEV)), (mask, i)
            elif n:
                assert not bool((o[:n] == SENTINEL).any()), (mask, i)           # fully overwritten
        gsh = ups[3].view(P, M, 3)
        if use[3]:
            assert torch.equal(outs[3][:P * 3], gsh[:, :1].reshape(-1))
        if use[4]:
            assert torch.equal(outs[4][:P * (M - 1) * 3], gsh[:, 1:].reshape(-1))
    # NULL upstream gradients: every requested output is exact zeros
    outs = [torch.full((n + GUARD,), SENTINEL, device=DEV) for n in sizes_bw]
    rc = lib.f3dgs_activate_backward(P, M, None, None, None, None, None, None, None, *[ptr(o) for o in outs], stream)
    assert rc == 0, lib.f3dgs_last_error()
    torch.cuda.synchronize()
    for o, n in zip(outs, sizes_bw):
        assert torch.equal(o[:n], torch.zeros(n, device=DEV)) and torch.equal(o[n:], torch.full((GUARD,), SENTINEL, device=DEV))


# ---- 4. statistics ----------------------------------------------------------------------------------------------------------

def _torch_stats(grad, radii, acc, den, mr):
    """train_step.densification_deltas plus the masked updates of dp_train_step, on the device."""
    import train_step
    P = radii.numel()
    vsp = torch.zeros(P, 3, device=DEV, requires_grad=True)
    vsp.grad = grad
    norm, count, r = train_step.densification_deltas({"viewspace_points": vsp, "radii": radii, "visibility_filter": radii > 0}, P, DEV)
    acc, den, mr = acc.clone(), den.clone(), mr.clone()
    acc += norm
    den += count
    seen = count.squeeze(-1) > 0
    mr[seen] = torch.maximum(mr[seen], r[seen].to(mr.dtype))
    return acc, den, mr


@pytest.mark.parametrize("P", PS)
def test_densification_statistics(P):
    """denom and max_radii2D equal the torch route bit for bit, xyz_gradient_accum is within one ulp of the fp64 oracle."""
    import model_front
    g = torch.Generator().manual_seed(11 + P)
    radii = torch.randint(-3, 60, (P,), generator=g, dtype=torch.int32)
    sp = torch.tensor([0, -1, 1, 1 << 24, -(1 << 24), 2], dtype=torch.int32)
    radii[:min(P, 6)] = sp[:min(P, 6)]
    if P == 1:
        radii[0] = 1 << 24
    radii = radii.to(DEV)
    grads = [(torch.randn(P, 3, generator=g) * s).to(DEV) for s in (1e-3, 7.0)]
    acc = torch.full((P, 1), SENTINEL, device=DEV).abs()        # sentinels: rows that are not visible must keep them
    den = torch.full((P, 1), 5.0, device=DEV)
    mr = torch.full((P,), 3.5, device=DEV)
    hidden = (radii <= 0).cpu()
    worst = 0.0
    for call, grad in enumerate(grads + [None]):            # two accumulating calls, then one with a NULL gradient
        o_acc, o_den, o_mr = mo.densify_stats(grad, radii, acc, den, mr)          # fed the state the call starts from
        t_acc, t_den, t_mr = _torch_stats(grad, radii, acc, den, mr)
        before = acc.clone()
        model_front.densification_stats(grad, radii, acc, den, mr)
        assert torch.equal(den, t_den) and torch.equal(mr, t_mr), call
        assert torch.equal(den.cpu().double().reshape(-1), o_den) and torch.equal(mr.cpu().double(), o_mr), call
        e = _ulps(acc.reshape(-1), o_acc)
        worst = max(worst, float(e.max()))
        assert float(e.max()) <= 1.0, (call, float(e.max()))
        if grad is None:
            assert torch.equal(acc, before)
    print(f"P={P}: xyz_gradient_accum within {worst:.3f} ulp of the oracle")
    assert torch.equal(acc.cpu().reshape(-1)[hidden], torch.full((int(hidden.sum()),), abs(SENTINEL)))
    assert torch.equal(den.cpu().reshape(-1)[hidden], torch.full((int(hidden.sum()),), 5.0))
    assert torch.equal(mr.cpu()[hidden], torch.full((int(hidden.sum()),), 3.5))
    if P >= 4:
        assert float(mr[3]) == float(1 << 24) and float(den[3]) == 8.0
    # each accumulator may be missing
    only = torch.zeros(P, device=DEV)
    model_front.densification_stats(None, radii, None, None, only)
    assert torch.equal(only, torch.where(radii > 0, radii.float(), torch.zeros_like(only)))
    model_front.densification_stats(grads[0], radii, None, None, None)


# ---- 5. plumbing ------------------------------------------------------------------------------------------------------------

class _Model:
    """What render() and the bookkeeping read from a GaussianModel (scene/gaussian_model.py:41-127): raw parameters."""

    def __init__(self, sc):
        par = lambda x: x.to(DEV).contiguous().clone().requires_grad_(True)
        self.active_sh_degree, self.max_sh_degree = sc["sh_degree"], 3
        self._xyz = par(sc["means3D"])
        self._features_dc, self._features_rest = par(sc["shs"][:, :1]), par(sc["shs"][:, 1:])
        self._scaling, self._rotation = par(torch.log(sc["scales"])), par(sc["rotations"] * 1.7)
        op = sc["opacities"].clamp(1e-4, 1 - 1e-4)
        self._opacity = par(torch.log(op / (1 - op)).reshape(-1, 1))
        self._semantic_feature = par(sc["semantic_feature"].reshape(sc["P"], 1, -1))
        P = sc["P"]
        self.xyz_gradient_accum, self.denom = torch.zeros(P, 1, device=DEV), torch.zeros(P, 1, device=DEV)
        self.max_radii2D = torch.zeros(P, device=DEV)

    get_xyz = property(lambda s: s._xyz)
    get_semantic_feature = property(lambda s: s._semantic_feature)
    get_scaling = property(lambda s: torch.exp(s._scaling))
    get_rotation = property(lambda s: F.normalize(s._rotation))
    get_opacity = property(lambda s: torch.sigmoid(s._opacity))
    get_features = property(lambda s: torch.cat((s._features_dc, s._features_rest), dim=1))

    def params(self):
        return {n: getattr(self, n) for n in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation",
                                              "_semantic_feature")}


def _camera(sc):
    c = types.SimpleNamespace()
    c.FoVx, c.FoVy = 2 * math.atan(sc["tanfovx"]), 2 * math.atan(sc["tanfovy"])
    c.image_height, c.image_width = sc["image_height"], sc["image_width"]
    c.world_view_transform, c.full_proj_transform = sc["viewmatrix"].to(DEV), sc["projmatrix"].to(DEV)
    c.camera_center = sc["campos"].to(DEV)
    return c


PIPE = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


def _plumbing_scene():
    from synth import make_scene
    return make_scene(P=6000, C=16, width=200, height=120)


def test_render_is_the_rasterizer_on_the_activations():
    import diff_gaussian_rasterization as dgr
    import model_front
    sc = _plumbing_scene()
    m, cam, bg = _Model(sc), _camera(sc), sc["bg"].to(DEV)
    pkg = model_front.render(cam, m, PIPE, bg)
    assert set(pkg) == {"render", "viewspace_points", "visibility_filter", "radii", "feature_map", "depth"}
    with torch.no_grad():
        scales, rotations, opacity, shs = model_front.activate(m._scaling, m._rotation, m._opacity, m._features_dc, m._features_rest)
        st = dgr.GaussianRasterizationSettings(
            image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
            tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform,
            projmatrix=cam.full_proj_transform, sh_degree=m.active_sh_degree, campos=cam.camera_center, prefiltered=False,
            debug=False)
        color, feat, radii, depth = dgr.GaussianRasterizer(st)(
            means3D=m._xyz, means2D=torch.zeros_like(m._xyz), shs=shs, colors_precomp=None, semantic_feature=m._semantic_feature,
            opacities=opacity, scales=scales, rotations=rotations, cov3D_precomp=None)
    assert int((radii > 0).sum()) > 1000
    assert torch.equal(pkg["render"], color) and torch.equal(pkg["feature_map"], feat) and torch.equal(pkg["depth"], depth)
    assert torch.equal(pkg["radii"], radii) and torch.equal(pkg["visibility_filter"], radii > 0)
    vsp = pkg["viewspace_points"]
    assert vsp.is_leaf and vsp.requires_grad and vsp.grad is None
    (pkg["render"] * sc["dL_dcolor"].to(DEV)).sum().backward()
    assert vsp.grad is not None and vsp.grad.shape == (sc["P"], 3) and float(vsp.grad.abs().max()) > 0
    assert all(p.grad is not None for n, p in m.params().items() if n != "_semantic_feature")
    # install(): the reference's module gets the fused render, anything else is refused
    mod = types.ModuleType("gaussian_renderer")
    mod.render, mod.GaussianRasterizer = (lambda *a, **k: None), dgr.GaussianRasterizer
    assert model_front.install(mod) is mod and mod.render is model_front.render
    with pytest.raises(AttributeError, match="not the reference's gaussian_renderer"):
        model_front.install(types.ModuleType("something_else"))


def test_render_python_fallback_switches_and_override_color():
    """pipe.compute_cov3D_python takes the covariance from the model's getter (no scale / rotation group), override_color
    skips the SH group: the images agree with the fused route to fp32 noise and the skipped parameters get no gradient."""
    import model_front
    from util import precompute_optionals
    sc = _plumbing_scene()
    m, cam, bg = _Model(sc), _camera(sc), sc["bg"].to(DEV)
    with torch.no_grad():
        s, q = torch.exp(m._scaling).cpu(), F.normalize(m._rotation).cpu()
    cov = precompute_optionals(dict(sc, scales=s, rotations=q))["cov3D_precomp"].to(DEV)
    m.get_covariance = lambda scaling_modifier=1: cov
    base = model_front.render(cam, m, PIPE, bg)
    alt = model_front.render(cam, m, types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=False), bg)
    assert float((base["render"] - alt["render"]).detach().abs().max()) < 2e-5
    alt["render"].sum().backward()
    assert m._scaling.grad is None and m._rotation.grad is None and m._opacity.grad is not None and m._features_rest.grad is not None
    m2 = _Model(sc)
    col = torch.rand(sc["P"], 3, device=DEV)
    out = model_front.render(cam, m2, PIPE, bg, override_color=col)
    out["render"].sum().backward()
    assert m2._features_dc.grad is None and m2._features_rest.grad is None and m2._scaling.grad is not None


# ---- 6. against the reference's glue ------------------------------------------------------------------------------------

def _loop_scene():
    from synth import make_scene
    return make_scene(P=6000, C=16, width=200, height=120, seed=41, yaw_deg=7.0, scale_lo=0.005, scale_hi=0.08)


def test_render_against_the_reference_glue(reference_render):  # noqa: F811
    import model_front
    from test_gpu_train_loop import _start, _camera as loop_camera
    Model = ru.load_reference_gaussian_model()
    sc = _loop_scene()
    cam, bg = loop_camera(sc), sc["bg"].to(DEV)
    up_c, up_f = sc["dL_dcolor"].to(DEV), sc["dL_dfeature"].to(DEV)
    res = {}
    for name, render in (("reference", reference_render), ("fused", model_front.render)):
        m = _start(Model, sc)
        pkg = render(cam, m, PIPE, bg)
        ((pkg["render"] * up_c).sum() + (pkg["feature_map"] * up_f).sum()).backward()
        res[name] = (pkg, m)
    (pa, ma), (pb, mb) = res["reference"], res["fused"]
    for k in ("render", "feature_map", "depth"):
        worst = float((pa[k] - pb[k]).abs().max())
        print(f"{k}: {worst:.3e} abs")
        assert worst <= 1e-4, k
    for n in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_semantic_feature"):
        want, got = getattr(ma, n).grad, getattr(mb, n).grad
        assert want is not None and got is not None and got.shape == want.shape, n
        _, worst = ru.grad_errors(got, want)
        print(f"{n}: worst element at {worst:.3f} of 1e-3 |g| + 1e-5 max|g|")
        assert worst <= 1.0, (n, worst)
    _, worst = ru.grad_errors(pb["viewspace_points"].grad, pa["viewspace_points"].grad)
    assert worst <= 1.0, ("viewspace_points", worst)
    with torch.no_grad():
        fused = model_front.activate(mb._scaling, mb._rotation, mb._opacity, None, None)[:3]
        same = torch.ones(sc["P"], dtype=torch.bool, device=DEV)
        for a, b in zip(fused, (ma.get_scaling, ma.get_rotation, ma.get_opacity)):
            same &= (a == b).reshape(sc["P"], -1).all(dim=1)
    ra, rb = pa["radii"], pb["radii"]
    print(f"activations bit-equal on {int(same.sum())} of {sc['P']} Gaussians; radii differ on {int((ra != rb).sum())}")
    assert torch.equal(ra[same], rb[same])
    assert int((ra - rb).abs().max()) <= 1


# ---- 7. the loop ------------------------------------------------------------------------------------------------------------

def test_training_loop_with_the_fused_front_end_tracks_the_reference_render(reference_render):  # noqa: F811
    """Configuration B of tests/test_gpu_train_loop.py (fused feature loss, dp_train_step, FusedAdam, densify), once with the
    reference's render and once with model_front.render and fused_stats=True; that test's bars."""
    import densify
    import model_front
    import train_step
    from feature_loss import fused_feature_l1
    from fused_adam import FusedAdam
    from test_gpu_train_loop import _Opt, _camera as loop_camera, _loss_utils, _start
    Model = ru.load_reference_gaussian_model()
    lu = _loss_utils()
    sc = _loop_scene()
    cam, bg = loop_camera(sc), sc["bg"].to(DEV)
    extent = 5.0
    g = torch.Generator().manual_seed(7)
    teacher = dict(sc)
    teacher["shs"] = sc["shs"] + 0.15 * torch.randn(sc["shs"].shape, generator=g)
    teacher["semantic_feature"] = sc["semantic_feature"] + 0.3 * torch.randn(sc["semantic_feature"].shape, generator=g)
    teacher["means3D"] = sc["means3D"] + 0.01 * torch.randn(sc["means3D"].shape, generator=g)
    with torch.no_grad():
        t = reference_render(cam, _start(Model, teacher), PIPE, bg)
        cam.original_image = t["render"].clone()
        cam.semantic_feature = F.interpolate(t["feature_map"].unsqueeze(0), size=(60, 100), mode="bilinear",
                                             align_corners=True).squeeze(0).clone()

    def loss_product(pkg, c):
        image = pkg["render"]
        Ll1 = lu.l1_loss(image, c.original_image)
        return ((1.0 - _Opt.lambda_dssim) * Ll1 + _Opt.lambda_dssim * (1.0 - lu.ssim(image, c.original_image))
                + fused_feature_l1(pkg["feature_map"], c.semantic_feature, None, None, lowres_grad=True))

    ITER, DENSIFY = 14, (6, 12)
    runs = {}
    for name, render, fused in (("reference render", reference_render, False), ("fused front end", model_front.render, True)):
        b = _start(Model, sc, FusedAdam)
        losses, points = [], []
        for it in range(1, ITER + 1):
            res = train_step.dp_train_step(render, loss_product, b, [cam], PIPE, bg, fused_stats=fused)
            with torch.no_grad():
                if it in DENSIFY:
                    torch.manual_seed(100 + it)
                    densify.densify_and_prune(b, _Opt.densify_grad_threshold, 0.005, extent, 20 if it > DENSIFY[0] else None)
                b.optimizer.step()
                b.optimizer.zero_grad(set_to_none=True)
            losses.append(float(res.loss)); points.append(b.get_xyz.shape[0])
        runs[name] = (losses, points)
    (la, na), (lb, nb) = runs["reference render"], runs["fused front end"]
    print("loss A", [round(x, 6) for x in la]); print("loss B", [round(x, 6) for x in lb]); print("points", na, nb)
    assert all(math.isfinite(x) for x in la + lb)
    k = DENSIFY[0] - 1
    assert la[k - 1] < la[0] and lb[k - 1] < lb[0], (la, lb)
    for x, y in zip(la, lb):
        assert abs(x - y) <= 0.03 * abs(x), (la, lb)
    assert na[-1] != sc["P"], "the densification thresholds of this test no longer select anything"
    for x, y in zip(na, nb):
        assert abs(x - y) <= max(2, 0.01 * x), (na, nb)


# ---- 8. capture -------------------------------------------------------------------------------------------------------------

def test_the_whole_iteration_is_captured_with_its_bookkeeping(option):
    """render, the two fused losses, backward and the statistics in one graph.  With the torch route for the statistics
    (train_step.densification_deltas: boolean-mask indexing reads the host) the same capture raises."""
    import model_front
    import train_step
    from feature_loss import fused_feature_l1
    from graph_step import CapturedStep
    from image_loss import fused_l1_dssim
    option("bwd_bf16", 1)           # one contraction of the blend backward, eager and captured
    sc = _plumbing_scene()
    m, cam, bg = _Model(sc), _camera(sc), sc["bg"].to(DEV)
    g = torch.Generator().manual_seed(2)
    gt_image = torch.rand(3, cam.image_height, cam.image_width, generator=g).to(DEV)
    gt_feature = torch.randn(sc["C"], 60, 100, generator=g).to(DEV)
    P = sc["P"]

    def iteration(stats):
        for p in m.params().values():
            p.grad = None
        pkg = model_front.render(cam, m, PIPE, bg)
        loss = fused_l1_dssim(pkg["render"], gt_image, 0.2) + fused_feature_l1(pkg["feature_map"], gt_feature, None, None)
        loss.backward()
        stats(pkg)
        return pkg["radii"]

    def reset():
        m.xyz_gradient_accum.zero_(); m.denom.zero_(); m.max_radii2D.zero_()

    fused = lambda: iteration(lambda pkg: model_front.add_densification_stats(m, pkg))
    radii = None
    for _ in range(3):
        radii = fused()
    torch.cuda.synchronize()
    visible = int((radii > 0).sum())
    want_acc, want_den, want_mr = m.xyz_gradient_accum.clone(), m.denom.clone(), m.max_radii2D.clone()
    assert visible > 1000 and float(want_den.sum()) == 3.0 * visible
    assert torch.equal(want_mr, torch.where(radii > 0, radii.float(), torch.zeros_like(want_mr)))

    step = CapturedStep(fused).capture()
    reset()                                     # the warm-up calls of the capture counted too
    for _ in range(3):
        step.replay()
    assert step.check()
    torch.cuda.synchronize()
    assert float(m.denom.sum()) == 3.0 * visible and torch.equal(m.denom, want_den)
    assert torch.equal(m.max_radii2D, want_mr)
    _, worst = ru.grad_errors(m.xyz_gradient_accum, want_acc)
    print(f"xyz_gradient_accum after three replays: worst element at {worst:.3f} of 1e-3 |g| + 1e-5 max|g| of three eager steps")
    assert worst <= 1.0

    def torch_route(pkg):
        with torch.no_grad():
            norm, count, r = train_step.densification_deltas(pkg, P, DEV)
            m.xyz_gradient_accum += norm
            m.denom += count
    with pytest.raises(Exception):
        CapturedStep(lambda: iteration(torch_route)).capture()
    torch.cuda.set_stream(torch.cuda.default_stream())          # (a capture that ends in an error leaves its side stream current)
    torch.cuda.synchronize()
    # the process is whole afterwards: an eager iteration still runs and counts
    reset()
    fused()
    torch.cuda.synchronize()
    assert float(m.denom.sum()) == float(visible)
