"""f-4 (optimizer): the HIP Adam kernels against the fp64 oracle of tests/adam_oracle.py, element by element.

Every entry point is driven: the per-tensor kernel (f3dgs_adam_step), its row-masked variant (f3dgs_adam_step_rows) and the
one-launch table (f3dgs_adam_step_multi, with and without the mask), through FusedAdam and through the binding.  The bar of a
single step is the decomposed one of the oracle (A, B, C ulp32 on m', v' and the update); layouts, masks and the table are
held to BIT identity with the plain aligned per-tensor step, which the single-step tests pin to the oracle."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import adam_oracle as ao

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B1, B2, EPS = 0.9, 0.999, 1e-15
PATHS = ("tensor", "rows", "multi", "multi_rows")
CANARY = -123456.7890625


def _C():
    from diff_gaussian_rasterization import _C as c
    return c


def _shapes(P, C):
    """The reference's seven per-Gaussian tensors (scene/gaussian_model.py:163-178)."""
    return [("xyz", (P, 3)), ("f_dc", (P, 1, 3)), ("f_rest", (P, 15, 3)), ("opacity", (P, 1)), ("scaling", (P, 3)),
            ("rotation", (P, 4)), ("semantic_feature", (P, 1, C))]


def _family(shape, seed, band=(-30.0, 2.0)):
    n = int(np.prod(shape))
    return [torch.from_numpy(a).reshape(shape).to(DEV) for a in ao.family(n, band, seed)]


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _fused(path, tensors, lrs, ts, betas=(B1, B2), eps=EPS):
    """FusedAdam over `tensors` = [(p, g, m, v)], one group each, state set to step t - 1, stepped ONCE along `path`.
    Returns [(p', m', v')]."""
    from fused_adam import FusedAdam
    params = [torch.nn.Parameter(p.clone()) for p, _, _, _ in tensors]
    opt = FusedAdam([{"params": [q], "lr": lr} for q, lr in zip(params, lrs)], lr=0.0, betas=betas, eps=eps,
                    multi_tensor=path.startswith("multi"))
    for q, (_, g, m, v), t in zip(params, tensors, ts):
        q.grad = g.clone()
        opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    vis = torch.ones(params[0].shape[0], dtype=torch.bool, device=DEV) if path.endswith("rows") else None
    opt.step(visibility=vis)
    torch.cuda.synchronize()
    assert [int(opt.state[q]["step"]) for q in params] == list(ts)
    return [(q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]) for q in params]


# ---- single step, all regimes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("t", ao.T_STEPS)
@pytest.mark.parametrize("P,C", [(4097, 1), (4098, 3), (4099, 5), (4100, 32), (3001, 128)])
def test_single_step_against_fp64(path, t, P, C, record_property):
    """Scales log-uniform over 1e-30 ... 1e2 in every tensor (the eps = 1e-15 regime and the ordinary one side by side),
    a fifth of the gradients 0, a seventh of the elements never stepped; P runs through every 3P % 4 and P % 4."""
    shapes = _shapes(P, C)
    tensors = [_family(s, seed=100 * C + i) for i, (_, s) in enumerate(shapes)]
    lrs = [ao.LRS[(i + C) % 3] for i in range(len(shapes))]
    got = _fused(path, tensors, lrs, [t] * len(shapes))
    worst = {"m": 0.0, "v": 0.0, "d": 0.0}
    for (name, _), (p, g, m, v), (p2, m2, v2), lr in zip(shapes, tensors, got, lrs):
        err = ao.step_errors(p, g, m, v, p2, m2, v2, lr, B1, B2, EPS, t)
        print(f"{path} t={t} P={P} C={C} {name} lr={lr}: {err}")
        assert ao.step_ok(err), (name, lr, err)
        worst = {k: max(worst[k], err[k]) for k in worst}
    for k, x in worst.items():
        record_property(f"worst_{k}", x)


# ---- layout -------------------------------------------------------------------------------------------------------------
def _guarded(x, off=0):
    """A copy of 1-d `x` as a view starting 4 + off floats into a canary-filled buffer (off = 0: 16-byte aligned)."""
    buf = torch.full((x.numel() + 12,), CANARY, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[4 + off: 4 + off + x.numel()]
    view.copy_(x)
    return buf, view


def _canaries_intact(buf, off, n):
    want = torch.full((1,), CANARY, device=DEV).view(torch.int32)
    b = buf.view(torch.int32)
    return bool((b[:4 + off] == want).all()) and bool((b[4 + off + n:] == want).all())


def _raw_step(path, views, lr, t, mask=None, companion=None):
    """One step of the binding on 1-d views (p, g, m, v), in place.  `multi`: the table holds a companion tensor too."""
    p, g, m, v = views
    c = _C()
    if path in ("tensor", "rows"):
        c.adam_step(p, g, m, v, lr, B1, B2, EPS, t, mask)
    else:
        q = companion
        c.adam_step_multi([q[0], p], [q[1], g], [q[2], m], [q[3], v], [1e-3, lr], B1, B2, EPS, [3, t], mask)
    torch.cuda.synchronize()


def _layout_case(path, n, offs, t=7, lr=1.6e-4, seed=0):
    """Steps n elements placed at offsets `offs` (floats, per p / g / m / v) inside guarded buffers; returns (p', m', v')
    clones after asserting that nothing outside the n elements changed (gradient included)."""
    data = _family((n,), seed=seed, band=(-6.0, 0.0))
    guarded = [_guarded(x, o) for x, o in zip(data, offs)]
    views = [gv[1] for gv in guarded]
    for vw, o in zip(views, offs):
        assert n == 0 or vw.data_ptr() % 16 == 4 * o
    mask = torch.ones(n, dtype=torch.bool, device=DEV) if path.endswith("rows") else None
    companion = [x.clone() for x in _family((n,), seed=99, band=(-6.0, 0.0))] if path.startswith("multi") else None
    _raw_step(path, views, lr, t, mask, companion)
    for (buf, _), o, name in zip(guarded, offs, "pgmv"):
        assert _canaries_intact(buf, o, n), (path, n, offs, name)
    assert _same_bits(views[1], data[1]), "the gradient was written"
    return data, [views[0].clone(), views[2].clone(), views[3].clone()]


@pytest.mark.parametrize("path", PATHS)
def test_every_length_keeps_inside_its_n_elements_and_matches_fp64(path):
    ns = [0, 1, 2, 3, 4, 5, 1023, 1024, 1025] + [4 * 256 * k + s for k in (1, 2, 3) for s in (-1, 0, 1)]
    for n in ns:
        data, got = _layout_case(path, n, (0, 0, 0, 0), seed=n)
        if n:
            ao.check_step(*data, *got, 1.6e-4, B1, B2, EPS, 7, what=f"{path} n={n}")


@pytest.mark.parametrize("path", PATHS)
def test_offset_views_are_bit_identical_to_the_aligned_run(path):
    """densify.py hands out views of pool buffers: each of p, g, m, v in turn (and all four) starting 1, 2 or 3 floats off a
    16-byte boundary takes the scalar path and must give the bits of the float4 path.  Only `tensor` and `multi` reach
    that float4 / scalar choice; the masked branch (`rows`, `multi_rows`) is scalar at every alignment, and is held here
    to the same bits and canaries, not to an alignment decision."""
    for n in (5, 1024, 2049, 3071):
        _, want = _layout_case(path, n, (0, 0, 0, 0), seed=n)
        for off in (1, 2, 3):
            for offs in [tuple(off if k == j else 0 for k in range(4)) for j in range(4)] + [(off,) * 4, (1, 2, 3, off)]:
                _, got = _layout_case(path, n, offs, seed=n)
                for a, b, name in zip(got, want, ("p", "m", "v")):
                    assert _same_bits(a, b), (path, n, offs, name)


@pytest.mark.parametrize("path", PATHS)
def test_non_contiguous_gradients_step_like_their_contiguous_copy(path):
    P, C = 1027, 5
    tensors = [_family((P, C), seed=1, band=(-6.0, 0.0)), _family((P, C), seed=2, band=(-6.0, 0.0)),
               _family((P, 1, C), seed=3, band=(-6.0, 0.0))]
    gt = _family((C, P), seed=4, band=(-6.0, 0.0))[1].t()                 # transposed
    ge = _family((P, 1), seed=5, band=(-6.0, 0.0))[1].expand(P, C)        # expanded: stride 0
    gs = _family((P, 2, C), seed=6, band=(-6.0, 0.0))[1][:, 1:2, :]       # a slice: row stride 2C
    assert not gt.is_contiguous() and not ge.is_contiguous() and not gs.is_contiguous()
    odd = [(t[0], g, t[2], t[3]) for t, g in zip(tensors, (gt, ge, gs))]
    flat = [(t[0], g.contiguous(), t[2], t[3]) for t, g in zip(tensors, (gt, ge, gs))]
    a = _fused(path, odd, [1e-3] * 3, [5] * 3)
    b = _fused(path, flat, [1e-3] * 3, [5] * 3)
    for i, (x, y) in enumerate(zip(a, b)):
        assert all(_same_bits(u, w) for u, w in zip(x, y)), (path, i)
    for (p, g, m, v), (p2, m2, v2) in zip(flat, a):
        ao.check_step(p, g, m, v, p2, m2, v2, 1e-3, B1, B2, EPS, 5, what=path)


# ---- mask ---------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 3, 4, 5, 45, 48, 128)


def _masks(P):
    single = torch.zeros(P, dtype=torch.bool)
    single[P // 2] = True
    return {"zero": torch.zeros(P, dtype=torch.bool), "one": torch.ones(P, dtype=torch.bool), "single": single,
            "alternating": torch.arange(P) % 2 == 1, "last_row": torch.arange(P) == P - 1}


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("dtype", ["bool", "uint8", "int32", "int32_radii"])
def test_masked_rows_step_densely_and_hidden_rows_keep_their_bits(multi, dtype):
    """Rows of 1 ... 128 floats straddle a float4 group in every phase.  `int32_radii`: a radius tensor handed in as it is -
    any non-zero value means visible, also 256 and 65536 whose low byte is 0."""
    P, c = 1027, _C()
    tensors = [[x.clone() for x in _family((P, w), seed=w, band=(-6.0, 0.0))] for w in WIDTHS]
    dense = [[x.clone() for x in t] for t in tensors]
    for p, g, m, v in dense:
        c.adam_step(p, g, m, v, 1e-3, B1, B2, EPS, 4, None)
    for kind, mk in _masks(P).items():
        if dtype == "int32_radii":
            mask = torch.where(mk, torch.tensor([256, 65536, 7, -256])[torch.arange(P) % 4], 0).to(torch.int32).to(DEV)
        else:
            mask = mk.to(getattr(torch, dtype)).to(DEV)
        vis = mk.to(DEV)
        got = [[x.clone() for x in t] for t in tensors]
        if multi:
            c.adam_step_multi(*[[t[k] for t in got] for k in range(4)], [1e-3] * len(got), B1, B2, EPS, [4] * len(got), mask)
        else:
            for p, g, m, v in got:
                c.adam_step(p, g, m, v, 1e-3, B1, B2, EPS, 4, mask)
        torch.cuda.synchronize()
        for w, before, want, now in zip(WIDTHS, tensors, dense, got):
            for k, name in ((0, "p"), (2, "m"), (3, "v")):
                assert _same_bits(now[k][vis], want[k][vis]), (kind, w, name, "visible rows differ from the dense step")
                assert _same_bits(now[k][~vis], before[k][~vis]), (kind, w, name, "hidden rows changed")
            assert _same_bits(now[1], before[1])


@pytest.mark.parametrize("multi_tensor", [False, True])
def test_a_tensor_with_another_row_count_is_stepped_densely(multi_tensor):
    """FusedAdam with a mask of P rows: a tensor of P + 1 rows, one of 2P elements (a multiple of P, but not P rows) and a
    scalar are not per-Gaussian data and take the dense step; the (P, 3) tensors beside them are masked."""
    from fused_adam import FusedAdam
    P = 515
    shapes = [(P, 3), (P + 1, 3), (2 * P,), (), (P, 4)]
    data = [_family(s, seed=i, band=(-6.0, 0.0)) for i, s in enumerate(shapes)]
    vis = (torch.arange(P) % 3 == 0).to(DEV)
    params = [torch.nn.Parameter(d[0].clone()) for d in data]
    opt = FusedAdam([{"params": [q], "lr": 1e-3} for q in params], lr=0.0, eps=EPS, multi_tensor=multi_tensor)
    for q, d in zip(params, data):
        q.grad = d[1].clone()
        opt.state[q] = {"step": torch.tensor(6.0), "exp_avg": d[2].clone(), "exp_avg_sq": d[3].clone()}
    opt.step(visibility=vis)
    for q, d, s in zip(params, data, shapes):
        want = [x.clone() for x in d]
        _C().adam_step(*want, 1e-3, B1, B2, EPS, 7, None)
        got = (q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"])
        if s in ((P, 3), (P, 4)):
            for a, w, b in zip(got, (want[0], want[2], want[3]), (d[0], d[2], d[3])):
                assert _same_bits(a[vis], w[vis]) and _same_bits(a[~vis], b[~vis]), s
        else:
            for a, w in zip(got, (want[0], want[2], want[3])):
                assert _same_bits(a, w), s


@pytest.mark.parametrize("multi_tensor", [False, True])
@pytest.mark.parametrize("dtype", ["bool", "uint8", "int32_radii"])
def test_fused_adam_routes_a_partial_mask_of_any_dtype(multi_tensor, dtype):
    """The same through FusedAdam.step(visibility=...) over the reference's seven tensors: `int32_radii` is the
    rasterizer's radii handed in as they are (256 and 65536 are visible)."""
    from fused_adam import FusedAdam
    P = 1027
    shapes = [s for _, s in _shapes(P, 5)]
    data = [_family(s, seed=20 + i, band=(-6.0, 0.0)) for i, s in enumerate(shapes)]
    mk = torch.arange(P) % 3 != 1
    if dtype == "int32_radii":
        vis = torch.where(mk, torch.tensor([256, 65536, 7, 512])[torch.arange(P) % 4], 0).to(torch.int32).to(DEV)
    else:
        vis = mk.to(getattr(torch, dtype)).to(DEV)
    mk = mk.to(DEV)
    params = [torch.nn.Parameter(d[0].clone()) for d in data]
    opt = FusedAdam([{"params": [q], "lr": 1e-3} for q in params], lr=0.0, eps=EPS, multi_tensor=multi_tensor)
    for q, d in zip(params, data):
        q.grad = d[1].clone()
        opt.state[q] = {"step": torch.tensor(3.0), "exp_avg": d[2].clone(), "exp_avg_sq": d[3].clone()}
    opt.step(visibility=vis)
    for q, d in zip(params, data):
        want = [x.clone() for x in d]
        _C().adam_step(*want, 1e-3, B1, B2, EPS, 4, None)
        got = (q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"])
        for a, w, b in zip(got, (want[0], want[2], want[3]), (d[0], d[2], d[3])):
            assert _same_bits(a[mk], w[mk]) and _same_bits(a[~mk], b[~mk]), tuple(q.shape)


# ---- the multi-tensor table -----------------------------------------------------------------------------------------------
class _Spy:
    def __init__(self, c):
        self._c, self.calls = c, []

    def adam_step(self, *a):
        self.calls.append(("adam_step", 1))
        return self._c.adam_step(*a)

    def adam_step_multi(self, ps, *a):
        self.calls.append(("adam_step_multi", len(ps)))
        return self._c.adam_step_multi(ps, *a)


@pytest.mark.parametrize("count", [16, 17])
def test_table_of_16_and_the_17th_beside_it(count, monkeypatch):
    """Sixteen tensors fill the table (F3DGS_ADAM_MAX_TENSORS), a 17th takes the per-tensor path; an empty tensor sits in
    the middle; every tensor has its own step count and learning rate.  Each must come out with the bits of stepping it
    alone, and inside the fp64 bar at ITS step and rate."""
    import fused_adam
    spy = _Spy(_C())
    monkeypatch.setattr(fused_adam, "_C", spy)
    sizes = [(1 + 37 * i, 1 + i % 5) for i in range(count)]
    sizes[7] = (0, 3)
    data = [_family(s, seed=i, band=(-8.0, 1.0)) for i, s in enumerate(sizes)]
    ts = [1 + (i * 211) % 1999 for i in range(count)]
    lrs = [1.6e-6 * 2.0 ** i for i in range(count)]
    got = _fused("multi", data, lrs, ts)
    assert spy.calls == [("adam_step_multi", 16)] + [("adam_step", 1)] * (count - 16)
    for i, (d, g3) in enumerate(zip(data, got)):
        alone = [x.clone() for x in d]
        _C().adam_step(*alone, lrs[i], B1, B2, EPS, ts[i], None)
        for a, w in zip(g3, (alone[0], alone[2], alone[3])):
            assert _same_bits(a, w), (i, sizes[i])
        if d[0].numel():
            ao.check_step(*d, *g3, lrs[i], B1, B2, EPS, ts[i], what=f"tensor {i}")


def test_other_betas_a_missing_gradient_and_the_rest_in_one_optimizer(monkeypatch):
    import fused_adam
    spy = _Spy(_C())
    monkeypatch.setattr(fused_adam, "_C", spy)
    data = [_family((257, 3), seed=i, band=(-8.0, 1.0)) for i in range(5)]
    params = [torch.nn.Parameter(d[0].clone()) for d in data]
    groups = [{"params": [q], "lr": 1e-3} for q in params]
    groups[1].update(betas=(0.8, 0.99), eps=1e-8)
    opt = fused_adam.FusedAdam(groups, lr=0.0, betas=(B1, B2), eps=EPS)
    for i, (q, d) in enumerate(zip(params, data)):
        if i != 3:
            q.grad = d[1].clone()
            opt.state[q] = {"step": torch.tensor(float(10 * i)), "exp_avg": d[2].clone(), "exp_avg_sq": d[3].clone()}
    opt.step()
    torch.cuda.synchronize()
    assert sorted(spy.calls) == [("adam_step", 1), ("adam_step_multi", 3)]
    assert _same_bits(params[3], data[3][0]) and len(opt.state[params[3]]) == 0          # no gradient: untouched, no state
    for i, (q, d) in enumerate(zip(params, data)):
        if i == 3:
            continue
        b1, b2, eps = (0.8, 0.99, 1e-8) if i == 1 else (B1, B2, EPS)
        ao.check_step(*d, q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"], 1e-3, b1, b2, eps, 10 * i + 1,
                      what=f"group {i}")
    # the wrong group's constants would not pass: the bar tells the two settings apart
    q = params[1]
    assert not ao.step_ok(ao.step_errors(*data[1], q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"], 1e-3,
                                         B1, B2, EPS, 11))


class _AdamTensor(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("n", ctypes.c_size_t), ("lr", ctypes.c_double), ("step", ctypes.c_int)]


def test_c_abi_argument_errors():
    """include/f3dgs.h: the documented argument errors are error RETURNS (negative status, a message, nothing launched)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    vp, sz, dbl = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double
    lib.f3dgs_adam_step.argtypes = [sz, vp, vp, vp, vp, dbl, dbl, dbl, dbl, ctypes.c_int, vp]
    lib.f3dgs_adam_step_rows.argtypes = [sz, sz, vp, vp, vp, vp, vp, dbl, dbl, dbl, dbl, ctypes.c_int, vp]
    lib.f3dgs_adam_step_multi.argtypes = [ctypes.c_int, ctypes.POINTER(_AdamTensor), dbl, dbl, dbl, vp, sz, vp]
    n = 64
    data = _family((n,), seed=1, band=(-6.0, 0.0))
    keep = [x.clone() for x in data]
    ptr = [x.data_ptr() for x in data]
    mask = torch.ones(n, dtype=torch.uint8, device=DEV)
    hp = (B1, B2, EPS)
    assert lib.f3dgs_adam_step(n, *ptr, 1e-3, *hp, 0, None) < 0 and b"step" in lib.f3dgs_last_error()
    assert lib.f3dgs_adam_step(n, *ptr, 1e-3, *hp, -3, None) < 0
    for k in range(4):
        bad = list(ptr)
        bad[k] = None
        assert lib.f3dgs_adam_step(n, *bad, 1e-3, *hp, 1, None) < 0 and b"null" in lib.f3dgs_last_error()
        assert lib.f3dgs_adam_step(0, *bad, 1e-3, *hp, 1, None) == 0          # n = 0 touches nothing: no pointer needed
    assert lib.f3dgs_adam_step_rows(n, 0, mask.data_ptr(), *ptr, 1e-3, *hp, 1, None) < 0
    assert lib.f3dgs_adam_step_rows(n, 5, mask.data_ptr(), *ptr, 1e-3, *hp, 1, None) < 0      # 64 is not rows of 5
    tab = (_AdamTensor * 17)(*[_AdamTensor(*ptr, n, 1e-3, 1) for _ in range(17)])
    assert lib.f3dgs_adam_step_multi(17, tab, *hp, None, 0, None) < 0 and b"tensors" in lib.f3dgs_last_error()
    assert lib.f3dgs_adam_step_multi(-1, tab, *hp, None, 0, None) < 0
    assert lib.f3dgs_adam_step_multi(1, None, *hp, None, 0, None) < 0
    assert lib.f3dgs_adam_step_multi(1, tab, *hp, mask.data_ptr(), 0, None) < 0 and b"row" in lib.f3dgs_last_error()
    tab[1].step = 0
    assert lib.f3dgs_adam_step_multi(2, tab, *hp, None, 0, None) < 0 and b"step" in lib.f3dgs_last_error()
    tab[1].step, tab[1].exp_avg = 1, None
    assert lib.f3dgs_adam_step_multi(2, tab, *hp, None, 0, None) < 0 and b"null" in lib.f3dgs_last_error()
    assert lib.f3dgs_adam_step_multi(0, None, *hp, None, 0, None) == 0           # an empty table is no error
    torch.cuda.synchronize()
    for a, b in zip(data, keep):
        assert _same_bits(a, b), "a rejected call wrote to a tensor"


# ---- non-finite gradients ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("t", [1, 7, 1000])
def test_non_finite_gradients_stay_in_their_element(path, t):
    """NaN, +Inf and -Inf in 3 % of the gradient elements (so most float4 groups that hold one also hold finite lanes): a
    finite-gradient element passes the fp64 bar whatever its neighbours hold; a non-finite one does what
    torch.optim.Adam(foreach=False) does to it on the same device."""
    shapes = [(4099, 3), (4099, 1), (4099, 4), (1027, 45)]
    tensors = [_family(s, seed=40 + i, band=(-8.0, 1.0)) for i, s in enumerate(shapes)]
    r = np.random.default_rng(5)
    for p, g, m, v in tensors:
        u = torch.from_numpy(r.random(g.numel())).reshape(g.shape).to(DEV)
        g[u < 0.01] = float("nan")
        g[(u >= 0.01) & (u < 0.02)] = float("inf")
        g[(u >= 0.02) & (u < 0.03)] = float("-inf")
    lrs = [ao.LRS[i % 3] for i in range(len(shapes))]
    got = _fused(path, tensors, lrs, [t] * len(shapes))
    for (p, g, m, v), (p2, m2, v2), lr in zip(tensors, got, lrs):
        finite = torch.isfinite(g)
        assert 0.9 < float(finite.float().mean()) < 0.99
        ao.check_step(p, torch.where(finite, g, 0.0), m, v, p2, m2, v2, lr, B1, B2, EPS, t, where=finite, what=path)
        q = torch.nn.Parameter(p.clone())
        q.grad = g.clone()
        ref = torch.optim.Adam([q], lr=lr, betas=(B1, B2), eps=EPS, foreach=False)
        ref.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        ref.step()
        for name, a, b in (("p", p2, q.detach()), ("m", m2, ref.state[q]["exp_avg"]), ("v", v2, ref.state[q]["exp_avg_sq"])):
            a, b = a[~finite].cpu().numpy(), b[~finite].cpu().numpy()
            assert np.array_equal(np.isnan(a), np.isnan(b)), (path, name, "NaN-ness differs from torch")
            inf = np.isinf(b)
            assert np.array_equal(np.isinf(a), inf) and np.array_equal(a[inf], b[inf]), (path, name)
            # NaN -> (NaN, NaN, NaN), +-Inf -> (+-Inf, Inf, NaN): torch leaves nothing finite here, so nothing is left
            # for a tolerance to compare; a finite result of either side is a failure of the two asserts above
            assert not np.isfinite(b).any() and not np.isfinite(a).any(), (path, name)


# ---- drift ------------------------------------------------------------------------------------------------------------------
def _xyz_lr(it, steps, lr0=1.6e-4, lr1=1.6e-6):
    """The reference's exponential schedule of the position rate (update_learning_rate -> get_expon_lr_func, no delay),
    compressed onto `steps` steps."""
    u = min(max(it / steps, 0.0), 1.0)
    return math.exp(math.log(lr0) * (1.0 - u) + math.log(lr1) * u)


def _rel_err(x32, x64):
    x64 = x64.double()
    return float(((x32.double() - x64).abs() / (x64.abs() + 1e-3 * x64.abs().max())).max())


def test_drift_over_3000_steps_is_torchs(record_property):
    """The reference's seven groups for 3000 steps from identical inputs, three times: FusedAdam, torch.optim.Adam in fp32
    on the same device, and the fp64 Trajectory.  Both fp32 runs round ONE recurrence, so their distance from the fp64 state
    is a random walk of one scale: E_product <= 2 E_torch + 1e-6 per tensor for p, m and v, with
    E = max |x32 - x64| / (|x64| + 1e-3 max |x64|).  (The factor 2: another operation order, fma against lerp / addcdiv;
    the floor: tensors where torch happens to be exact.)"""
    from fused_adam import FusedAdam
    P, C, steps = 20000, 32, 3000
    specs = [("xyz", (3,), 1.6e-4), ("f_dc", (1, 3), 2.5e-3), ("f_rest", (15, 3), 1.25e-4), ("opacity", (1,), 0.05),
             ("scaling", (3,), 5e-3), ("rotation", (4,), 1e-3), ("semantic_feature", (1, C), 1e-3)]
    gen = torch.Generator(device=DEV).manual_seed(17)
    init = [torch.randn((P,) + s, generator=gen, device=DEV) for _, s, _ in specs]
    mk = lambda: [{"params": [torch.nn.Parameter(x.clone())], "lr": lr, "name": n} for x, (n, _, lr) in zip(init, specs)]
    prod, ref = FusedAdam(mk(), lr=0.0, eps=EPS), torch.optim.Adam(mk(), lr=0.0, eps=EPS)
    traj = [ao.Trajectory(x, B1, B2, EPS) for x in init]
    row_scale = 10.0 ** (torch.rand(P, generator=gen, device=DEV) * 6.0 - 7.0)        # six decades, per row
    for it in range(1, steps + 1):
        lr_xyz = _xyz_lr(it, steps)
        seen = (torch.rand(row_scale.shape[0], generator=gen, device=DEV) >= 1.0 / 3.0).float() * row_scale
        for k, (_, s, lr) in enumerate(specs):
            g = torch.randn((row_scale.shape[0],) + s, generator=gen, device=DEV) * seen.view(-1, *([1] * len(s)))
            for opt in (prod, ref):
                opt.param_groups[k]["params"][0].grad = g
                if k == 0:
                    opt.param_groups[0]["lr"] = lr_xyz
            traj[k].step(g, lr_xyz if k == 0 else lr)
        prod.step()
        ref.step()
        if it % 500 == 0 and it < steps:       # prune a fifth, append as many fresh rows: _prune_optimizer / cat_tensors_to_optimizer
            n = row_scale.shape[0]
            keep = (torch.arange(n, device=DEV) + it // 500) % 5 != 0
            n_new = n - int(keep.sum())
            for k, (_, s, _) in enumerate(specs):
                extra = 0.25 + 0.01 * torch.randn((n_new,) + s, generator=gen, device=DEV)
                for opt in (prod, ref):
                    grp = opt.param_groups[k]
                    p = grp["params"][0]
                    st = opt.state.pop(p)
                    newp = torch.nn.Parameter(torch.cat([p.detach()[keep], extra], 0))
                    st["exp_avg"] = torch.cat([st["exp_avg"][keep], torch.zeros_like(extra)], 0)
                    st["exp_avg_sq"] = torch.cat([st["exp_avg_sq"][keep], torch.zeros_like(extra)], 0)
                    grp["params"][0] = newp
                    opt.state[newp] = st
                traj[k].prune_and_append(keep, extra)
            row_scale = torch.cat([row_scale[keep], 10.0 ** (torch.rand(n_new, generator=gen, device=DEV) * 6.0 - 7.0)])
    torch.cuda.synchronize()
    failures = []
    for k, (name, _, _) in enumerate(specs):
        pp, pr = prod.param_groups[k]["params"][0], ref.param_groups[k]["params"][0]
        assert int(prod.state[pp]["step"]) == int(ref.state[pr]["step"]) == traj[k].t == steps
        for what, a, b, x64 in (("p", pp.detach(), pr.detach(), traj[k].p),
                                ("m", prod.state[pp]["exp_avg"], ref.state[pr]["exp_avg"], traj[k].m),
                                ("v", prod.state[pp]["exp_avg_sq"], ref.state[pr]["exp_avg_sq"], traj[k].v)):
            e_prod, e_torch = _rel_err(a, x64), _rel_err(b, x64)
            print(f"drift {name}.{what}: E_product = {e_prod:.3e}  E_torch = {e_torch:.3e}")
            record_property(f"E_product_{name}_{what}", e_prod)
            record_property(f"E_torch_{name}_{what}", e_torch)
            if not e_prod <= 2.0 * e_torch + 1e-6:
                failures.append((name, what, e_prod, e_torch))
    assert not failures, failures
