"""CPU checks of the model front end (include/f3dgs.h: f3dgs_activate_forward, f3dgs_activate_backward, f3dgs_densify_stats):
the fp64 oracle the GPU tests measure against is itself pinned to torch's autograd and to the repository's torch route for the
statistics, and the library's argument checks answer before any device work."""
import ctypes
import os
import types

import pytest
import torch
import torch.nn.functional as F

import model_front_oracle as mo
from util import ROOT


def _raw(P, M, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    q = r(P, 4)
    q[0] = 0.0                                                  # the clamp of F.normalize is active ...
    q[1] = torch.tensor([0.6, 0.0, -0.8, 0.0]) * 1e-13          # ... also for a norm of 1e-13
    q[2] = torch.tensor([1e-12, 0.0, 0.0, 0.0]) * 1.5           # just above it
    return r(P, 3), q, r(P, 1), r(P, 1, 3), r(P, M - 1, 3)


@pytest.mark.parametrize("M", [1, 4, 16])
def test_oracle_backward_is_torch_fp64_autograd(M):
    P = 37
    raw = [t.clone().requires_grad_(True) for t in _raw(P, M, 5 + M)]
    s, q, o, dc, rest = raw
    outs = (torch.exp(s), F.normalize(q), torch.sigmoid(o), torch.cat((dc, rest), dim=1))
    want_fw = mo.activate_forward(*raw)
    for a, b in zip(outs, want_fw):
        assert a.shape == b.shape
        torch.testing.assert_close(b, a.detach(), rtol=1e-13, atol=0)
    assert torch.equal(want_fw[3], outs[3].detach())
    g = torch.Generator().manual_seed(77)
    ups = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in outs]
    torch.autograd.backward(outs, ups)
    got = mo.activate_backward(outs[0], q, outs[2], ups[0], ups[1], ups[2], ups[3], P, M)
    for name, a, p in zip(("scaling", "rotation", "opacity", "dc", "rest"), got, raw):
        assert a.shape == p.grad.shape, name
        if name == "rotation":      # (g - h (h . g)) / n cancels: errors are relative to max|g| / n of the row
            n = q.detach().norm(dim=-1, keepdim=True).clamp_min(1e-12)
            e_row = ups[1].abs().amax(dim=-1, keepdim=True) / n
            assert float(((a - p.grad).abs() / (p.grad.abs() + e_row)).max()) <= 1e-12
        else:
            torch.testing.assert_close(a, p.grad, rtol=1e-12, atol=0, msg=lambda m: f"{name}: {m}")
    assert torch.equal(got[3], raw[3].grad) and torch.equal(got[4], raw[4].grad)        # copies
    # the clamped rows: the gradient is the upstream over the constant
    assert torch.equal(got[1][:2], ups[1][:2] / 1e-12)
    # None upstream gradients count as zeros
    zero = mo.activate_backward(outs[0], q, outs[2], None, None, None, None, P, M)
    assert all(float(z.abs().max()) == 0.0 if z.numel() else True for z in zero)
    assert [tuple(z.shape) for z in zero] == [(P, 3), (P, 4), (P, 1), (P, 1, 3), (P, M - 1, 3)]


def test_oracle_statistics_are_the_torch_route():
    import train_step
    P = 301
    g = torch.Generator().manual_seed(3)
    grad = torch.randn(P, 3, generator=g) * 1e-3
    radii = torch.randint(-2, 40, (P,), generator=g, dtype=torch.int32)
    radii[:4] = torch.tensor([0, -1, 1, 1 << 24], dtype=torch.int32)
    acc0, den0 = torch.rand(P, 1, generator=g), torch.randint(0, 5, (P, 1), generator=g).float()
    mr0 = torch.randint(0, 30, (P,), generator=g).float()
    for with_grad in (True, False):
        vsp = torch.zeros(P, 3, requires_grad=True)
        vsp.grad = grad.clone() if with_grad else None
        pkg = {"viewspace_points": vsp, "radii": radii, "visibility_filter": radii > 0}
        norm, count, r = train_step.densification_deltas(pkg, P, "cpu")
        acc, den, mr = acc0.clone(), den0.clone(), mr0.clone()
        acc += norm                                                  # train_step.dp_train_step
        den += count
        seen = count.squeeze(-1) > 0
        mr[seen] = torch.maximum(mr[seen], r[seen].to(mr.dtype))
        o_acc, o_den, o_mr = mo.densify_stats(grad if with_grad else None, radii, acc0, den0, mr0)
        assert torch.equal(o_den.float(), den.reshape(-1)) and torch.equal(o_mr.float(), mr)
        torch.testing.assert_close(o_acc.float(), acc.reshape(-1), rtol=3e-7, atol=0)       # the route sums in fp32
        hidden = radii <= 0
        assert torch.equal(o_acc[hidden].float(), acc0.reshape(-1)[hidden])
        # the deltas themselves: the same call on zeroed buffers
        z = torch.zeros(P)
        d_acc, d_den, d_mr = mo.densify_stats(grad if with_grad else None, radii, z, z, z)
        assert torch.equal(d_den.float(), count.reshape(-1)) and torch.equal(d_mr.float(), r)
        torch.testing.assert_close(d_acc.float(), norm.reshape(-1), rtol=3e-7, atol=0)
    assert mo.densify_stats(grad, radii, None, None, None) == (None, None, None)


def _lib():
    so = os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(so)
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    vp = ctypes.c_void_p
    lib.f3dgs_activate_forward.argtypes = [ctypes.c_int] * 2 + [vp] * 10
    lib.f3dgs_activate_backward.argtypes = [ctypes.c_int] * 2 + [vp] * 13
    lib.f3dgs_densify_stats.argtypes = [ctypes.c_int] + [vp] * 6
    return lib


A = 0x10000         # a 16-byte aligned address that is never dereferenced: every call below is refused before any device work
INVALID = -1        # F3DGS_ERR_INVALID_ARGUMENT


def test_argument_validation_without_gpu():
    lib = _lib()
    fw, bw, st = lib.f3dgs_activate_forward, lib.f3dgs_activate_backward, lib.f3dgs_densify_stats
    ok_fw = [A] * 9 + [None]
    ok_bw = [A] * 12 + [None]

    def refused(rc, word):
        assert rc == INVALID and word in lib.f3dgs_last_error(), (rc, lib.f3dgs_last_error())

    # sizes
    refused(fw(-1, 16, *ok_fw), b"P < 0")
    refused(bw(-1, 16, *ok_bw), b"P < 0")
    refused(st(-1, A, A, A, A, A, None), b"P < 0")
    for M in (0, -3):
        refused(fw(5, M, *ok_fw), b"M =")
        refused(bw(5, M, *ok_bw), b"M =")
    # forward: a NULL input of a group whose output was requested (inputs 0..4, outputs 5..8)
    for inp, M in ((0, 16), (1, 16), (2, 16), (3, 16), (4, 16), (4, 2)):
        args = list(ok_fw)
        args[inp] = None
        refused(fw(5, M, *args), b"null input")
    # forward: misaligned rotations / shs
    for out, off in ((6, 4), (6, 8), (8, 4), (8, 12)):
        args = list(ok_fw)
        args[out] = A + off
        refused(fw(5, 16, *args), b"16-byte")
    # backward: a saved input missing while its upstream gradient and its output are given (saved 0..2, upstream 3..6, outputs 7..11)
    for inp in (0, 1, 2):
        args = list(ok_bw)
        args[inp] = None
        refused(bw(5, 16, *args), b"null input")
    args = list(ok_bw)
    args[6] = A + 4
    refused(bw(5, 16, *args), b"16-byte")
    # statistics: radii is the one required input
    refused(st(5, A, None, A, A, A, None), b"radii")


def test_empty_model_is_ok_without_gpu():
    lib = _lib()
    assert lib.f3dgs_activate_forward(0, 16, *([None] * 10)) == 0
    assert lib.f3dgs_activate_forward(0, 1, *([A] * 9), None) == 0
    assert lib.f3dgs_activate_backward(0, 16, *([None] * 13)) == 0
    assert lib.f3dgs_densify_stats(0, *([None] * 6)) == 0
    assert lib.f3dgs_version() >= 32300
