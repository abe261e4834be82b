"""CPU checks of the capturable optimizer step (include/f3dgs.h: f3dgs_adam_schedule, f3dgs_adam_step_multi_device,
f3dgs_reset_opacity): the schedule oracle the GPU tests measure against is pinned to a numpy evaluation of the formula, the
library's argument checks answer before any device work, and FusedAdam(capturable=True) refuses CPU tensors."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import capturable_adam_oracle as co
from util import ROOT


def _numpy_schedule(i, lr_init, lr_final, lr_delay_steps, lr_delay_mult, max_steps):
    if lr_init == 0.0 and lr_final == 0.0:
        return np.float64(0.0)
    i = np.float64(i)
    delay = np.float64(1.0)
    if lr_delay_steps > 0:
        delay = lr_delay_mult + (1 - lr_delay_mult) * np.sin(np.pi / 2 * np.clip(i / lr_delay_steps, 0, 1))
    u = np.clip(i / max_steps, 0, 1)
    return delay * np.exp(np.log(np.float64(lr_init)) * (1 - u) + np.log(np.float64(lr_final)) * u)


def test_schedule_oracle_is_the_formula():
    n = 0
    for i, mult, steps, (a, b) in itertools.product(co.ITERATIONS, co.DELAY_MULTS, co.DELAY_STEPS, co.RATES):
        got = co.schedule(i, a, b, steps, mult, co.MAX_STEPS)
        want = float(_numpy_schedule(i, a, b, steps, mult, co.MAX_STEPS))
        assert got == pytest.approx(want, rel=1e-15, abs=0.0), (i, mult, steps, a, b, got, want)
        n += 1
    assert n == 7 * 2 * 2 * 2
    # the ends: lr_init at 0 without a delay, lr_final from max_steps on, the delay factor's own ends
    assert co.schedule(0, 1.6e-4, 1.6e-6, 0, 1.0, co.MAX_STEPS) == pytest.approx(1.6e-4, rel=1e-15)
    assert co.schedule(co.MAX_STEPS + 5, 1.6e-4, 1.6e-6, 0, 1.0, co.MAX_STEPS) == pytest.approx(1.6e-6, rel=1e-15)
    assert co.schedule(0, 1.6e-4, 1.6e-6, 100, 0.01, co.MAX_STEPS) == pytest.approx(1.6e-6, rel=1e-15)


def test_constants_oracle_rounds_once():
    for t in co.STEP_WORDS:
        s, c = co.constants(1.6e-4, 0.9, 0.999, t + 1)
        assert s.dtype == np.float32 and c.dtype == np.float32
        assert float(s) == float(np.float32(1.6e-4 / (1.0 - 0.9 ** (t + 1))))
        assert float(c) == float(np.float32(1.0 / np.sqrt(1.0 - 0.999 ** (t + 1))))


def test_reset_oracle_edges():
    cap = float(np.float32(0.01))
    raw = np.array([-np.inf, -20.0, 0.0, 20.0, np.inf, np.nan], np.float32)
    out = co.reset_opacity(raw, cap)
    assert out[0] == -np.inf and np.isnan(out[5])
    top = np.log(cap / (1.0 - cap))
    assert out[2] == pytest.approx(top, rel=1e-15) and out[3] == pytest.approx(top, rel=1e-15) and out[4] == pytest.approx(top, rel=1e-15)
    assert out[1] == pytest.approx(-20.0, rel=1e-9)


# ---- the C ABI's argument checks ---------------------------------------------------------------------------------------------

class _Tensor(ctypes.Structure):        # include/f3dgs.h: f3dgs_adam_device_tensor
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("n", ctypes.c_size_t), ("step", ctypes.c_void_p), ("lr", ctypes.c_void_p), ("scheduled", ctypes.c_int),
                ("lr_init", ctypes.c_double), ("lr_final", ctypes.c_double), ("lr_delay_mult", ctypes.c_double),
                ("lr_delay_steps", ctypes.c_longlong), ("max_steps", ctypes.c_longlong)]


A = 0x10000         # an aligned address that is never dereferenced: every call below is refused before any device work
INVALID = -1        # F3DGS_ERR_INVALID_ARGUMENT


def _lib():
    so = os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(so)
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    vp, d = ctypes.c_void_p, ctypes.c_double
    lib.f3dgs_adam_schedule.argtypes = [ctypes.c_int, vp, d, d, vp, ctypes.c_int, vp, vp]
    lib.f3dgs_adam_step_multi_device.argtypes = [ctypes.c_int, vp, d, d, d, vp, ctypes.c_size_t, vp, vp]
    lib.f3dgs_reset_opacity.argtypes = [ctypes.c_size_t, vp, vp, vp, ctypes.c_float, vp]
    lib.f3dgs_version.restype = ctypes.c_int
    return lib


def _entry(**kw):
    e = dict(param=A, grad=A, exp_avg=A, exp_avg_sq=A, n=8, step=A, lr=A, scheduled=0, lr_init=0.0, lr_final=0.0, lr_delay_mult=1.0,
             lr_delay_steps=0, max_steps=1)
    e.update(kw)
    return _Tensor(**e)


def _table(*entries):
    return (_Tensor * max(1, len(entries)))(*entries)


def test_argument_validation_without_gpu():
    lib = _lib()
    assert lib.f3dgs_version() >= 32400

    def both(n, tab, b1=0.9, b2=0.999, iteration=A, consts=A):
        p = ctypes.addressof(tab) if tab is not None else None
        return (lib.f3dgs_adam_schedule(n, p, b1, b2, iteration, 1, consts, None),
                lib.f3dgs_adam_step_multi_device(n, p, b1, b2, 1e-15, None, 0, consts, None))

    def refused(rcs, text):
        for rc in (rcs if isinstance(rcs, tuple) else (rcs,)):
            assert rc == INVALID, rc
        assert text in lib.f3dgs_last_error(), lib.f3dgs_last_error()

    ok = _table(_entry())
    # the count and the tables
    for n in (-1, 17):
        refused(both(n, ok), b"tensors per call")
    assert both(0, None) == (0, 0)                        # nothing to do, nothing launched
    refused(both(1, None), b"null table")
    refused(both(1, ok, consts=None), b"null table of constants")
    # an entry with n > 0 and a null pointer, step word or rate word; with n == 0 the pointers are not looked at
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        refused(both(1, _table(_entry(**{field: None}))), b"null pointer")
    refused(both(1, _table(_entry(step=None))), b"null step word")
    refused(both(1, _table(_entry(lr=None))), b"null rate word")
    refused(both(2, _table(_entry(), _entry(step=None))), b"tensor 1")
    # the schedule's constants
    sched = dict(scheduled=1, lr_init=1.6e-4, lr_final=1.6e-6, max_steps=30000)
    refused(both(1, _table(_entry(**{**sched, "max_steps": 0}))), b"max_steps")
    refused(both(1, _table(_entry(**{**sched, "max_steps": -4}))), b"max_steps")
    refused(both(1, _table(_entry(**{**sched, "lr_delay_steps": -1}))), b"lr_delay_steps")
    refused(both(1, _table(_entry(**{**sched, "lr_init": 0.0}))), b"both positive or both zero")
    refused(both(1, _table(_entry(**{**sched, "lr_final": 0.0}))), b"both positive or both zero")
    refused(both(1, _table(_entry(**{**sched, "lr_init": -1e-4}))), b"both positive or both zero")
    refused(both(1, _table(_entry(**{**sched, "lr_final": -1e-6}))), b"both positive or both zero")
    refused(both(1, _table(_entry(**{**sched, "lr_final": float("nan")}))), b"both positive or both zero")
    # a scheduled entry needs the iteration word (the schedule call reads it; the step call does not take one)
    tab = _table(_entry(**sched, lr=None))
    refused(lib.f3dgs_adam_schedule(1, ctypes.addressof(tab), 0.9, 0.999, None, 1, A, None), b"no iteration word")
    # betas
    for b1, b2 in ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, -1e-3), (float("nan"), 0.999)):
        refused(both(1, ok, b1=b1, b2=b2), b"outside [0, 1)")
    # a mask without rows
    refused(lib.f3dgs_adam_step_multi_device(1, ctypes.addressof(ok), 0.9, 0.999, 1e-15, A, 0, A, None), b"without a row count")
    # the opacity reset
    assert lib.f3dgs_reset_opacity(0, None, None, None, 0.01, None) == 0
    refused(lib.f3dgs_reset_opacity(5, None, A, A, 0.01, None), b"null pointer")
    for cap in (0.0, 1.0, -0.5, float("nan")):
        refused(lib.f3dgs_reset_opacity(5, A, A, A, cap, None), b"cap")


def test_capturable_refuses_cpu_tensors():
    from fused_adam import FusedAdam
    p = torch.nn.Parameter(torch.zeros(5, 3))
    with pytest.raises(ValueError, match="HIP tensors only"):
        FusedAdam([p], lr=1e-3, capturable=True)
    opt = FusedAdam([p], lr=1e-3)                      # the default mode constructs as before
    assert opt.capturable is False and "capturable" not in opt.param_groups[0]
    for call in (opt.push_lrs, opt.iteration, opt.current_lrs, lambda: opt.set_iteration(3),
                 lambda: opt.set_lr_schedule("xyz", 1e-4, 1e-6)):
        with pytest.raises(RuntimeError, match="capturable=True"):
            call()
