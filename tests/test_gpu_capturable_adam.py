"""The capturable optimizer step: FusedAdam(capturable=True) - step counts, rates and the learning-rate schedule
on the device -, the in-place opacity reset, and train_step.CapturedTrainer, which replays a whole iteration from a graph."""
import itertools
import math
import types

import numpy as np
import pytest
import torch

import adam_oracle as ao
import capturable_adam_oracle as co

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
B1, B2, EPS = 0.9, 0.999, 1e-15
WIDTHS7 = (3, 3, 45, 1, 3, 4, 32)
NAMES7 = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "semantic_feature")
LRS7 = (1.6e-4, 2.5e-3, 1.25e-4, 0.05, 5e-3, 1e-3, 1e-3)


def _ulp32_apart(a, b):
    """|a - b| in units of the spacing of float32 at b."""
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) / float(np.spacing(np.abs(b)))


def _bits(t):
    return t.detach().cpu().contiguous().view(-1).numpy().view(np.int32)


# ---- 1. constants and schedule --------------------------------------------------------------------------------------------------

def test_schedule_kernel_counts_steps_and_forms_rates_and_constants():
    """One schedule launch per point of the CPU grid over seven tensors: four follow the schedule, three their base rate."""
    from diff_gaussian_rasterization import _C
    n_t = 7
    ps = [torch.zeros(4, device=DEV) for _ in range(n_t)]
    lr_table = torch.tensor(LRS7, dtype=torch.float64, device=DEV)
    consts = torch.zeros(16, 2, dtype=torch.float64, device=DEV)
    iteration = torch.zeros((), dtype=torch.int64, device=DEV)
    differ = total = 0
    worst_lr = 0.0
    for case, (i, mult, delay, (lr0, lr1)) in enumerate(itertools.product(co.ITERATIONS, co.DELAY_MULTS, co.DELAY_STEPS, co.RATES)):
        words = [co.STEP_WORDS[(k + case) % len(co.STEP_WORDS)] for k in range(n_t)]
        steps = [torch.tensor(float(w), device=DEV) for w in words]
        sched = [[lr0, lr1, float(delay), mult, float(co.MAX_STEPS)] if k < 4 else [] for k in range(n_t)]
        iteration.fill_(i)
        consts.fill_(-1.0)
        _C.adam_step_multi_device(ps, ps, ps, ps, steps, lr_table, list(range(n_t)), sched, B1, B2, EPS, iteration, True, consts,
                                  None, 1)
        got = consts.cpu()
        assert int(iteration.item()) == i + 1
        assert [float(s.item()) for s in steps] == [float(w + 1) for w in words]
        pair = got[:, 1].contiguous().view(torch.float32).reshape(16, 2).numpy()
        assert float(got[n_t:, 0].max()) == -1.0 and float(got[n_t:, 0].min()) == -1.0        # slots beyond the table: untouched
        for k in range(n_t):
            want_lr = co.schedule(i + 1, lr0, lr1, delay, mult, co.MAX_STEPS) if k < 4 else LRS7[k]
            lr = float(got[k, 0])
            assert abs(lr - want_lr) <= 1e-12 * abs(want_lr), (i, mult, delay, lr0, k, lr, want_lr)
            if want_lr:
                worst_lr = max(worst_lr, abs(lr - want_lr) / want_lr)
            if k >= 4:
                assert lr == want_lr
            for have, want in zip(pair[k], co.constants(want_lr, B1, B2, words[k] + 1)):
                total += 1
                differ += int(np.float32(have) != want)
                assert _ulp32_apart(have, want) <= 1.0, (i, mult, delay, lr0, k, have, want)
    print(f"scheduled rates: worst {worst_lr:.3e} relative to the fp64 oracle; {differ} of {total} fp32 constants differ from "
          f"the host-formed ones (each by at most 1 ulp32)")
    # advance == 0: the word is read as it is and stays
    iteration.fill_(50)
    steps = [torch.zeros((), device=DEV) for _ in range(n_t)]
    sched = [[1.6e-4, 1.6e-6, 100.0, 0.01, float(co.MAX_STEPS)]] + [[] for _ in range(n_t - 1)]
    _C.adam_step_multi_device(ps, ps, ps, ps, steps, lr_table, list(range(n_t)), sched, B1, B2, EPS, iteration, False, consts, None, 1)
    assert int(iteration.item()) == 50
    want = co.schedule(50, 1.6e-4, 1.6e-6, 100, 0.01, co.MAX_STEPS)
    assert abs(float(consts[0, 0]) - want) <= 1e-12 * want


# ---- 2. one step, every shape ---------------------------------------------------------------------------------------------------

def _placed(arr, shape, offset):
    """`arr` as a contiguous view of `shape` at `offset` floats into a buffer with GUARD floats behind it."""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + GUARD,), -7.25, device=DEV)
    buf[offset:offset + n] = torch.from_numpy(np.ascontiguousarray(arr)).to(DEV).reshape(-1)
    return buf, buf[offset:offset + n].view(shape)


def _strided_grad(arr, shape):
    """The gradient as a non-contiguous tensor: every second element of the last dimension of a wider one."""
    wide = torch.zeros(tuple(shape[:-1]) + (2 * shape[-1],), device=DEV)
    g = wide[..., ::2]
    g.copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(DEV).reshape(shape))
    assert g.numel() <= 1 or not g.is_contiguous()
    return g


def _pair_step(shapes, offset, strided, visibility=None, seed=0):
    """One step of FusedAdam(capturable=False) and of FusedAdam(capturable=True) from the same preset state; the issue's
    checks for every tensor.  Returns how many tensors had bit-equal constants."""
    from fused_adam import FusedAdam
    n_t = len(shapes)
    lrs = [ao.LRS[k % 3] * (1.0 + 0.01 * k) for k in range(n_t)]
    t0s = [co.STEP_WORDS[k % len(co.STEP_WORDS)] for k in range(n_t)]
    data = [ao.family(int(np.prod(s)), ao.BANDS[2 + k % 2], 100 * seed + k) for k, s in enumerate(shapes)]
    sides = {}
    for mode in (False, True):
        groups, held = [], []
        for k, (shape, (p, g, m, v)) in enumerate(zip(shapes, data)):
            bp, vp = _placed(p, shape, offset)
            bm, vm = _placed(m, shape, offset)
            bv, vv = _placed(v, shape, offset)
            par = torch.nn.Parameter(vp)
            assert par.data_ptr() == vp.data_ptr()
            par.grad = _strided_grad(g, shape) if strided and k % 2 == 0 else torch.from_numpy(g).to(DEV).reshape(shape)
            groups.append({"params": [par], "lr": lrs[k], "name": f"t{k}"})
            held.append((par, (bp, bm, bv), (vm, vv)))
        opt = FusedAdam(groups, lr=0.0, eps=EPS, capturable=mode)
        for k, (par, _, (vm, vv)) in enumerate(held):
            step = torch.tensor(float(t0s[k]), device=DEV) if mode else torch.tensor(float(t0s[k]))
            opt.state[par] = {"step": step, "exp_avg": vm, "exp_avg_sq": vv}
        opt.step(visibility=visibility)
        sides[mode] = (opt, held)
    torch.cuda.synchronize()
    opt, held = sides[True]
    equal_consts = 0
    rows = None if visibility is None else (visibility != 0).cpu().numpy()
    for k, shape in enumerate(shapes):
        n = int(np.prod(shape))
        par, bufs, (vm, vv) = held[k]
        par0, bufs0, (vm0, vv0) = sides[False][1][k]
        p, g, m, v = data[k]
        t = t0s[k] + 1
        if n:
            assert float(opt.state[par]["step"].item()) == float(t), k
        # the moments are the default path's, bit for bit; the parameter too where the device formed the host's constants
        assert np.array_equal(_bits(vm), _bits(vm0)) and np.array_equal(_bits(vv), _bits(vv0)), k
        table, slot = next((j, tab.index(k)) for j, tab in enumerate(opt._last) if k in tab)       # one parameter per group
        have =opt._consts[table][slot, 1:2].contiguous().view(torch.float32).cpu().numpy()
        want = co.constants(lrs[k], B1, B2, t)
        if n:
            assert _ulp32_apart(have[0], want[0]) <= 1.0 and _ulp32_apart(have[1], want[1]) <= 1.0, (k, have, want)
            if have[0] == want[0] and have[1] == want[1]:
                equal_consts += 1
                assert np.array_equal(_bits(par), _bits(par0)), k
        # everywhere: inside A / B / C of the fp64 step with the oracle's rate and step count
        where = None
        if rows is not None and len(shape) >= 1 and shape[0] == rows.shape[0]:
            where = np.repeat(rows, n // max(1, shape[0])) if n else None
        if n:
            ao.check_step(p, g, m, v, par, vm, vv, lrs[k], B1, B2, EPS, t, where=where, what=f"tensor {k} {tuple(shape)}")
        if where is not None:          # hidden rows keep their bits
            hid = ~where
            for got, was in ((par, p), (vm, m), (vv, v)):
                assert np.array_equal(_bits(got)[hid], was.view(np.int32)[hid]), k
        for b in bufs:                 # the guard behind every buffer, and the float in front of an offset view
            assert bool((b[offset + n:] == -7.25).all()) and bool((b[:offset] == -7.25).all()), k
    return equal_consts


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("offset", [0, 1])
def test_one_step_equals_the_default_path_at_every_length(offset, strided):
    shapes = [(n,) for n in (0, 1, 3, 4, 5, 1023, 1024, 1025, 4099)]
    same = _pair_step(shapes, offset, strided, seed=1 + offset)
    print(f"offset {offset} strided {strided}: {same} of {len(shapes) - 1} tensors stepped with bit-equal constants")


@pytest.mark.parametrize("count", [16, 17])
def test_one_step_over_one_and_two_tables(count):
    shapes = [(37 + 5 * k,) for k in range(count)]
    same = _pair_step(shapes, 0, False, seed=7)
    print(f"{count} tensors: {same} stepped with bit-equal constants")


@pytest.mark.parametrize("kind", ["bool", "uint8", "radii"])
@pytest.mark.parametrize("P", [1, 63, 65, 257])
def test_one_masked_step_touches_only_visible_rows(P, kind):
    g = torch.Generator().manual_seed(P)
    seen = torch.rand(P, generator=g) < 0.5
    if P > 1:
        seen[0], seen[1] = True, False
    vis = {"bool": seen, "uint8": seen.to(torch.uint8), "radii": torch.where(seen, 256, 0).to(torch.int32)}[kind].to(DEV)
    shapes = [(P, w) for w in (1, 3, 4, 48)] + [(P + 3,)]          # the last one is not per-row data: stepped densely
    _pair_step(shapes, 1, True, visibility=vis, seed=P)


# ---- 3. replayed ----------------------------------------------------------------------------------------------------------------

def _seven(P, capturable=True):
    from fused_adam import FusedAdam
    g = torch.Generator().manual_seed(P)
    groups = [{"params": [torch.nn.Parameter(torch.randn(P, w, generator=g).to(DEV))], "lr": lr, "name": n}
              for n, w, lr in zip(NAMES7, WIDTHS7, LRS7)]
    return FusedAdam(groups, lr=0.0, eps=EPS, capturable=capturable)


def test_a_captured_step_counts_and_follows_the_schedule_over_replays():
    P = 257
    opt = _seven(P)
    sched = dict(lr_init=1.6e-4, lr_final=1.6e-6, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=8)
    opt.set_lr_schedule("xyz", **sched)
    params = [g["params"][0] for g in opt.param_groups]
    gen = torch.Generator().manual_seed(9)
    fresh = lambda p: (torch.randn(p.shape, generator=gen) * 0.01).to(DEV)
    for p in params:
        p.grad = fresh(p)
    start = [p.detach().clone() for p in params]
    opt.step()                                  # eager: allocates state and tables; undone below
    with torch.no_grad():
        for p, s in zip(params, start):
            p.copy_(s)
            for k in ("step", "exp_avg", "exp_avg_sq"):
                opt.state[p][k].zero_()
    opt.set_iteration(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    assert opt.iteration() == 0 and all(float(opt.state[p]["step"].item()) == 0.0 for p in params)     # a capture runs nothing

    def replay_and_check(t, lrs):
        before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
        grads = [fresh(p) for p in params]
        for p, g in zip(params, grads):
            p.grad.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        for p, g, (p0, m0, v0), lr, name in zip(params, grads, before, lrs, NAMES7):
            st = opt.state[p]
            ao.check_step(p0, g, m0, v0, p, st["exp_avg"], st["exp_avg_sq"], lr, B1, B2, EPS, t, what=f"replay {t} {name}")

    seen = []
    for t in range(1, 6):
        lr_xyz = co.schedule(t, **sched)
        seen.append(lr_xyz)
        replay_and_check(t, (lr_xyz,) + LRS7[1:])
    assert seen[0] > 1.5 * seen[4]                               # the rate did move
    assert opt.iteration() == 5 and all(float(opt.state[p]["step"].item()) == 5.0 for p in params)
    lrs = opt.current_lrs()
    assert abs(lrs["xyz"] - seen[4]) <= 1e-12 * seen[4] and lrs["opacity"] == 0.05
    assert abs(opt.param_groups[0]["lr"] - seen[4]) <= 1e-12 * seen[4]
    # a new iteration count and a new base rate reach the SAME graph
    opt.set_iteration(100)
    opt.param_groups[3]["lr"] = 0.02
    opt.push_lrs()
    want = list(LRS7)
    want[0], want[3] = co.schedule(101, **sched), 0.02
    assert want[0] == pytest.approx(1.6e-6, rel=1e-12)
    replay_and_check(6, want)
    assert opt.iteration() == 101 and opt.current_lrs()["opacity"] == 0.02
    # the state dictionary round-trips the device step words
    other = _seven(P)
    other.load_state_dict(opt.state_dict())
    for g in other.param_groups:
        s = other.state[g["params"][0]]["step"]
        assert s.is_cuda and s.dtype == torch.float32 and float(s.item()) == 6.0


def test_a_parameter_without_a_gradient_is_skipped():
    opt = _seven(65)
    params = [g["params"][0] for g in opt.param_groups]
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()
    kept = params[2].detach().clone()
    params[2].grad = None
    opt.step()
    torch.cuda.synchronize()
    assert [float(opt.state[p]["step"].item()) for p in params] == [2.0, 2.0, 1.0, 2.0, 2.0, 2.0, 2.0]
    assert torch.equal(params[2].detach(), kept) and opt.iteration() == 2


# ---- 4. opacity reset -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("P", [1, 63, 1025])
def test_opacity_reset_in_place(P, capturable):
    import model_front
    from fused_adam import FusedAdam
    cap = np.float32(0.01)
    edge = np.float32(np.log(np.float64(cap) / (1.0 - np.float64(cap))))
    specials = np.array([edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(-100)), np.inf, -np.inf, np.nan],
                        np.float32)
    raw = np.concatenate([specials, np.linspace(-20.0, 20.0, max(P, 2)).astype(np.float32)])[:P]
    model = types.SimpleNamespace(_opacity=torch.nn.Parameter(torch.from_numpy(raw).to(DEV).reshape(P, 1)))
    model.optimizer = FusedAdam([{"params": [model._opacity], "lr": 0.05, "name": "opacity"}], lr=0.0, eps=EPS, capturable=capturable)
    model._opacity.grad = torch.full((P, 1), 0.5, device=DEV)
    model.optimizer.step()                       # moments that are not zero, a step count of 1
    with torch.no_grad():
        model._opacity.copy_(torch.from_numpy(raw).to(DEV).reshape(P, 1))
    st = model.optimizer.state[model._opacity]
    assert float(st["exp_avg"].abs().min()) > 0 and float(st["step"]) == 1.0
    ptr, ident = model._opacity.data_ptr(), id(model._opacity)
    x = model._opacity.detach()
    s = torch.sigmoid(x)
    chain = torch.min(s, torch.full_like(s, float(cap)))
    chain = torch.log(chain / (1 - chain)).cpu().numpy().reshape(-1)          # the reference's reset_opacity in torch's fp32 kernels
    model_front.reset_opacity_(model, cap=float(cap))
    torch.cuda.synchronize()
    got = model._opacity.detach().cpu().numpy().reshape(-1)
    want = co.reset_opacity(raw, float(cap))
    assert model._opacity.data_ptr() == ptr and id(model._opacity) == ident and model.optimizer.state[model._opacity] is st
    assert float(st["exp_avg"].abs().max()) == 0.0 and float(st["exp_avg_sq"].abs().max()) == 0.0 and float(st["step"]) == 1.0
    assert np.array_equal(np.isnan(got), np.isnan(chain)) and np.array_equal(np.isinf(got), np.isinf(chain))
    assert np.array_equal(got[np.isinf(got)], chain[np.isinf(chain)])
    fin = np.isfinite(want)
    if fin.any():
        ulp = ao.ulp32(want[fin])
        e_k = float((np.abs(got[fin].astype(np.float64) - want[fin]) / ulp).max())
        e_t = float((np.abs(chain[fin].astype(np.float64) - want[fin]) / ulp).max())
        print(f"P={P}: kernel {e_k:.3f} ulp32, torch chain {e_t:.3f} ulp32 of the fp64 oracle")
        assert e_k <= e_t + 1.0
        assert float(got[fin].max()) <= float(np.nextafter(edge, np.float32(0))) + 1e-6        # nothing stays above the cap


# ---- 5. the whole iteration -----------------------------------------------------------------------------------------------------

def _train_model(sc, capturable=True):
    """test_gpu_model_front's model with the reference's optimizer groups (scene/gaussian_model.py:168-176)."""
    from fused_adam import FusedAdam
    from test_gpu_model_front import _Model
    m = _Model(sc)
    for n in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_semantic_feature"):
        setattr(m, n, torch.nn.Parameter(getattr(m, n).detach().clone()))
    m.percent_dense = 0.01
    attrs = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_semantic_feature")
    groups = [{"params": [getattr(m, a)], "lr": lr, "name": n} for n, a, lr in zip(NAMES7, attrs, LRS7)]
    m.optimizer = FusedAdam(groups, lr=0.0, eps=EPS, capturable=capturable)
    return m


XYZ_SCHEDULE = dict(lr_init=1.6e-4, lr_final=1.6e-6, lr_delay_steps=0, lr_delay_mult=0.01, max_steps=30000)
ATTRS7 = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_semantic_feature")


def _checked_step(trainer, m, cam, targets):
    """One CapturedTrainer.step, then: every parameter moved as Adam dictates for the gradient that replay produced."""
    opt = m.optimizer
    torch.cuda.synchronize()
    it = opt.iteration()
    before = {}
    for a in ATTRS7:
        p = getattr(m, a)
        st = opt.state.get(p, {})
        zeros = torch.zeros_like(p)
        before[a] = (p.detach().clone(), st["exp_avg"].clone() if "exp_avg" in st else zeros,
                     st["exp_avg_sq"].clone() if "exp_avg_sq" in st else zeros.clone(), float(st["step"].item()) if "step" in st else 0.0)
    loss, radii = trainer.step(cam, *targets)
    torch.cuda.synchronize()
    assert opt.iteration() == it + 1
    for a, name, lr in zip(ATTRS7, NAMES7, LRS7):
        p = getattr(m, a)
        p0, m0, v0, t0 = before[a]
        st = opt.state[p]
        assert float(st["step"].item()) == t0 + 1.0, name
        assert p.grad is not None and p.grad.shape == p.shape, name
        if name == "xyz":
            lr = co.schedule(it + 1, **XYZ_SCHEDULE)
        ao.check_step(p0, p.grad, m0, v0, p, st["exp_avg"], st["exp_avg_sq"], lr, B1, B2, EPS, int(t0) + 1, what=f"iteration {it + 1} {name}")
    return float(loss), radii


def _targets(sc, cam):
    g = torch.Generator().manual_seed(2)
    return (torch.rand(3, cam.image_height, cam.image_width, generator=g).to(DEV), torch.randn(sc["C"], 60, 100, generator=g).to(DEV))


def _loss(pkg, gt_image, gt_feature):
    from feature_loss import fused_feature_l1
    from image_loss import fused_l1_dssim
    return fused_l1_dssim(pkg["render"], gt_image, 0.2) + fused_feature_l1(pkg["feature_map"], gt_feature, None, None)


def test_the_whole_iteration_with_its_optimizer_step_is_replayed(option):
    """The scene, model, camera and losses of test_the_whole_iteration_is_captured_with_its_bookkeeping.  The statistics count
    every replay's own visible Gaussians (the parameters move now; with an unchanged count that is 3 x visible)."""
    import model_front
    import train_step
    from test_gpu_model_front import PIPE, _camera, _plumbing_scene
    option("bwd_bf16", 1)
    sc = _plumbing_scene()
    cam, bg = _camera(sc), sc["bg"].to(DEV)
    targets = _targets(sc, cam)
    # three eager iterations from the same state
    e = _train_model(sc)
    e.optimizer.set_lr_schedule("xyz", **XYZ_SCHEDULE)
    eager = []
    for _ in range(3):
        e.optimizer.zero_grad(set_to_none=True)
        pkg = model_front.render(cam, e, PIPE, bg)
        loss = _loss(pkg, *targets)
        loss.backward()
        model_front.add_densification_stats(e, pkg)
        e.optimizer.step()
        eager.append(float(loss.detach()))
    m = _train_model(sc)
    m.optimizer.set_lr_schedule("xyz", **XYZ_SCHEDULE)
    trainer = train_step.CapturedTrainer(m, _loss, PIPE, bg)
    losses, visible = [], []
    for _ in range(3):
        loss, radii = _checked_step(trainer, m, cam, targets)
        losses.append(loss)
        visible.append(int((radii > 0).sum()))
    assert trainer.check() and trainer.captures == 1
    print("eager", eager, "replayed", losses, "visible", visible)
    assert visible[0] > 1000 and float(m.denom.sum()) == float(sum(visible))
    if len(set(visible)) == 1:
        assert float(m.denom.sum()) == 3.0 * visible[0]
    for x, y in zip(eager, losses):
        assert abs(x - y) <= 0.03 * abs(x), (eager, losses)
    assert m.optimizer.iteration() == 3


# ---- 6. the graph cache ---------------------------------------------------------------------------------------------------------

def test_the_graph_cache_follows_what_a_capture_freezes(option):
    import copy
    import densify
    import model_front
    import train_step
    from synth import make_scene
    from test_gpu_model_front import PIPE, _camera, _plumbing_scene
    option("bwd_bf16", 1)
    sc = _plumbing_scene()
    cam_a, bg = _camera(sc), sc["bg"].to(DEV)
    cam_b = _camera(make_scene(P=6000, C=16, width=200, height=120, yaw_deg=4.0))          # the same intrinsics, another pose
    assert cam_b.FoVx == cam_a.FoVx and not torch.equal(cam_b.world_view_transform, cam_a.world_view_transform)
    targets = _targets(sc, cam_a)
    m = _train_model(sc)
    m.active_sh_degree = 2
    m.optimizer.set_lr_schedule("xyz", **XYZ_SCHEDULE)
    trainer = train_step.CapturedTrainer(m, _loss, PIPE, bg)
    for cam in (cam_a, cam_b, cam_a):
        with torch.no_grad():
            want = model_front.render(cam, m, PIPE, bg)["render"].clone()
        trainer.step(cam, *targets)
        torch.cuda.synchronize()
        assert torch.equal(trainer.render_pkg["render"], want)
    assert trainer.captures == 1
    # another field of view: a second graph; the first one is still there
    cam_c = copy.copy(cam_a)
    cam_c.FoVx = cam_a.FoVx * 1.1
    trainer.step(cam_c, *targets)
    assert trainer.captures == 2
    trainer.step(cam_a, *targets)
    assert trainer.captures == 2
    # another SH degree
    m.active_sh_degree += 1
    _checked_step(trainer, m, cam_a, targets)
    assert trainer.captures == 3
    # a densification moves the parameters: no notification, a new capture, and the step words go on counting
    torch.cuda.synchronize()
    words = [float(m.optimizer.state[getattr(m, a)]["step"].item()) for a in ATTRS7]
    assert words == [6.0] * 7 and m.optimizer.iteration() == 6
    rows = m._xyz.shape[0]
    torch.manual_seed(5)
    plan = densify.densify_and_prune(m, 1e-7, 0.005, 5.0, None)
    assert m._xyz.shape[0] != rows and plan["cloned"] + plan["split"] > 0, plan
    _checked_step(trainer, m, cam_a, targets)
    assert trainer.captures == 4 and trainer.check()
    assert [float(m.optimizer.state[getattr(m, a)]["step"].item()) for a in ATTRS7] == [7.0] * 7
    assert float(m.denom.sum()) == float((trainer.render_pkg["radii"] > 0).sum())       # the capture's warm-up iterations left no trace
    # the in-place opacity reset keeps the addresses, and with them the graph
    model_front.reset_opacity_(m)
    torch.cuda.synchronize()
    assert float(torch.sigmoid(m._opacity.detach()).max()) <= 0.01 + 1e-6
    _checked_step(trainer, m, cam_a, targets)
    assert trainer.captures == 4 and trainer.check()
