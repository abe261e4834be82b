"""What the capturable optimizer step costs and what a wholly captured iteration takes.  Writes a markdown report.

(a) One training iteration - zero_grad, model_front.render, the fused losses, backward, add_densification_stats, optimizer step -
    at the configurations c1 and c3 of synth.CONFIGS, five ways, alternating in one process:
      eager with FusedAdam() as it was; eager with FusedAdam(capturable=True); train_step.CapturedTrainer (the whole iteration
      replayed, pose and targets copied into its static tensors by one launch; and once more with the targets already there); the
      earlier captured iteration WITHOUT the optimizer (graph_step.CapturedStep, no copies at all) followed by an eager FusedAdam.step.
(b) The optimizer step alone at 1,000,000 Gaussians over seven tensors of widths 3, 3, 45, 1, 3, 4, 32: today's
    adam_step_multi in two interleaved blocks (their difference is its own run-to-run spread), the new pair of launches, and a
    one-element launch (the library has no empty kernel: f3dgs_reset_opacity over one float stands in for it).

Every figure: `rounds` rounds, the variants alternating inside each round, device events around `reps` calls including their
host enqueue; median, minimum and maximum over the rounds.  python tools/captured_iteration_bench.py [--quick] [--out FILE]
"""
import argparse
import math
import os
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd")):
    sys.path.insert(0, p)

import model_front  # noqa: E402
import train_step  # noqa: E402
from diff_gaussian_rasterization import _C  # noqa: E402
from fused_adam import FusedAdam  # noqa: E402

DEV = "cuda:0"
LINES = []
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "semantic_feature")
ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_semantic_feature")
LRS = (1.6e-4, 2.5e-3, 1.25e-4, 0.05, 5e-3, 1e-3, 1e-3)
LR_SCALE = 1e-3     # (a): the reference's rates times this, so that thousands of timed iterations on random targets leave the scene,
                    # and with it the rasterizer's work and the captured instance provision, where they were; a step costs the same


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def time_round_robin(fns, reps, rounds):
    """Per fn (median, min, max) ms per call over `rounds` rounds; the fns alternate inside every round."""
    for f in fns:
        for _ in range(3):
            f()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[i].append(e0.elapsed_time(e1) / reps)
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in times]


class Model:
    """Raw parameters as the reference's GaussianModel holds them, and its optimizer groups (scene/gaussian_model.py:41-178)."""

    def __init__(self, sc, capturable):
        par = lambda x: torch.nn.Parameter(x.to(DEV).contiguous().clone())
        self.active_sh_degree, self.max_sh_degree = sc["sh_degree"], 3
        self._xyz = par(sc["means3D"])
        self._features_dc, self._features_rest = par(sc["shs"][:, :1]), par(sc["shs"][:, 1:])
        self._scaling, self._rotation = par(torch.log(sc["scales"])), par(sc["rotations"])
        op = sc["opacities"].clamp(1e-4, 1 - 1e-4)
        self._opacity = par(torch.log(op / (1 - op)).reshape(-1, 1))
        self._semantic_feature = par(sc["semantic_feature"].reshape(sc["P"], 1, sc["C"]))
        P = sc["P"]
        self.xyz_gradient_accum, self.denom = torch.zeros(P, 1, device=DEV), torch.zeros(P, 1, device=DEV)
        self.max_radii2D = torch.zeros(P, device=DEV)
        groups = [{"params": [getattr(self, a)], "lr": lr * LR_SCALE, "name": n} for n, a, lr in zip(NAMES, ATTRS, LRS)
                  if getattr(self, a).numel()]
        self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15, capturable=capturable)
        if capturable:
            self.optimizer.set_lr_schedule("xyz", 1.6e-4 * LR_SCALE, 1.6e-6 * LR_SCALE, lr_delay_mult=0.01, max_steps=30000)

    get_xyz = property(lambda s: s._xyz)
    get_semantic_feature = property(lambda s: s._semantic_feature)
    get_scaling = property(lambda s: torch.exp(s._scaling))
    get_rotation = property(lambda s: F.normalize(s._rotation))
    get_opacity = property(lambda s: torch.sigmoid(s._opacity))
    get_features = property(lambda s: torch.cat((s._features_dc, s._features_rest), dim=1))


def iterations(config, reps, rounds):
    from feature_loss import fused_feature_l1
    from graph_step import CapturedStep
    from image_loss import fused_l1_dssim
    from synth import CONFIGS, make_scene
    sc = make_scene(seed=0, **CONFIGS[config])
    cam = types.SimpleNamespace(FoVx=2 * math.atan(sc["tanfovx"]), FoVy=2 * math.atan(sc["tanfovy"]), image_height=sc["image_height"],
                                image_width=sc["image_width"], world_view_transform=sc["viewmatrix"].to(DEV),
                                full_proj_transform=sc["projmatrix"].to(DEV), camera_center=sc["campos"].to(DEV))
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg, C = sc["bg"].to(DEV), sc["C"]
    g = torch.Generator().manual_seed(2)
    gt_image = torch.rand(3, cam.image_height, cam.image_width, generator=g).to(DEV)
    targets = [gt_image]
    if C:
        targets.append(torch.randn(C, cam.image_height // 2, cam.image_width // 2, generator=g).to(DEV))

    def loss_fn(pkg, image, feature=None):
        loss = fused_l1_dssim(pkg["render"], image, 0.2)
        if feature is not None:
            loss = loss + fused_feature_l1(pkg["feature_map"], feature, None, None)
        return loss

    def up_to_the_step(m):
        m.optimizer.zero_grad(set_to_none=True)
        pkg = model_front.render(cam, m, pipe, bg)
        loss = loss_fn(pkg, *targets)
        loss.backward()
        model_front.add_densification_stats(m, pkg)
        return loss.detach()

    def eager(m):
        def it():
            loss = up_to_the_step(m)
            m.optimizer.step()
            return loss
        return it

    m_a, m_b, m_c, m_d = Model(sc, False), Model(sc, True), Model(sc, True), Model(sc, False)
    trainer = train_step.CapturedTrainer(m_c, loss_fn, pipe, bg)
    replay_whole = lambda: trainer.step(cam, *targets)
    eager(m_d)()                                   # the state exists before the capture of the optimizer-less iteration
    partial = CapturedStep(lambda: up_to_the_step(m_d)).capture()

    def replay_then_step():
        partial.replay()
        m_d.optimizer.step()

    replay_whole()
    in_place = trainer.static_targets
    replay_in_place = lambda: trainer.step(cam, *in_place)        # the same graph and model as replay_whole

    t = time_round_robin([eager(m_a), eager(m_b), replay_whole, replay_then_step, replay_in_place], reps, rounds)
    counts = partial.counts()          # (entries, num_rendered, long-axis flag, entries provided for, no-room word) of the last frame
    fits = (trainer.check(), partial.check())
    assert fits == (True, True) and trainer.captures == 1, \
        f"{config}: a frame outgrew its captured provision (checks {fits}, captures {trainer.captures}, counts {counts}): the figures are void"
    for name, (med, lo, hi) in zip(("eager, FusedAdam()", "eager, FusedAdam(capturable=True)", "CapturedTrainer: the whole iteration replayed",
                                    "captured without the optimizer, then an eager FusedAdam.step",
                                    "CapturedTrainer, the targets already in its static tensors (no target copy)"), t):
        say(f"| {config} | {name} | {med:.4f} | {lo:.4f} | {hi:.4f} |")


def optimizer_alone(P, reps, rounds):
    widths = (3, 3, 45, 1, 3, 4, 32)
    g = torch.Generator().manual_seed(1)
    mk = lambda w: (torch.randn(P, w, generator=g) * 0.01).to(DEV)
    ps, gs = [mk(w) for w in widths], [mk(w) for w in widths]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    steps = [torch.zeros((), device=DEV) for _ in widths]
    lr_table = torch.tensor(LRS, dtype=torch.float64, device=DEV)
    consts = torch.zeros(16, 2, dtype=torch.float64, device=DEV)
    iteration = torch.zeros((), dtype=torch.int64, device=DEV)
    sched = [[1.6e-4, 1.6e-6, 0.0, 0.01, 30000.0]] + [[] for _ in widths[1:]]
    one = torch.zeros(1, device=DEV)
    count = [0]

    def today():
        count[0] += 1
        _C.adam_step_multi(ps, gs, ms, vs, list(LRS), 0.9, 0.999, 1e-15, [count[0]] * len(ps), None)

    def pair():
        _C.adam_step_multi_device(ps, gs, ms, vs, steps, lr_table, list(range(len(ps))), sched, 0.9, 0.999, 1e-15, iteration, True,
                                  consts, None, 3)

    def one_element():
        _C.reset_opacity(one, None, None, 0.01)

    t = time_round_robin([today, pair, one_element, today], reps, rounds)
    (a, a_lo, a_hi), (n, n_lo, n_hi), (e, e_lo, e_hi), (b, b_lo, b_hi) = t
    floats = sum(widths) * P
    say(f"### the optimizer step alone, P = {P:,}, seven tensors of widths {widths}: {floats * 28 / 1e9:.3f} GB moved per step "
        f"(16 bytes read, 12 written per element)")
    say("| variant | median ms | min ms | max ms |")
    say("|---|---|---|---|")
    say(f"| today's adam_step_multi, block A | {a:.4f} | {a_lo:.4f} | {a_hi:.4f} |")
    say(f"| today's adam_step_multi, block B | {b:.4f} | {b_lo:.4f} | {b_hi:.4f} |")
    say(f"| schedule launch + step launch (device constants) | {n:.4f} | {n_lo:.4f} | {n_hi:.4f} |")
    say(f"| a one-element launch | {e:.4f} | {e_lo:.4f} | {e_hi:.4f} |")
    today_ms, spread = min(a, b), abs(a - b)
    bound = today_ms + max(spread, e)
    say()
    say(f"today's path {today_ms:.4f} ms (the lower block median), its spread between the blocks {spread:.4f} ms, one launch {e:.4f} ms: "
        f"bound {bound:.4f} ms; the new pair takes {n:.4f} ms: {'within' if n <= bound else 'ABOVE'} the bound "
        f"({(n - today_ms) * 1e3:+.1f} us against today's path).")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes and few repetitions: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "captured_iteration_bench.py measures on the GPU: no GPU, no numbers"
    say(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say()
    say("### one training iteration (ms per iteration, host enqueue included)")
    say("| config | iteration | median ms | min ms | max ms |")
    say("|---|---|---|---|---|")
    iterations("c1", 5 if a.quick else 200, 3 if a.quick else 7)
    if not a.quick:
        iterations("c3", 20, 7)
    say()
    optimizer_alone(10_000 if a.quick else 1_000_000, 5 if a.quick else 100, 3 if a.quick else 9)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
