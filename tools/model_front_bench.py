"""Time the model front end (model_front.py, csrc/model_front.hip) against the torch chains it replaces, on the GPU.

    python tools/model_front_bench.py [--out FILE] [--quick]

Stages, at P = 10,000 and 1,000,000 with M = 16 (each fused stage against its torch chain, alternating, in the same run):
  forward     model_front.activate                 | exp, F.normalize, sigmoid, cat (the getters of scene/gaussian_model.py:98-127)
  backward    one activate_backward launch         | autograd through that chain
  statistics  model_front.densification_stats x 2  | train_step.densification_deltas + the masked updates of dp_train_step
Per stage: time per call (device events around `reps` calls, median of `rounds`), launches per call (torch.profiler's kernel
and memcpy events), peak extra memory (allocator peak over the stage, above what was live before it).
Iterations (render, the two fused losses, backward, statistics): the reference's glue - getters, `zeros + 0`, mask-indexed
statistics - against model_front.render + add_densification_stats, eager at c1 and c3, and replayed from a graph at c1
(where the mask-indexed statistics cannot be captured: the captured glue iteration runs WITHOUT statistics).
Also prints the ulp maxima of the forward against the fp64 oracle (tests/model_front_oracle.py), kernel and torch chain.
"""
import argparse
import math
import os
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import model_front  # noqa: E402
import train_step  # noqa: E402
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402

DEV = "cuda:0"
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def time_pair(fns, reps, rounds):
    """Median ms per call of each fn: `rounds` rounds, the fns alternating inside each, device events around `reps` calls."""
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
    return [sorted(t)[len(t) // 2] for t in times]


def launches(fn):
    """Device operations (kernels, memcpys, memsets) of one call."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def peak_extra(fn):
    """Allocator peak during one call above what was allocated before it, MB."""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return (peak - base) / 1e6


def raw_params(P, M, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV).requires_grad_(True)
    return r(P, 3), r(P, 4), r(P, 1), r(P, 1, 3), r(P, M - 1, 3)


def torch_chain(s, q, o, dc, rest):
    return torch.exp(s), F.normalize(q), torch.sigmoid(o), torch.cat((dc, rest), dim=1)


def stages(P, M, reps, rounds):
    say(f"### stages at P = {P:,}, M = {M}")
    say("| stage | fused ms | torch chain ms | fused launches | torch launches | fused peak extra MB | torch peak extra MB |")
    say("|---|---|---|---|---|---|---|")
    raw = raw_params(P, M)
    # forward (under autograd, as render() runs it: the saved tensors are part of the memory)
    fw_f = lambda: model_front.activate(*raw)
    fw_t = lambda: torch_chain(*raw)
    t = time_pair([fw_f, fw_t], reps, rounds)
    say(f"| forward | {t[0]:.4f} | {t[1]:.4f} | {launches(fw_f)} | {launches(fw_t)} | {peak_extra(fw_f):.1f} | {peak_extra(fw_t):.1f} |")
    # backward alone: the forward graphs are built once and kept, each call runs the backward through them
    ups = [torch.randn_like(x) for x in fw_t()]
    outs_f, outs_t = fw_f(), fw_t()
    bw_f = lambda: torch.autograd.grad(outs_f, raw, ups, retain_graph=True)
    bw_t = lambda: torch.autograd.grad(outs_t, raw, ups, retain_graph=True)
    t = time_pair([bw_f, bw_t], reps, rounds)
    say(f"| backward | {t[0]:.4f} | {t[1]:.4f} | {launches(bw_f)} | {launches(bw_t)} | {peak_extra(bw_f):.1f} | {peak_extra(bw_t):.1f} |")
    del outs_f, outs_t
    # statistics: one view's deltas and the update of the model's tensors (dp_train_step's two halves)
    g = torch.Generator().manual_seed(1)
    radii = torch.randint(-20, 40, (P,), generator=g, dtype=torch.int32).to(DEV)
    vsp = torch.zeros(P, 3, device=DEV, requires_grad=True)
    vsp.grad = (torch.randn(P, 3, generator=g) * 1e-3).to(DEV)
    pkg = {"viewspace_points": vsp, "radii": radii, "visibility_filter": radii > 0}
    model = types.SimpleNamespace(xyz_gradient_accum=torch.zeros(P, 1, device=DEV), denom=torch.zeros(P, 1, device=DEV),
                                  max_radii2D=torch.zeros(P, device=DEV))

    def st_t():
        with torch.no_grad():
            norm, count, r = train_step.densification_deltas(pkg, P, DEV)
            model.xyz_gradient_accum += norm
            model.denom += count
            seen = count.squeeze(-1) > 0
            mr = model.max_radii2D
            mr[seen] = torch.maximum(mr[seen], r[seen].to(mr.dtype))

    def st_f():       # dp_train_step(fused_stats=True)
        with torch.no_grad():
            norm, count, r = torch.zeros(P, 1, device=DEV), torch.zeros(P, 1, device=DEV), torch.zeros(P, device=DEV)
            model_front.densification_stats(vsp.grad, radii, norm, count, r)
            model.xyz_gradient_accum += norm
            model.denom += count
            model_front.densification_stats(None, r.to(torch.int32), None, None, model.max_radii2D)

    st_1 = lambda: model_front.add_densification_stats(model, pkg)      # one view, one process: the one launch
    t = time_pair([st_f, st_t, st_1], reps, rounds)
    say(f"| statistics (deltas + update) | {t[0]:.4f} | {t[1]:.4f} | {launches(st_f)} | {launches(st_t)} | {peak_extra(st_f):.1f} | {peak_extra(st_t):.1f} |")
    say(f"| statistics (add_densification_stats) | {t[2]:.4f} | {t[1]:.4f} | {launches(st_1)} | {launches(st_t)} | {peak_extra(st_1):.1f} | {peak_extra(st_t):.1f} |")
    say()


def ulp_maxima(P=100_000, M=16):
    import model_front_oracle as mo
    raw = [x.detach() for x in raw_params(P, M, seed=5)]
    raw[2] = raw[2] * 3.0
    got, ref, want = model_front.activate(*raw), torch_chain(*raw), mo.activate_forward(*raw)
    say(f"### forward error against the fp64 oracle, P = {P:,} normal raw values (ulps of the oracle rounded to fp32)")
    say("| tensor | kernel max ulp | torch chain max ulp |")
    say("|---|---|---|")
    for name, k, t, o in zip(("scales", "rotations", "opacities"), got, ref, want):
        r = o.float()
        ulp = (torch.nextafter(r.abs(), torch.full_like(r, float("inf"))) - r.abs()).double()
        e = lambda x: float(((x.double().cpu() - o).abs() / ulp).max())
        say(f"| {name} | {e(k):.3f} | {e(t):.3f} |")
    say(f"| shs | bit-equal to torch.cat: {torch.equal(got[3], ref[3])} | |")
    say()


class Model:
    """Raw parameters and the reference's getters (scene/gaussian_model.py:98-127)."""

    def __init__(self, sc):
        par = lambda x: x.to(DEV).contiguous().clone().requires_grad_(True)
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

    get_xyz = property(lambda s: s._xyz)
    get_semantic_feature = property(lambda s: s._semantic_feature)
    get_scaling = property(lambda s: torch.exp(s._scaling))
    get_rotation = property(lambda s: F.normalize(s._rotation))
    get_opacity = property(lambda s: torch.sigmoid(s._opacity))
    get_features = property(lambda s: torch.cat((s._features_dc, s._features_rest), dim=1))

    def params(self):
        return [self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation, self._semantic_feature]


def glue_render(cam, pc, pipe, bg):
    """The reference's render as its callers in this repository carry it (edit.render_edit): the model's getters and the
    retained `zeros + 0` in front of the same rasterizer."""
    screenspace_points = torch.zeros_like(pc.get_xyz, dtype=pc.get_xyz.dtype, requires_grad=True, device="cuda") + 0
    screenspace_points.retain_grad()
    st = GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=pc.active_sh_degree, campos=cam.camera_center, prefiltered=False,
        debug=pipe.debug)
    image, feature_map, radii, depth = GaussianRasterizer(raster_settings=st)(
        means3D=pc.get_xyz, means2D=screenspace_points, shs=pc.get_features, colors_precomp=None,
        semantic_feature=pc.get_semantic_feature, opacities=pc.get_opacity, scales=pc.get_scaling, rotations=pc.get_rotation,
        cov3D_precomp=None)
    return {"render": image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii,
            "feature_map": feature_map, "depth": depth}


def iterations(config, reps, rounds, captured):
    from feature_loss import fused_feature_l1
    from graph_step import CapturedStep
    from image_loss import fused_l1_dssim
    from synth import CONFIGS, make_scene
    sc = make_scene(seed=0, **CONFIGS[config])
    m = Model(sc)
    cam = types.SimpleNamespace(FoVx=2 * math.atan(sc["tanfovx"]), FoVy=2 * math.atan(sc["tanfovy"]), image_height=sc["image_height"],
                                image_width=sc["image_width"], world_view_transform=sc["viewmatrix"].to(DEV),
                                full_proj_transform=sc["projmatrix"].to(DEV), camera_center=sc["campos"].to(DEV))
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg, P, C = sc["bg"].to(DEV), sc["P"], sc["C"]
    g = torch.Generator().manual_seed(2)
    gt_image = torch.rand(3, cam.image_height, cam.image_width, generator=g).to(DEV)
    gt_feature = torch.randn(C, cam.image_height // 2, cam.image_width // 2, generator=g).to(DEV) if C else None

    def iteration(render, stats):
        for p in m.params():
            p.grad = None
        pkg = render(cam, m, pipe, bg)
        loss = fused_l1_dssim(pkg["render"], gt_image, 0.2)
        if C:
            loss = loss + fused_feature_l1(pkg["feature_map"], gt_feature, None, None)
        loss.backward()
        if stats is not None:
            stats(pkg)
        return loss.detach()

    def glue_stats(pkg):          # train.py:132-133
        with torch.no_grad():
            vis, radii = pkg["visibility_filter"], pkg["radii"]
            m.max_radii2D[vis] = torch.max(m.max_radii2D[vis], radii[vis].float())
            grad = pkg["viewspace_points"].grad
            m.xyz_gradient_accum[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True)
            m.denom[vis] += 1

    fused_stats = lambda pkg: model_front.add_densification_stats(m, pkg)
    it_glue = lambda: iteration(glue_render, glue_stats)
    it_fused = lambda: iteration(model_front.render, fused_stats)
    t = time_pair([it_fused, it_glue], reps, rounds)
    say(f"| {config} eager: render, fused losses, backward, statistics | {t[0]:.4f} | {t[1]:.4f} | {launches(it_fused)} | {launches(it_glue)} |")
    if captured:
        steps = [CapturedStep(lambda: iteration(model_front.render, fused_stats)).capture(),
                 CapturedStep(lambda: iteration(model_front.render, None)).capture(),
                 CapturedStep(lambda: iteration(glue_render, None)).capture()]
        t = time_pair([s.replay for s in steps], reps, rounds)
        assert all(s.check() for s in steps)
        say(f"| {config} replayed: fused front end WITH statistics | {t[0]:.4f} | | | |")
        say(f"| {config} replayed: fused front end, no statistics | {t[1]:.4f} | | | |")
        say(f"| {config} replayed: reference glue, no statistics (its statistics cannot be captured) | | {t[2]:.4f} | | |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes and few repetitions: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "model_front_bench.py measures on the GPU: no GPU, no numbers"
    say(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say()
    if a.quick:
        stages(1000, 16, 3, 3)
        ulp_maxima(1000)
    else:
        stages(10_000, 16, 200, 7)
        stages(1_000_000, 16, 50, 7)
        ulp_maxima()
    say("### iterations (ms per iteration)")
    say("| iteration | fused front end ms | reference glue ms | fused launches | glue launches |")
    say("|---|---|---|---|---|")
    iterations("c1", 5 if a.quick else 100, 3 if a.quick else 7, captured=True)
    if not a.quick:
        iterations("c3", 10, 5, captured=False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
