"""Times the contribution pass (csrc/contrib.hip) on one frame against the route the package had before it.

    python tools/contrib_bench.py [--config c3] [--reps 50] [--warmup 10] [--out profiles/contrib.txt]

On the frame of bench.py's configuration (default c3: 1M Gaussians, 1080p, C = 32), one forward call, then - device events,
warm-up, median of `reps` - the pass with the per-pixel outputs only, with `acc` at K = 1 and K = 7 (no per-pixel outputs), with
both and with wmax; and, for the same `acc`, the earlier route: the product's forward with C = K + 1 feature channels holding
the masks' columns as upstream gradient plus its backward().  The blend backward ALONE (no preprocess backward, no zero fill)
is taken from the library's own stage events (option profile = 2) in the same process, for the frame itself (C channels) and
for the route's frames: a mean over `reps`, the one number here that is not a median.  Needs the GPU: there is no CPU path.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    for i in range(reps):
        evs[i].record()
        fn()
    evs[reps].record()
    torch.cuda.synchronize()
    t = [evs[i].elapsed_time(evs[i + 1]) for i in range(reps)]
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrib_bench needs a GPU: a timing taken anywhere else says nothing")
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    from synth import CONFIGS, make_scene

    dev = torch.device("cuda:0")
    cfg = dict(CONFIGS[args.config])
    sc = make_scene(seed=0, **cfg)
    P, C, W, H = sc["P"], sc["C"], sc["image_width"], sc["image_height"]
    t = lambda x: x.to(dev).contiguous()
    e = torch.Tensor([])
    base = dict(bg=t(sc["bg"]), means3D=t(sc["means3D"]), opacities=t(sc["opacities"]), shs=t(sc["shs"]), scales=t(sc["scales"]),
                rotations=t(sc["rotations"]), view=t(sc["viewmatrix"]), proj=t(sc["projmatrix"]), campos=t(sc["campos"]))

    def forward(feat):
        return _C.rasterize_gaussians(base["bg"], base["means3D"], e, feat, base["opacities"], base["scales"], base["rotations"], 1.0, e,
                                      base["view"], base["proj"], sc["tanfovx"], sc["tanfovy"], H, W, base["shs"], sc["sh_degree"],
                                      base["campos"], False, False)

    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    say(f"contribution pass, config {args.config}: P = {P}, {W} x {H}, C = {C}; {torch.cuda.get_device_name(0)}; "
        f"median of {args.reps} after {args.warmup} warm-up calls, device events (min .. max)")
    g = torch.Generator().manual_seed(1)
    masks = (torch.rand(7, H, W, generator=g) < 0.5).to(torch.float32).to(dev)
    feat_dev = t(sc["semantic_feature"])
    fwd = forward(feat_dev)
    n, _, _, _, radii, geom, binning, img = fwd
    state = (geom, binning, img, P, int(n), H, W)
    fwd_ms = median_ms(lambda: forward(feat_dev), args.reps, args.warmup)
    say(f"  forward call of the frame (C = {C})                    {fwd_ms[0]:8.3f} ms  ({fwd_ms[1]:.3f} .. {fwd_ms[2]:.3f})")
    acc = {k: torch.zeros(P, k + 1, device=dev) for k in (0, 1, 7)}
    wmax = torch.zeros(P, device=dev)
    legs = [("pass: per-pixel outputs only", lambda: _C.contributions(*state, None, None, None, True)),
            ("pass: acc, K = 0 (weight total)", lambda: _C.contributions(*state, None, acc[0], None, False)),
            ("pass: acc, K = 1", lambda: _C.contributions(*state, masks[:1], acc[1], None, False)),
            ("pass: acc, K = 7", lambda: _C.contributions(*state, masks, acc[7], None, False)),
            ("pass: acc K = 1 + per-pixel outputs", lambda: _C.contributions(*state, masks[:1], acc[1], None, True)),
            ("pass: acc K = 7 + per-pixel outputs + wmax", lambda: _C.contributions(*state, masks, acc[7], wmax, True))]
    res = {}
    for name, fn in legs:
        res[name] = median_ms(fn, args.reps, args.warmup)
        say(f"  {name:52s} {res[name][0]:8.3f} ms  ({res[name][1]:.3f} .. {res[name][2]:.3f})")

    # the blend backward alone, from the library's stage events
    def blend_backward_ms(feat, dfeat, reps):
        st = dgr.GaussianRasterizationSettings(H, W, sc["tanfovx"], sc["tanfovy"], base["bg"], 1.0, base["view"], base["proj"],
                                               sc["sh_degree"], base["campos"], False, False)
        leaves = dict(means3D=base["means3D"].clone().requires_grad_(True), means2D=torch.zeros(P, 3, device=dev, requires_grad=True),
                      opacities=base["opacities"].clone().requires_grad_(True), shs=base["shs"].clone().requires_grad_(True),
                      scales=base["scales"].clone().requires_grad_(True), rotations=base["rotations"].clone().requires_grad_(True),
                      semantic_feature=feat.clone().requires_grad_(True))

        def step():
            for v in leaves.values():
                v.grad = None
            _color, fmap, _radii, _depth = dgr.GaussianRasterizer(st)(**leaves)
            fmap.backward(dfeat)
        whole = median_ms(step, reps, args.warmup)
        _C.set_option("profile", 2)
        for _ in range(reps):        # creates the library's pooled events outside the measured pass
            step()
        _C.profile_read()
        _C.profile_reset()
        for _ in range(reps):
            step()
        torch.cuda.synchronize()
        prof = {name: (ms, calls) for name, ms, calls in _C.profile_read()}
        _C.set_option("profile", 0)
        ms, calls = prof["render_bwd"]
        return whole, ms / max(1, calls), _C.last_backward_contraction()

    hw = float(W * H)
    whole, blend_frame, contraction = blend_backward_ms(feat_dev, torch.randn(C, H, W, device=dev) / hw, args.reps)
    say(f"  frame (C = {C}): forward + backward()                 {whole[0]:8.3f} ms  ({whole[1]:.3f} .. {whole[2]:.3f})")
    say(f"  frame (C = {C}): blend backward alone (mean, contraction {contraction})  {blend_frame:8.3f} ms")
    route = {}
    for K in (1, 7):
        up = torch.cat([masks[:K], torch.ones(1, H, W, device=dev)])
        whole, blend, contraction = blend_backward_ms(torch.zeros(P, 1, K + 1, device=dev), up, args.reps)
        route[K] = (whole, blend)
        say(f"  earlier route, K = {K}: forward (C = {K + 1}) + backward()  {whole[0]:8.3f} ms  ({whole[1]:.3f} .. {whole[2]:.3f}); "
            f"its blend backward alone (mean, contraction {contraction}) {blend:.3f} ms")
    k1 = res["pass: acc, K = 1"][0]
    verdict = "less" if k1 < blend_frame else "NOT less"
    say(f"  condition: the pass at K = 1 ({k1:.3f} ms) takes {verdict} time than the blend backward alone of the frame ({blend_frame:.3f} ms); "
        f"of the K = 1 route's own frame: {route[1][1]:.3f} ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
