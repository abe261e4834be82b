"""Times the label vote (csrc/contrib.hip: label_votes_kernel) on one frame against the route the package had before it.

    python tools/label_votes_bench.py [--config c3] [--classes 150] [--reps 50] [--warmup 10] [--out profiles/label_votes.txt]

On the frame of bench.py's configuration (default c3: 1M Gaussians, 1080p), one forward call, then - device events, warm-up,
median of `reps`, all in one process - over that call's state:
  (a) the vote for a piecewise label map: every pixel takes the class of the nearest of about 200 random seeds;
  (b) the vote for the noise map, uniform integers in [-1, L]: the stated worst case (up to 57 classes in a quadrant);
  (c) one walk of the contribution pass with K = 7 masks and no per-pixel outputs;
  (d) the grouped route for map (a): MaskLifter.from_label_map and ceil(L / 7) walks, as contrib.contributions takes them.
The peak of torch.cuda.max_memory_allocated above the inputs is recorded for (a) and (d), and the two results are compared at
this size.  Needs the GPU: there is no CPU path.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from contrib_bench import median_ms  # noqa: E402


def piecewise_map(H, W, L, seeds, dev, seed=2):
    """(H, W) int64: the class of the nearest of `seeds` random points, classes drawn from [0, L)."""
    g = torch.Generator().manual_seed(seed)
    sy, sx = (torch.rand(seeds, generator=g) * H).to(dev), (torch.rand(seeds, generator=g) * W).to(dev)
    cls = torch.randint(0, L, (seeds,), generator=g).to(dev)
    y, x = torch.arange(H, device=dev, dtype=torch.float32)[:, None], torch.arange(W, device=dev, dtype=torch.float32)[None]
    best = torch.full((H, W), float("inf"), device=dev)
    lab = torch.zeros(H, W, dtype=torch.int64, device=dev)
    for i in range(seeds):
        d = (y - sy[i]) ** 2 + (x - sx[i]) ** 2
        nearer = d < best
        best = torch.where(nearer, d, best)
        lab = torch.where(nearer, cls[i], lab)
    return lab


def distinct_per_quadrant(lab, L):
    """(mean, max) number of distinct valid classes over the 8 x 8 quadrants of a map whose sides are multiples of 8."""
    H, W = lab.shape
    q = lab[:H // 8 * 8, :W // 8 * 8].reshape(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64)
    q = torch.where((q >= 0) & (q < L), q, torch.full_like(q, -1)).sort(dim=1)[0]
    n = ((q[:, 1:] != q[:, :-1]) & (q[:, 1:] >= 0)).sum(1) + (q[:, 0] >= 0)
    return float(n.float().mean()), int(n.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--classes", type=int, default=150)
    ap.add_argument("--seeds", type=int, default=200)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("label_votes_bench needs a GPU: a timing taken anywhere else says nothing")
    import contrib
    from diff_gaussian_rasterization import _C
    from synth import CONFIGS, make_scene

    dev = torch.device("cuda:0")
    sc = make_scene(seed=0, **dict(CONFIGS[args.config]))
    P, W, H, L = sc["P"], sc["image_width"], sc["image_height"], args.classes
    t = lambda x: x.to(dev).contiguous()
    e = torch.Tensor([])
    n, _, _, _, _, geom, binning, img = _C.rasterize_gaussians(
        t(sc["bg"]), t(sc["means3D"]), e, t(sc["semantic_feature"]), t(sc["opacities"]), t(sc["scales"]), t(sc["rotations"]), 1.0, e,
        t(sc["viewmatrix"]), t(sc["projmatrix"]), sc["tanfovx"], sc["tanfovy"], H, W, t(sc["shs"]), sc["sh_degree"], t(sc["campos"]), False,
        False)
    state = (geom, binning, img, P, int(n), H, W)

    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    say(f"label vote, config {args.config}: P = {P}, {W} x {H}, L = {L}; {torch.cuda.get_device_name(0)}; "
        f"median of {args.reps} after {args.warmup} warm-up calls, device events (min .. max)")
    g = torch.Generator().manual_seed(1)
    maps = {"a": piecewise_map(H, W, L, args.seeds, dev), "b": torch.randint(-1, L + 1, (H, W), generator=g).to(dev)}
    masks7 = (torch.rand(7, H, W, generator=g) < 0.5).to(torch.float32).to(dev)
    acc = torch.zeros(P, L + 1, device=dev)
    acc7 = torch.zeros(P, 8, device=dev)

    def grouped(lab, out):
        """contrib.contributions' loop over groups of seven masks, on the state of the one forward call"""
        masks = contrib.MaskLifter.from_label_map(lab, L)
        for k0 in range(0, L, contrib.MAX_MASKS):
            k1 = min(L, k0 + contrib.MAX_MASKS)
            part = torch.zeros(P, k1 - k0 + 1, device=dev)
            _C.contributions(*state, masks[k0:k1], part, None, False)
            out[:, k0:k1] += part[:, :-1]
            if k0 == 0:
                out[:, L] += part[:, -1]

    def peak_mb(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - before) / 2 ** 20

    res = {}
    legs = [("a", "(a) vote, piecewise map", lambda: _C.label_votes(*state, maps["a"], L, acc)),
            ("b", "(b) vote, noise map", lambda: _C.label_votes(*state, maps["b"], L, acc)),
            ("c", "(c) contribution pass, K = 7, acc only", lambda: _C.contributions(*state, masks7, acc7, None, False)),
            ("d", f"(d) grouped route for (a): one-hot + {-(-L // 7)} walks", lambda: grouped(maps["a"], acc))]
    if L <= 255:
        a_u8 = maps["a"].to(torch.uint8)
        legs.insert(1, ("a8", "(a) vote, the same map as uint8", lambda: _C.label_votes(*state, a_u8, L, acc)))
    for key, name, fn in legs:
        r = res[key] = median_ms(fn, args.reps, args.warmup)
        say(f"  {name:52s} {r[0]:8.3f} ms  ({r[1]:.3f} .. {r[2]:.3f})")
    for k in ("a", "b"):
        mean, mx = distinct_per_quadrant(maps[k], L)
        say(f"  map ({k}): {mean:.2f} distinct valid classes per 8 x 8 quadrant on average, {mx} at most")
    new_mb = peak_mb(lambda: _C.label_votes(*state, maps["a"], L, acc))
    old_mb = peak_mb(lambda: grouped(maps["a"], acc))
    say(f"  peak memory above the inputs (label map and acc, {acc.numel() * 4 / 2 ** 20:.0f} MiB, included in them): "
        f"(a) {new_mb:.1f} MiB, (d) {old_mb:.1f} MiB")
    # the two routes' results at this size
    one, many = torch.zeros_like(acc), torch.zeros_like(acc)
    _C.label_votes(*state, maps["a"], L, one)
    grouped(maps["a"], many)
    torch.cuda.synchronize()
    scale = float(many.abs().max())
    err = (one - many).abs()
    worst = float((err / (1e-3 * many.abs() + 1e-5 * scale)).max())
    say(f"  (a) against (d): max |difference| / max|acc| = {float(err.max()) / scale:.2e}, worst element {worst:.3f} x the bar "
        f"1e-3 |g| + 1e-5 max|g|")
    a, c, d = res["a"][0], res["c"][0], res["d"][0]
    say(f"  ratios: (a) / (c) = {a / c:.2f}, (b) / (c) = {res['b'][0] / c:.2f}, (d) / (a) = {d / a:.1f}")
    ok = a < d and new_mb < old_mb
    say(f"  condition: the vote on (a) takes {'less' if a < d else 'NOT less'} time ({a:.3f} ms against {d:.3f} ms) and "
        f"{'less' if new_mb < old_mb else 'NOT less'} peak memory than the grouped route: {'met' if ok else 'NOT met'}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
