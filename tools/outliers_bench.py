"""Times the density kernels (csrc/outliers.hip) against the neighbour search, one mode-filter step and the route torch offers.

    python tools/outliers_bench.py [--points 1000000] [--torch-points 100000] [--reps 10] [--warmup 2]
                                   [--out profiles/outliers_bench.md]

Two point sets of `--points` points: the clustered family of tests/test_knn.py (SfM-like clumps far from the origin) and the
means of a synth scene.  Median of `reps` calls, host clock from the call to the end of a device synchronise, all in one process,
the legs of one table interleaved round by round:
  radius_count   at the radius where the mean count is about 8 (found by bisection on the device), with cap none, 1 and 8, and
                 with 21 labels; beside it neighbors.knn at K = 8 and K = 16 on the same points - the search that answers the
                 same question through its K-th distance - the yardstick
  outlier_scores at K = 3, 8, 16 over knn's lists, beside one iteration of neighbors.mode_filter on the same lists: that step
                 reads the lists once and is the floor
  torch          the same counts from chunked cdist on the first `--torch-points` points (its time grows with the square of the
                 count), beside the fused route on those points, with the peak of torch.cuda.max_memory_allocated above the inputs
Needs the GPU.
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def clustered(P, seed):
    g = np.random.default_rng(seed)
    c = g.normal(0, 4, (max(1, P // 500), 3))
    return (c[g.integers(0, len(c), P)] + g.normal(0, 0.05, (P, 3)) + np.array([50.0, -20.0, 7.0])).astype(np.float32)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def interleaved(legs, reps, warmup):
    """{name: (median, min, max) ms} of `reps` rounds; every round runs every leg once"""
    for _ in range(warmup):
        for fn in legs.values():
            wall_ms(fn)
    t = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t[k].append(wall_ms(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20, out


def radius_of_mean_count(neighbors, pts, target):
    """bisection between half and twice the median distance to the `target`-th neighbour"""
    _, d2 = neighbors.knn(pts, target)
    mid = float(d2[:, target - 1].sqrt().median())
    lo, hi = 0.5 * mid, 2.0 * mid
    for _ in range(14):
        r = math.sqrt(lo * hi)
        mean = float(neighbors.radius_count(pts, r).float().mean())
        lo, hi = (r, hi) if mean < target else (lo, r)
    r = math.sqrt(lo * hi)
    return r, float(neighbors.radius_count(pts, r).float().mean())


def torch_count(pts, radius, chunk):
    """the counts from cdist, chunk rows at a time (self excluded by index)"""
    P = pts.shape[0]
    out = torch.empty(P, device=pts.device, dtype=torch.int32)
    r = torch.tensor(radius, dtype=torch.float32)
    r2 = float(r * r)
    for a in range(0, P, chunk):
        d = torch.cdist(pts[a:a + chunk], pts).square_()
        rows = torch.arange(d.shape[0], device=pts.device)
        d[rows, rows + a] = float("inf")
        out[a:a + chunk] = (d <= r2).sum(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--torch-points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("outliers_bench needs a GPU: a timing taken anywhere else says nothing")
    import neighbors
    from synth import make_scene

    dev = torch.device("cuda:0")
    P, Pt, L = args.points, min(args.torch_points, args.points), 21
    sets = {"clustered": torch.from_numpy(clustered(P, 21)).to(dev),
            "synth": make_scene(P=P, C=0, width=64, height=64, seed=3)["means3D"].to(dev).contiguous()}
    g = torch.Generator(device=dev).manual_seed(0)
    labels = torch.randint(-1, L, (P,), device=dev, generator=g)
    weight = torch.rand(P, device=dev, generator=g)
    lines = []
    say = lambda s="": (print(s, flush=True), lines.append(s))
    f = lambda v: f"{v[0]:.2f} ({v[1]:.2f} .. {v[2]:.2f})"
    say(f"# Radius counts and statistical outlier scores: {torch.cuda.get_device_name(0)}")
    say()
    say(f"P = {P} points; median of {args.reps} calls after {args.warmup} warm-up calls, host clock to the end of a device "
        f"synchronise (min .. max), the legs of one table row interleaved in one process.")
    say()
    say("## radius_count at a mean count of about 8, beside the search")
    say()
    say("| set | radius | mean count | no cap (ms) | cap 1 (ms) | cap 8 (ms) | 21 labels, no cap (ms) | knn K = 8 (ms) | knn K = 16 (ms) | "
        "no cap / knn 8 | no cap / knn 16 | cap 8 / knn 8 |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|")
    radii, verdict = {}, []
    for name, pts in sets.items():
        radius, mean = radius_of_mean_count(neighbors, pts, 8)
        radii[name] = radius
        r = interleaved({"none": lambda: neighbors.radius_count(pts, radius),
                         "cap1": lambda: neighbors.radius_count(pts, radius, cap=1),
                         "cap8": lambda: neighbors.radius_count(pts, radius, cap=8),
                         "labels": lambda: neighbors.radius_count(pts, radius, labels=labels),
                         "knn8": lambda: neighbors.knn(pts, 8), "knn16": lambda: neighbors.knn(pts, 16)}, args.reps, args.warmup)
        say(f"| {name} | {radius:.5g} | {mean:.2f} | {f(r['none'])} | {f(r['cap1'])} | {f(r['cap8'])} | {f(r['labels'])} | {f(r['knn8'])} | "
            f"{f(r['knn16'])} | {r['none'][0] / r['knn8'][0]:.2f} | {r['none'][0] / r['knn16'][0]:.2f} | {r['cap8'][0] / r['knn8'][0]:.2f} |")
        verdict.append((name, r["none"][0], r["knn16"][0]))
    say()
    for name, rc, knn16 in verdict:
        say(f"{name}: radius_count without a cap at mean count 8 costs {'MORE' if rc > knn16 else 'less'} than knn at K = 16 "
            f"({rc:.2f} against {knn16:.2f} ms).")
    say()
    say("## outlier_scores beside one mode-filter step on the same lists")
    say()
    say("| set | K | outlier_scores (ms) | with 21 labels (ms) | one filter step (ms) | scores / filter step |")
    say("|---|---|---|---|---|---|")
    for name, pts in sets.items():
        for K in (3, 8, 16):
            idx, d2 = neighbors.knn(pts, K)
            r = interleaved({"scores": lambda: neighbors.outlier_scores(idx, d2),
                             "labelled": lambda: neighbors.outlier_scores(idx, d2, labels=labels, num_labels=L),
                             "filter": lambda: neighbors.mode_filter(labels, idx, weight=weight)}, args.reps, args.warmup)
            say(f"| {name} | {K} | {f(r['scores'])} | {f(r['labelled'])} | {f(r['filter'])} | {r['scores'][0] / r['filter'][0]:.2f} |")
            del idx, d2
    say()
    say(f"## The torch route, on the first {Pt} points of each set")
    say()
    say("cdist in chunks of 2048 rows, a comparison and a row sum; 3 calls, median.  The radius is the full set's times the cube root of the thinning "
        "(about the same mean count).  Peak memory above the inputs (torch.cuda.max_memory_allocated), outputs included.")
    say()
    say("| set | fused count (ms) | torch count (ms) | torch / fused | fused peak (MiB) | torch peak (MiB) | same counts |")
    say("|---|---|---|---|---|---|---|")
    for name, full in sets.items():
        pts = full[:Pt].contiguous()
        radius = radii[name] * (P / Pt) ** (1 / 3)          # the same mean count on a thinner cloud, roughly
        same = float((neighbors.radius_count(pts, radius) == torch_count(pts, radius, 2048)).float().mean())
        r = interleaved({"fused": lambda: neighbors.radius_count(pts, radius), "torch": lambda: torch_count(pts, radius, 2048)}, 3, 1)
        fused_mb, _ = peak_mb(lambda: neighbors.radius_count(pts, radius))
        torch_mb, _ = peak_mb(lambda: torch_count(pts, radius, 2048))
        say(f"| {name} | {r['fused'][0]:.2f} | {r['torch'][0]:.1f} | {r['torch'][0] / r['fused'][0]:.0f} | {fused_mb:.1f} | {torch_mb:.1f} | "
            f"{same:.2%} of the points |")
    say()
    say("Not measured: P other than the one above, radii of other mean counts (the cost of an uncapped count grows with the count), "
        "K-d tree routes on the host, the kernels alone under a profiler (every figure includes the search's front end - the sort and "
        "the gather - and the Python layer), more than one device.")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
