"""Times the neighbour search and the mode filter (csrc/neighbors.hip) against distCUDA2 and against the route torch offers.

    python tools/neighbors_bench.py [--points 1000000] [--torch-points 100000] [--reps 10] [--warmup 2]
                                    [--out profiles/neighbors_bench.md]

Two point sets of `--points` points: the clustered family of tests/test_knn.py (SfM-like clumps far from the origin) and the
means of a synth scene.  For K in {3, 8, 16}, median of `reps` calls, host clock from the call to the end of a device
synchronise, all in one process, the variants of one K interleaved round by round:
  knn       neighbors.knn with option knn_outward = 1 (leaves walked outward from the wave's own) and = 0 (in storage order)
  filter    one iteration of neighbors.mode_filter over those lists (21 labels, random weights)
  distCUDA2 the existing product on the same points: the same walk keeping three distances and no indices - the yardstick
  torch     the same lists and the same vote from torch operators - chunked cdist + topk, gather, one_hot vote - on the first
            `--torch-points` points (its time grows with the square of the count), beside the fused route on those points
and the peak of torch.cuda.max_memory_allocated above the inputs for both routes.  Needs the GPU.
"""
import argparse
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
    """{name: median ms} of `reps` rounds; every round runs every leg once"""
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


def torch_knn(pts, K, chunk):
    """(idx, dist2) from cdist + topk, chunk rows at a time (self excluded by index)"""
    P = pts.shape[0]
    idx = torch.empty(P, K, device=pts.device, dtype=torch.int64)
    d2 = torch.empty(P, K, device=pts.device)
    for a in range(0, P, chunk):
        d = torch.cdist(pts[a:a + chunk], pts).square_()
        rows = torch.arange(d.shape[0], device=pts.device)
        d[rows, rows + a] = float("inf")
        v, i = torch.topk(d, K, dim=1, largest=False)
        idx[a:a + chunk], d2[a:a + chunk] = i, v
    return idx, d2


def torch_vote(labels, weight, idx, L):
    """one filter step from torch operators: gather, one_hot, weighted sum, argmax (ties go to the lowest label)"""
    voters = torch.cat([torch.arange(idx.shape[0], device=idx.device)[:, None], idx], 1)
    lab, w = labels[voters], weight[voters]
    score = (torch.nn.functional.one_hot(lab.clamp_min(0), L).to(torch.float32) * (w * (lab >= 0))[..., None]).sum(1)
    top, win = score.max(1)
    return torch.where(top > 0, win, torch.full_like(win, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--torch-points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neighbors_bench needs a GPU: a timing taken anywhere else says nothing")
    import neighbors
    from diff_gaussian_rasterization import _C as raster
    from simple_knn._C import distCUDA2
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
    say(f"# Neighbour search and mode filter: {torch.cuda.get_device_name(0)}")
    say()
    say(f"P = {P} points; median of {args.reps} calls after {args.warmup} warm-up calls, host clock to the end of a device "
        f"synchronise (min .. max), the legs of one K interleaved in one process.  `outward` / `in order`: option knn_outward 1 / 0.")
    ratios = {}
    for name, pts in sets.items():
        say()
        say(f"## {name}")
        say()
        say("| K | knn, outward (ms) | knn, in order (ms) | one filter step (ms) | distCUDA2 (ms) | knn outward / distCUDA2 |")
        say("|---|---|---|---|---|---|")
        for K in (3, 8, 16):
            raster.set_option("knn_outward", 1)
            idx, d2 = neighbors.knn(pts, K)

            def knn_with(v):
                raster.set_option("knn_outward", v)
                neighbors.knn(pts, K)

            legs = {"out": lambda: knn_with(1), "in": lambda: knn_with(0),
                    "filter": lambda: neighbors.mode_filter(labels, idx, weight=weight),
                    "dist": lambda: distCUDA2(pts)}
            r = interleaved(legs, args.reps, args.warmup)
            raster.set_option("knn_outward", 1)
            f = lambda k: f"{r[k][0]:.2f} ({r[k][1]:.2f} .. {r[k][2]:.2f})"
            ratios[(name, K)] = (r["out"][0] / r["dist"][0], r["in"][0] / r["dist"][0])
            say(f"| {K} | {f('out')} | {f('in')} | {f('filter')} | {f('dist')} | {ratios[(name, K)][0]:.2f} |")
            del idx, d2
    say()
    say(f"## The torch route, on the first {Pt} points of each set")
    say()
    say("cdist + topk in chunks of 2048 rows, then gather + one_hot + sum + argmax for the vote; 3 calls, median.  Peak memory above "
        "the inputs (torch.cuda.max_memory_allocated), outputs included.")
    say()
    say("| set | K | fused knn (ms) | torch knn (ms) | fused filter (ms) | torch vote (ms) | fused peak (MiB) | torch peak (MiB) | same lists |")
    say("|---|---|---|---|---|---|---|---|---|")
    for name, full in sets.items():
        pts = full[:Pt].contiguous()
        lab, w = labels[:Pt].contiguous(), weight[:Pt].contiguous()
        for K in (3, 8, 16):
            idx, d2 = neighbors.knn(pts, K)
            tidx, td2 = torch_knn(pts, K, 2048)
            same = float((idx.long() == tidx).all(1).float().mean())
            r = interleaved({"knn": lambda: neighbors.knn(pts, K), "tknn": lambda: torch_knn(pts, K, 2048),
                             "filter": lambda: neighbors.mode_filter(lab, idx, weight=w),
                             "tvote": lambda: torch_vote(lab, w, tidx, L)}, 3, 1)
            del tidx, td2
            fused_mb, _ = peak_mb(lambda: neighbors.mode_filter(lab, neighbors.knn(pts, K)[0], weight=w))
            torch_mb, _ = peak_mb(lambda: torch_vote(lab, w, torch_knn(pts, K, 2048)[0], L))
            say(f"| {name} | {K} | {r['knn'][0]:.2f} | {r['tknn'][0]:.1f} | {r['filter'][0]:.3f} | {r['tvote'][0]:.2f} | {fused_mb:.1f} | "
                f"{torch_mb:.1f} | {same:.1%} of the rows |")
    say()
    k3 = [ratios[(n, 3)][0] for n in sets]
    say(f"K = 3 against distCUDA2 (the same walk, three distances, no indices): {', '.join(f'{v:.2f} x' for v in k3)} "
        f"({', '.join(sets)}).")
    better = sum(ratios[k][0] < ratios[k][1] for k in ratios)
    say(f"Walk order: the outward walk is the faster one in {better} of {len(ratios)} (set, K) pairs; at K = 16 it takes "
        + ", ".join(f"{ratios[(n, 16)][0] / ratios[(n, 16)][1]:.2f} x" for n in sets) + f" the time of the in-order walk ({', '.join(sets)}).")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
