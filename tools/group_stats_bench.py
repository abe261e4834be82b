"""Times the per-group statistics and the group merge (csrc/group_stats.hip) against the torch route to the same numbers and
against a plain read of the inputs.

    python tools/group_stats_bench.py [--points 1000000] [--reps 10] [--warmup 2] [--out profiles/group_stats_bench.md]

The clustered point set of tools/neighbors_bench.py, stored cell by cell of a coarse grid (a model after a spatial sort); no weights;
C in {0, 32, 128} feature channels; G in {1, 300, 4096} groups; the ids `random` (uniform, nothing to do with the place) or `coherent`
(the nearest of G random centres: runs of equal ids in storage, as split_labels or an InstanceLifter leave them).  Median of `reps`
calls, host clock from the call to the end of a device synchronise, the legs of one row interleaved round by round:
  hip        simple_knn._C.group_stats, every output (outputs and scratch allocated inside)
  no cov     the same without cov: no second pass
  torch      bincount, index_add_ in fp64, scatter_reduce amin / amax, the centred second pass: the same numbers; its peak memory
  read       the time a plain read of the inputs would take at 6.29 TB/s (the float4 copy rate measured on this device): ids, xyz
             and the feature rows once, ids and xyz once more for the second pass
and merge_similar's native call at K in {3, 16} on 300 and 4096 coherent instances with 32-channel means.  Needs the GPU.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from neighbors_bench import clustered, interleaved, peak_mb      # noqa: E402

INF = float("inf")
READ_TBS = 6.29


def torch_route(ids, xyz, G, feats):
    """(count, mass, centroid, cov6, lo, hi, feature_mean) by torch ops, every sum in fp64"""
    ok = (ids >= 0) & (ids < G) & torch.isfinite(xyz).all(1)
    g = torch.where(ok, ids, torch.full_like(ids, G)).long()
    count = torch.bincount(g, minlength=G + 1)[:G]
    m = count.double().clamp_min(1)
    x64 = xyz.double()
    c = torch.zeros(G + 1, 3, device=xyz.device, dtype=torch.float64).index_add_(0, g, x64)[:G] / m[:, None]
    gi = g[:, None].expand(-1, 3)
    lo = torch.full((G + 1, 3), INF, device=xyz.device).scatter_reduce_(0, gi, xyz, "amin")[:G]
    hi = torch.full((G + 1, 3), -INF, device=xyz.device).scatter_reduce_(0, gi, xyz, "amax")[:G]
    d = x64 - torch.cat([c, c.new_zeros(1, 3)])[g]
    prod = torch.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
    cov = torch.zeros(G + 1, 6, device=xyz.device, dtype=torch.float64).index_add_(0, g, prod)[:G] / m[:, None]
    fm = None
    if feats is not None:
        fm = torch.zeros(G + 1, feats.shape[1], device=xyz.device, dtype=torch.float64).index_add_(0, g, feats.double())[:G] / m[:, None]
        fm = fm.float()
    return count, count.float(), c.float(), cov.float(), lo, hi, fm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_stats_bench needs a GPU: a timing taken anywhere else says nothing")
    import neighbors
    from simple_knn import _C

    dev = torch.device("cuda:0")
    P = args.points
    pts = clustered(P, 21)
    cell = np.floor((pts - pts.min(0)) / 0.5).astype(np.int64)
    pts = pts[np.lexsort((cell[:, 2], cell[:, 1], cell[:, 0]))]
    xyz = torch.from_numpy(pts).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    everything = _C.GROUP_COUNT | _C.GROUP_MASS | _C.GROUP_CENTROID | _C.GROUP_COV | _C.GROUP_AABB

    def coherent(G):
        centres = xyz[torch.randint(0, P, (G,), device=dev, generator=gen)]
        return torch.cat([torch.cdist(xyz[a:a + 65536], centres).argmin(1) for a in range(0, P, 65536)]).to(torch.int32)

    lines = []
    say = lambda s="": (print(s, flush=True), lines.append(s))
    say(f"# Per-group statistics and the group merge: {torch.cuda.get_device_name(0)}")
    say()
    say(f"P = {P} points; median of {args.reps} calls after {args.warmup} warm-up calls, host clock to the end of a device synchronise, "
        f"the legs of one row interleaved in one process.  Times in ms.  `read`: the inputs once (ids and xyz twice: the second pass) at "
        f"{READ_TBS} TB/s.  `x torch`: the torch route over `hip`.")
    say()
    say("| C | G | ids | hip | no cov | torch | x torch | torch peak MiB | hip peak MiB | read | worst difference to torch |")
    say("|---|---|---|---|---|---|---|---|---|---|---|")
    slower = []
    for C in (0, 32, 128):
        feats = torch.randn(P, C, device=dev, generator=gen) if C else None
        for G in (1, 300, 4096):
            for kind in ("random", "coherent"):
                if G == 1 and kind == "coherent":
                    continue
                ids = torch.randint(0, G, (P,), device=dev, generator=gen).to(torch.int32) if kind == "random" else coherent(G)
                want = everything | (_C.GROUP_FEATURE_MEAN if C else 0)
                legs = {"hip": lambda: _C.group_stats(ids, xyz, G, None, feats, want),
                        "nocov": lambda: _C.group_stats(ids, xyz, G, None, feats, want & ~_C.GROUP_COV),
                        "torch": lambda: torch_route(ids, xyz, G, feats)}
                r = interleaved(legs, args.reps, args.warmup)
                peak_t, ref = peak_mb(legs["torch"])
                peak_h, got = peak_mb(legs["hip"])
                aabb = torch.cat([ref[4], ref[5]], 1)
                pairs = [(got[0].long(), ref[0]), (got[1], ref[1]), (got[2], ref[2]), (got[3], ref[3]), (got[4], aabb)]
                if C:
                    pairs.append((got[5], ref[6]))
                worst = max(float((a.double() - b.double()).abs().nan_to_num(0.0).max()) for a, b in pairs)
                read_ms = P * (2 * (4 + 12) + 4 * C) / (READ_TBS * 1e12) * 1e3
                ratio = r["torch"][0] / r["hip"][0]
                if ratio < 1:
                    slower.append(f"C = {C}, G = {G}, {kind}")
                say(f"| {C} | {G} | {kind} | {r['hip'][0]:.3f} | {r['nocov'][0]:.3f} | {r['torch'][0]:.3f} | {ratio:.1f} | {peak_t:.0f} | "
                    f"{peak_h:.0f} | {read_ms:.3f} | {worst:.2e} |")
                del ids, ref, got
        del feats
    say()
    say("Rows slower than the torch route: " + ("; ".join(slower) if slower else "none") + ".")
    say()
    say("## merge_similar")
    say()
    say("The native call (group_merge: adjacency, unite, flatten, gather) on coherent instances, 32-channel means, min_cos 0.9, no max_dist.")
    say()
    say("| K | G | merge | roots left | status |")
    say("|---|---|---|---|---|")
    for K in (3, 16):
        idx, _ = neighbors.knn(xyz, K, return_dist2=False)
        for G in (300, 4096):
            ids = coherent(G)
            fm = torch.randn(G, 32, device=dev, generator=gen) + 2.0
            r = interleaved({"merge": lambda: _C.group_merge(ids, idx, None, INF, False, fm, 0.9, None)}, args.reps, args.warmup)
            out, root, status = _C.group_merge(ids, idx, None, INF, False, fm, 0.9, None)
            say(f"| {K} | {G} | {r['merge'][0]:.3f} | {int((root == torch.arange(G, device=dev)).sum())} | {int(status)} |")
        del idx
    say()
    say("Not measured: the kernels one by one (the second pass is the difference of `hip` and `no cov`); hardware counters; weights; "
        "strided or misaligned feature rows (the scalar loads); point counts other than the one above; G above 4096; a privatised "
        "LDS table in the place of the runs.")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
