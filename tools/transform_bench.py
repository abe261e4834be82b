"""Times the object transforms (csrc/transform.hip) against a torch route to the same numbers and against a plain device copy of
the same bytes.

    python tools/transform_bench.py [--points 1000000] [--reps 10] [--warmup 2] [--out profiles/transform_bench.md]

A model of P Gaussians at SH degree 3: xyz, rotations, log-scales and the (P, 15, 3) higher-order coefficients, 220 bytes a
Gaussian.  G in {1, 300, 4096} groups with a random similarity transform each; the ids `random` (uniform) or `coherent` (runs of
equal ids in storage, as split_labels or an InstanceLifter leave them); one id in ten outside [0, G).  Median of `reps` calls, host
clock from the call to the end of a device synchronise, the legs of one row interleaved round by round:
  in place   simple_knn._C.transform_gaussians into the inputs (the table kernel and the scratch allocation inside)
  new        the same into new tensors
  gather     the gather form over a random tenth of the rows
  torch      the table of the judge (tests/transform_oracle.py: built on the host beforehand, not timed) gathered per Gaussian -
             (P, 3, 3), (P, 5, 5) and (P, 7, 7) matrices in fp64 -, bmm band by band, torch.where for the rows that stay: the same
             numbers, into new tensors; its peak memory
  copy       clone() of the four tensors: the same bytes read and written once
Needs the GPU.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from neighbors_bench import interleaved, peak_mb      # noqa: E402


def judge_table(quat, scale, trans, pivot, dev):
    """the per-group fp64 tensors of the torch route, from the judge's own formulas"""
    import transform_oracle as to
    G = len(scale)
    R = np.stack([to.quat_to_rot(q) for q in quat.astype(np.float64)])
    D = [np.stack([to.sh_matrices(R[k])[l] for k in range(G)]) for l in range(3)]
    qn = quat.astype(np.float64)
    qn /= np.sqrt((qn * qn).sum(1, keepdims=True))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    s = scale.astype(np.float64)
    return dict(A=t(s[:, None, None] * R), p=t(pivot), shift=t(pivot.astype(np.float64) + trans), qn=t(qn), logs=t(np.log(s)), D=[t(d) for d in D])


def torch_route(ids, G, tab, xyz, rot, scales, rest):
    ok = (ids >= 0) & (ids < G)
    g = torch.where(ok, ids, torch.zeros_like(ids)).long()
    x = torch.bmm(tab["A"][g], (xyz.double() - tab["p"][g])[:, :, None])[:, :, 0] + tab["shift"][g]
    a, b = tab["qn"][g].unbind(1), rot.double().unbind(1)
    q = torch.stack([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]], 1)
    s = scales.double() + tab["logs"][g][:, None]
    c = rest.double()
    bands = torch.cat([torch.bmm(tab["D"][l][g], c[:, lo:hi, :]) for l, (lo, hi) in enumerate(((0, 3), (3, 8), (8, 15)))], 1)
    return (torch.where(ok[:, None], x.float(), xyz), torch.where(ok[:, None], q.float(), rot), torch.where(ok[:, None], s.float(), scales),
            torch.where(ok[:, None, None], bands.float(), rest))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transform_bench needs a GPU: a timing taken anywhere else says nothing")
    from simple_knn import _C

    dev = torch.device("cuda:0")
    P = args.points
    gen = torch.Generator(device=dev).manual_seed(1)
    xyz0 = torch.randn(P, 3, device=dev, generator=gen) * 3 + torch.tensor([50.0, -20.0, 7.0], device=dev)
    rot0 = torch.randn(P, 4, device=dev, generator=gen)
    scales0 = torch.rand(P, 3, device=dev, generator=gen) * 4 - 5
    rest0 = torch.randn(P, 15, 3, device=dev, generator=gen) * 0.3
    nbytes = P * (3 + 4 + 3 + 45) * 4
    rows = torch.randperm(P, device=dev, generator=gen)[:P // 10].to(torch.int32)
    lines = []
    say = lambda s="": (print(s, flush=True), lines.append(s))
    say(f"# Object transforms: {torch.cuda.get_device_name(0)}")
    say()
    say(f"P = {P} Gaussians at SH degree 3 ({nbytes / 1e6:.0f} MB of xyz, rotations, log-scales and 45 SH coefficients); median of {args.reps} "
        f"calls after {args.warmup} warm-up calls, host clock to the end of a device synchronise, the legs of one row interleaved in one "
        f"process.  Times in ms.  `GB/s`: bytes read plus bytes written by `in place` (nine tenths of the rows move) over its time.  "
        f"`x copy`: `new` over `copy`; `x torch`: `torch` over `new`.")
    say()
    say("| G | ids | in place | new | gather 10 % | torch | copy | GB/s in place | x copy | x torch | torch peak MiB | hip peak MiB | worst difference to torch |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    slower = []
    rng = np.random.default_rng(3)
    for G in (1, 300, 4096):
        quat = rng.normal(0, 1, (G, 4)).astype(np.float32)
        scale = np.exp(rng.uniform(-0.1, 0.1, G)).astype(np.float32)
        trans = rng.normal(0, 1, (G, 3)).astype(np.float32)
        pivot = (rng.normal(0, 3, (G, 3)) + [50.0, -20.0, 7.0]).astype(np.float32)
        tab = judge_table(quat, scale, trans, pivot, dev)
        t_quat, t_scale, t_trans, t_pivot = [torch.from_numpy(a).to(dev) for a in (quat, scale, trans, pivot)]
        for kind in ("random", "coherent"):
            if G == 1 and kind == "coherent":
                continue
            ids = torch.randint(0, G, (P,), device=dev, generator=gen) if kind == "random" else (torch.arange(P, device=dev) * G // P)
            ids = torch.where(torch.rand(P, device=dev, generator=gen) < 0.1, torch.full_like(ids, -1), ids).to(torch.int32)
            work = [t.clone() for t in (xyz0, rot0, scales0, rest0)]              # the in-place leg's own tensors
            call = lambda tensors, r, inplace: _C.transform_gaussians(ids, t_quat, t_scale, t_trans, t_pivot, tensors[0], tensors[1], tensors[2],
                                                                      False, None, tensors[3], r, inplace)
            src = (xyz0, rot0, scales0, rest0)
            legs = {"inplace": lambda: call(work, None, True), "new": lambda: call(src, None, False), "gather": lambda: call(src, rows, False),
                    "torch": lambda: torch_route(ids, G, tab, *src), "copy": lambda: [t.clone() for t in src]}
            r = interleaved(legs, args.reps, args.warmup)
            peak_t, ref = peak_mb(legs["torch"])
            peak_h, got = peak_mb(legs["new"])
            worst = max(float((a.double() - b.double()).abs().max()) for a, b in zip((got[0], got[1], got[2], got[4]), ref))
            gbs = (nbytes + 0.9 * nbytes) / (r["inplace"][0] * 1e-3) / 1e9
            if r["torch"][0] < r["new"][0]:
                slower.append(f"G = {G}, {kind}")
            say(f"| {G} | {kind} | {r['inplace'][0]:.3f} | {r['new'][0]:.3f} | {r['gather'][0]:.3f} | {r['torch'][0]:.3f} | {r['copy'][0]:.3f} | "
                f"{gbs:.0f} | {r['new'][0] / r['copy'][0]:.2f} | {r['torch'][0] / r['new'][0]:.1f} | {peak_t:.0f} | {peak_h:.0f} | {worst:.2e} |")
            del ids, work, ref, got
    say()
    say("Rows slower than the torch route: " + ("; ".join(slower) if slower else "none") + ".")
    say()
    say("Not measured: the two kernels one by one (the table kernel is inside every hip leg); hardware counters; SH degrees below 3; "
        "cov3d; the strided (P, 16, 3) layout; point counts other than the one above; G above 4096; the torch route's own table "
        "(built on the host, outside the clock).")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
