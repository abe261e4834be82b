"""Times the feature codebooks (csrc/codebook.hip) against the torch route to the same codes, against the fp32 matrix floor and
against a plain read of the inputs.

    python tools/codebook_bench.py [--points 1000000] [--reps 5] [--torch-reps 2] [--warmup 1] [--out profiles/codebook_bench.md]

Features: P rows around 64 random centres (sigma 1 around centres of sigma 2), C in {32, 128} channels; centroids: K in {16, 256,
4096} rows of the features.  Median of `reps` calls, host clock from the call to the end of a device synchronise, the legs of one
row interleaved round by round:
  assign     simple_knn._C.codebook_assign, codes only (output and workspace allocated inside): prepare + the MFMA kernel
  +dist2     the same with dist2 and inertia: the fp64 pass over the winners on top
  update     simple_knn._C.codebook_update on those codes (scratch allocated inside)
  kmeans     codebook.kmeans(iterations=10) from those centroids: 10 x (assign with inertia and moved, update) and a closing assign
  t.assign   torch: |c|^2 - 2 x c^T by `mm` and argmin in row chunks whose (rows, K) scores stay below 256 MiB; its peak memory
  t.update   torch: index_add_ of the rows in fp64, bincount, the quotient
  matrix     2 P K C / 157 TFLOP/s, the fp32 matrix floor of one assign
  read       the features once at 6.29 TB/s (the float4 copy rate measured on this device)
Needs the GPU.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from neighbors_bench import interleaved, peak_mb      # noqa: E402

READ_TBS = 6.29
MATRIX_TFLOPS = 157.0


def torch_assign(x, cent, chunk):
    c2 = (cent * cent).sum(1)
    ct = cent.t().contiguous()
    return torch.cat([torch.addmm(c2[None, :], x[a:a + chunk], ct, alpha=-2.0).argmin(1) for a in range(0, x.shape[0], chunk)])


def torch_update(x, codes, K):
    sums = torch.zeros(K, x.shape[1], device=x.device, dtype=torch.float64).index_add_(0, codes, x.double())
    count = torch.bincount(codes, minlength=K)
    return (sums / count.clamp_min(1)[:, None]).float(), count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("codebook_bench needs a GPU: a timing taken anywhere else says nothing")
    import codebook
    from simple_knn import _C

    dev = torch.device("cuda:0")
    P = args.points
    gen = torch.Generator(device=dev).manual_seed(1)
    lines = []
    say = lambda s="": (print(s, flush=True), lines.append(s))
    say(f"# Feature codebooks: {torch.cuda.get_device_name(0)}")
    say()
    say(f"P = {P} rows; median of {args.reps} calls ({args.torch_reps} for the torch legs) after {args.warmup} warm-up, host clock to the end of "
        f"a device synchronise, the legs of one row interleaved in one process.  Times in ms.  `matrix`: 2 P K C / {MATRIX_TFLOPS:.0f} TFLOP/s; "
        f"`read`: the features once at {READ_TBS} TB/s; `x floor`: assign over the larger of the two; `x torch`: the torch leg over ours.")
    say()
    say("| C | K | assign | +dist2 | update | kmeans(10) | matrix | read | x floor | TFLOP/s | t.assign | x torch | t.update | x torch | "
        "torch peak MiB | assign peak MiB | codes equal |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for C in (32, 128):
        centres = torch.randn(64, C, device=dev, generator=gen) * 2
        x = centres[torch.randint(0, 64, (P,), device=dev, generator=gen)] + torch.randn(P, C, device=dev, generator=gen)
        for K in (16, 256, 4096):
            cent = x[(torch.arange(K, device=dev) * P) // K].contiguous()
            chunk = max(1, min(P, (64 << 20) // K))
            codes, _ = _C.codebook_assign(x, cent, 0, None, None, None, False, None, None)
            inertia = torch.zeros(1, dtype=torch.float64, device=dev)
            moving = cent.clone()
            long_codes = codes.long()
            ours = {"assign": lambda: _C.codebook_assign(x, cent, 0, None, None, None, False, None, None),
                    "dist2": lambda: _C.codebook_assign(x, cent, 0, None, None, None, True, inertia, None),
                    "update": lambda: _C.codebook_update(x, codes, None, moving, 0, 0, None),
                    "kmeans": lambda: codebook.kmeans(x, K, iterations=10, init=cent)}
            theirs = {"t.assign": lambda: torch_assign(x, cent, chunk), "t.update": lambda: torch_update(x, long_codes, K)}
            r = interleaved(ours, args.reps, args.warmup)
            t = interleaved(theirs, args.torch_reps, args.warmup)
            peak_t, ref = peak_mb(theirs["t.assign"])
            peak_h, got = peak_mb(ours["assign"])
            same = float((got[0].long() == ref).double().mean())
            matrix_ms = 2.0 * P * K * C / (MATRIX_TFLOPS * 1e12) * 1e3
            read_ms = P * C * 4 / (READ_TBS * 1e12) * 1e3
            a = r["assign"][0]
            say(f"| {C} | {K} | {a:.3f} | {r['dist2'][0]:.3f} | {r['update'][0]:.3f} | {r['kmeans'][0]:.2f} | {matrix_ms:.3f} | {read_ms:.3f} | "
                f"{a / max(matrix_ms, read_ms):.1f} | {2.0 * P * K * C / a / 1e9:.1f} | {t['t.assign'][0]:.3f} | {t['t.assign'][0] / a:.1f} | "
                f"{t['t.update'][0]:.3f} | {t['t.update'][0] / r['update'][0]:.1f} | {peak_t:.0f} | {peak_h:.1f} | {same:.6f} |")
            del ref, got, codes, long_codes
        del x
    say()
    say("`codes equal`: the share of rows on which the torch route (another summation order) picks the same centroid.")
    say()
    say("Not measured: the kernels one by one; hardware counters; the cosine metric (one more prepare pass over the centroids, the same "
        "kernel); strided or misaligned rows (scalar loads); weights; K above 4096; row counts other than the one above.")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
