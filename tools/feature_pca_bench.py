"""Timing and memory of the PCA colour image (feature_pca.feature_visualize, csrc/feature_pca.hip) against the two ways to get the
same picture without it, on the same GPU in the same process:

  (a) the reference's chain with torch ops on the GPU: normalize -> permute -> centred matmul of every third pixel ->
      torch.linalg.eigh -> matmul of the whole map -> quantile -> clamp;
  (b) the reference's chain as written (render.py:38-53): the samples to the host, sklearn.decomposition.PCA(3) there, mean and
      components back - where scikit-learn is installed.

3 warm-up calls, 10 calls timed by device events ((b): wall clock around a synchronize), median; peak memory of one call above
what was allocated before it.  Also the measured errors of every case of tests/test_gpu_feature_pca.py against the float64
oracle (--errors).  One JSON line per shape, then a table.

    python tools/feature_pca_bench.py [--small | --shape C,H,W] [--errors] [--fused-only]

Which kernel bounds the fit is a question for per-kernel times, which this tool does not take: run it under
`rocprofv3 --kernel-trace --stats -- python tools/feature_pca_bench.py --shape 512,360,480 --fused-only` (one shape and no
comparison chains, so that the averages of the pca_* kernels are those of one size).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from feature_pca import apply_feature_pca, feature_visualize, fit_feature_pca      # noqa: E402
import feature_pca_oracle as O                                                      # noqa: E402

DEV = "cuda:0"


def median_ms(fn, warmup=3, calls=10, wall=False):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        if wall:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return rise / 2 ** 20


def torch_chain(fm):
    fmap = F.normalize(fm[None], dim=1)
    f = fmap.permute(0, 2, 3, 1).reshape(-1, fm.shape[0])
    s = f[::3]
    mean = s.mean(0)
    z = s - mean
    cov = (z.t() @ z / (s.shape[0] - 1)).double()
    w, v = torch.linalg.eigh(cov)
    comp = v[:, -3:].flip(1).t()
    big = comp.gather(1, comp.abs().argmax(dim=1, keepdim=True))
    comp = (comp * torch.where(big < 0, -1.0, 1.0)).float()
    t = (f - mean[None]) @ comp.t()
    q = torch.quantile(t[::3].reshape(-1), torch.tensor([0.01, 0.99], device=fm.device))
    return ((t - q[0]) / (q[1] - q[0])).clamp(0.0, 1.0).reshape(fm.shape[1], fm.shape[2], 3)


def sklearn_chain(fm):
    import sklearn.decomposition
    fmap = F.normalize(fm[None], dim=1)
    pca = sklearn.decomposition.PCA(3, random_state=42)
    f_samples = fmap.permute(0, 2, 3, 1).reshape(-1, fmap.shape[1])[::3].cpu().numpy()
    transformed = pca.fit_transform(f_samples)
    mean = torch.tensor(f_samples.mean(0)).float().to(fm.device)
    comp = torch.tensor(pca.components_).float().to(fm.device)
    q1, q99 = np.percentile(transformed, [1, 99])
    vis = (fmap.permute(0, 2, 3, 1).reshape(-1, fmap.shape[1]) - mean[None, :]) @ comp.T
    vis = (vis - q1) / (q99 - q1)
    return vis.clamp(0.0, 1.0).float().reshape((fmap.shape[2], fmap.shape[3], 3)).cpu()


def errors():
    from diff_gaussian_rasterization import _C
    cases = [("c3_20x31", 3), ("c4_1x7", 3), ("c20_45x60", 3), ("c32_45x61", 3), ("c33_37x53", 3), ("c128_90x121", 3),
             ("c512_36x48", 3), ("c16_37x53_zeros", 3), ("c20_45x60", 1), ("c128_90x121", 1), ("c128_180x240", 3)]
    print("case                     stride      e_cov     e_mean  e_img (end to end)")
    for name, stride in cases:
        f = O.make_inputs(name, stride)
        want = O.oracle(f, stride)
        fd = torch.from_numpy(f).to(DEV)
        mean, cov = _C.feature_pca_moments(fd, stride)
        e_cov = np.abs(cov.cpu().numpy() - want.cov).max() / np.abs(want.cov).max()
        e_mean = np.abs(mean.cpu().numpy() - want.mean).max()
        diff = np.abs(feature_visualize(fd, stride).cpu().numpy().astype(np.float64) - want.image)
        k = O.determined_components(f.shape[0], -(-f.shape[1] * f.shape[2] // stride))
        e_img = max(diff[..., :k].max(), diff.reshape(-1, 3)[::stride].max())
        print(f"{name:24s} {stride:6d} {e_cov:10.2e} {e_mean:10.2e} {e_img:10.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="128 x 180 x 240 only")
    ap.add_argument("--shape", help="C,H,W: this shape only")
    ap.add_argument("--fused-only", action="store_true", help="fit and apply only, no comparison chains (for a kernel trace)")
    ap.add_argument("--errors", action="store_true", help="the errors of the test cases against the float64 oracle, no timing")
    args = ap.parse_args()
    if args.errors:
        return errors()
    try:
        import sklearn.decomposition      # noqa: F401
        have_sklearn = True
    except ImportError:
        have_sklearn = False
    rows = []
    shapes = ((128, 180, 240),) if args.small else ((512, 360, 480), (128, 1080, 1920))
    if args.shape:
        shapes = (tuple(int(v) for v in args.shape.split(",")),)
    for C, H, W in shapes:
        g = torch.Generator().manual_seed(C)
        # the test family's structure at size: an offset, three smooth fields, noise
        yy, xx = torch.meshgrid(torch.arange(H) / H, torch.arange(W) / W, indexing="ij")
        fm = torch.randn(C, 1, 1, generator=g) * 3 / C ** 0.5 + 0.05 * torch.randn(C, H, W, generator=g)
        for k, amp in enumerate((1.0, 0.6, 0.35)):
            d = torch.randn(C, generator=g)
            fm += amp * (d / d.norm())[:, None, None] * torch.sin(6.28 * ((k + 1) * 0.7 * yy + (3 - k) * 0.6 * xx) + k)[None]
        fm = fm.to(DEV)
        with torch.no_grad():
            pca = fit_feature_pca(fm)
            if args.fused_only:
                print(json.dumps({"C": C, "H": H, "W": W, "fit_ms": median_ms(lambda: fit_feature_pca(fm)),
                                  "apply_ms": median_ms(lambda: apply_feature_pca(fm, pca))}), flush=True)
                continue
            row = {"C": C, "H": H, "W": W, "map_mb": fm.numel() * 4 / 2 ** 20,
                   "visualize_ms": median_ms(lambda: feature_visualize(fm)),
                   "fit_ms": median_ms(lambda: fit_feature_pca(fm)),
                   "apply_ms": median_ms(lambda: apply_feature_pca(fm, pca)),
                   "torch_ms": median_ms(lambda: torch_chain(fm)),
                   "visualize_peak_mb": peak_mb(lambda: feature_visualize(fm)),
                   "torch_peak_mb": peak_mb(lambda: torch_chain(fm))}
            row["apply_gbs"] = fm.numel() * 4 / (row["apply_ms"] * 1e-3) / 1e9
            if have_sklearn:
                row["sklearn_ms"] = median_ms(lambda: sklearn_chain(fm), warmup=1, calls=3, wall=True)
                row["sklearn_peak_mb"] = peak_mb(lambda: sklearn_chain(fm))
            row["max_diff_vs_torch"] = float((feature_visualize(fm) - torch_chain(fm)).abs().max())
        rows.append(row)
        print(json.dumps(row), flush=True)
        del fm
        torch.cuda.empty_cache()
    print("\n   C     H     W   map MB  visualize       fit     apply  apply GB/s  (a) torch  (b) sklearn   peak MB: fused / torch")
    for r in rows:
        sk = f"{r['sklearn_ms']:9.1f} ms" if "sklearn_ms" in r else "           -"
        print(f"{r['C']:4d} {r['H']:5d} {r['W']:5d} {r['map_mb']:8.0f} {r['visualize_ms']:7.3f} ms {r['fit_ms']:6.3f} ms {r['apply_ms']:6.3f} ms "
              f"{r['apply_gbs']:10.0f} {r['torch_ms']:7.3f} ms {sk} {r['visualize_peak_mb']:14.1f} / {r['torch_peak_mb']:.1f}")


if __name__ == "__main__":
    main()
