"""Times the connected components over the neighbour lists (csrc/components.hip) against one mode-filter step on the same lists
and against scipy on the host.

    python tools/components_bench.py [--points 1000000] [--reps 10] [--warmup 2] [--out profiles/components_bench.md]

The two point sets of tools/neighbors_bench.py, K in {3, 8, 16}; the lists are built outside the timing.  Median of `reps` calls,
host clock from the call to the end of a device synchronise, the legs of one K interleaved round by round, every leg the native
call itself (simple_knn._C, outputs and scratch allocated inside; the int64 conversions of neighbors.py are not in it):
  plain      knn_components without labels (the scene is one giant component, or a few)
  labels     with ~300 instance labels (the nearest of 300 random centres)
  mutual     without labels, mutual neighbours only
  dense      without labels, with the dense ids
  largest    component_filter with largest over the `labels` leg's result
  node/slot/none   f3dgs_debug_knn_components_shape 0 / 1 / 2: the link stage as one thread per node, per (node, slot), left out
  filter     one step of label_mode_filter on the same lists: it reads idx once - the floor of any pass over the lists
  scipy      scipy.sparse.csgraph.connected_components on the host, the device-to-host copy of idx included, one call
and a chain of `--points` nodes (a line, idx[i] = {i - 1, i + 1}: the same lists whether the indices ascend or descend along it)
in storage order and shuffled: the deepest walks.  Needs the GPU.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from neighbors_bench import clustered, interleaved      # noqa: E402

INF = float("inf")


def scipy_components(idx):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = idx.cpu().numpy()
    P, K = host.shape
    rows = np.repeat(np.arange(P, dtype=np.int32), K)
    cols = host.reshape(-1)
    ok = cols >= 0
    a = coo_matrix((np.ones(int(ok.sum()), np.int8), (rows[ok], cols[ok])), shape=(P, P))
    n, _ = connected_components(a, directed=False)
    return (time.perf_counter() - t0) * 1e3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("components_bench needs a GPU: a timing taken anywhere else says nothing")
    import neighbors
    from simple_knn import _C
    from synth import make_scene

    dev = torch.device("cuda:0")
    P, L = args.points, 300
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.f3dgs_debug_knn_components_shape.argtypes = [ci, ci, vp, vp, ctypes.c_float, vp, ci, ci, vp, vp, vp, vp]
    root, size = torch.empty(P, device=dev, dtype=torch.int32), torch.empty(P, device=dev, dtype=torch.int32)
    status = torch.zeros((), device=dev, dtype=torch.int32)
    stream = torch.cuda.current_stream().cuda_stream

    def shaped(idx, shape):
        rc = lib.f3dgs_debug_knn_components_shape(idx.shape[0], idx.shape[1], idx.data_ptr(), None, INF, None, 0, shape, root.data_ptr(),
                                                  size.data_ptr(), status.data_ptr(), stream)
        assert rc == 0

    sets = {"clustered": torch.from_numpy(clustered(P, 21)).to(dev),
            "synth": make_scene(P=P, C=0, width=64, height=64, seed=3)["means3D"].to(dev).contiguous()}
    lines = []
    say = lambda s="": (print(s, flush=True), lines.append(s))
    say(f"# Connected components over the neighbour lists: {torch.cuda.get_device_name(0)}")
    say()
    say(f"P = {P} points; median of {args.reps} calls after {args.warmup} warm-up calls, host clock to the end of a device synchronise, "
        f"the legs of one K interleaved in one process; scipy: one call.  Times in ms.  `x filter`: the `plain` leg over one mode-filter "
        f"step on the same lists.")
    for name, pts in sets.items():
        g = torch.Generator(device=dev).manual_seed(1)
        centres = pts[torch.randint(0, P, (L,), device=dev, generator=g)]
        labels = torch.cat([torch.cdist(pts[a:a + 65536], centres).argmin(1) for a in range(0, P, 65536)]).to(torch.int32)
        say()
        say(f"## {name}")
        say()
        say("| K | plain | labels | mutual | dense | largest | link: node | link: slot | no link | filter step | x filter | scipy, host | "
            "components plain / labels / mutual |")
        say("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        for K in (3, 8, 16):
            idx, _ = neighbors.knn(pts, K, return_dist2=False)
            res = _C.knn_components(idx, None, INF, labels, False, False)
            out, nxt = torch.empty_like(labels), torch.empty_like(labels)
            legs = {"plain": lambda: _C.knn_components(idx, None, INF, None, False, False),
                    "labels": lambda: _C.knn_components(idx, None, INF, labels, False, False),
                    "mutual": lambda: _C.knn_components(idx, None, INF, None, True, False),
                    "dense": lambda: _C.knn_components(idx, None, INF, None, False, True),
                    "largest": lambda: _C.component_filter(labels, res[0], res[1], 1, True, L, out),
                    "node": lambda: shaped(idx, 0), "slot": lambda: shaped(idx, 1), "none": lambda: shaped(idx, 2),
                    "filter": lambda: _C.label_mode_filter(labels, None, idx, None, INF, True, nxt, None)}
            r = interleaved(legs, args.reps, args.warmup)
            counts = [int(_C.knn_components(idx, None, INF, lab, mut, True)[4]) for lab, mut in ((None, False), (labels, False), (None, True))]
            assert int(status) == 0
            host_ms, n_host = scipy_components(idx)
            assert n_host == counts[0], (n_host, counts)
            f = lambda k: f"{r[k][0]:.3f}"
            say(f"| {K} | {f('plain')} | {f('labels')} | {f('mutual')} | {f('dense')} | {f('largest')} | {f('node')} | {f('slot')} | "
                f"{f('none')} | {f('filter')} | {r['plain'][0] / r['filter'][0]:.2f} | {host_ms:.0f} | "
                f"{counts[0]} / {counts[1]} / {counts[2]} |")
            del idx, res
    say()
    say(f"## A chain of {P} nodes, K = 2")
    say()
    say("idx[i] = {i - 1, i + 1}: one component, the deepest walks.  `shuffled`: the same chain under a random numbering.")
    say()
    say("| numbering | plain | link: node | link: slot | no link | status |")
    say("|---|---|---|---|---|---|")
    i = torch.arange(P, device=dev, dtype=torch.int32)
    chain = torch.stack([i - 1, torch.where(i + 1 < P, i + 1, torch.full_like(i, -1))], 1).contiguous()
    perm = torch.randperm(P, device=dev, generator=torch.Generator(device=dev).manual_seed(2)).to(torch.int32)
    inv = torch.empty_like(perm)
    inv[perm.long()] = i                                      # node perm[a] sits at place a of the chain
    shuffled = torch.where(chain[inv.long()] >= 0, perm[chain[inv.long()].clamp_min(0).long()], torch.full_like(chain, -1)).contiguous()
    for name, idx in (("in order", chain), ("shuffled", shuffled)):
        r = interleaved({"plain": lambda: _C.knn_components(idx, None, INF, None, False, False), "node": lambda: shaped(idx, 0),
                         "slot": lambda: shaped(idx, 1), "none": lambda: shaped(idx, 2)}, args.reps, args.warmup)
        res = _C.knn_components(idx, None, INF, None, False, True)
        assert int(res[4]) == 1, int(res[4])
        say(f"| {name} | {r['plain'][0]:.3f} | {r['node'][0]:.3f} | {r['slot'][0]:.3f} | {r['none'][0]:.3f} | {int(res[5])} |")
    say()
    say("Not measured: K other than 3, 8 and 16; a finite max_dist; point counts other than the one above; the kernels one by one "
        "(the link stage is the difference of a `link` column and `no link`); one atomic per distinct root per WORKGROUP in the count.")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
