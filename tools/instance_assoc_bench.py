"""Times the instance association (csrc/instances.hip) against the route torch offers for the same step.

    python tools/instance_assoc_bench.py [--gaussians 1000000] [--masks 255] [--instances 512] [--reps 50] [--warmup 10]
                                         [--out profiles/instance_assoc.txt]

Synthetic dense inputs (no rasterizer): P Gaussians of which about 40 % are seen in the view, about 1.2 non-zero masks per seen
row of the view's vote (P, M + 1), an accumulator (P, L + 1) with `--used` instances in use.  Timed, with device events around
every call, warm-up, median of `reps`, all in one process:
  fused   associate_votes + merge_votes (seven launches), and each of the two by itself; the merge also with clear_view; the
          association also on a vote without weight outside the masks (no atomics into the table's last row)
  torch   acc[:, :L].max(1) -> one_hot -> acc_view.T @ one_hot -> the match in torch -> index_add_
Every call starts from the same count; the view's vote is restored outside the timed span where a call clears it.  The peak of
torch.cuda.max_memory_allocated above the inputs is recorded for both routes, and the two mappings are compared.  Needs the GPU.
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


def timed_ms(fn, reps, warmup, prepare=None):
    """median, min, max of `reps` calls of fn, each between its own pair of events; prepare() runs in front of every call, untimed"""
    for _ in range(warmup):
        if prepare:
            prepare()
        fn()
    torch.cuda.synchronize()
    a = [torch.cuda.Event(enable_timing=True) for _ in range(reps)]
    b = [torch.cuda.Event(enable_timing=True) for _ in range(reps)]
    for i in range(reps):
        if prepare:
            prepare()
        a[i].record()
        fn()
        b[i].record()
    torch.cuda.synchronize()
    t = [a[i].elapsed_time(b[i]) for i in range(reps)]
    return statistics.median(t), min(t), max(t)


def make_inputs(P, M, L, used, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g)
    objects = min(M, used)
    obj = torch.randint(0, objects, (P,), device=dev, generator=g)
    mask_of = torch.randperm(M, device=dev, generator=g)[:objects]
    inst_of = torch.randperm(used, device=dev, generator=g)[:objects]
    rows = torch.arange(P, device=dev)
    seen = rnd(P) < 0.4
    view = torch.zeros(P, M + 1, device=dev)
    view[rows, mask_of[obj]] = 0.2 + rnd(P)
    second = rnd(P) < 0.2                                   # a second mask on a fifth of the rows: 1.2 non-zeros per seen row
    view[rows[second], torch.randint(0, M, (int(second.sum()),), device=dev, generator=g)] += 0.1
    view[:, M] = view[:, :M].sum(1) + 0.05 * rnd(P)
    view *= seen[:, None]
    acc = torch.zeros(P, L + 1, device=dev)
    labelled = rnd(P) < 0.8
    acc[rows[labelled], inst_of[obj[labelled]]] = 1.0 + rnd(int(labelled.sum()))
    acc[:, L] = acc[:, :L].sum(1) + 0.1
    return view, acc


def torch_route(view, acc, count, iou_thresh, min_weight):
    """The same step from torch operators (count: a host int).  Returns (mapping, new count); acc is added to."""
    P, M, L = view.shape[0], view.shape[1] - 1, acc.shape[1] - 1
    top, idx = acc[:, :L].max(1)
    c = torch.where(top > 0, idx, torch.full_like(idx, L))
    seen = view[:, M] > 0
    v = view * seen[:, None]
    rest = (v[:, M] - v[:, :M].sum(1)).clamp_min(0)
    T = torch.cat([v[:, :M], rest[:, None]], 1).t() @ torch.nn.functional.one_hot(c, L + 1).to(torch.float32)
    Td = T.double()
    row = Td[:M, :L].sum(1)
    rowall = row + Td[:M, L]
    col = Td[:, :L].sum(0)
    x = Td[:M, :count]
    den = (row[:, None] + col[None, :count]) - x
    iou = torch.where(den == 0, torch.zeros_like(den), x / den)
    mapping = torch.full((M,), -1, dtype=torch.int64, device=view.device)
    if count:
        best, lab = iou.max(1)
        claims = (best >= iou_thresh) & (best > 0)
        score = torch.full((M, count), -1.0, dtype=torch.float64, device=view.device)
        score[claims, lab[claims]] = best[claims]
        wbest, wm = score.max(0)                                # per instance: its best claimant
        taken = wbest >= 0
        mapping[wm[taken]] = torch.arange(count, device=view.device)[taken]
    fresh = (mapping < 0) & (rowall > min_weight)
    ids = count + torch.cumsum(fresh, 0) - 1
    mapping = torch.where(fresh & (ids < L), ids, mapping)
    valid = mapping >= 0
    acc.index_add_(1, mapping[valid], v[:, :M][:, valid])
    acc[:, L] += v[:, M]
    return mapping, torch.clamp(count + fresh.sum(), max=L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1000000)
    ap.add_argument("--masks", type=int, default=255)
    ap.add_argument("--instances", type=int, default=512)
    ap.add_argument("--used", type=int, default=300)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("instance_assoc_bench needs a GPU: a timing taken anywhere else says nothing")
    import instances as ins

    dev = torch.device("cuda:0")
    P, M, L, used = args.gaussians, args.masks, args.instances, args.used
    view0, acc0 = make_inputs(P, M, L, used, dev)
    view, acc = view0.clone(), acc0.clone()
    count, dropped = torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.int32)
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    nz = int((view0[:, :M] != 0).sum())
    seen = int((view0[:, M] > 0).sum())
    say(f"instance association: P = {P}, M = {M}, L = {L}, {used} instances in use; {seen / P:.1%} of the rows seen, "
        f"{nz / max(seen, 1):.2f} non-zero masks per seen row; {torch.cuda.get_device_name(0)}; median of {args.reps} after "
        f"{args.warmup} warm-up calls, device events (min .. max)")
    say(f"  inputs: the view's vote {view.numel() * 4 / 2 ** 20:.0f} MiB, the accumulator {acc.numel() * 4 / 2 ** 20:.0f} MiB")

    def reset():
        count.fill_(used)

    state = {}

    def associate():
        state["r"] = ins.associate_votes(view, acc, count, iou_thresh=0.5, dropped=dropped)

    def fused(clear=False):
        associate()
        ins.merge_votes(view, state["r"]["mapping"], acc, clear_view=clear)

    def restore():
        reset()
        view.copy_(view0)

    reset()
    associate()
    mapping = state["r"]["mapping"].clone()
    # the same vote with no weight outside the masks: multiples of 1 / 64 add exactly, so total - sum is 0 and row M gets no atomic
    exact = torch.round(view0 * 64) / 64
    exact[:, M] = exact[:, :M].sum(1)

    def associate_exact():
        ins.associate_votes(exact, acc, count, iou_thresh=0.5, dropped=dropped)

    legs = [("assoc", "associate_votes (six launches)", associate, reset),
            ("assoc0", "associate_votes, no weight outside the masks", associate_exact, reset),
            ("merge", "merge_votes", lambda: ins.merge_votes(view, mapping, acc), None),
            ("fused", "fused: associate + merge", fused, reset),
            ("clear", "fused with clear_view (vote restored untimed)", lambda: fused(True), restore),
            ("torch", "torch: max, one_hot, matmul, match, index_add_", lambda: torch_route(view, acc, used, 0.5, 0.0), None)]
    res = {}
    for key, name, fn, prep in legs:
        acc.copy_(acc0)
        view.copy_(view0)
        r = res[key] = timed_ms(fn, args.reps, args.warmup, prep)
        say(f"  {name:52s} {r[0]:8.3f} ms  ({r[1]:.3f} .. {r[2]:.3f})")
    say(f"  the vote alone streams in {view.numel() * 4 / 6.3e12 * 1e3:.3f} ms at 6.3 TB/s, of which the seen rows are "
        f"{seen * (M + 1) * 4 / 6.3e12 * 1e3:.3f} ms")

    def peak_mb(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - before) / 2 ** 20, out

    acc.copy_(acc0)
    view.copy_(view0)
    reset()
    state.clear()
    new_mb, _ = peak_mb(fused)
    got, got_count = state["r"]["mapping"].long().clone(), int(count.item())
    state.clear()
    acc.copy_(acc0)
    old_mb, (want, want_count) = peak_mb(lambda: torch_route(view, acc, used, 0.5, 0.0))
    table_mb = ((M + 1) * (L + 1) * 4 + 20 * M + 12 * L) / 2 ** 20
    say(f"  peak memory above the inputs: fused {new_mb:.2f} MiB (the table and the vectors of M and L: {table_mb:.2f} MiB), "
        f"torch {old_mb:.1f} MiB")
    same = bool(torch.equal(got, want)) and got_count == int(want_count)
    say(f"  the two routes' mappings {'agree' if same else 'DIFFER'}: {int((got >= 0).sum())} of {M} masks placed, "
        f"{int(((got >= 0) & (got < used)).sum())} matched with an instance in use, count {used} -> {got_count}")
    f, t = res["fused"][0], res["torch"][0]
    say(f"  expectation: the fused route is no slower than the torch route: {f:.3f} ms against {t:.3f} ms: "
        f"{'met' if f <= t else 'NOT met'}")
    say(f"  expectation: its memory above the inputs is the table plus vectors of M and L (within allocator rounding, 2 MiB): "
        f"{'met' if new_mb <= table_mb + 2.0 else 'NOT met'}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
