"""Cases of the fused feature-map loss / decode (csrc/feature_loss.hip) at every tile, list and store-path edge of its kernels,
with a MARGIN ground truth: `gt = decoded64 + s m`, s = +-1, m uniform in [0.25, 1], so that every residual is at least
0.25 - ulp away from zero.  The L1 gradient is sign(residual) / n; with such a margin no sign can differ between the fp32
kernels and the float64 chain (oracle/feature_loss_oracle.py), and the gradients are compared without any slack for flips.

A case is (C, H, W, Cout, Hg, Wg, decoder).  `build_case` is cached: the loss tests and the decode tests of one case share one
float64 evaluation.  `describe` restates, on the host, which kernel paths a case takes (tests/test_feature_loss_cases_cpu.py
checks that the lists reach every one of them).  Helper module: no tests here."""
import functools
import itertools

import torch

from test_resize_taps import build as tap_list, scale_of

N_EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 257)
# N as a ragged rectangle where it has one
RECT = {32: (4, 8), 33: (3, 11), 63: (7, 9), 64: (4, 16), 65: (5, 13), 128: (8, 16), 129: (3, 43)}
SRC = (9, 13)                        # the small source of the N sweeps
RB_MAXT = 6                          # list capacity of fl_resize_backward_kernel


def _shape_of(N, form):
    """form 0: (1, N); 1: (N, 1); 2: the ragged rectangle (N without one: (1, N) / (N, 1) by parity)."""
    if form == 2 and N in RECT:
        return RECT[N]
    if form == 2:
        form = N & 1
    return (1, N) if form == 0 else (N, 1)


def _decoder_cases():
    # every (C, Cout): 18 pairs, two N each -> every C meets every Cout (so every remainder mod 32 and mod 128) and every N
    out = []
    for idx, (C, Cout) in enumerate(itertools.product((32, 64, 128), (1, 31, 33, 100, 129, 160))):
        for j in range(2):
            N = N_EDGES[(2 * idx + j) % len(N_EDGES)]
            Hg, Wg = _shape_of(N, (idx + 2 * j) % 3)
            out.append((C, SRC[0], SRC[1], Cout, Hg, Wg, True))
    return out


def _plain_cases():
    out = []
    for ci, C in enumerate((1, 5, 31, 33, 40)):
        for ni, N in enumerate(N_EDGES):
            Hg, Wg = _shape_of(N, (ci + ni) % 3)
            out.append((C, SRC[0], SRC[1], C, Hg, Wg, False))
    return out


DECODER_CASES = _decoder_cases()
PLAIN_CASES = _plain_cases()
# K3's pixel-range split: more tiles than 512 / cblocks ranges -> `per` = 2 and the upper blockIdx.y ranges are empty
K3_CASES = [
    (32, 9, 13, 33, 114, 288, True),         # 513 tiles, cblocks = 1: splits = 512, per = 2, ranges 257.. empty
    (32, 9, 13, 640, 64, 103, True),         # 103 tiles, cblocks = 5: splits = 102, per = 2, ranges 52.. empty
]
GEOMETRIES = [
    # (H, W) -> (Hg, Wg)
    ((1, 50), (7, 17)),            # H = 1 source
    ((30, 1), (12, 5)),            # W = 1 source
    ((30, 50), (1, 17)),           # scale 0 on the row axis only
    ((30, 50), (12, 1)),           # scale 0 on the column axis only
    ((40, 16), (13, 56)),          # shrink x enlarge above 2.5x
    ((16, 40), (56, 13)),          # the reverse
    ((4, 4), (64, 64)),            # 16x enlargement: the general loop on both axes
    ((16, 16), (40, 40)),          # 40 / 16 = 2.5 (the taps step by 39 / 15): the longest lists are five entries
    ((8, 9), (23, 26)),            # lists of exactly six entries on both axes: the capacity, without overflow
    ((24, 68), (8, 23)),           # W = 68: a vector and a scalar block in one row; 3x shrink: ny == 0 zero-fill in both forms
    ((24, 128), (8, 43)),          # ny == 0 on the pure vec4 path
    ((24, 60), (8, 20)),           # W < 64, W % 4 == 0
    ((24, 67), (24, 67)),          # identity resize
]
GEOMETRY_CASES = [(5, H, W, 5, Hg, Wg, False) for (H, W), (Hg, Wg) in GEOMETRIES] + \
                 [(32, H, W, 33, Hg, Wg, True) for (H, W), (Hg, Wg) in GEOMETRIES]
LOSS_CASES = DECODER_CASES + K3_CASES + PLAIN_CASES + GEOMETRY_CASES
# the forward-only decode: the same decoder, no-decoder and geometry lists (K3 does not run there)
DECODE_CASES = DECODER_CASES + PLAIN_CASES + GEOMETRY_CASES


def case_id(case):
    C, H, W, Cout, Hg, Wg, dec = case
    return f"{C}x{H}x{W}-{'dec' if dec else 'plain'}{Cout}x{Hg}x{Wg}"


@functools.lru_cache(maxsize=None)
def build_case(case):
    """fm, w, b from a seed; the chain in float64; gt = decoded64 + s m rounded to fp32.  Returns a dict with the fp32 inputs
    and `want` = reference_feature_l1(...) in float64 (loss, gradients, decoded).  Nothing in it may be modified."""
    from oracle.feature_loss_oracle import reference_feature_l1
    C, H, W, Cout, Hg, Wg, dec = case
    g = torch.Generator().manual_seed(1000003 * C + 7919 * Cout + 613 * H + 389 * W + 31 * Hg + Wg)
    fm = torch.randn(C, H, W, generator=g)
    w = (torch.randn(Cout, C, generator=g) / C ** 0.5) if dec else None
    b = (torch.randn(Cout, generator=g) * 0.1) if dec else None
    decoded = reference_feature_l1(fm, torch.zeros(Cout, Hg, Wg), w, b)["decoded"]
    s = torch.randint(0, 2, (Cout, Hg, Wg), generator=g).double() * 2 - 1
    m = 0.25 + 0.75 * torch.rand(Cout, Hg, Wg, generator=g, dtype=torch.float64)
    gt = (decoded + s * m).float()
    margin = float((decoded - gt.double()).abs().min())
    assert margin >= 0.2, (case, margin)        # a condition on the reference alone: no residual sign can flip in fp32
    want = reference_feature_l1(fm, gt, w, b)
    return dict(fm=fm, w=w, b=b, gt=gt, want=want, margin=margin)


# ---- which paths a case takes (host restatement of the launch arithmetic of feature_loss.hip) -------------------------------

def k3_ranges(N, Cout):
    """run_decoder / fl_dweight_kernel: (splits, per, number of empty blockIdx.y ranges)."""
    cblocks, tiles = (Cout + 127) // 128, (N + 63) // 64
    splits = max(1, min(tiles, 512 // cblocks))
    per = (tiles + splits - 1) // splits
    empty = sum(1 for y in range(splits) if y * per >= min(tiles, y * per + per))
    return splits, per, empty


def axis_lists(n_in, n_out):
    """Per source index of one axis: the length of its (output, weight) list, or -1 where it exceeds the capacity."""
    s = scale_of(n_in, n_out)
    lens = [len(tap_list(i, s, n_in, n_out)) for i in range(n_in)]
    return [n if n <= RB_MAXT else -1 for n in lens]


def describe(case):
    """The set of edge classes `case` reaches."""
    C, H, W, Cout, Hg, Wg, dec = case
    N = Hg * Wg
    got = {f"N%64={N % 64}", f"N%128={N % 128}", f"N%32={N % 32}", f"ntiles64={min((N + 63) // 64, 3)}"}
    if dec:
        got |= {f"Cout%32={Cout % 32}", f"Cout%128={Cout % 128}", f"C={C}:Cout%32={Cout % 32}", f"C={C}:Cout%128={Cout % 128}",
                f"C={C}:N={N}"}
        # K3's last tile: `valid` of the upper half (h = 1) is N - 64 tI - 32: the whole half is pad, part of it, none of it
        v = N - 64 * ((N + 63) // 64 - 1) - 32
        got.add("k3-upper-half-" + ("all-pad" if v <= 0 else "part-pad" if v < 32 else "no-pad"))
        if k3_ranges(N, Cout)[2] > 0:
            got.add(f"k3-empty-ranges:cblocks={(Cout + 127) // 128}")
        if Cout > 128 and Cout % 128:
            got.add("k3-ragged-later-cblock")
    else:
        got |= {f"plainC%32={C % 32}", f"plainC={C}:N={N}"}
        if C > 32:
            got.add("plain-two-channel-blocks")
    got.add("form-" + ("1xN" if Hg == 1 and Wg > 1 else "Nx1" if Wg == 1 and Hg > 1 else "one" if N == 1 else "rect"))
    ny, nx = axis_lists(H, Hg), axis_lists(W, Wg)
    if any(a < 0 for a in ny) and any(b > 0 for b in nx):
        got.add("k4-ny-overflow-nx-list")
    if any(a > 0 for a in ny) and any(b < 0 for b in nx):
        got.add("k4-ny-list-nx-overflow")
    if any(a < 0 for a in ny) and any(b < 0 for b in nx):
        got.add("k4-both-overflow")
    if max(ny) == RB_MAXT or max(nx) == RB_MAXT:
        got.add("k4-list-full")
    blocks = [(x0, W % 4 == 0 and x0 + 64 <= W) for x0 in range(0, W, 64)]
    for _x0, vec in blocks:
        got.add("k4-store-vec4" if vec else "k4-store-scalar")
        if 0 in ny:
            got.add("k4-zero-row-vec4" if vec else "k4-zero-row-scalar")
    if len({v for _x0, v in blocks}) == 2:
        got.add("k4-vec4-and-scalar-in-one-row")
    if W < 64 and W % 4 == 0:
        got.add("k4-narrow-W%4==0")
    if W % 64 and W > 64:
        got.add("k4-ragged-last-block")
    if 0 in nx:
        got.add("k4-empty-column-list")
    if Hg == 1 and Wg > 1 and H > 1:
        got.add("scale0-rows-only")
    if Wg == 1 and Hg > 1 and W > 1:
        got.add("scale0-cols-only")
    if H == 1 and Hg > 1:
        got.add("source-H=1")
    if W == 1 and Wg > 1:
        got.add("source-W=1")
    if (H, W) == (Hg, Wg):
        got.add("identity")
    return got
