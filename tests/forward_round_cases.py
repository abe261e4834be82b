"""Scenes with a DESIGNED tile list, for the round / queue structure of the blend forward (csrc/render_fwd.hip,
render_forward_mfma_body): a wave tests 64 list positions per round (option fwd_round = 64) or 32, appends the entries that reach
its 8 x 8 quadrant to a queue and blends chunks of 32 off it.  What a case fixes is the length L of ONE tile's list and which
positions of it reach which quadrant:

  quad    every entry a small splat inside quadrant 0 of the tile: wave 0 hits at every position, the other three waves see
          all-miss rounds and an empty queue at the end of the list
  full    every entry covers the whole tile (faint, nothing saturates): 64 hits per round in all four waves, the queue at capacity
  alt     positions alternate between quadrant 0 and quadrant 3: hit, miss, hit, ... - the two waves end on different (odd and
          even) hit counts, the other two see nothing
  opaque  `full` with a front of six opaque entries from position 5 L / 8 on: every pixel saturates inside the front - in the
          middle of a round and of a queued chunk - and the entries behind it are never blended

The camera is the identity (synth.make_camera), the Gaussians are isotropic (the rotation plays no part), list position i has
depth 4 + 0.02 i (no ties: the list order is the construction order).  Two small bystanders in tile (0, 0), in front of
everything, keep P > 0 at L = 0.  The lists meant are the reference's (option tile_cull = 0).
tests/test_forward_round_cases_cpu.py proves every design with the scalar oracle.  Helper module: no tests here."""
import functools

import numpy as np
import torch

LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 128, 129, 200)
PLACEMENTS = ("quad", "full", "alt", "opaque")
# feature width -> image and the designed tile (tx, ty); never tile (0, 0), which holds the bystanders
SIZES = {5: (64, 48, (2, 1)), 16: (32, 32, (1, 0)), 32: (32, 32, (0, 1)), 40: (64, 48, (1, 2)), 137: (32, 32, (1, 1)), 150: (32, 32, (1, 0))}
FRONT = 6                   # opaque entries of the `opaque` placement
FAINT = 0.03                # opacity of a whole-tile entry: 0.97^200 = 2e-3, far above the 1e-4 at which a pixel ends


def front_start(L):
    return (5 * L) // 8


def quadrant_of(placement, i):
    """The quadrant (0..3) a small entry at list position i lies in; None: the entry covers the whole tile."""
    if placement == "quad":
        return 0
    if placement == "alt":
        return 0 if i % 2 == 0 else 3
    return None


@functools.lru_cache(maxsize=None)
def scene(L, placement, C):
    """The scene of a case (shared: read, never written)."""
    from synth import make_scene
    W, H, (tx, ty) = SIZES[C]
    P = L + 2
    sc = make_scene(P=P, C=C, width=W, height=H, seed=1000 + 10 * L + PLACEMENTS.index(placement), sh_degree=0, with_depth_grad=True)
    fx, fy = W / (2.0 * sc["tanfovx"]), H / (2.0 * sc["tanfovy"])
    px, py, z = np.zeros(P), np.zeros(P), np.zeros(P)
    sig, op = np.zeros(P), np.zeros(P)
    # bystanders: ids L, L + 1 (the depth sort puts them first, their tile is not the designed one)
    px[L:], py[L:], z[L:], sig[L:], op[L:] = (4.0, 5.0), (4.0, 3.0), (2.0, 2.5), 0.3, 0.6
    rng = np.random.default_rng(77 + L)
    for i in range(L):
        z[i] = 4.0 + 0.02 * i
        q = quadrant_of(placement, i)
        if q is None:
            px[i], py[i] = 16 * tx + 7.5, 16 * ty + 7.5
            sig[i] = 40.0
            op[i] = 0.99 if placement == "opaque" and front_start(L) <= i < front_start(L) + FRONT else FAINT
        else:
            # sigma^2 = 0.09 + the 0.3 low-pass: radius 2, and the 1/255 footprint (3.3 sigma at most) ends 2.1 pixels from the
            # centre - centres 3 .. 4 pixels into the quadrant keep both inside it
            px[i] = 16 * tx + 8 * (q & 1) + 3.0 + 0.5 * (i % 3)
            py[i] = 16 * ty + 8 * (q >> 1) + 3.0 + 0.5 * ((i // 3) % 3)
            sig[i] = 0.3
            op[i] = rng.uniform(0.015, 0.03)      # faint: 200 of them on one pixel leave T above 2e-3, yet each is above 1/255 within a pixel of its centre
    x = ((2.0 * px + 1.0) / W - 1.0) * sc["tanfovx"] * z
    y = ((2.0 * py + 1.0) / H - 1.0) * sc["tanfovy"] * z
    sc["means3D"] = torch.from_numpy(np.stack([x, y, z], 1).astype(np.float32)).contiguous()
    sc["scales"] = torch.from_numpy(np.repeat((sig * z / fx)[:, None], 3, 1).astype(np.float32)).contiguous()
    sc["opacities"] = torch.from_numpy(op.astype(np.float32)[:, None]).contiguous()
    sc["case"] = dict(L=L, placement=placement, tile=(tx, ty), tile_index=ty * ((W + 15) // 16) + tx)
    return sc


def tile_block(plane, sc):
    """The designed tile's 16 x 16 block of a per-pixel plane (flat or H x W)."""
    W, H = sc["image_width"], sc["image_height"]
    tx, ty = sc["case"]["tile"]
    return np.asarray(plane).reshape(H, W)[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16]


def quadrants(block):
    """The four 8 x 8 quadrants of a tile block, in the kernel's order (q & 1: x half, q >> 1: y half)."""
    return [block[8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8] for q in range(4)]
