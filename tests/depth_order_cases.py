"""Scenes built from DESIGNED depth keys, for the order checks of the depth sort (csrc/binning.hip: launch_depth_sort).

The depth sort reads one uint32 key per Gaussian - the float bits of its view-space z, all-ones where it is culled - and leaves
the ids in ascending key order, equal keys in ascending id.  Its complete, exact reference is `np.argsort(keys, kind="stable")`.
A case here chooses the keys so that the bucket path (one stable pass on (key - kmin) >> shift, then one workgroup per bucket)
meets one named situation: a bucket of exactly n pairs whose keys differ in exactly m low bits, which fixes the number of 8-bit
passes of the in-LDS sort (n <= 8,064) or of the streaming sort (n > 8,064).

A designed case is
  * one GROUP of n alive Gaussians with keys base + r, r drawn with repetition from [0, 2^m) (ties are wanted),
  * two alive OUTLIERS, the nearest and the farthest Gaussian of the frame: they fix kmin, kmax and so the shift s,
  * everything else behind the camera (culled: thousands of ids for the workgroups that move the culled bin),
with base = kmin + j 2^s, so that the whole group is bucket j.  P = 20,000, where the pass uses 32 bins.

`depth_bucket_count / _bits / _shift` restate common.h in a handful of lines; tests/test_depth_order_cases_cpu.py checks them
against the header's own static_asserts and proves every design with the scalar oracle alone.  Helper module: no tests here."""
import functools

import numpy as np
import torch

P_DESIGNED = 20000
CAPACITY = 8064              # common.h: DEPTH_BUCKET_CAP
STREAM_CHUNK = 4096          # depth_bucket_stream_sort: 512 threads x 8 items
CULLED_KEY = np.uint32(0xFFFFFFFF)
IMG = dict(width=272, height=256)
SMALL = dict(scale_lo=0.005, scale_hi=0.03)      # a few tiles per Gaussian: the oracle's forward stays within seconds


# ---- common.h, restated -----------------------------------------------------------------------------------------------------

def depth_bucket_bits(P):
    return 11 if P > 1250000 else 10


def depth_bucket_count(P):
    most, c = 1 << depth_bucket_bits(P), 16
    while c < most and c * 1024 < P:
        c <<= 1
    return c


def depth_bucket_shift(kmin, kmax, count):
    rng = int(kmax) - int(kmin) if int(kmax) > int(kmin) else 0
    s = 0
    while (rng >> s) > count - 2:
        s += 1
    return s


def bits_of(x):
    return int(x).bit_length()


def bucket_layout(keys, P=None):
    """What the bucket pass makes of `keys` (uint32, all-ones = culled): kmin, kmax, count, shift, every alive key's bucket, the
    bucket sizes, the largest one and how many are above the capacity."""
    keys = np.asarray(keys, np.uint32)
    P = keys.size if P is None else P
    alive = keys != CULLED_KEY
    count = depth_bucket_count(P)
    if not alive.any():
        return dict(kmin=0xFFFFFFFF, kmax=0, count=count, shift=0, alive=alive, bucket=np.zeros(0, np.int64),
                    sizes=np.zeros(count - 1, np.int64), largest=0, oversized=0)
    kmin, kmax = int(keys[alive].min()), int(keys[alive].max())
    s = depth_bucket_shift(kmin, kmax, count)
    bucket = (keys[alive].astype(np.int64) - kmin) >> s
    sizes = np.bincount(bucket, minlength=count - 1)
    return dict(kmin=kmin, kmax=kmax, count=count, shift=s, alive=alive, bucket=bucket, sizes=sizes,
                largest=int(sizes.max()), oversized=int((sizes > CAPACITY).sum()))


def sort_passes(keys_of_bucket, kmin, s):
    """8-bit passes a bucket's workgroup needs: bits(OR of ((key - kmin) & (2^s - 1)) ^ the first one), in digits of 8.
    keys_of_bucket in id order (the stable bucket pass keeps it)."""
    rel = (np.asarray(keys_of_bucket).astype(np.int64) - int(kmin)) & ((1 << s) - 1)
    diff = int(np.bitwise_or.reduce(rel ^ rel[0]))
    return (bits_of(diff) + 7) // 8


def stream_passes(real):
    """The streaming sort ends on the other buffer side: an even pass count (zero included) gets a copy pass on top."""
    return real + 1 if real % 2 == 0 else real


def expected_order(keys):
    """The depth order: a stable argsort of the uint32 keys.  Culled keys are all-ones: they come last, in id order."""
    return np.argsort(np.asarray(keys, np.uint32), kind="stable").astype(np.uint32)


def f32_bits(z):
    return int(np.float32(z).view(np.uint32))


# ---- scenes -----------------------------------------------------------------------------------------------------------------

def scene_from_keys(keys_u32, P, seed, culled=None, center=()):
    """synth.make_scene (C = 0, SH degree 0, 272 x 256, small splats) with every Gaussian moved along its view ray to
    z = keys.view(float32), as tests/test_gpu_depth_bucket_sort._set_z does - the camera is the identity, so view z is z bit for
    bit.  The rays are kept inside 0.9 of the frustum (the recipe puts a share of them outside the image, where a small splat owns
    no tile and is not alive): a Gaussian on a ray through the image is alive at any z > 0.2.  `culled` (bool mask) go behind the
    camera, `center` (ids) onto the optical axis."""
    from synth import make_scene
    keys = np.ascontiguousarray(keys_u32, np.uint32)
    assert keys.shape == (P,)
    sc = make_scene(P=P, C=0, seed=seed, sh_degree=0, **IMG, **SMALL)
    culled = np.zeros(P, bool) if culled is None else np.asarray(culled, bool)
    z = torch.from_numpy(np.where(culled, np.float32(1.0).view(np.uint32), keys).astype(np.uint32).view(np.float32).copy())
    assert bool(torch.isfinite(z).all()) and bool((z > 0.2).all())
    m = sc["means3D"]
    ray = torch.nan_to_num(m[:, :2] / m[:, 2:3], nan=0.0, posinf=0.0, neginf=0.0)
    lim = 0.9 * torch.tensor([sc["tanfovx"], sc["tanfovy"]], dtype=torch.float32)
    ray = torch.minimum(torch.maximum(ray, -lim), lim)
    if len(center):
        ray[torch.tensor(list(center), dtype=torch.long)] = 0.0
    m[:, :2] = ray * z.unsqueeze(1)
    m[:, 2] = z          # exactly
    cm = torch.from_numpy(culled.copy())
    m[cm] = torch.tensor([0.0, 0.0, -1.0])
    return sc


def ties_scene(P, seed):
    """A plain make_scene scene whose second half is a copy of the first (the odd last one a copy of the first Gaussian): every
    depth key occurs at least twice."""
    from synth import make_scene
    sc = make_scene(P=P, C=0, seed=seed, sh_degree=0, **IMG, **SMALL)
    h = P // 2
    for k in ("means3D", "scales", "rotations", "opacities", "shs", "semantic_feature"):
        sc[k][h:2 * h] = sc[k][:h]
        sc[k][2 * h:] = sc[k][:1]
    return sc


def keys_of_plain_scene(scene, radii):
    """The depth keys of a scene under the identity camera, given which Gaussians the forward kept (radii > 0)."""
    k = scene["means3D"][:, 2].numpy().view(np.uint32).copy()
    k[np.asarray(radii).reshape(-1) <= 0] = CULLED_KEY
    return k


# ---- the designed cases -----------------------------------------------------------------------------------------------------

NEAR_FAR = (0.21, 1e5)           # kmin, kmax of most cases: range 0x096C45C3, 18 buckets of 2^23 keys (one octave each)
# The fourth pass needs differing bits above 24, so a shift of 25 at least: (kmax - kmin) >> 24 > 30, 62 octaves and more over the
# 31 bins in use.  0.25 .. 2^61 is 63 octaves (range 0x1F800000, shift 25: 15 buckets of four octaves).  2^61 squared is 2^122 and
# still a float, which the EWA setup needs; the oracle reports that Gaussian alive with a finite radius (the CPU test asserts
# it), so nothing had to be moved inward.
WIDE = (0.25, 2.0 ** 61)

#        name                 n      m   outliers  j    (the group is bucket j: base = kmin + j 2^s)
_TABLE = [
    ("lds-1pass-64",          64,    8,  NEAR_FAR, 4),
    ("lds-1pass-65",          65,    8,  NEAR_FAR, 4),
    ("lds-1pass-512",         512,   8,  NEAR_FAR, 4),
    ("lds-1pass-513",         513,   8,  NEAR_FAR, 4),
    ("lds-2pass-8063",        8063,  16, NEAR_FAR, 4),
    ("lds-2pass-8064",        8064,  16, NEAR_FAR, 4),
    ("lds-3pass-5000",        5000,  23, NEAR_FAR, 4),
    ("lds-4pass-5000",        5000,  25, WIDE,     1),
    ("lds-onekey-700",        700,   0,  NEAR_FAR, 4),
    ("stream-1pass-8065",     8065,  5,  NEAR_FAR, 4),
    ("stream-3pass-8192",     8192,  12, NEAR_FAR, 4),
    ("stream-3pass-8193",     8193,  12, NEAR_FAR, 4),
    ("stream-3pass-18000",    18000, 20, NEAR_FAR, 4),
    ("stream-5pass-12289",    12289, 25, WIDE,     1),
]
GROUP_CASES = [t[0] for t in _TABLE]
DESIGNED = GROUP_CASES + ["mixed"]
ORACLE_LIST_CASES = ["stream-3pass-8193", "stream-5pass-12289", "lds-4pass-5000"]
OTHER_FLAVOUR_CASES = ["stream-3pass-18000", "lds-4pass-5000", "mixed"]
MIXED_PLANES = (3.0, 7.0)
MIXED_N, MIXED_M, MIXED_SPREAD = 9000, 12, 1600


@functools.lru_cache(maxsize=None)
def design(name):
    """The keys of a designed case and what they are meant to reach.  Nothing in the result may be modified."""
    P = P_DESIGNED
    idx = DESIGNED.index(name)
    rng = np.random.default_rng(7000 + idx)
    keys = np.full(P, CULLED_KEY, np.uint32)
    ids = rng.permutation(P)
    if name == "mixed":
        # `skew` with jitter on both planes: two buckets above the capacity whose keys differ in 12 bits, a spread over 2 .. 10
        # beside them (its ends pinned, so that kmin, kmax and the shift do not hang on the draw), the rest culled
        lo, hi = f32_bits(2.0), f32_bits(10.0)
        a, b = np.sort(ids[:MIXED_N]), np.sort(ids[MIXED_N:2 * MIXED_N])
        spread = np.sort(ids[2 * MIXED_N:2 * MIXED_N + MIXED_SPREAD])
        keys[a] = f32_bits(MIXED_PLANES[0]) + rng.integers(0, 1 << MIXED_M, a.size)
        keys[b] = f32_bits(MIXED_PLANES[1]) + rng.integers(0, 1 << MIXED_M, b.size)
        keys[spread] = rng.uniform(2.0, 10.0, spread.size).astype(np.float32).view(np.uint32)
        keys[spread[0]], keys[spread[-1]] = lo, hi
        s = depth_bucket_shift(lo, hi, depth_bucket_count(P))
        d = dict(name=name, P=P, keys=keys, culled=keys == CULLED_KEY, groups=(a, b), outliers=(spread[0], spread[-1]),
                 kmin=lo, kmax=hi, shift=s, m=MIXED_M, n=MIXED_N, stream=True, oversized=2,
                 group_buckets=tuple((f32_bits(z) - lo) >> s for z in MIXED_PLANES))
    else:
        _, n, m, (near, far), j = _TABLE[idx]
        kmin, kmax = f32_bits(near), f32_bits(far)
        s = depth_bucket_shift(kmin, kmax, depth_bucket_count(P))
        assert m <= s
        group = np.sort(ids[:n])
        o_near, o_far = ids[n], ids[n + 1]
        base = kmin + (j << s)
        keys[group] = base + rng.integers(0, 1 << m, n)
        keys[o_near], keys[o_far] = kmin, kmax
        real = (m + 7) // 8
        stream = n > CAPACITY
        d = dict(name=name, P=P, keys=keys, culled=keys == CULLED_KEY, groups=(group,), outliers=(o_near, o_far), kmin=kmin,
                 kmax=kmax, shift=s, m=m, n=n, stream=stream, oversized=int(stream), group_buckets=(j,), real_passes=real,
                 passes=stream_passes(real) if stream else real, chunks=-(-n // STREAM_CHUNK) if stream else 0)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    for g in d["groups"]:
        g.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def designed_scene(name):
    """The scene of a designed case (shared by every test of it: read, never written)."""
    d = design(name)
    center = [int(i) for i in d["outliers"]] if name != "mixed" else []
    return scene_from_keys(d["keys"], d["P"], seed=900 + DESIGNED.index(name), culled=d["culled"], center=center)


@functools.lru_cache(maxsize=None)
def designed_oracle(name):
    """The scalar oracle's forward of a designed case, run once: radii, depths, tile counts and lists (read-only)."""
    from util import run_oracle
    o, out, _ = run_oracle(designed_scene(name), backward=False)
    want = dict(n=out["num_rendered"], radii=out["radii"].copy(), depths=o.read("depths").copy(),
                tiles_touched=o.read("tiles_touched").copy(), point_list=o.read("point_list").copy(),
                ranges=o.read("ranges").copy())
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return want
