"""Designed depth keys for the LAYOUT edges of the bucket depth sort (csrc/binning.hip: the B side as (key, id) pairs, the
row-major histogram matrix and its column scan).  Same conventions as tests/depth_order_cases.py, whose arithmetic and scene
builder are reused: P = 20,000 (32 bins), the nearest and the farthest Gaussian fix kmin, kmax and the shift, one GROUP of n
alive Gaussians is one bucket, everything else is culled.

What is new here is WHERE the group's bucket starts.  A bucket above the capacity is sorted by its workgroup alone in streaming
passes; its scratch is its own 2 n words of the B side, which begin at pair index `offset` = alive keys in the buckets in front.
`lead` extra alive keys in a bucket between the near outlier and the group make that offset odd (1 + lead), and n itself is odd,
so the scratch's value half starts on an odd word.

  equal-8065      8,065 equal keys: no two differ, the streaming sort is its single copy pass (pairs in, A side out)
  scratch-8065    8,065 keys that differ in 12 bits: two real passes and a copy, so the scratch is written and read back

Helper module: no tests here; tests/test_depth_bucket_layout_cases_cpu.py proves both with the scalar oracle."""
import functools

import numpy as np

import depth_order_cases as doc

SORT_CHUNK = 2048            # common.h: SORT_THREADS x SORT_ITEMS keys per histogram row
COLSCAN_SWEEP_ROWS = 512     # common.h: COLSCAN_ROW_LANES x COLSCAN_RUN rows per sweep of radix_colscan_kernel

#        name             n     m   lead  j   lead bucket
_TABLE = [
    ("equal-8065",        8065, 0,  2,    4,  2),
    ("scratch-8065",      8065, 12, 2,    4,  2),
]
CASES = [t[0] for t in _TABLE]


def matrix_rows(P):
    return -(-P // SORT_CHUNK)


@functools.lru_cache(maxsize=None)
def design(name):
    """The keys of a case and what they are meant to reach.  Nothing in the result may be modified."""
    P = doc.P_DESIGNED
    idx = CASES.index(name)
    _, n, m, lead, j, jl = _TABLE[idx]
    rng = np.random.default_rng(7700 + idx)
    kmin, kmax = doc.f32_bits(doc.NEAR_FAR[0]), doc.f32_bits(doc.NEAR_FAR[1])
    s = doc.depth_bucket_shift(kmin, kmax, doc.depth_bucket_count(P))
    assert m <= s and 0 < jl < j
    keys = np.full(P, doc.CULLED_KEY, np.uint32)
    ids = rng.permutation(P)
    group = np.sort(ids[:n])
    o_near, o_far = ids[n], ids[n + 1]
    leads = np.sort(ids[n + 2:n + 2 + lead])
    base = kmin + (j << s)
    keys[group] = base + 12345 + (rng.integers(0, 1 << m, n) if m else 0)
    keys[leads] = kmin + (jl << s) + rng.integers(0, 1 << 8, lead)
    keys[o_near], keys[o_far] = kmin, kmax
    real = (m + 7) // 8
    d = dict(name=name, P=P, keys=keys, culled=keys == doc.CULLED_KEY, group=group, leads=leads, outliers=(o_near, o_far),
             kmin=kmin, kmax=kmax, shift=s, m=m, n=n, bucket=j, offset=1 + lead, real_passes=real, passes=doc.stream_passes(real))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def designed_scene(name):
    """The scene of a case (shared by every test of it: read, never written)."""
    d = design(name)
    return doc.scene_from_keys(d["keys"], d["P"], seed=950 + CASES.index(name), culled=d["culled"],
                               center=[int(i) for i in d["outliers"]])
