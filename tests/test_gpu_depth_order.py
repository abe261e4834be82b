"""The depth ORDER of every sort path, against a stable argsort of the keys (binning.hip: launch_depth_sort and the look-back passes).

A depth sort reads `depth_key` (uint32 per Gaussian: the float bits of view z, all-ones where culled) and leaves the ids in `order`
(GeomState::val_a), ascending by key, equal keys in ascending id.  `np.argsort(keys, kind="stable")` is its complete and exact
reference, at any P, in milliseconds.  Every case here checks

  keys     depth_key read back is the DESIGNED key on the alive set and all-ones elsewhere (designed cases), or the float bits of
           the input's z where the forward kept the Gaussian (plain scenes) - so the reference never depends on the sort
  order    `order` read back equals the stable argsort of those keys, all P entries, no tolerance
  counts   behind a multi-launch sort key_a holds tiles_touched[order[i]] ("order_counts": what every later stage reads its
           offsets from); behind the one-launch sort it holds the sorted keys
  path     _C.depth_sort_info(): the path, bin count, largest bucket and oversized buckets the case's name claims

  designed cases   tests/depth_order_cases.py: one bucket of exactly n pairs that differ in exactly m bits - the in-LDS sort at
                   steps 1 / 2, a wave's partial step, the capacity, zero to FOUR passes; the streaming sort of a bucket above
                   the capacity at its first size, at exactly two chunks, two chunks and one item, five chunks, with one, three
                   and five passes (the fifth past bit 32); two oversized buckets beside ordinary ones.  Proven on the CPU by the
                   scalar oracle (tests/test_depth_order_cases_cpu.py); three of them also compared with the oracle's lists here
  other flavours   the same keys through the three 11-bit LSD passes and through the look-back passes
  LSD regimes      P = 16,385 / 200,000 (three 11-bit passes) and 200,001 (four 8-bit passes, the reordering scatter), tied keys
  one launch       P = 1, 63, 64, 65, 1,024, 1,025, 15,360, 15,361, 16,383, 16,384; 16,384 equal keys; 16,384 culled
  large P          1,250,000 (buckets, 1,024 bins), 1,250,001 (passes by default; 2,048 bins under option 1 - the 11-bit bucket
                   pass), 1,250,001 with 60 % of the keys on two jittered planes (oversized buckets beside ordinary bins); there
                   also the tile sort over millions of entries, by numpy alone: sorted tile ids, ranges = run boundaries, every
                   Gaussian listed tiles_touched times, and depth rank rising strictly inside every tile's run
"""
import numpy as np
import pytest
import torch

import depth_order_cases as doc
from test_gpu_parity import _lib, _raw_forward, _read, _scene

pytestmark = pytest.mark.gpu

AUTO_UPTO = 1250000          # common.h: DEPTH_BUCKET_AUTO_UPTO = DEPTH_BUCKET_WIDE_ABOVE


def _info():
    from diff_gaussian_rasterization import _C
    torch.cuda.synchronize()
    return _C.depth_sort_info()


def _tiles(scene):
    return ((scene["image_width"] + 15) // 16) * ((scene["image_height"] + 15) // 16)


def _same(got, want, what):
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, (f"{what}: {wrong.size} of {want.size} entries differ, the first at {wrong[0]}: "
                             f"{got[wrong[0]]} for {want[wrong[0]]}")


def _check_order(label, scene, path, keys=None, counts=True):
    """One forward; keys, order, counts in order and the path against the stable argsort.  `keys` None: a plain scene under the
    identity camera - the keys are the float bits of the input's z where the forward's radii are positive.
    Returns (res, info, keys, expected order)."""
    P = scene["P"]
    res = _raw_forward(scene)
    info = _info()
    print(label, info)
    assert info["path"] == path, info
    lib = _lib()
    radii = res[4].cpu().numpy()
    if keys is None:
        keys = doc.keys_of_plain_scene(scene, radii)
    assert np.array_equal(radii > 0, keys != doc.CULLED_KEY)
    _same(_read(lib, "depth_key", scene, res, np.uint32, P), keys, "depth_key")
    want = doc.expected_order(keys)
    _same(_read(lib, "order", scene, res, np.uint32, P), want, "order")
    if counts:
        got = _read(lib, "order_counts", scene, res, np.uint32, P)
        if path == "one_launch":
            _same(got, keys[want], "sorted keys in key_a")
        else:
            assert path in ("buckets", "passes")
            tt = _read(lib, "tiles_touched", scene, res, np.uint32, P)
            assert np.all(tt[keys == doc.CULLED_KEY] == 0)
            _same(got, tt[want], "order_counts")
    return res, info, keys, want


def _assert_oracle_lists(name, res):
    scene, want = doc.designed_scene(name), doc.designed_oracle(name)
    lib = _lib()
    n = res[0]
    assert n == want["n"] > 0
    assert np.array_equal(res[4].cpu().numpy(), want["radii"])
    assert np.array_equal(_read(lib, "tiles_touched", scene, res, np.uint32, scene["P"]), want["tiles_touched"])
    _same(_read(lib, "point_list", scene, res, np.uint32, n), want["point_list"], "point_list")
    assert np.array_equal(_read(lib, "ranges", scene, res, np.uint32, 2 * _tiles(scene)), want["ranges"])


# ---- designed cases ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", doc.DESIGNED)
def test_designed_buckets_come_out_in_key_order(name, option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 1)
    d = doc.design(name)
    res, info, _k, _o = _check_order(name, doc.designed_scene(name), "buckets", d["keys"])
    lay = doc.bucket_layout(d["keys"], d["P"])
    assert info["buckets"] == 32 and info["capacity"] == doc.CAPACITY
    assert info["largest"] == lay["largest"] and info["oversized"] == d["oversized"] == lay["oversized"]
    if name != "mixed":
        assert info["largest"] == d["n"]
    if name in doc.ORACLE_LIST_CASES:
        _assert_oracle_lists(name, res)


@pytest.mark.parametrize("flavour", ["passes", "lookback"])
@pytest.mark.parametrize("name", doc.OTHER_FLAVOUR_CASES)
def test_designed_keys_through_the_other_flavours(name, flavour, option):
    option("tile_cull", 0)
    if flavour == "passes":
        option("depth_sort_buckets", 0)
    else:
        option("sort_onesweep", 1)
    _check_order(f"{name}/{flavour}", doc.designed_scene(name), flavour, doc.design(name)["keys"], counts=flavour == "passes")


# ---- the LSD passes at their regime edges -----------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [16385, 200000, 200001])
def test_lsd_regime_edges_on_tied_keys(P, option):
    """Three 11-bit passes up to 200,000 Gaussians, four 8-bit passes with the reordering scatter beyond; the second half of the
    scene is a copy of the first, so every key is tied and the copy must follow its original."""
    option("tile_cull", 0)
    option("depth_sort_buckets", 0)
    scene = doc.ties_scene(P, seed=81 + P % 5)
    _res, _info_, keys, want = _check_order(f"ties P={P}", scene, "passes")
    h = P // 2
    assert np.array_equal(keys[:h], keys[h:2 * h]) and (keys != doc.CULLED_KEY).sum() > P // 2
    rank = np.empty(P, np.int64)
    rank[want] = np.arange(P)
    alive = np.flatnonzero(keys[:h] != doc.CULLED_KEY)
    twins = rank[alive + h] - rank[alive]
    assert np.all(twins >= 1) and (twins == 1).sum() > alive.size // 2      # (apart only where more than two keys tie)


# ---- the one-launch sort ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 63, 64, 65, 1024, 1025, 15360, 15361, 16383, 16384])
def test_one_launch_sizes(P, option):
    # (1,024 / 1,025 and 15,360 / 15,361: one step of the shared in-LDS pass against two, fifteen against sixteen; at every size the
    # scalar oracle keeps more than half of the scene of seed 90 + P % 11 alive)
    option("tile_cull", 0)
    scene = _scene(P=P, C=0, seed=90 + P % 11, sh_degree=0, **doc.IMG, **doc.SMALL)
    if P == 1:
        scene["means3D"][0] = torch.tensor([0.1, -0.1, 3.0])
    _res, _i, keys, _o = _check_order(f"P={P}", scene, "one_launch")
    assert (keys != doc.CULLED_KEY).sum() >= max(1, P // 2)


@pytest.mark.parametrize("kind", ["equal-keys", "all-culled"])
def test_one_launch_at_its_capacity_on_one_key(kind, option):
    option("tile_cull", 0)
    P = 16384
    keys = np.full(P, doc.f32_bits(5.0) if kind == "equal-keys" else doc.CULLED_KEY, np.uint32)
    scene = doc.scene_from_keys(keys, P, seed=97, culled=keys == doc.CULLED_KEY)
    res, _i, _k, want = _check_order(kind, scene, "one_launch", keys)
    assert np.array_equal(want, np.arange(P, dtype=np.uint32)) and (res[0] > 0) == (kind == "equal-keys")


# ---- large P: the upper end of the bucket path, the 11-bit bucket pass, the tile sort at millions of entries -----------------

@pytest.fixture(scope="module")
def large():
    """One scene of 1,250,001 Gaussians, its cut to 1,250,000, and the same with 60 % of the depths on two jittered planes."""
    P = AUTO_UPTO + 1
    full = _scene(P=P, C=0, seed=70, sh_degree=0, **doc.IMG, scale_lo=0.002, scale_hi=0.006)
    cut = dict(full, P=AUTO_UPTO, **{k: v[:AUTO_UPTO].contiguous() for k, v in full.items()
                                     if torch.is_tensor(v) and v.dim() and v.shape[0] == P})
    rng = np.random.default_rng(71)
    m = full["means3D"].clone()
    i = torch.arange(P)
    for plane, lo in ((3.0, 0), (7.0, 3)):
        sel = (i % 10 >= lo) & (i % 10 < lo + 3) & (m[:, 2] >= 2.0)            # (not the recipe's near-plane share)
        bits = doc.f32_bits(plane) + rng.integers(0, 1 << 12, int(sel.sum()))
        z = torch.from_numpy(bits.astype(np.uint32).view(np.float32).copy())
        m[sel] = m[sel] * (z / m[sel, 2]).unsqueeze(1)                         # along the view ray, as _set_z does
        m[sel, 2] = z          # exactly
    planes = dict(full, means3D=m.contiguous())
    return dict(full=full, cut=cut, planes=planes)


def _assert_tile_sort(scene, res, want_order):
    """The tile sort behind a correct depth order, by numpy alone (tile_cull = 0)."""
    lib = _lib()
    P, tiles = scene["P"], _tiles(scene)
    n = int(_read(lib, "counters", scene, res, np.uint32, 16)[0])
    assert n == res[0] > 10 ** 6
    ts = _read(lib, "tile_sorted", scene, res, np.uint32, n)
    pl = _read(lib, "point_list", scene, res, np.uint32, n)
    rg = _read(lib, "ranges", scene, res, np.uint32, 2 * tiles).reshape(tiles, 2)
    tt = _read(lib, "tiles_touched", scene, res, np.uint32, P)
    assert int(ts.max()) < tiles and np.all(ts[1:] >= ts[:-1])
    t = np.arange(tiles, dtype=np.uint32)
    lo, hi = np.searchsorted(ts, t, "left"), np.searchsorted(ts, t, "right")
    want_rg = np.stack([lo, hi], 1).astype(np.uint32)
    want_rg[hi == lo] = 0                                    # (an empty tile: both zero, as the oracle writes them)
    assert np.array_equal(rg, want_rg)
    assert int(pl.max()) < P and np.array_equal(np.bincount(pl, minlength=P), tt)
    rank = np.empty(P, np.int64)
    rank[want_order] = np.arange(P)
    r = rank[pl]
    bad = np.flatnonzero((ts[1:] == ts[:-1]) & (r[1:] <= r[:-1]))
    assert bad.size == 0, f"{bad.size} entries not behind their predecessor in depth, the first at {bad[0] + 1}"


@pytest.mark.parametrize("which,opt,path,bins", [("cut", -1, "buckets", 1024), ("full", -1, "passes", 0),
                                                 ("full", 1, "buckets", 2048), ("planes", 1, "buckets", 2048)])
def test_large_p(which, opt, path, bins, large, option):
    from diff_gaussian_rasterization import _C
    option("tile_cull", 0)
    assert _C.get_option("depth_sort_buckets") == -1
    if opt != -1:
        option("depth_sort_buckets", opt)
    scene = large[which]
    assert scene["P"] == (AUTO_UPTO if which == "cut" else AUTO_UPTO + 1)
    res, info, keys, want = _check_order(f"{which}/{opt}", scene, path)
    assert info["buckets"] == bins
    if path == "buckets":
        lay = doc.bucket_layout(keys, scene["P"])
        assert lay["count"] == bins and info["largest"] == lay["largest"] and info["oversized"] == lay["oversized"]
        if which == "planes":
            on_planes = sum(int(((keys >= doc.f32_bits(z)) & (keys < doc.f32_bits(z) + 4096)).sum()) for z in (3.0, 7.0))
            # (the shift is the smallest that fits the range: more than half of the bins are spanned, and the spread fills them)
            assert on_planes > scene["P"] // 2 and lay["oversized"] >= 2 and (lay["sizes"] > 0).sum() > bins // 2
        else:
            assert lay["oversized"] == 0 and lay["largest"] > 0
    _assert_tile_sort(scene, res, want)
