"""The binning chain between preprocess and the blend forward, on the edges its kernels switch at.

Between those two kernels the forward sorts the Gaussians by depth, hands their tile counts on IN DEPTH ORDER (the last pass of
the depth sort stores them where it used to store the sorted keys), adds them up, emits the (tile, id) entries and sorts those
by tile id in digits as wide as the tile count needs (binning.hip).  Every case here is compared with the scalar C++ oracle,
element for element and without a tolerance, as test_gpu_parity.test_binning_is_bit_exact does: `point_list` and `ranges`
under tile_cull = 0 are the reference's own lists.  Nothing is compared with the code under test.

  depth-sort regimes   the LSD passes, asked for by depth_sort_buckets = 0 (they are the default above 1,250,000 Gaussians; up to
                       there the default is the sort by buckets, tests/test_gpu_depth_bucket_sort.py) and confirmed by
                       depth_sort_info: P = 16,385 (first size beyond the one-workgroup sort: three 11-bit passes, the counts
                       handed on by the plain scatter), 200,000 (last size of that path), 200,001 (first size of the four 8-bit
                       passes, the counts handed on by the scatter that reorders its chunk in LDS) - all at 272 x 256 (272
                       tiles: 9 bits, digits of 5 + 4)
  tile-digit splits    256 tiles (8 bits, one pass), 255 tiles (8), 4,160 tiles (13 bits: 7 + 6, what 1080p runs),
                       8,256 tiles (14: 7 + 7), 16,512 tiles (15: 8 + 7)
  ties                 every depth key at least twice: equal keys keep ascending id through both sorts
  empty rows           a tenth of the Gaussians visible with NO tile (opacity 1e-6 under tile_cull = 1): zeros in the counts
  sync-free            the same lists from buffers carved for a provision, the count read on the device: the LSD passes at
                       both regimes, the sort by buckets at 16,385
"""
import numpy as np
import pytest

from test_gpu_parity import _lib, _raw_forward, _read, _scene
from util import run_oracle

pytestmark = pytest.mark.gpu

SMALL = dict(scale_lo=0.005, scale_hi=0.03)      # a few tiles per Gaussian: the oracle's forward stays within seconds

CASES = {
    # depth-sort regimes (17 x 16 tiles)
    "P16385": dict(P=16385, width=272, height=256, C=0, seed=31, **SMALL),
    "P200000": dict(P=200000, width=272, height=256, C=0, seed=32, **SMALL),
    "P200001": dict(P=200001, width=272, height=256, C=0, seed=33, **SMALL),
    # tile-digit splits
    "tiles256": dict(P=20000, width=256, height=256, C=0, seed=34, **SMALL),
    "tiles255": dict(P=20000, width=272, height=240, C=0, seed=35, **SMALL),
    "tiles4160": dict(P=20000, width=1024, height=1040, C=0, seed=36, **SMALL),
    "tiles8256": dict(P=20000, width=1536, height=1376, C=0, seed=37, **SMALL),
    "tiles16512": dict(P=3000, width=2048, height=2064, C=0, seed=38, **SMALL),      # 4.2 M pixels over near-empty lists
    # every depth key at least twice
    "ties": dict(P=16385, width=272, height=256, C=0, seed=39, **SMALL),
    # a tenth of the Gaussians without a tile
    "empty-rows": dict(P=20000, width=272, height=256, C=8, seed=40, **SMALL),
}
PER_GAUSSIAN = ("means3D", "scales", "rotations", "opacities", "shs", "semantic_feature")

_scenes, _wants = {}, {}


def _tiles(scene):
    return ((scene["image_width"] + 15) // 16) * ((scene["image_height"] + 15) // 16)


def _case_scene(name):
    if name not in _scenes:
        scene = _scene(**CASES[name])
        if name == "ties":
            # second half = first half, the odd last one = the first: every Gaussian has a twin at a higher id
            h = scene["P"] // 2
            for k in PER_GAUSSIAN:
                scene[k][h:2 * h] = scene[k][:h]
                scene[k][2 * h:] = scene[k][:1]
        if name == "empty-rows":
            scene["opacities"][::10] = 1e-6
        _scenes[name] = scene
    return _scenes[name]


def _oracle_lists(name):
    """The oracle's lists of a case, computed once and only read afterwards."""
    if name not in _wants:
        o, out, _ = run_oracle(_case_scene(name), backward=False)
        want = dict(n=out["num_rendered"], point_list=o.read("point_list").copy(), ranges=o.read("ranges").copy(),
                    tiles_touched=o.read("tiles_touched").copy(), radii=out["radii"].copy())
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _wants[name] = want
    return _wants[name]


def _sort_path():
    """Which depth sort the last forward call took (f3dgs_depth_sort_info)."""
    from diff_gaussian_rasterization import _C
    return _C.depth_sort_info()["path"]


def _assert_oracle_lists(name):
    scene, want = _case_scene(name), _oracle_lists(name)
    res = _raw_forward(scene)
    lib = _lib()
    n = res[0]
    assert n == want["n"]
    assert np.array_equal(res[4].cpu().numpy(), want["radii"])
    tt = _read(lib, "tiles_touched", scene, res, np.uint32, scene["P"])
    assert np.array_equal(tt, want["tiles_touched"])
    pl = _read(lib, "point_list", scene, res, np.uint32, n)
    wrong = np.flatnonzero(pl != want["point_list"])
    assert wrong.size == 0, f"{wrong.size} of {n} entries differ, the first at {wrong[0]}"
    rg = _read(lib, "ranges", scene, res, np.uint32, 2 * _tiles(scene))
    assert np.array_equal(rg, want["ranges"])
    return res


@pytest.mark.parametrize("name", ["P16385", "P200000", "P200001"])
def test_depth_sort_regimes_give_the_oracles_lists(name, option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 0)
    _assert_oracle_lists(name)
    assert _sort_path() == "passes"


@pytest.mark.parametrize("name,tiles", [("tiles256", 256), ("tiles255", 255), ("tiles4160", 4160), ("tiles8256", 8256),
                                        ("tiles16512", 16512)])
def test_tile_digit_splits_give_the_oracles_lists(name, tiles, option):
    option("tile_cull", 0)
    assert _tiles(_case_scene(name)) == tiles
    _assert_oracle_lists(name)


def test_tied_depth_keys_keep_ascending_id(option):
    """Every Gaussian has an exact copy at a higher id, so every depth key occurs at least twice: the oracle's stable sort lists
    the copies of a tile in ascending id, and so must two stable sorts one behind the other."""
    option("tile_cull", 0)
    scene, want = _case_scene("ties"), _oracle_lists("ties")
    h = scene["P"] // 2
    assert np.array_equal(want["tiles_touched"][:h], want["tiles_touched"][h:2 * h]) and want["n"] > 0
    _assert_oracle_lists("ties")


def test_gaussians_without_a_tile_leave_the_lists_in_order(option):
    """tile_cull = 1 with a tenth of the opacities at 1e-6: those Gaussians are visible (radius > 0) and own no list entry, so
    the counts handed through the depth sort hold zeros.  Every tile's list is the oracle's list of that tile with entries
    left out - the same order - and the images are those of the tile_cull = 0 run, bit for bit."""
    scene, want = _case_scene("empty-rows"), _oracle_lists("empty-rows")
    lib = _lib()
    tiles = _tiles(scene)
    option("tile_cull", 0)
    full = _assert_oracle_lists("empty-rows")
    images = [full[k].cpu().numpy() for k in (1, 2, 3)]
    option("tile_cull", 1)
    res = _raw_forward(scene)
    assert res[0] == want["n"]                      # the reference's count, whatever the lists hold
    radii = res[4].cpu().numpy()
    assert np.array_equal(radii, want["radii"])
    tt = _read(lib, "tiles_touched", scene, res, np.uint32, scene["P"])
    faint = np.zeros(scene["P"], bool)
    faint[::10] = True
    n_faint_visible = int((radii[faint] > 0).sum())
    print(f"faint and visible: {n_faint_visible}, their list entries: {int(tt[faint].sum())}")
    assert n_faint_visible > scene["P"] // 40 and int(tt[faint].sum()) == 0
    assert np.all(tt <= want["tiles_touched"])
    n_own = int(_read(lib, "counters", scene, res, np.uint32, 16)[0])
    assert n_own == int(tt.sum()) and 0 < n_own < want["n"]
    pl = _read(lib, "point_list", scene, res, np.uint32, n_own)
    rg = _read(lib, "ranges", scene, res, np.uint32, 2 * tiles).reshape(tiles, 2)
    org = want["ranges"].reshape(tiles, 2)
    listed = 0
    where = np.full(scene["P"], -1, np.int64)
    for t in range(tiles):
        mine = pl[rg[t, 0]:rg[t, 1]]
        theirs = want["point_list"][org[t, 0]:org[t, 1]]
        where[theirs] = np.arange(theirs.size)      # (a Gaussian is listed once per tile)
        at = where[mine]
        assert np.all(at >= 0) and np.all(np.diff(at) > 0), f"tile {t}: not the oracle's list with entries left out"
        where[theirs] = -1
        listed += mine.size
    assert listed == n_own
    for got, ref in zip((res[k].cpu().numpy() for k in (1, 2, 3)), images):
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("name,buckets,path", [("P16385", 0, "passes"), ("P200001", 0, "passes"), ("P16385", 1, "buckets")],
                         ids=["P16385", "P200001", "P16385-buckets"])
def test_sync_free_provision_gives_the_oracles_lists(name, buckets, path, option):
    """sync_free = 1 with room to spare: every launch is sized by the provision, the kernels take the count from the device."""
    option("tile_cull", 0)
    option("depth_sort_buckets", buckets)
    option("sync_free", 1)
    option("instance_capacity", 2 * _oracle_lists(name)["n"] + 1000)
    _assert_oracle_lists(name)
    assert _sort_path() == path
    from diff_gaussian_rasterization import _C
    c = _C.forward_counts()
    assert c[0] == _oracle_lists(name)["n"] and c[3] == 2 * c[0] + 1000 and c[4] == 0
