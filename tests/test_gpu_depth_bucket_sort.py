"""The depth sort by buckets (option depth_sort_buckets, binning.hip): one stable pass cuts the depth keys into buckets by
(key - smallest alive key) >> shift, one launch sorts every bucket inside LDS - in place of three or four LSD passes.

Every expectation is the scalar C++ oracle's: `point_list`, `ranges`, `tiles_touched`, `radii` and `num_rendered`, element for
element and without a tolerance, under tile_cull = 0 (the reference's own lists) unless a case says otherwise.  Nothing is
compared with the code under test, except where a case IS the equality of two paths.  `_C.depth_sort_info()` says which path the
forward took, so no case passes without reaching the one it names.

  sizes        P = 16,385 (the first size beyond the one-workgroup sort), 20,000, 70,001 (no multiple of any workgroup size)
  ties         every depth key at least twice: equal keys keep ascending id
  one depth    20,000 Gaussians at one view-space z: kmin == kmax (shift 0), one bucket above the in-LDS capacity, sorted by
               its workgroup alone in streaming passes
  skew         90 % on two depth planes, 10 % over 2 .. 10: buckets above the capacity beside ordinary ones
  outliers     z in 2 .. 10, one Gaussian at 0.21 and one at 1e5: nineteen octaves more of range, the same order
  few / none   every Gaussian behind the camera; exactly one in front
  culled share half of the Gaussians outside the frustum: the last bin holds them
  path equality, auto threshold, graph capture
"""
import numpy as np
import pytest
import torch

from test_gpu_parity import _lib, _raw_forward, _read, _scene
from util import run_oracle

pytestmark = pytest.mark.gpu

SMALL = dict(scale_lo=0.005, scale_hi=0.03)      # a few tiles per Gaussian: the oracle's forward stays within seconds
IMG = dict(width=272, height=256)
CAPACITY = 8064              # common.h: DEPTH_BUCKET_CAP
AUTO_ABOVE = 16384           # common.h: DEPTH_BUCKET_AUTO_ABOVE (= SMALL_SORT_MAX: the one-launch sort below it)
AUTO_UPTO = 1250000          # common.h: DEPTH_BUCKET_AUTO_UPTO

_scenes, _wants = {}, {}


def _plain(P, seed, C=0):
    return _scene(P=P, C=C, seed=seed, **IMG, **SMALL)


def _set_z(scene, z):
    """Move the Gaussians along their view rays to depth z (the camera of synth.make_scene is the identity: view z = z)."""
    m = scene["means3D"]
    f = (z / m[:, 2]).unsqueeze(1)
    m.mul_(f)
    m[:, 2] = z          # exactly


def _build(name):
    if name.startswith("P"):
        return _plain(int(name[1:]), seed=50 + int(name[1:]) % 7)
    if name == "ties":
        sc = _plain(16385, seed=61)
        h = sc["P"] // 2
        for k in ("means3D", "scales", "rotations", "opacities", "shs", "semantic_feature"):
            sc[k][h:2 * h] = sc[k][:h]
            sc[k][2 * h:] = sc[k][:1]
        return sc
    if name == "one-depth":
        sc = _plain(20000, seed=62)
        _set_z(sc, torch.full((sc["P"],), 5.0))
        return sc
    if name == "skew":
        sc = _plain(30000, seed=63)
        z = sc["means3D"][:, 2].clone()
        i = torch.arange(sc["P"])
        z[i % 20 < 9] = 3.0
        z[(i % 20 >= 9) & (i % 20 < 18)] = 7.0
        z[z <= 0.2] = 4.5            # (the recipe's near-plane share joins the spread tenth)
        _set_z(sc, z)
        return sc
    if name == "outliers":
        sc = _plain(20000, seed=64)
        z = sc["means3D"][:, 2].clone()
        z[z <= 0.2] = 6.0
        _set_z(sc, z)
        sc["means3D"][777] = torch.tensor([0.0, 0.0, 0.21])
        sc["means3D"][12345] = torch.tensor([0.0, 0.0, 1e5])
        return sc
    if name == "none-alive":
        sc = _plain(20000, seed=65)
        sc["means3D"][:, 2] = -sc["means3D"][:, 2].abs() - 0.5
        return sc
    if name == "one-alive":
        sc = _plain(20000, seed=66)
        sc["means3D"][:, 2] = -sc["means3D"][:, 2].abs() - 0.5
        sc["means3D"][4321] = torch.tensor([0.0, 0.0, 5.0])
        return sc
    if name == "half-culled":
        sc = _plain(20000, seed=67)
        sc["means3D"][1::2, 0] = 100.0 * sc["means3D"][1::2, 2].abs() + 100.0      # far outside the frustum
        return sc
    raise KeyError(name)


def _case(name):
    if name not in _scenes:
        _scenes[name] = _build(name)
    return _scenes[name]


def _oracle(name):
    """The oracle's lists of a case, computed once and only read afterwards."""
    if name not in _wants:
        o, out, _ = run_oracle(_case(name), backward=False)
        want = dict(n=out["num_rendered"], point_list=o.read("point_list").copy(), ranges=o.read("ranges").copy(),
                    tiles_touched=o.read("tiles_touched").copy(), radii=out["radii"].copy())
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _wants[name] = want
    return _wants[name]


def _tiles(scene):
    return ((scene["image_width"] + 15) // 16) * ((scene["image_height"] + 15) // 16)


def _info():
    from diff_gaussian_rasterization import _C
    torch.cuda.synchronize()
    return _C.depth_sort_info()


def _assert_oracle_lists(name, path="buckets"):
    scene, want = _case(name), _oracle(name)
    res = _raw_forward(scene)
    info = _info()
    print(name, info)
    assert info["path"] == path, info
    lib = _lib()
    n = res[0]
    assert n == want["n"]
    assert np.array_equal(res[4].cpu().numpy(), want["radii"])
    tt = _read(lib, "tiles_touched", scene, res, np.uint32, scene["P"])
    assert np.array_equal(tt, want["tiles_touched"])
    if n:
        pl = _read(lib, "point_list", scene, res, np.uint32, n)
        wrong = np.flatnonzero(pl != want["point_list"])
        assert wrong.size == 0, f"{wrong.size} of {n} entries differ, the first at {wrong[0]}"
    else:
        assert want["point_list"].size == 0
    rg = _read(lib, "ranges", scene, res, np.uint32, 2 * _tiles(scene))
    assert np.array_equal(rg, want["ranges"])
    return info


def _alive_z(name):
    return _case(name)["means3D"][:, 2].numpy()[_oracle(name)["radii"] > 0]


@pytest.mark.parametrize("name", ["P16385", "P20000", "P70001"])
def test_sizes_give_the_oracles_lists(name, option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 1)
    info = _assert_oracle_lists(name)
    assert info["capacity"] == CAPACITY and 16 <= info["buckets"] <= 2048
    assert 0 < info["largest"] <= CAPACITY and info["oversized"] == 0


def test_tied_depth_keys_keep_ascending_id(option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 1)
    want = _oracle("ties")
    h = _case("ties")["P"] // 2
    assert np.array_equal(want["tiles_touched"][:h], want["tiles_touched"][h:2 * h]) and want["n"] > 0
    _assert_oracle_lists("ties")


def test_one_depth_is_one_bucket_above_the_capacity(option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 1)
    z = _alive_z("one-depth")
    assert z.size > CAPACITY and np.unique(z.view(np.uint32)).size == 1       # the oracle's own key multiset forces it
    info = _assert_oracle_lists("one-depth")
    assert info["oversized"] >= 1 and info["largest"] == z.size


def test_skewed_depths_mix_oversized_and_ordinary_buckets(option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 1)
    z = _alive_z("skew")
    assert (z == 3.0).sum() > CAPACITY and (z == 7.0).sum() > CAPACITY and np.unique(z).size > 1000
    info = _assert_oracle_lists("skew")
    assert info["oversized"] >= 2


def test_outliers_widen_the_range_not_the_order(option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 1)
    z = _alive_z("outliers")
    assert z.min() == np.float32(0.21) and z.max() == np.float32(1e5)
    _assert_oracle_lists("outliers")


@pytest.mark.parametrize("name,alive", [("none-alive", 0), ("one-alive", 1)])
def test_few_or_none_alive(name, alive, option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 1)
    assert int((_oracle(name)["radii"] > 0).sum()) == alive
    info = _assert_oracle_lists(name)
    assert info["largest"] == alive and info["oversized"] == 0


def test_culled_half_fills_the_last_bin(option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 1)
    radii = _oracle("half-culled")["radii"]
    assert np.all(radii[1::2] == 0) and (radii[0::2] > 0).sum() > 5000
    _assert_oracle_lists("half-culled")


def test_both_paths_give_the_same_bits(option):
    """tile_cull = 1 at C = 8: images, radii and lists of the bucket path equal those of the LSD passes bit for bit."""
    scene = _scene(P=30000, C=8, seed=68, **IMG, **SMALL)
    lib = _lib()
    got = {}
    for value, path in ((0, "passes"), (1, "buckets")):
        option("depth_sort_buckets", value)
        res = _raw_forward(scene)
        assert _info()["path"] == path
        n_own = int(_read(lib, "counters", scene, res, np.uint32, 16)[0])
        got[value] = dict(n=res[0], n_own=n_own, color=res[1].cpu().numpy(), feat=res[2].cpu().numpy(), depth=res[3].cpu().numpy(),
                          radii=res[4].cpu().numpy(), point_list=_read(lib, "point_list", scene, res, np.uint32, n_own),
                          ranges=_read(lib, "ranges", scene, res, np.uint32, 2 * _tiles(scene)))
    assert got[0]["n"] == got[1]["n"] and got[0]["n_own"] == got[1]["n_own"] > 0
    for k in ("color", "feat", "depth", "radii", "point_list", "ranges"):
        assert np.array_equal(got[0][k], got[1][k]), k


@pytest.mark.parametrize("P,path", [(AUTO_ABOVE, "one_launch"), (AUTO_ABOVE + 1, "buckets")])
def test_auto_threshold(P, path, option):
    """depth_sort_buckets = -1 (default): the buckets from the first size beyond the one-launch sort on (they were measured faster
    than the LSD passes at every size from there to the upper end)."""
    from diff_gaussian_rasterization import _C
    option("tile_cull", 0)
    assert _C.get_option("depth_sort_buckets") == -1
    _assert_oracle_lists(f"P{P}", path)


def test_auto_upper_end(option):
    """The last size of the bucket path under -1 and the first beyond it.  The oracle would run for minutes on 1.25M Gaussians, so
    the two sizes are covered by the equality of the paths instead: the lists of the default equal those of option 0."""
    lib = _lib()
    option("tile_cull", 0)
    scene = _scene(P=AUTO_UPTO + 1, C=0, seed=70, **IMG, scale_lo=0.002, scale_hi=0.006)
    cut = {k: v[:AUTO_UPTO].contiguous() for k, v in scene.items() if torch.is_tensor(v) and v.dim() and v.shape[0] == AUTO_UPTO + 1}
    for sc, path in ((scene, "passes"), (dict(scene, P=AUTO_UPTO, **cut), "buckets")):
        got = {}
        for value in (0, -1):
            option("depth_sort_buckets", value)
            res = _raw_forward(sc)
            assert _info()["path"] == (path if value else "passes")
            got[value] = (res[0], _read(lib, "point_list", sc, res, np.uint32, res[0]),
                          _read(lib, "ranges", sc, res, np.uint32, 2 * _tiles(sc)))
        assert got[0][0] == got[-1][0] > 0
        assert np.array_equal(got[0][1], got[-1][1]) and np.array_equal(got[0][2], got[-1][2])


def test_captured_step_replays_the_eager_step(option):
    from graph_step import CapturedStep
    from test_gpu_sync_free import _snapshot, _static_step
    option("bwd_bf16", 1)
    option("depth_sort_buckets", 1)
    scene = _scene(P=30000, C=8, seed=69, width=320, height=200, **SMALL)
    fn, L, outs, grads = _static_step(scene)
    fn()
    assert _info()["path"] == "buckets"
    o_want, _g = _snapshot(outs, grads)
    step = CapturedStep(fn).capture()
    assert _info()["path"] == "buckets"
    graph_outs = dict(outs)
    for _ in range(2):
        step.replay()
    assert step.check()
    o_got, _g = _snapshot(graph_outs, grads)
    for k in o_want:
        assert np.array_equal(o_got[k], o_want[k]), k
