"""The label vote and the instance map without a GPU: the argument errors of f3dgs_label_votes and f3dgs_mask_instance_map
(raised before any device work), those of the Python wrappers, the test maps' own coverage, and paint_order against the
numpy painter."""
import ctypes
import os

import numpy as np
import pytest
import torch

import label_maps as lm
from util import ROOT

U8, I32, I64 = 0, 1, 2          # F3DGS_LABELS_*
A = 0x10000                     # a never dereferenced address, aligned for every element


def _lib():
    import diff_gaussian_rasterization  # noqa: F401  (its bundled HIP runtime must be the one the library binds to)
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.f3dgs_label_votes.restype = ci
    lib.f3dgs_label_votes.argtypes = [ci] * 4 + [vp] * 3 + [vp, ci, ci, vp, vp]
    lib.f3dgs_mask_instance_map.restype = ci
    lib.f3dgs_mask_instance_map.argtypes = [ci] * 3 + [vp] * 4
    lib.f3dgs_version.restype = ci
    return lib


def test_label_votes_argument_errors_before_any_device_work():
    lib = _lib()
    call = lambda P, R, W, H, geom, binning, img, labels, fmt, L, acc: lib.f3dgs_label_votes(P, R, W, H, geom, binning, img, labels, fmt, L,
                                                                                              acc, None)
    err = lib.f3dgs_last_error
    assert call(-1, 0, 8, 8, A, A, A, A, I64, 5, A) == -1 and b"P < 0" in err()
    for R, W, H in ((-1, 8, 8), (3, 0, 8), (3, 8, 0), (3, -4, 8)):
        assert call(5, R, W, H, A, A, A, A, I64, 5, A) == -1 and b"sizes" in err()
    for L in (0, -3, 65537):
        assert call(5, 3, 8, 8, A, A, A, A, I64, L, A) == -1 and b"labels, 1 .. 65536" in err()
    for fmt in (-1, 3, 7):
        assert call(5, 3, 8, 8, A, A, A, A, fmt, 5, A) == -1 and b"format" in err()
    assert call(5, 3, 8, 8, A, A, A, None, I64, 5, A) == -1 and b"labels is null" in err()
    assert call(5, 3, 8, 8, A, A, A, A, U8, 5, None) == -1 and b"acc is null" in err()
    for fmt, off in ((I32, 2), (I64, 4), (I64, 1)):
        assert call(5, 3, 8, 8, A, A, A, A + off, fmt, 5, A) == -1 and b"alignment" in err()
    for geom, binning, img in ((None, A, A), (A, None, A), (A, A, None)):
        assert call(5, 3, 8, 8, geom, binning, img, A, I32, 5, A) == -1 and b"null state buffer" in err()
    # nothing to do, no device touched: no Gaussians; nothing rendered (binning may then be null); any byte address for uint8
    assert call(0, 0, 8, 8, None, None, None, A, I64, 5, A) == 0
    assert call(5, 0, 8, 8, A, None, A, A + 1, U8, 65536, A) == 0
    assert call(0, 0, 8, 8, None, None, None, None, I64, 5, A) == -1          # the checks still answer first
    assert lib.f3dgs_version() >= 31600


def test_instance_map_argument_errors_before_any_device_work():
    lib = _lib()
    call = lambda K, FH, FW, packed, index, out: lib.f3dgs_mask_instance_map(K, FH, FW, packed, index, out, None)
    err = lib.f3dgs_last_error
    for K, FH, FW in ((-1, 8, 8), (2, 0, 8), (2, 8, 0)):
        assert call(K, FH, FW, A, None, A) == -1 and b"sizes" in err()
    assert call(2, 1 << 16, 1 << 15, A, None, A) == -4 and b"2^30" in err()              # F3DGS_ERR_UNSUPPORTED
    assert call(2, 8, 8, A, None, None) == -1 and b"null pointer" in err()
    assert call(0, 8, 8, None, None, None) == -1 and b"null pointer" in err()
    assert call(2, 8, 8, None, A, A) == -1 and b"null pointer" in err()


def _settings(sc):
    import diff_gaussian_rasterization as dgr
    return dgr.GaussianRasterizationSettings(sc["image_height"], sc["image_width"], sc["tanfovx"], sc["tanfovy"], sc["bg"], 1.0,
                                             sc["viewmatrix"], sc["projmatrix"], 3, sc["campos"], False, False)


def test_wrapper_errors_and_no_cpu_path():
    import contrib
    from synth import make_scene
    sc = make_scene(50, 0, 32, 24)
    st = _settings(sc)
    kw = dict(means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    labels = torch.zeros(24, 32, dtype=torch.int64)
    with pytest.raises(ValueError, match="HIP device"):                              # CPU Gaussians
        contrib.label_votes(st, labels=labels, num_classes=3, **kw)
    with pytest.raises(ValueError, match="exactly one of shs"):
        contrib.label_votes(st, labels=labels, num_classes=3, **dict(kw, colors_precomp=torch.zeros(50, 3)))
    with pytest.raises(TypeError):                                                   # labels and num_classes are required
        contrib.label_votes(st, **kw)
    cpu = torch.device("cpu")
    # _check_labels / _check_votes answer before the device is touched: exercised directly, as label_votes refuses CPU Gaussians first
    with pytest.raises(ValueError, match=r"torch.float32 \(24, 32\)"):
        contrib._check_labels(torch.zeros(24, 32), 24, 32, cpu)
    with pytest.raises(ValueError, match=r"torch.bool \(24, 32\)"):
        contrib._check_labels(torch.zeros(24, 32, dtype=torch.bool), 24, 32, cpu)
    with pytest.raises(ValueError, match=r"torch.int16 \(24, 32\)"):
        contrib._check_labels(torch.zeros(24, 32, dtype=torch.int16), 24, 32, cpu)
    for shape in ((24, 31), (1, 24, 32), (32, 24), (24 * 32,)):
        with pytest.raises(ValueError, match=r"\(24, 32\) tensor expected.*torch.int64 \(%s" % ", ".join(map(str, shape))):
            contrib._check_labels(torch.zeros(*shape, dtype=torch.int64), 24, 32, cpu)
    with pytest.raises(ValueError, match="ndarray"):
        contrib._check_labels(np.zeros((24, 32), np.int64), 24, 32, cpu)
    with pytest.raises(ValueError, match="HIP device"):                              # a CPU map of the right type and shape
        contrib._check_labels(labels, 24, 32, cpu)
    with pytest.raises(ValueError, match="HIP device"):
        contrib._check_votes(torch.zeros(50, 4), 50, 3, cpu)
    # num_classes is checked before the labels are looked at
    for L in (0, -1, 65537):
        with pytest.raises(ValueError, match="num_classes"):
            _votes_with_fake_device(contrib, st, kw, labels, L)
    with pytest.raises(ValueError, match=r"LabelLifter\(P=5, L=0\)"):
        contrib.LabelLifter(5, 0, "cuda")
    with pytest.raises(ValueError, match=r"LabelLifter\(P=-1, L=3\)"):
        contrib.LabelLifter(-1, 3, "cuda")
    with pytest.raises(ValueError, match=r"L=65537"):
        contrib.LabelLifter(5, 65537, "cuda")
    with pytest.raises(ValueError, match="HIP device"):
        contrib.LabelLifter(5, 3, "cpu")
    assert contrib.MAX_LABELS == 65536 and contrib.MAX_MASKS == 7


def _votes_with_fake_device(contrib, st, kw, labels, L):
    """label_votes past its first check (CPU Gaussians) without a device: _need_device is the only thing that looks at it."""
    keep = contrib._need_device
    contrib._need_device = lambda t, name: None
    try:
        contrib.label_votes(st, labels=labels, num_classes=L, **kw)
    finally:
        contrib._need_device = keep


def test_instance_map_wrapper_errors():
    import sam_masks as sm
    words = torch.zeros(2, 8, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="PackedMasks"):
        sm.instance_map(words)
    with pytest.raises(ValueError, match=r"int32 \(M,8,2\)"):
        sm.instance_map(sm.PackedMasks(words, (40, 8)))
    with pytest.raises(ValueError, match="index"):
        sm.instance_map(sm.PackedMasks(words, (32, 8)), torch.zeros(2))
    with pytest.raises(ValueError, match="no CPU path"):
        sm.instance_map(sm.PackedMasks(words, (32, 8)))
    with pytest.raises(ValueError, match="areas"):
        sm.paint_order(torch.zeros(2, 3))
    with pytest.raises(ValueError, match="areas"):
        sm.paint_order(torch.zeros(3, dtype=torch.bool))


def test_paint_order_is_the_stable_descending_sort_and_drives_the_painter():
    """sorted(anns, key=area, reverse=True) keeps tied areas in their former order; painting in that order leaves, per pixel,
    the LAST mask of the order that covers it - what instance_map computes as the largest position."""
    import sam_masks as sm
    rng = np.random.default_rng(3)
    K, FH, FW = 12, 20, 27
    masks = np.zeros((K, FH, FW), bool)
    for k in range(K):
        y0, x0 = rng.integers(0, FH - 4), rng.integers(0, FW - 4)
        masks[k, y0:y0 + rng.integers(2, 10), x0:x0 + rng.integers(2, 10)] = True
    masks[5] = masks[2]                       # equal areas, the same pixels: the later of a tie paints over the earlier
    masks[9] = np.roll(masks[2], 1, axis=1)   # equal area, other pixels
    areas = masks.reshape(K, -1).sum(1)
    assert len(set(areas.tolist())) < K
    want = sorted(range(K), key=lambda j: areas[j], reverse=True)
    for given in (areas, areas.tolist(), torch.from_numpy(areas), torch.from_numpy(areas).float()):
        order = sm.paint_order(given)
        assert order.dtype == torch.int64 and order.tolist() == want
    assert want.index(2) < want.index(5) < want.index(9)
    img = lm.painter(masks, want)
    assert img.dtype == np.int32 and (img[~masks.any(0)] == -1).all()
    # the painter leaves the largest position whose mask covers the pixel
    pos = np.where(masks[want], np.arange(K)[:, None, None], -1).max(0)
    assert np.array_equal(img, pos)
    assert (img[masks[2]] >= want.index(5)).all()
    assert np.array_equal(lm.painter(masks), np.where(masks, np.arange(K)[:, None, None], -1).max(0))
    assert sm.paint_order([]).tolist() == []


@pytest.mark.parametrize("W,H,reach", [(17, 23, 8), (129, 64, 12), (100, 70, 12), (70, 33, 12)])
def test_the_test_maps_cover_what_they_claim(W, H, reach):
    """The ladder gives the quadrants of every scene of tests/test_gpu_label_votes.py each number of distinct labels from 1 to
    `reach` (12, across the 7 / 8 / 9 round boundary; the ragged scene has nine quadrants and reaches 8), all of them valid; the
    noise map has both kinds of invalid label and far more than one round's labels in a quadrant."""
    for L in (20, 150, 300):
        lab = lm.ladder(W, H, L)
        assert lab.min() >= 0 and lab.max() < L
        D = set(lm.distinct_per_quadrant(lab, L).tolist())
        assert max(D) == reach and ({7, 8} <= D if reach == 8 else D == set(range(1, 13))), (W, H, L, D)
        nz = lm.noise(W, H, L)
        assert nz.min() == -1 and nz.max() == L
        assert lm.distinct_per_quadrant(nz, L).max() >= min(L, 16) - 4
        hot = lm.one_hot(nz, L)
        assert hot.shape == (L, H, W) and np.array_equal(hot.sum(0) == 0, (nz < 0) | (nz >= L))
    assert lm.as_dtype(lm.noise(W, H, 150), np.uint8).max() == 255
    assert (lm.constant(W, H, 1) == 0).all()
