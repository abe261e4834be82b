"""CPU checks of the segmentation scores: the numpy oracle (tests/seg_metrics_oracle.py) against the reference's own
`calculate_accuracy`, `calculate_accuracy_mask`, `calculate_iou` and `calculate_iou_mask` and its pictures
(tests/golden/reference_seg_metrics.npz), the oracle's tie and invalid-pixel rules, the palette, and the argument errors of the C
ABI and of the Python surface (no device work)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import seg_metrics_oracle as O
from util import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_seg_metrics.npz")
CASES = ("big", "seven", "few", "same", "nomatch", "gtonly")
IOU_TOL = 1e-10      # at most 256 terms in [0, 1] summed in fp64 in another order: < 256 * 256 * 2^-53 = 7e-12


def same_float(a, b):
    """bit for bit, NaN equal to NaN"""
    return (math.isnan(a) and math.isnan(b)) or a == b


def close_iou(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= IOU_TOL


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_the_reference_fixture(name):
    """accuracy and accuracy_masked are one fp64 division of exact integers: bit for bit.  iou and iou_masked: 1e-10 absolute
    (IOU_TOL), NaN where the reference has NaN."""
    z = np.load(GOLDEN)
    t, s, g, L = z[f"{name}/teacher"], z[f"{name}/student"], z[f"{name}/gt"], int(z[f"{name}/L"])
    for nc in z[f"{name}/num_classes"].tolist():
        (view,), pooled, _ = O.scores([t], [s], [g], L, nc)
        assert same_float(view["accuracy"], float(z[f"{name}/accuracy"]))
        assert same_float(view["accuracy_masked"], float(z[f"{name}/accuracy_masked"]))
        assert close_iou(view["iou"], float(z[f"{name}/iou_{nc}"])), (view["iou"], float(z[f"{name}/iou_{nc}"]))
        assert close_iou(view["iou_masked"], float(z[f"{name}/iou_masked_{nc}"]))
        assert view["invalid"] == 0
        for k in ("accuracy", "accuracy_masked", "iou", "iou_masked"):          # one view: the pooled row is the view
            assert same_float(pooled[k], view[k])
        # without gt the unmasked results are the same
        (plain,), _, _ = O.scores([t], [s], None, L, nc)
        assert same_float(plain["accuracy"], view["accuracy"]) and same_float(plain["iou"], view["iou"]) and "iou_masked" not in plain
    if name == "nomatch":
        assert math.isnan(view["accuracy_masked"]) and math.isnan(view["iou_masked"])
    if name == "few":
        assert (view["labels_ranked"] >= 0).sum() == 4 and view["labels_ranked"][4:].tolist() == [-1, -1, -1]
    if name == "gtonly":
        assert 30 in view["labels_ranked_masked"].tolist() and 30 not in view["labels_ranked"].tolist()
        assert math.isnan(view["iou_per_label_masked"][30])          # ranked, no matching pixel: skipped by the mean


def test_oracle_tie_rule_and_invalid_pixels():
    # labels 1 and 2 both count 4 across the cut at num_classes = 2: the lower label is kept
    t = np.array([[0, 0, 0, 1, 1, 2, 2, 3]])
    s = np.array([[0, 0, 0, 1, 2, 2, 1, 3]])
    (v,), _, _ = O.scores([t], [s], None, 4, 2)
    assert v["labels_ranked"].tolist() == [0, 1] and v["iou"] == (1.0 + 1.0 / 3.0) / 2
    assert math.isnan(v["iou_per_label"][2]) and v["iou_per_label"][1] == 1.0 / 3.0
    # a pixel with any label outside [0, L) takes part in nothing else
    t2 = np.array([[0, 1, 5, -1, 1, 1 << 40]], np.int64)
    s2 = np.array([[0, 1, 1, 1, 7, 1]], np.int64)
    c = O.counts(t2, s2, None, 5)
    assert c["invalid"] == 4 and c["valid"] == 2 and c["equal"] == 2 and c["n_t"].tolist() == [1, 1, 0, 0, 0]
    # pooling adds counters, not scores
    views_t = [np.array([[0, 0, 0, 0, 1]]), np.array([[1, 1, 1, 1, 0]])]
    views_s = [np.array([[0, 0, 0, 0, 0]]), np.array([[1, 1, 0, 0, 0]])]
    per_view, pooled, _ = O.scores(views_t, views_s, None, 2, 2)
    assert pooled["accuracy"] == 7 / 10 and pooled["iou"] != (per_view[0]["iou"] + per_view[1]["iou"]) / 2


def test_oracle_pictures_match_the_reference_fixture():
    z = np.load(GOLDEN)
    for name in ("color_a", "color_b"):
        labels, palette, image = z[f"{name}/labels"], z[f"{name}/palette"], z[f"{name}/image"]
        assert image.dtype == np.float32 and image.min() >= 0.0 and image.max() <= 1.0
        assert np.array_equal(O.colorize(labels, palette), z[f"{name}/mask"])
        strip = O.overlay(labels, palette, image, strip=True)
        assert strip.shape == labels.shape[:1] + (3 * labels.shape[1], 3) and np.array_equal(strip, z[f"{name}/strip"])
        W = labels.shape[1]
        assert np.array_equal(O.overlay(labels, palette, image), z[f"{name}/strip"][:, W:2 * W])
    assert {0, 255} <= set(z["color_b/labels"].reshape(-1).tolist())
    # the strip's third part goes through mask / 255 * 255 in fp32: every byte comes back, so it equals the mask picture
    b = np.arange(256, dtype=np.float32)
    assert np.array_equal(((b / np.float32(255.0)) * np.float32(255.0)).astype(np.uint8), np.arange(256, dtype=np.uint8))
    # out-of-range labels take the fill colour
    lab = np.array([[0, 3, -1, 2, 1 << 40]], np.int64)
    pal = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint8)
    assert O.colorize(lab, pal, fill=(9, 9, 1)).tolist() == [[[1, 2, 3], [9, 9, 1], [9, 9, 1], [7, 8, 9], [9, 9, 1]]]


def test_default_palette_is_deterministic_and_distinct():
    import seg_metrics as M
    p = M.default_palette(256)
    assert p.dtype == torch.uint8 and tuple(p.shape) == (256, 3)
    assert len({tuple(r) for r in p.tolist()}) == 256
    assert torch.equal(p, M.default_palette(256)) and torch.equal(p[:150], M.default_palette(150))
    assert p[0].tolist() == [0, 0, 0] and tuple(M.default_palette(1).shape) == (1, 3)
    for bad in (0, 257, -1, 2.0, True):
        with pytest.raises(ValueError, match="num_labels"):
            M.default_palette(bad)


def _lib():
    so = os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_seg_metrics_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_seg_metrics_scratch_bytes.argtypes = [ci] * 3
    lib.f3dgs_seg_metrics.argtypes = [ci] * 5 + [vp, ci, vp, ci, vp, ci] + [vp] * 7
    lib.f3dgs_seg_colorize.argtypes = [ci] * 4 + [vp, ci, vp, vp, ci, ctypes.c_float, ctypes.c_float, vp, vp, vp]
    return lib


def test_c_abi_rejects_bad_arguments():
    """Everything here returns before a launch: the addresses are host memory that is never dereferenced."""
    lib = _lib()
    dummy = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(dummy)
    INVALID, UNSUPPORTED = -1, -4
    U8, I32, I64 = 0, 1, 2
    # counts[A][N + 1][L] and scalars[5][N + 1], int64
    assert lib.f3dgs_seg_metrics_scratch_bytes(2, 150, 0) == 8 * (3 * 3 * 150 + 5 * 3)
    assert lib.f3dgs_seg_metrics_scratch_bytes(2, 150, 1) == 8 * (7 * 3 * 150 + 5 * 3)
    for bad in ((0, 150, 0), (1, 0, 0), (1, 257, 1), (-1, 5, 0), ((1 << 16) + 1, 5, 0)):
        assert lib.f3dgs_seg_metrics_scratch_bytes(*bad) == 0

    def call(N=1, H=4, W=4, L=5, nc=3, t=p, ft=I64, s=p, fs=I64, g=None, fg=U8, cc=None, cs=None, counters=p, scores=p, per=p, ranked=p):
        return lib.f3dgs_seg_metrics(N, H, W, L, nc, t, ft, s, fs, g, fg, cc, cs, counters, scores, per, ranked, None)

    assert call(N=0) == 0                                                   # N = 0: a no-op
    for kw in (dict(N=-1), dict(H=0), dict(W=-3)):
        assert call(**kw) == INVALID and b"bad sizes" in lib.f3dgs_last_error()
    for L in (0, 257, -1):
        assert call(L=L, nc=1) == UNSUPPORTED and b"label slots" in lib.f3dgs_last_error()
    assert call(H=1 << 16, W=1 << 15) == UNSUPPORTED
    assert call(N=(1 << 16) + 1) == UNSUPPORTED and b"views" in lib.f3dgs_last_error()      # (the count grid's launch limit)
    assert call(scores=None, per=None, ranked=None, t=None) == INVALID                       # the counters alone: checked alike
    for nc in (0, 6, -1):
        assert call(nc=nc) == INVALID and b"num_classes" in lib.f3dgs_last_error()
    for kw in (dict(ft=3), dict(fs=-1), dict(g=p, fg=9)):
        assert call(**kw) == INVALID and b"unknown label format" in lib.f3dgs_last_error()
    for kw in (dict(t=None), dict(s=None), dict(counters=None)):
        assert call(**kw) == INVALID and b"null" in lib.f3dgs_last_error()
    assert call(scores=None) == INVALID and b"go together" in lib.f3dgs_last_error()
    assert call(cc=p) == INVALID and b"go together" in lib.f3dgs_last_error()
    assert call(t=p + 4) == INVALID and b"aligned" in lib.f3dgs_last_error()          # an int64 map off its 8 bytes
    assert call(s=p + 2, fs=I32) == INVALID and b"aligned" in lib.f3dgs_last_error()

    def colour(N=1, H=4, W=4, L=5, labels=p, fl=U8, palette=p, image=p, mode=2, out=p):
        return lib.f3dgs_seg_colorize(N, H, W, L, labels, fl, palette, image, mode, 0.4, 0.6, None, out, None)

    assert colour(N=0) == 0
    assert colour(H=0) == INVALID and b"bad sizes" in lib.f3dgs_last_error()
    for L in (0, 257):
        assert colour(L=L) == UNSUPPORTED
    assert colour(mode=3) == INVALID and b"unknown mode" in lib.f3dgs_last_error()
    assert colour(fl=5) == INVALID and b"unknown label format" in lib.f3dgs_last_error()
    for kw in (dict(labels=None), dict(palette=None), dict(out=None), dict(image=None, mode=1), dict(image=None, mode=2)):
        assert colour(**kw) == INVALID and b"null" in lib.f3dgs_last_error()
    assert colour(labels=p + 4, fl=I64, mode=0) == INVALID and b"aligned" in lib.f3dgs_last_error()
    lib.f3dgs_version.restype = ctypes.c_int
    assert lib.f3dgs_version() >= 31300


def test_python_surface_raises_value_errors_before_any_device_work():
    import seg_metrics as M
    a = torch.randint(0, 5, (2, 6, 7))
    b = torch.randint(0, 5, (2, 6, 7))
    kw = dict(num_labels=5, num_classes=3)
    for f in (M.segmentation_scores, lambda *x, **k: M.segmentation_counts(*x, num_labels=k["num_labels"])):
        with pytest.raises(ValueError, match="shapes differ"):
            f(a, b[:, :, :6], **kw)
        with pytest.raises(ValueError, match="shapes differ"):
            f(a, b, b[:1], **kw)
        with pytest.raises(ValueError, match="uint8, int32 or int64"):
            f(a.float(), b, **kw)
        with pytest.raises(ValueError, match="uint8, int32 or int64"):
            f(a, b.to(torch.int16), **kw)
        with pytest.raises(ValueError, match=r"\(H,W\) or \(N,H,W\)"):
            f(a[0, 0], b[0, 0], **kw)
        with pytest.raises(ValueError, match="a tensor expected"):
            f(a.numpy(), b, **kw)
        with pytest.raises(ValueError, match="empty"):
            f(a[:0], b[:0], **kw)
        with pytest.raises(ValueError, match="HIP device"):          # well-formed, on the host: refused, no CPU path
            f(a, b.to(torch.uint8), a.to(torch.int32), **kw)
    for L in (0, 257, 5.0, None):
        with pytest.raises(ValueError, match="num_labels"):
            M.segmentation_scores(a, b, num_labels=L)
    for nc in (0, 6, -1, 2.5):
        with pytest.raises(ValueError, match="num_classes"):
            M.segmentation_scores(a, b, num_labels=5, num_classes=nc)
    with pytest.raises(ValueError, match="num_classes"):
        M.segmentation_scores(a, b, num_labels=5)                    # the default of 7 needs 7 label slots
    good = (torch.zeros(3, 5, dtype=torch.int64), torch.zeros(5, dtype=torch.int64))
    for carry in (good[0], (good[0],), (good[0].float(), good[1]), (good[0][:, :4], good[1]), (good[0], good[1][:4]),
                  (torch.zeros(7, 5, dtype=torch.int64), good[1])):          # (7 arrays: a carry of a call with gt)
        with pytest.raises(ValueError, match="carry"):
            M.segmentation_scores(a, b, num_labels=5, num_classes=3, carry=carry)
    with pytest.raises(ValueError, match="HIP device"):
        M.segmentation_scores(a, b, num_labels=5, num_classes=3, carry=good)
    with pytest.raises(ValueError, match="2 teacher, 1 student"):
        M.evaluate_segmentation([a[0], a[1]], [b[0]], num_labels=5, num_classes=3)
    with pytest.raises(ValueError, match="and 1 gt"):
        M.evaluate_segmentation([a[0], a[1]], [b[0], b[1]], [a[0]], num_labels=5, num_classes=3)
    with pytest.raises(ValueError, match="one label map per list entry"):
        M.evaluate_segmentation([a], [b], num_labels=5, num_classes=3)
    with pytest.raises(ValueError, match="HIP device"):
        M.evaluate_segmentation([a[0], a[1]], [b[0], b[1]], num_labels=5, num_classes=3)
    empty = M.evaluate_segmentation([], [], num_labels=5, num_classes=3)
    assert empty["per_view"] == {"accuracy": [], "iou": []} and math.isnan(empty["iou"])
    assert set(M.evaluate_segmentation([], [], [], num_labels=5, num_classes=3)["per_view"]) == {"accuracy", "iou", "accuracy_masked", "iou_masked"}
    # the drop-ins take the label count from the data
    big = np.array([[0, 300]])
    for call in (lambda: M.calculate_accuracy(big, big), lambda: M.calculate_iou(big, big, 7),
                 lambda: M.calculate_accuracy_mask(big, big, big, 0), lambda: M.calculate_iou_mask(big, big, big, 7)):
        with pytest.raises(ValueError, match="at most 256"):
            call()
    with pytest.raises(ValueError, match="negative label"):
        M.calculate_accuracy(np.array([[0, -1]]), np.array([[0, 1]]))
    with pytest.raises(ValueError, match="negative label"):
        M.calculate_iou(torch.tensor([[0, 1]]), torch.tensor([[0, -2]], dtype=torch.int16), 7)
    with pytest.raises(ValueError, match="integer labels"):
        M.calculate_accuracy(np.array([[0.0, 1.0]]), np.array([[0, 1]]))
    with pytest.raises(ValueError, match="pixels"):
        M.calculate_iou(np.zeros((2, 3), np.int64), np.zeros((2, 2), np.int64), 7)
    with pytest.raises(ValueError, match="num_classes"):
        M.calculate_iou(np.zeros((2, 3), np.int64), np.zeros((2, 3), np.int64), 0)
    with pytest.raises(ValueError, match="a numpy array or a tensor"):
        M.calculate_accuracy([[0, 1]], [[0, 1]])
    # pictures
    pal = M.default_palette(5)
    img = torch.rand(2, 3, 6, 7)
    with pytest.raises(ValueError, match="uint8, int32 or int64"):
        M.colorize(a.float(), pal)
    with pytest.raises(ValueError, match=r"\(L,3\)"):
        M.colorize(a, pal[:, :2])
    with pytest.raises(ValueError, match=r"\(L,3\)"):
        M.colorize(a, torch.zeros(257, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="byte values"):
        M.colorize(a, pal.to(torch.int64) + 300)
    with pytest.raises(ValueError, match="three byte values"):
        M.colorize(a, pal, fill=(0, 0, 256))
    with pytest.raises(ValueError, match="does not match"):
        M.overlay(a, pal, img[:, :, :5])
    with pytest.raises(ValueError, match="float32"):
        M.overlay(a, pal, img.double())
    with pytest.raises(ValueError, match="weights"):
        M.overlay(a, pal, img, weights=(1, 2, 3))
    with pytest.raises(ValueError, match="HIP device"):
        M.colorize(a, pal)
    with pytest.raises(ValueError, match="HIP device"):
        M.overlay(a, pal, img, strip=True)


def test_install_sets_the_four_names():
    import types
    import seg_metrics as M
    mod = types.ModuleType("segmentation_metric")
    mod.calculate_iou = mod.other = lambda *a: None
    keep = mod.other
    assert M.install(mod) is mod and mod.other is keep
    for name in ("calculate_accuracy", "calculate_accuracy_mask", "calculate_iou", "calculate_iou_mask"):
        assert getattr(mod, name) is getattr(M, name)
    with pytest.raises(AttributeError, match="none of"):
        M.install(types.ModuleType("something_else"))
