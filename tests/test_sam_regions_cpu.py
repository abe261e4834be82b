"""CPU checks of the small-region removal: the numpy oracle (tests/sam_regions_oracle.py: horizontal runs, two-pass union-find)
against the reference's own remove_small_regions (tests/golden/reference_small_regions.npz, made over scipy.ndimage.label by
tests/golden/make_reference_small_region_vectors.py) on every case, bit for bit; the argument errors of the Python entry points,
raised before any device work; and the C ABI's argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import sam_masks_oracle as O
import sam_regions_oracle as R
from util import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_small_regions.npz")
_Z = {}


def golden():
    if not _Z:
        _Z.update(np.load(GOLDEN))
    return _Z


def case_names():
    return sorted({k.split("/")[0] for k in np.load(GOLDEN).files} - {"pipeline"})


@pytest.mark.parametrize("name", case_names())
def test_oracle_against_the_reference(name):
    z = golden()
    FH, FW = z[f"{name}/frame"].tolist()
    masks = O.unpack(z[f"{name}/input"], FH)
    if f"{name}/index" in z:
        masks = masks[z[f"{name}/index"]]
    for j, t in enumerate(z[f"{name}/thresholds"].tolist()):
        holes, final, ch_h, ch_i, area, box = R.postprocess(masks, t)
        assert np.array_equal(O.pack(holes), z[f"{name}/{j}/holes"]), (name, t)
        assert np.array_equal(O.pack(final), z[f"{name}/{j}/islands"]), (name, t)
        assert np.array_equal(np.stack([ch_h, ch_i], 1), z[f"{name}/{j}/changed"]), (name, t)
        assert np.array_equal(area, z[f"{name}/{j}/area"]) and np.array_equal(box, z[f"{name}/{j}/box"])


def test_the_recorded_cases_hold_what_they_are_for():
    z = golden()
    assert {"boundaries", "depth", "threshold_edges", "quirks", "selection", "medium", "tie_rule"} <= set(case_names())
    assert len([n for n in case_names() if n.startswith("edges_")]) == 8
    b = O.unpack(z["boundaries/1/islands"], 100)                          # t = 2: the corner pair (area 2) stays, the split pair goes
    assert b[0, 31, 1] and b[0, 32, 2] and not b[1, 31, 1] and not b[1, 33, 2] and b[3, 31, 2] and b[3, 64, 5]
    q = z["quirks/2/changed"]                                             # t = 10
    assert q[0].tolist() == [False, False] and q[1].tolist() == [False, False]
    assert q[2].tolist() == [False, True] and np.array_equal(z["quirks/2/islands"][2], z["quirks/input"][2])     # the same bits, changed
    assert z["quirks/2/area"][3] == 6 and z["quirks/2/area"][4] == 20 * 24
    assert q[5].tolist() == [True, False] and q[6].tolist() == [False, True] and q[7].tolist() == [True, True] and not q[8].any()
    assert z["quirks/1/area"][9] == 20 * 24                               # a corner hole of one pixel, t = 2: filled
    t = O.unpack(z["tie_rule/0/islands"], 16)
    assert t[0, 2, 15] and not t[0, 8, 3] and t[1, 9, 2] and not t[1, 8, 10] and t[2, 4, 9] and t[2].sum() == 1
    te = z["threshold_edges/thresholds"].tolist()
    assert te == [7, 7.5, 8, 9] and z["threshold_edges/0/changed"].tolist() == [[False, False]]
    probes = ((8, 8), (20, 8), (34, 4), (34, 20))                          # the hole of 8, the hole of 7, the island of 8, the island of 7
    seen = [[bool(O.unpack(z[f"threshold_edges/{j}/islands"], 40)[0][p]) for p in probes] for j in range(4)]
    assert seen == [[False, False, True, True], [False, True, True, False], [False, True, True, False], [True, True, False, False]]
    records = json.loads(bytes(z["pipeline/records"]))
    assert len(records) == 4 and [r["point_coords"][0][0] for r in records] == [12.5, 16.5, 0.5, 14.5]


def test_new_entry_points_reject_arguments_without_a_device():
    import sam_masks as sm
    packed = sm.pack_masks(torch.zeros(2, 33, 5, dtype=torch.bool))
    for bad in (-1, float("nan"), float("inf"), True, "3", None):
        with pytest.raises(ValueError, match="area_thresh"):
            sm.remove_small_regions(packed, bad, "holes")
        with pytest.raises(ValueError, match="min_area"):
            sm.postprocess_small_regions(packed, bad)
        with pytest.raises(ValueError, match="min_mask_region_area"):
            sm.MaskPostprocessor((32, 32), min_mask_region_area=bad)
    with pytest.raises(ValueError, match="mode"):
        sm.remove_small_regions(packed, 3, "both")
    with pytest.raises(ValueError, match="mode"):
        sm.remove_small_regions(packed, 3, None)
    with pytest.raises(ValueError, match="PackedMasks"):
        sm.remove_small_regions(packed.words, 3, "holes")
    with pytest.raises(ValueError, match="packed.words"):
        sm.postprocess_small_regions(sm.PackedMasks(torch.zeros(1, 4, 2, dtype=torch.int32), (33, 5)), 3)
    with pytest.raises(ValueError, match="index"):
        sm.remove_small_regions(packed, 3, "islands", index=torch.zeros(2))
    with pytest.raises(ValueError, match="index"):
        sm.postprocess_small_regions(packed, 3, index=[0, 1])
    with pytest.raises(ValueError, match="HIP device"):                    # last: every other error is met without a device
        sm.remove_small_regions(packed, 3.5, "islands")
    with pytest.raises(ValueError, match="HIP device"):
        sm.postprocess_small_regions(packed, 0, index=torch.tensor([1, 0]))
    assert sm.SmallRegions._fields == ("packed", "changed", "area", "box")


def test_postprocessor_takes_min_mask_region_area():
    import sam_masks as sm
    assert sm.MaskPostprocessor((32, 32), min_mask_region_area=0).min_mask_region_area == 0
    assert sm.MaskPostprocessor((32, 32)).min_mask_region_area == 0
    assert sm.MaskPostprocessor((32, 32), min_mask_region_area=7.5).min_mask_region_area == 7.5
    assert sm.MaskPostprocessor((32, 32), min_mask_region_area=100).finish() == []
    with pytest.raises(ValueError, match="min_mask_region_area"):
        sm.MaskPostprocessor((32, 32), min_mask_region_area=-1)
    with pytest.raises(ValueError, match="min_mask_region_area"):
        sm.MaskPostprocessor((32, 32), min_mask_region_area=float("nan"))
    assert "postprocess_small_regions (min_mask_region_area > 0) and coco_rle" not in sm.MaskPostprocessor.__doc__


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    assert lib.f3dgs_version() >= 31500
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.f3dgs_mask_regions_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_mask_regions_scratch_bytes.argtypes = [ctypes.c_int, ctypes.c_int, i64]
    assert lib.f3dgs_mask_regions_scratch_bytes(3, 10, 100) == 4 * (4 + 4 * 3 + 4 + 30 + 400)
    assert lib.f3dgs_mask_regions_scratch_bytes(65536, 10, 100) == 0 and lib.f3dgs_mask_regions_scratch_bytes(3, 10, 1 << 31) == 0
    lib.f3dgs_mask_regions.argtypes = [ctypes.c_int] * 3 + [vp, vp, ctypes.c_int, ctypes.c_double, i64] + [vp] * 7
    runs = i64(-5)
    call = lambda K, FH, FW, t, cap, r=ctypes.byref(runs), p=None: lib.f3dgs_mask_regions(K, FH, FW, p, None, 1, t, cap, p, p, p, p, r, p, None)
    assert call(1, 0, 8, 1.0, 10) == -1 and b"bad sizes" in lib.f3dgs_last_error()
    assert call(1, 8, 8, 1.0, -1) == -1
    assert call(1, 8, 8, -1.0, 10) == -1 and b"area_thresh" in lib.f3dgs_last_error()
    assert call(1, 8, 8, float("nan"), 10) == -1 and call(1, 8, 8, float("inf"), 10) == -1
    assert call(70000, 8, 8, 1.0, 10) == -4 and call(1, 40000, 8, 1.0, 10) == -4 and call(1, 8, 8, 1.0, 1 << 31) == -4
    assert call(1, 8, 8, 1.0, 10, r=None) == -1 and b"null" in lib.f3dgs_last_error()
    assert call(1, 8, 8, 1.0, 10) == -1 and b"null" in lib.f3dgs_last_error()
    assert call(1, 8, 8, 1.0, 10, p=0x10004) == -1 and b"8-byte" in lib.f3dgs_last_error()      # (never dereferenced)
    assert call(0, 8, 8, 1.0, 0) == 0 and runs.value == 0
