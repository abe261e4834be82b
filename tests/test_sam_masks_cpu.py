"""CPU checks of the SAM mask post-processing: the numpy oracle (tests/sam_masks_oracle.py) against the reference's own code
(tests/golden/reference_sam_masks.npz: postprocess_masks, calculate_stability_score, batched_mask_to_box, is_box_near_crop_edge,
mask_to_rle_pytorch), the oracle's NMS on hand-made cases, and the argument errors of the C ABI and of the Python surface (no device
work; the module imports without a device)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sam_masks_oracle as O
from util import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_sam_masks.npz")
EXACT = ("exact_64", "exact_32", "exact_128")
GENERAL = ("general_27x48", "general_135x240", "general_121x70", "general_270x480")
EDGES = ("edge_1x1", "edge_1x40", "edge_40x1", "edge_m1", "edge_m67", "edge_special", "crop")


def load(z, name):
    S, ih, iw, H, W, FH, FW, x0, y0, x1, y1 = z[f"{name}/geom"].tolist()
    lr = z[f"{name}/low_res"] if f"{name}/low_res" in z else O.expand_logits(z[f"{name}/grid"], int(z[f"{name}/h"]))
    return lr, S, (ih, iw), (H, W), (FH, FW), (x0, y0, x1, y1)


@pytest.mark.parametrize("name", EXACT + GENERAL[:3] + EDGES)
def test_oracle_matches_the_reference_fixture(name):
    """The exact cases: every float and integer equal.  The others: the dense result within delta of the reference's float32
    (whole, or on the recorded sample); integers equal where the case has no open pixel."""
    z = np.load(GOLDEN)
    lr, S, inp, orig, frame, crop = load(z, name)
    v = O.chain(lr, S, inp, orig)
    delta = float(z[f"{name}/delta"])
    if f"{name}/dense32" in z:
        assert np.abs(v - z[f"{name}/dense32"]).max() <= delta
    else:
        assert np.abs(v.reshape(-1)[z[f"{name}/sample_idx"]] - z[f"{name}/sample32"]).max() <= delta
    if z[f"{name}/nopen"].sum() == 0:
        n_hi, n_lo, area, box, stab = O.stats(v, 0.0, 1.0)
        assert np.array_equal(np.stack([n_hi, n_lo, area], 1), z[f"{name}/ref_counts"])
        assert np.array_equal(box, z[f"{name}/ref_boxes"])
        assert np.array_equal(stab, z[f"{name}/ref_stability"], equal_nan=True)
        box_frame = box + np.array([crop[0], crop[1], crop[0], crop[1]], np.int32)
        assert np.array_equal(O.near_crop_edge(box_frame, crop, frame), z[f"{name}/ref_near_edge"])
        full = O.uncrop(v > 0, crop, frame)
        stops = np.cumsum(z[f"{name}/ref_rle_lens"])
        for m in range(v.shape[0]):
            counts = O.rle(full[m])
            assert counts == z[f"{name}/ref_rle_flat"][stops[m] - len(counts):stops[m]].tolist()
            assert np.array_equal(O.rle_to_mask(counts, frame), full[m])
        assert np.array_equal(O.unpack(O.pack(full), frame[0]), full)


def test_oracle_nms_rule():
    a, b, c = [0, 0, 10, 10], [0, 1, 10, 11], [0, 2, 10, 12]          # IoU(a,b) = IoU(b,c) = 9/11, IoU(a,c) = 8/12
    assert O.nms([a, b, c], [0.9, 0.8, 0.7], 0.7) == [0, 2]            # a suppresses b; c survives although IoU(b,c) > thr
    assert O.nms([a, a], [0.5, 0.5], 0.5) == [0]
    assert O.nms([[0, 0, 0, 0], [0, 0, 0, 0]], [1.0, 0.5], 0.1) == [0, 1]     # NaN never suppresses
    assert O.nms([[0, 0, 2, 2], [0, 0, 2, 1]], [1.0, 0.5], 0.5) == [0, 1]      # IoU exactly the threshold: kept


def test_module_imports_and_rejects_arguments_without_a_device():
    import sam_masks as sm
    lr = torch.zeros(2, 16, 16)
    ok = dict(img_size=64, input_size=(64, 64), original_size=(32, 32))
    with pytest.raises(ValueError, match="HIP device"):
        sm.mask_pass(lr, **ok)
    with pytest.raises(ValueError, match="float32"):
        sm.mask_pass(lr.double(), **ok)
    with pytest.raises(ValueError, match=r"\(M,h,w\)"):
        sm.mask_pass(lr[0], **ok)
    with pytest.raises(ValueError, match="beyond img_size"):
        sm.mask_pass(lr, 64, (65, 64), (32, 32))
    with pytest.raises(ValueError, match="original_size"):
        sm.mask_pass(lr, 64, (64, 64), (0, 32))
    with pytest.raises(ValueError, match="iou_preds"):
        sm.mask_pass(lr, iou_preds=torch.zeros(3), **ok)
    with pytest.raises(ValueError, match="not of original_size"):
        sm.mask_pass(lr, crop_box=(0, 0, 30, 32), frame_size=(40, 40), **ok)
    with pytest.raises(ValueError, match="does not lie in the frame"):
        sm.mask_pass(lr, crop_box=(10, 10, 42, 42), frame_size=(40, 40), **ok)
    with pytest.raises(ValueError, match="mask_threshold"):
        sm.mask_pass(lr, mask_threshold="0", **ok)
    with pytest.raises(ValueError, match="torch.float32 or torch.bool"):
        sm.upscale_masks(lr, 64, (64, 64), (32, 32), out=torch.int32)
    with pytest.raises(ValueError, match="HIP device"):
        sm.upscale_masks(lr, 64, (64, 64), (32, 32))
    with pytest.raises(ValueError, match=r"\(M,4\)"):
        sm.box_nms(torch.zeros(3, 3), torch.zeros(3), 0.5)
    with pytest.raises(ValueError, match="scores"):
        sm.box_nms(torch.zeros(3, 4), torch.zeros(2), 0.5)
    with pytest.raises(ValueError, match="up to 16384"):
        sm.box_nms(torch.zeros(16385, 4), torch.zeros(16385), 0.5)
    with pytest.raises(ValueError, match="HIP device"):
        sm.batched_nms(torch.zeros(3, 4), torch.zeros(3), torch.zeros(3, dtype=torch.int64), 0.5)
    with pytest.raises(ValueError, match="PackedMasks"):
        sm.masks_to_rle(torch.zeros(1, 4, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="packed.words"):
        sm.unpack_masks(sm.PackedMasks(torch.zeros(1, 4, 2, dtype=torch.int32), (33, 5)))
    with pytest.raises(ValueError, match="HIP device"):
        sm.masks_to_rle(sm.pack_masks(torch.zeros(1, 33, 5, dtype=torch.bool)))
    with pytest.raises(ValueError, match="output_mode"):
        sm.MaskPostprocessor((32, 32), output_mode="coco_rle")
    assert np.array_equal(sm.pack_masks(torch.ones(1, 33, 2, dtype=torch.bool)).words.numpy(), O.pack(np.ones((1, 33, 2), bool)))


def test_c_abi_rejects_bad_arguments_before_any_launch():
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    assert lib.f3dgs_version() >= 31400
    lib.f3dgs_sam_masks_scratch_bytes.restype = lib.f3dgs_box_nms_scratch_bytes.restype = ctypes.c_size_t
    assert lib.f3dgs_sam_masks_scratch_bytes(3) == 96 and lib.f3dgs_sam_masks_scratch_bytes(65536) == 0
    assert lib.f3dgs_box_nms_scratch_bytes(130) == 130 * 3 * 8 and lib.f3dgs_box_nms_scratch_bytes(16385) == 0
    vp, f = ctypes.c_void_p, ctypes.c_float
    lib.f3dgs_sam_upscale.argtypes = [ctypes.c_int] * 8 + [vp, f, ctypes.c_int, vp, vp]
    assert lib.f3dgs_sam_upscale(1, 16, 16, 64, 65, 64, 8, 8, None, 0.0, 0, None, None) == -1 and b"beyond img_size" in lib.f3dgs_last_error()
    assert lib.f3dgs_sam_upscale(1, 16, 16, 64, 64, 64, 8, 8, None, 0.0, 0, None, None) == -1 and b"null" in lib.f3dgs_last_error()
    assert lib.f3dgs_sam_upscale(70000, 16, 16, 64, 64, 64, 8, 8, None, 0.0, 0, None, None) == -4
    lib.f3dgs_sam_masks.argtypes = [ctypes.c_int] * 12 + [vp, vp] + [f] * 5 + [ctypes.c_int] + [vp] * 10
    rc = lib.f3dgs_sam_masks(1, 16, 16, 64, 64, 64, 8, 8, 8, 8, 1, 0, *([None] * 2), 0.0, 0.0, 1.0, -1.0, 0.0, 1, *([None] * 10))
    assert rc == -1 and b"does not lie in the frame" in lib.f3dgs_last_error()
    lib.f3dgs_box_nms.argtypes = [ctypes.c_int, vp, vp, f, vp, vp, vp, vp, vp]
    assert lib.f3dgs_box_nms(16385, *([None] * 2), 0.5, *([None] * 5)) == -4
    assert lib.f3dgs_box_nms(4, *([None] * 2), 0.5, *([None] * 5)) == -1
