#!/usr/bin/env python3
"""Records what the argument checks of the operators' C entry points answer: return code and f3dgs_last_error() text.

    python tests/golden/make_entry_validation.py path/to/libf3dgs_hip.so [out.json]

writes tests/golden/entry_validation.json (or out.json): one record {"fn", "label", "rc", "error"} per call of CALLS, in order.
tests/test_entry_validation_cpu.py replays the same list against the library of the tree and compares every record exactly.
The committed file was recorded from the library of the commit BEFORE the entry points moved from api.hip into their units, so
it pins every answer across that move.

The list needs no GPU, and must never need one: NO CALL HERE MAY PASS ITS VALIDATION AND REACH A LAUNCH.  Every call either
fails a check or takes an early F3DGS_OK return (P == 0, n == 0, HW == 0, Hs == 0), all of which come before the first HIP call.
Pointers that the checks only compare or test for alignment are fake (A, A2: 16-byte aligned; B: 8 mod 16; B4: 4 mod 8); the
tables the checks read on the host (Adam, densify) are real ctypes arrays.
"rc" is the returned int; for the *_scratch_bytes functions the byte count, for f3dgs_feature_l1_lowres_grad the returned
address (the scratch base here is fake, so it is an offset from A) - "error" is null for those and for F3DGS_OK.
"""
import ctypes
import json
import os
import sys
from ctypes import c_double as D, c_float as F, c_int as I, c_longlong as LL, c_size_t as Z, c_void_p as P

A, A2, B, B4 = 0x10000, 0x20000, 0x10008, 0x10004
NAN, INF = float("nan"), float("inf")


class AdamTensor(ctypes.Structure):
    _fields_ = [("param", P), ("grad", P), ("exp_avg", P), ("exp_avg_sq", P), ("n", Z), ("lr", D), ("step", I)]


class AdamDeviceTensor(ctypes.Structure):
    _fields_ = [("param", P), ("grad", P), ("exp_avg", P), ("exp_avg_sq", P), ("n", Z), ("step", P), ("lr", P), ("scheduled", I),
                ("lr_init", D), ("lr_final", D), ("lr_delay_mult", D), ("lr_delay_steps", LL), ("max_steps", LL)]


class DensifyTensor(ctypes.Structure):
    _fields_ = [("src", P), ("dst", P), ("override_src", P), ("width", I), ("mode", I)]


def adam(*rows):
    """rows of (n, step) or (n, step, param): a table of f3dgs_adam_tensor with fake pointers"""
    t = (AdamTensor * len(rows))()
    for k, r in enumerate(rows):
        p = r[2] if len(r) > 2 else A
        t[k] = AdamTensor(p, A, A, A, r[0], 1e-3, r[1])
    return t


def adam_dev(*rows):
    """rows of dicts over the defaults: a table of f3dgs_adam_device_tensor with fake pointers"""
    t = (AdamDeviceTensor * len(rows))()
    for k, r in enumerate(rows):
        v = dict(param=A, grad=A, exp_avg=A, exp_avg_sq=A, n=8, step=A, lr=A, scheduled=0, lr_init=1e-2, lr_final=1e-4,
                 lr_delay_mult=1.0, lr_delay_steps=0, max_steps=100)
        v.update(r)
        t[k] = AdamDeviceTensor(**v)
    return t


def densify(*rows):
    """rows of (src, dst, override_src, width, mode)"""
    t = (DensifyTensor * len(rows))()
    for k, r in enumerate(rows):
        t[k] = DensifyTensor(*r)
    return t


SIZE, ADDR = "size", "addr"      # what a function returns where it is not an int code

# fn -> (kind of result, argtypes)
SIGNATURES = {
    "f3dgs_instance_scratch_bytes": (SIZE, [I, I]),
    "f3dgs_instance_associate": (I, [I, I, I, P, P, D, D, P, P, P, P, P, P, P, P]),
    "f3dgs_instance_merge": (I, [I, I, I, P, I, P, P, P]),
    "f3dgs_feature_l1_scratch_bytes": (SIZE, [I, I, I, I, I]),
    "f3dgs_feature_l1": (I, [I] * 6 + [P] * 10),
    "f3dgs_feature_l1_lowres_grad": (ADDR, [I, I, I, I, I, P]),
    "f3dgs_feature_decode_scratch_bytes": (SIZE, [I, I, I, I]),
    "f3dgs_feature_decode": (I, [I] * 6 + [P] * 4 + [I, P, P]),
    "f3dgs_segment_scratch_bytes": (SIZE, [I] * 6),
    "f3dgs_segment": (I, [I] * 7 + [P] * 4 + [I] + [P] * 4),
    "f3dgs_feature_pca_scratch_bytes": (SIZE, [I, LL, I]),
    "f3dgs_feature_pca_moments": (I, [I, LL, I, P, P, P, P, P]),
    "f3dgs_feature_pca_project": (I, [I, LL] + [P] * 7),
    "f3dgs_view_normals": (I, [I, I, P, P, P, P, I, P]),
    "f3dgs_view_gradient": (I, [I, I, I, P, P, P, P]),
    "f3dgs_view_curvature": (I, [I, I, P, P, P, P, P, P]),
    "f3dgs_view_minmax": (I, [LL, P, P, P]),
    "f3dgs_view_palette": (I, [LL, P, P, P, I, I, P, P, P]),
    "f3dgs_view_bytes": (I, [LL, P, P, P]),
    "f3dgs_adam_step": (I, [Z, P, P, P, P, D, D, D, D, I, P]),
    "f3dgs_adam_step_rows": (I, [Z, Z, P, P, P, P, P, D, D, D, D, I, P]),
    "f3dgs_adam_step_multi": (I, [I, P, D, D, D, P, Z, P]),
    "f3dgs_adam_schedule": (I, [I, P, D, D, P, I, P, P]),
    "f3dgs_adam_step_multi_device": (I, [I, P, D, D, D, P, Z, P, P]),
    "f3dgs_reset_opacity": (I, [Z, P, P, P, F, P]),
    "f3dgs_densify_gather": (I, [Z, P, P, P, I, P, P]),
    "f3dgs_knn_scratch_bytes": (SIZE, [I]),
    "f3dgs_knn_mean_dist2": (I, [I, P, P, P, P]),
    "f3dgs_knn_neighbors_scratch_bytes": (SIZE, [I, I]),
    "f3dgs_knn_neighbors": (I, [I, I, P, P, P, P, P]),
    "f3dgs_label_mode_filter": (I, [I, I, P, P, P, P, F, I, P, P, P]),
    # these three stay in api.hip: the shared formatter must leave them alone
    "f3dgs_contributions": (I, [I, I, I, I, P, P, P, I] + [P] * 8),
    "f3dgs_label_votes": (I, [I, I, I, I, P, P, P, P, I, I, P, P]),
    "f3dgs_backward": (I, [I] * 5 + [P, I, I] + [P] * 5 + [F] + [P] * 5 + [F, F] + [P] * 7 + [P] * 11 + [P, I, P]),
}

B1, B2, EPS = 0.9, 0.999, 1e-15
BIG_N = 1 << 41           # elements of one Adam tensor that alone need 2^31 workgroups


def _device_table_calls(fn, tail):
    """The checks f3dgs_adam_schedule and f3dgs_adam_step_multi_device share; tail(consts) -> the arguments behind beta2."""
    def call(label, n, table, b1=B1, b2=B2, consts=A):
        return (fn, label, (n, table, b1, b2) + tail(consts))
    return [
        call("n_tensors -1", -1, adam_dev({})),
        call("n_tensors 17", 17, adam_dev({})),
        call("beta1 1", 1, adam_dev({}), b1=1.0),
        call("beta2 negative", 1, adam_dev({}), b2=-0.1),
        call("beta1 nan", 1, adam_dev({}), b1=NAN),
        call("n_tensors 0: ok", 0, None),
        call("null table", 1, None),
        call("null consts", 1, adam_dev({}), consts=None),
        call("consts misaligned", 1, adam_dev({}), consts=B4),
        call("max_steps 0", 2, adam_dev({}, dict(scheduled=1, max_steps=0))),
        call("lr_delay_steps -1", 1, adam_dev(dict(scheduled=1, lr_delay_steps=-1))),
        call("rates: final zero only", 1, adam_dev(dict(scheduled=1, lr_final=0.0))),
        call("rates: negative", 1, adam_dev(dict(scheduled=1, lr_init=-1.0))),
        call("null pointer", 2, adam_dev({}, dict(grad=None))),
        call("null step word", 1, adam_dev(dict(step=None))),
        call("null rate word", 1, adam_dev(dict(lr=None))),
        call("too large", 1, adam_dev(dict(n=BIG_N))),
    ]


CALLS = [
    # ---- instances.hip
    ("f3dgs_instance_scratch_bytes", "valid 1 x 1", (1, 1)),
    ("f3dgs_instance_scratch_bytes", "valid 1024 x 4096", (1024, 4096)),
    ("f3dgs_instance_scratch_bytes", "refused M 0", (0, 1)),
    ("f3dgs_instance_scratch_bytes", "refused L 4097", (1, 4097)),
    ("f3dgs_instance_associate", "P -1", (-1, 4, 4, A, A, 0.5, 0.0, A, A, A, A, A, A, A, None)),
    ("f3dgs_instance_associate", "M 0", (10, 0, 4, A, A, 0.5, 0.0, A, A, A, A, A, A, A, None)),
    ("f3dgs_instance_associate", "M 1025", (10, 1025, 4, A, A, 0.5, 0.0, A, A, A, A, A, A, A, None)),
    ("f3dgs_instance_associate", "L 0", (10, 4, 0, A, A, 0.5, 0.0, A, A, A, A, A, A, A, None)),
    ("f3dgs_instance_associate", "L 4097", (10, 4, 4097, A, A, 0.5, 0.0, A, A, A, A, A, A, A, None)),
    ("f3dgs_instance_associate", "iou_thresh negative", (10, 4, 4, A, A, -0.5, 0.0, A, A, A, A, A, A, A, None)),
    ("f3dgs_instance_associate", "iou_thresh nan", (10, 4, 4, A, A, NAN, 0.0, A, A, A, A, A, A, A, None)),
    ("f3dgs_instance_associate", "min_weight negative", (10, 4, 4, A, A, 0.5, -1.0, A, A, A, A, A, A, A, None)),
    ("f3dgs_instance_associate", "min_weight nan", (10, 4, 4, A, A, 0.5, NAN, A, A, A, A, A, A, A, None)),
    ("f3dgs_instance_associate", "null count, P 0", (0, 4, 4, None, None, 0.5, 0.0, None, A, A, A, A, A, A, None)),
    ("f3dgs_instance_associate", "null scratch", (0, 4, 4, None, None, 0.5, 0.0, A, A, A, A, A, A, None, None)),
    ("f3dgs_instance_associate", "null acc_view, P 10", (10, 4, 4, None, A, 0.5, 0.0, A, A, A, A, A, A, A, None)),
    ("f3dgs_instance_associate", "scratch misaligned", (10, 4, 4, A, A, 0.5, 0.0, A, A, A, A, A, A, B, None)),
    ("f3dgs_instance_merge", "P -1", (-1, 4, 4, A, 0, A, A, None)),
    ("f3dgs_instance_merge", "M 0", (10, 0, 4, A, 0, A, A, None)),
    ("f3dgs_instance_merge", "L 4097", (10, 4, 4097, A, 0, A, A, None)),
    ("f3dgs_instance_merge", "null mapping", (0, 4, 4, None, 0, None, None, None)),
    ("f3dgs_instance_merge", "null acc, P 10", (10, 4, 4, A, 1, A, None, None)),
    ("f3dgs_instance_merge", "P 0: ok", (0, 4, 4, None, 0, A, None, None)),
    # ---- feature_loss.hip
    ("f3dgs_feature_l1_scratch_bytes", "valid decoder 32 -> 64, 10 x 12", (32, 64, 10, 12, 1)),
    ("f3dgs_feature_l1_scratch_bytes", "valid plain 16, 5 x 7", (16, 16, 5, 7, 0)),
    ("f3dgs_feature_l1_scratch_bytes", "refused C 0", (0, 64, 10, 12, 1)),
    ("f3dgs_feature_l1_scratch_bytes", "refused Hg 0", (32, 64, 0, 12, 1)),
    ("f3dgs_feature_l1", "C 0", (0, 20, 24, 64, 10, 12, A, A, A, A, A, A, A, A, A, None)),
    ("f3dgs_feature_l1", "Wg 0", (32, 20, 24, 64, 10, 0, A, A, A, A, A, A, A, A, A, None)),
    ("f3dgs_feature_l1", "null feature_map", (32, 20, 24, 64, 10, 12, None, A, A, A, A, A, A, A, A, None)),
    ("f3dgs_feature_l1", "null scratch", (32, 20, 24, 64, 10, 12, A, A, A, A, A, A, A, A, None, None)),
    ("f3dgs_feature_l1", "weight without bias", (32, 20, 24, 64, 10, 12, A, A, None, A, A, A, A, A, A, None)),
    ("f3dgs_feature_l1", "bias without weight", (32, 20, 24, 64, 10, 12, A, None, A, A, A, A, A, A, A, None)),
    ("f3dgs_feature_l1", "null d_weight", (32, 20, 24, 64, 10, 12, A, A, A, A, A, A, None, A, A, None)),
    ("f3dgs_feature_l1", "decoder width 48", (48, 20, 24, 64, 10, 12, A, A, A, A, A, A, A, A, A, None)),
    ("f3dgs_feature_l1", "plain, Cout != C", (32, 20, 24, 64, 10, 12, A, None, None, A, A, A, None, None, A, None)),
    ("f3dgs_feature_l1", "plain, too large", (1024, 20, 24, 1024, 1 << 15, 1 << 15, A, None, None, A, A, A, None, None, A, None)),
    ("f3dgs_feature_l1", "decoder, too large", (32, 20, 24, 1024, 1 << 15, 1 << 15, A, A, A, A, A, A, A, A, A, None)),
    ("f3dgs_feature_l1", "weight misaligned", (32, 20, 24, 64, 10, 12, A, B, A, A, A, A, A, A, A, None)),
    ("f3dgs_feature_l1", "scratch misaligned", (32, 20, 24, 64, 10, 12, A, A, A, A, A, A, A, A, B, None)),
    ("f3dgs_feature_l1_lowres_grad", "valid decoder 32 -> 64, 10 x 12", (32, 64, 10, 12, 1, A)),
    ("f3dgs_feature_l1_lowres_grad", "valid plain 16, 5 x 7", (16, 16, 5, 7, 0, A)),
    ("f3dgs_feature_l1_lowres_grad", "refused C 0", (0, 64, 10, 12, 1, A)),
    ("f3dgs_feature_l1_lowres_grad", "refused null scratch", (32, 64, 10, 12, 1, None)),
    ("f3dgs_feature_decode_scratch_bytes", "valid decoder 32, 10 x 12", (32, 10, 12, 1)),
    ("f3dgs_feature_decode_scratch_bytes", "valid plain 64, 7 x 9", (64, 7, 9, 0)),
    ("f3dgs_feature_decode_scratch_bytes", "refused C 0", (0, 10, 12, 1)),
    ("f3dgs_feature_decode_scratch_bytes", "refused Wg 0", (32, 10, 0, 1)),
    ("f3dgs_feature_decode", "H 0", (32, 0, 24, 64, 10, 12, A, A, A, A, 0, A, None)),
    ("f3dgs_feature_decode", "null out", (32, 20, 24, 64, 10, 12, A, A, A, None, 0, A, None)),
    ("f3dgs_feature_decode", "weight without bias", (32, 20, 24, 64, 10, 12, A, A, None, A, 0, A, None)),
    ("f3dgs_feature_decode", "decoder, null scratch", (32, 20, 24, 64, 10, 12, A, A, A, A, 1, None, None)),
    ("f3dgs_feature_decode", "decoder width 48", (48, 20, 24, 64, 10, 12, A, A, A, A, 0, A, None)),
    ("f3dgs_feature_decode", "weight misaligned", (32, 20, 24, 64, 10, 12, A, B, A, A, 0, A, None)),
    ("f3dgs_feature_decode", "scratch misaligned", (32, 20, 24, 64, 10, 12, A, A, A, A, 0, B, None)),
    ("f3dgs_feature_decode", "plain, Cout != C", (32, 20, 24, 64, 10, 12, A, None, None, A, 0, None, None)),
    # ---- segment.hip
    ("f3dgs_segment_scratch_bytes", "valid decoder 32 -> 64, 10 x 12, K 5", (32, 64, 10, 12, 5, 1)),
    ("f3dgs_segment_scratch_bytes", "valid plain 16, empty map, K 3", (16, 16, 0, 0, 3, 0)),
    ("f3dgs_segment_scratch_bytes", "refused K 0", (32, 64, 10, 12, 0, 1)),
    ("f3dgs_segment_scratch_bytes", "refused Hs Ws above 2^30", (32, 64, 1 << 16, 1 << 15, 5, 1)),
    ("f3dgs_segment", "C 0", (0, 20, 24, 64, 10, 12, 5, A, A, A, A, 0, A, A, A, None)),
    ("f3dgs_segment", "Hs -1", (32, 20, 24, 64, -1, 12, 5, A, A, A, A, 0, A, A, A, None)),
    ("f3dgs_segment", "unknown flag", (32, 20, 24, 64, 10, 12, 5, A, A, A, A, 0x4, A, A, A, None)),
    ("f3dgs_segment", "weight without bias", (32, 20, 24, 64, 10, 12, 5, A, A, None, A, 0, A, A, A, None)),
    ("f3dgs_segment", "plain, Cout != C", (32, 20, 24, 64, 10, 12, 5, A, None, None, A, 0, A, A, A, None)),
    ("f3dgs_segment", "K 257", (32, 20, 24, 64, 10, 12, 257, A, A, A, A, 0, A, A, A, None)),
    ("f3dgs_segment", "decoder width 48", (48, 20, 24, 64, 10, 12, 5, A, A, A, A, 0, A, A, A, None)),
    ("f3dgs_segment", "decoder output 48", (32, 20, 24, 48, 10, 12, 5, A, A, A, A, 0, A, A, A, None)),
    ("f3dgs_segment", "Hs Ws above 2^30", (32, 20, 24, 64, 1 << 16, 1 << 15, 5, A, A, A, A, 0, A, A, A, None)),
    ("f3dgs_segment", "H W above 2^28", (32, 1 << 15, 1 << 15, 64, 10, 12, 5, A, A, A, A, 0, A, A, A, None)),
    ("f3dgs_segment", "Hs 0: ok", (32, 20, 24, 64, 0, 12, 5, A, A, A, A, 0, A, A, A, None)),
    ("f3dgs_segment", "Ws 0: ok", (32, 20, 24, 32, 10, 0, 5, None, None, None, None, 0, None, None, None, None)),
    ("f3dgs_segment", "null text", (32, 20, 24, 64, 10, 12, 5, A, A, A, None, 0, A, A, A, None)),
    ("f3dgs_segment", "decoder, null scratch", (32, 20, 24, 64, 10, 12, 5, A, A, A, A, 0x2, A, A, None, None)),
    ("f3dgs_segment", "plain, text to normalise, null scratch", (32, 20, 24, 32, 10, 12, 5, A, None, None, A, 0x1, A, A, None, None)),
    # ---- feature_pca.hip
    ("f3dgs_feature_pca_scratch_bytes", "valid C 3, 100", (3, 100, 1)),
    ("f3dgs_feature_pca_scratch_bytes", "valid C 64, 10000, stride 4", (64, 10000, 4)),
    ("f3dgs_feature_pca_scratch_bytes", "refused C 2", (2, 100, 1)),
    ("f3dgs_feature_pca_scratch_bytes", "refused stride 0", (64, 100, 0)),
    ("f3dgs_feature_pca_scratch_bytes", "empty map", (64, 0, 1)),
    ("f3dgs_feature_pca_moments", "C 2", (2, 100, 1, A, A, A, A, None)),
    ("f3dgs_feature_pca_moments", "C 4097", (4097, 100, 1, A, A, A, A, None)),
    ("f3dgs_feature_pca_moments", "HW -1", (64, -1, 1, A, A, A, A, None)),
    ("f3dgs_feature_pca_moments", "HW above 2^30", (64, (1 << 30) + 1, 1, A, A, A, A, None)),
    ("f3dgs_feature_pca_moments", "stride 0", (64, 100, 0, A, A, A, A, None)),
    ("f3dgs_feature_pca_moments", "HW 0: ok", (64, 0, 1, None, None, None, None, None)),
    ("f3dgs_feature_pca_moments", "2 samples", (64, 2, 1, A, A, A, A, None)),
    ("f3dgs_feature_pca_moments", "2 samples by the stride", (64, 10, 5, A, A, A, A, None)),
    ("f3dgs_feature_pca_moments", "null cov", (64, 100, 1, A, A, None, A, None)),
    ("f3dgs_feature_pca_project", "C 2", (2, 100, A, A, A, None, None, A, None)),
    ("f3dgs_feature_pca_project", "HW above 2^30", (64, (1 << 30) + 1, A, A, A, None, None, A, None)),
    ("f3dgs_feature_pca_project", "lo without hi", (64, 100, A, A, A, A, None, A, None)),
    ("f3dgs_feature_pca_project", "HW 0: ok", (64, 0, None, None, None, None, None, None, None)),
    ("f3dgs_feature_pca_project", "null out", (64, 100, A, A, A, None, None, None, None)),
    # ---- view_modes.hip
    ("f3dgs_view_normals", "H -1", (-1, 8, A, A, A, A, 0, None)),
    ("f3dgs_view_normals", "unknown flag", (8, 8, A, A, A, A, 0x4, None)),
    ("f3dgs_view_normals", "too large", (1 << 16, 1 << 15, A, A, A, A, 0, None)),
    ("f3dgs_view_normals", "one row", (1, 8, A, A, A, A, 0, None)),
    ("f3dgs_view_normals", "H 0: ok", (0, 8, None, None, None, None, 0x3, None)),
    ("f3dgs_view_normals", "null proj", (8, 8, A, None, A, A, 0, None)),
    ("f3dgs_view_gradient", "Cn 0", (0, 8, 8, A, A, None, None)),
    ("f3dgs_view_gradient", "W -1", (3, 8, -1, A, A, None, None)),
    ("f3dgs_view_gradient", "too large", (3, 1 << 16, 1 << 15, A, A, None, None)),
    ("f3dgs_view_gradient", "H 0: ok", (3, 0, 8, None, None, None, None)),
    ("f3dgs_view_gradient", "W 0: ok", (3, 8, 0, None, None, None, None)),
    ("f3dgs_view_gradient", "null out", (3, 1, 8, A, None, None, None)),
    ("f3dgs_view_curvature", "W -1", (8, -1, A, A, A, A, None, None)),
    ("f3dgs_view_curvature", "too large", (1 << 16, 1 << 15, A, A, A, A, None, None)),
    ("f3dgs_view_curvature", "one column", (8, 1, A, A, A, A, None, None)),
    ("f3dgs_view_curvature", "W 0: ok", (8, 0, None, None, None, None, None, None)),
    ("f3dgs_view_curvature", "null depth", (8, 8, None, A, A, A, None, None)),
    ("f3dgs_view_minmax", "n -1", (-1, A, A, None)),
    ("f3dgs_view_minmax", "n above 2^30", ((1 << 30) + 1, A, A, None)),
    ("f3dgs_view_minmax", "n 0: ok", (0, None, None, None)),
    ("f3dgs_view_minmax", "null minmax", (100, A, None, None)),
    ("f3dgs_view_palette", "HW -1", (-1, A, A, A, 256, 0, A, None, None)),
    ("f3dgs_view_palette", "unknown mode", (100, A, A, A, 256, 2, A, None, None)),
    ("f3dgs_view_palette", "HW above 2^30", ((1 << 30) + 1, A, A, A, 256, 0, A, None, None)),
    ("f3dgs_view_palette", "L 1", (100, A, A, A, 1, 0, A, None, None)),
    ("f3dgs_view_palette", "L 4097", (100, A, A, A, 4097, 1, A, None, None)),
    ("f3dgs_view_palette", "HW 0: ok", (0, None, None, None, 2, 1, None, None, None)),
    ("f3dgs_view_palette", "no output", (100, A, A, A, 256, 0, None, None, None)),
    ("f3dgs_view_bytes", "HW -1", (-1, A, A, None)),
    ("f3dgs_view_bytes", "HW above 2^30", ((1 << 30) + 1, A, A, None)),
    ("f3dgs_view_bytes", "HW 0: ok", (0, None, None, None)),
    ("f3dgs_view_bytes", "null image", (100, None, A, None)),
    # ---- adam.hip
    ("f3dgs_adam_step", "n 0: ok", (0, None, None, None, None, 1e-3, B1, B2, EPS, 1, None)),
    ("f3dgs_adam_step", "null grad", (100, A, None, A, A, 1e-3, B1, B2, EPS, 1, None)),
    ("f3dgs_adam_step", "step 0", (100, A, A, A, A, 1e-3, B1, B2, EPS, 0, None)),
    ("f3dgs_adam_step_rows", "n 0: ok", (0, 4, None, None, None, None, None, 1e-3, B1, B2, EPS, 1, None)),
    ("f3dgs_adam_step_rows", "null exp_avg_sq", (100, 4, A, A, A, A, None, 1e-3, B1, B2, EPS, 1, None)),
    ("f3dgs_adam_step_rows", "step 0", (100, 4, A, A, A, A, A, 1e-3, B1, B2, EPS, 0, None)),
    ("f3dgs_adam_step_rows", "mask, width 0", (100, 0, A, A, A, A, A, 1e-3, B1, B2, EPS, 1, None)),
    ("f3dgs_adam_step_rows", "mask, n no multiple of the width", (100, 3, A, A, A, A, A, 1e-3, B1, B2, EPS, 1, None)),
    ("f3dgs_adam_step_rows", "mask, width of 2^32", (1 << 32, 1 << 32, A, A, A, A, A, 1e-3, B1, B2, EPS, 1, None)),
    ("f3dgs_adam_step_multi", "n_tensors -1", (-1, adam((8, 1)), B1, B2, EPS, None, 0, None)),
    ("f3dgs_adam_step_multi", "n_tensors 17", (17, adam((8, 1)), B1, B2, EPS, None, 0, None)),
    ("f3dgs_adam_step_multi", "n_tensors 0: ok", (0, None, B1, B2, EPS, None, 0, None)),
    ("f3dgs_adam_step_multi", "null table", (1, None, B1, B2, EPS, None, 0, None)),
    ("f3dgs_adam_step_multi", "tensor 1: null pointer", (2, adam((8, 1), (8, 1, None)), B1, B2, EPS, None, 0, None)),
    ("f3dgs_adam_step_multi", "tensor 2: step 0", (3, adam((8, 1), (0, 0), (8, 0)), B1, B2, EPS, None, 0, None)),
    ("f3dgs_adam_step_multi", "too large", (1, adam((BIG_N, 1)), B1, B2, EPS, None, 0, None)),
    ("f3dgs_adam_step_multi", "mask without rows", (1, adam((8, 1)), B1, B2, EPS, A, 0, None)),
] + _device_table_calls("f3dgs_adam_schedule", lambda consts: (A, 1, consts, None)) + [
    ("f3dgs_adam_schedule", "scheduled, null iteration", (2, adam_dev({}, dict(scheduled=1)), B1, B2, None, 1, A, None)),
    ("f3dgs_adam_schedule", "iteration misaligned", (1, adam_dev({}), B1, B2, B4, 1, A, None)),
] + _device_table_calls("f3dgs_adam_step_multi_device", lambda consts: (EPS, None, 0, consts, None)) + [
    ("f3dgs_adam_step_multi_device", "mask without rows", (1, adam_dev({}), B1, B2, EPS, A, 0, A, None)),
    ("f3dgs_adam_step_multi_device", "mask without rows, n_tensors 0", (0, None, B1, B2, EPS, A, 0, None, None)),
    ("f3dgs_reset_opacity", "cap 0", (100, A, A, A, 0.0, None)),
    ("f3dgs_reset_opacity", "cap 1", (100, A, A, A, 1.0, None)),
    ("f3dgs_reset_opacity", "cap nan", (100, A, A, A, NAN, None)),
    ("f3dgs_reset_opacity", "n 0: ok", (0, None, None, None, 0.5, None)),
    ("f3dgs_reset_opacity", "null raw", (100, None, A, A, 0.5, None)),
    ("f3dgs_reset_opacity", "n 2^39", (1 << 39, A, A, A, 0.5, None)),
    # ---- densify.hip
    ("f3dgs_densify_gather", "n_tensors -1", (100, A, A, A, -1, densify((A, A2, None, 3, 0)), None)),
    ("f3dgs_densify_gather", "n_tensors 33", (100, A, A, A, 33, densify((A, A2, None, 3, 0)), None)),
    ("f3dgs_densify_gather", "n_out 0: ok", (0, None, None, None, 1, None, None)),
    ("f3dgs_densify_gather", "n_tensors 0: ok", (100, None, None, None, 0, None, None)),
    ("f3dgs_densify_gather", "null kind", (100, A, None, A, 1, densify((A, A2, None, 3, 0)), None)),
    ("f3dgs_densify_gather", "null table", (100, A, A, A, 1, None, None)),
    ("f3dgs_densify_gather", "tensor 1: null dst", (100, A, A, A, 2, densify((A, A2, None, 3, 0), (A, None, None, 3, 0)), None)),
    ("f3dgs_densify_gather", "tensor 0: width 0", (100, A, A, A, 1, densify((A, A2, None, 0, 0)), None)),
    ("f3dgs_densify_gather", "tensor 0: width 65537", (100, A, A, A, 1, densify((A, A2, None, 65537, 0)), None)),
    ("f3dgs_densify_gather", "tensor 0: mode 3", (100, A, A, A, 1, densify((A, A2, None, 3, 3)), None)),
    ("f3dgs_densify_gather", "tensor 0: mode -1", (100, A, A, A, 1, densify((A, A2, None, 3, -1)), None)),
    ("f3dgs_densify_gather", "override child without override_src", (100, A, A, A, 1, densify((A, A2, None, 3, 2)), None)),
    ("f3dgs_densify_gather", "override child without override_row", (100, A, A, None, 1, densify((A, A2, A, 3, 2)), None)),
    # ---- knn.hip
    ("f3dgs_knn_scratch_bytes", "valid P 1", (1,)),
    ("f3dgs_knn_scratch_bytes", "valid P 1000", (1000,)),
    ("f3dgs_knn_scratch_bytes", "P -1 counts as none", (-1,)),
    ("f3dgs_knn_scratch_bytes", "P 0", (0,)),
    ("f3dgs_knn_mean_dist2", "P -1", (-1, A, A, A, None)),
    ("f3dgs_knn_mean_dist2", "P 0: ok", (0, None, None, None, None)),
    ("f3dgs_knn_mean_dist2", "null scratch", (100, A, A, None, None)),
    # ---- neighbors.hip
    ("f3dgs_knn_neighbors_scratch_bytes", "valid P 1, K 4", (1, 4)),
    ("f3dgs_knn_neighbors_scratch_bytes", "valid P 1000, K 16", (1000, 16)),
    ("f3dgs_knn_neighbors_scratch_bytes", "P -1 counts as none", (-1, 4)),
    ("f3dgs_knn_neighbors_scratch_bytes", "P 0, K 0", (0, 0)),
    ("f3dgs_knn_neighbors", "P -1", (-1, 4, A, A, A, A, None)),
    ("f3dgs_knn_neighbors", "K 0", (5, 0, A, A, A, A, None)),
    ("f3dgs_knn_neighbors", "K 17", (5, 17, A, A, A, A, None)),
    ("f3dgs_knn_neighbors", "P 0: ok", (0, 4, None, None, None, None, None)),
    ("f3dgs_knn_neighbors", "P above 2^30", ((1 << 30) + 1, 4, A, A, A, A, None)),
    ("f3dgs_knn_neighbors", "null idx", (5, 4, A, None, A, A, None)),
    ("f3dgs_knn_neighbors", "scratch misaligned", (5, 4, A, A, A, B, None)),
    ("f3dgs_label_mode_filter", "P -1", (-1, 4, A, None, A, A, INF, 0, A2, None, None)),
    ("f3dgs_label_mode_filter", "K 0", (5, 0, A, None, A, A, INF, 0, A2, None, None)),
    ("f3dgs_label_mode_filter", "K 17", (5, 17, A, None, A, A, INF, 0, A2, None, None)),
    ("f3dgs_label_mode_filter", "max_dist2 negative", (5, 4, A, None, A, A, -1.0, 0, A2, None, None)),
    ("f3dgs_label_mode_filter", "max_dist2 nan", (5, 4, A, None, A, A, NAN, 0, A2, None, None)),
    ("f3dgs_label_mode_filter", "P 0: ok", (0, 4, None, None, None, None, INF, 1, None, None, None)),
    ("f3dgs_label_mode_filter", "null labels_out", (5, 4, A, None, A, A, INF, 0, None, None, None)),
    ("f3dgs_label_mode_filter", "in place", (5, 4, A, None, A, A, INF, 0, A, None, None)),
    ("f3dgs_label_mode_filter", "finite max_dist2 without dist2", (5, 4, A, None, A, None, 2.5, 0, A2, None, None)),
    # ---- api.hip: the walks over the rasterizer's state and the backward call, which did not move
    ("f3dgs_contributions", "P -1", (-1, 0, 64, 64, A, A, A, 0) + (None,) * 8),
    ("f3dgs_contributions", "R -1", (10, -1, 64, 48, A, A, A, 0) + (None,) * 8),
    ("f3dgs_label_votes", "width 0", (10, 5, 0, 48, A, A, A, A, 0, 4, A, None)),
    ("f3dgs_backward", "P -1", (-1, 3, 16, 8, 5, A, 64, 48) + (A,) * 5 + (1.0,) + (A,) * 5 + (0.5, 0.5) + (A,) * 7 + (A,) * 11 + (A, 0, None)),
    ("f3dgs_backward", "R -1", (10, 3, 16, 8, -1, A, 64, 48) + (A,) * 5 + (1.0,) + (A,) * 5 + (0.5, 0.5) + (A,) * 7 + (A,) * 11 + (A, 0, None)),
]


def replay(lib):
    """Makes every call of CALLS against `lib` (a ctypes.CDLL of libf3dgs_hip.so); returns the list of records."""
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_last_error.argtypes = []
    records = []
    for fn, label, args in CALLS:
        kind, argtypes = SIGNATURES[fn]
        assert len(args) == len(argtypes), (fn, label, len(args), len(argtypes))
        f = getattr(lib, fn)
        f.argtypes = argtypes
        f.restype = Z if kind == SIZE else P if kind == ADDR else I
        rc = f(*args)
        rc = int(rc or 0)
        error = lib.f3dgs_last_error().decode() if kind is I and rc != 0 else None
        records.append({"fn": fn, "label": label, "rc": rc, "error": error})
    return records


def main():
    import torch  # noqa: F401  (its bundled HIP runtime must be the one the library binds to)
    here = os.path.dirname(os.path.abspath(__file__))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "entry_validation.json")
    records = replay(ctypes.CDLL(os.path.abspath(sys.argv[1])))
    with open(out, "w") as fh:
        json.dump(records, fh, indent=0)
        fh.write("\n")
    print(f"{len(records)} records, {sum(r['error'] is not None for r in records)} refusals -> {out}")


if __name__ == "__main__":
    main()
