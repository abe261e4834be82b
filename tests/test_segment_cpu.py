"""CPU checks of the open-vocabulary segmentation (segment.py, csrc/segment.hip): the argument errors of `segment` and of
the C-ABI entry point (no device work), `label_agreement` against a numpy restatement of the reference's metric, and the
precondition of every GPU case - the reference chain in float32 stays inside the label rule's cap against the float64
judge (tests/segment_oracle.py), so that a GPU failure is the kernel's and not the inputs'."""
import ctypes
import os

import numpy as np
import pytest
import torch

import segment as S
import segment_oracle as O
from util import ROOT


def test_segment_refuses_bad_arguments_before_any_device_work():
    fm, t = torch.rand(32, 6, 7), torch.rand(5, 128)
    w, b = torch.rand(128, 32), torch.rand(128)
    with pytest.raises(ValueError, match="expected"):
        S.segment(torch.rand(6, 7), t)
    with pytest.raises(ValueError, match="expected"):
        S.segment(fm, torch.rand(5))
    with pytest.raises(ValueError, match="float32"):
        S.segment(fm.half(), torch.rand(5, 32))
    with pytest.raises(ValueError, match="float32"):
        S.segment(fm, torch.rand(5, 32).double())
    with pytest.raises(ValueError, match="text embeddings"):
        S.segment(fm, torch.rand(257, 32))
    with pytest.raises(ValueError, match="text embeddings"):
        S.segment(fm, torch.rand(0, 32))
    with pytest.raises(ValueError, match="channels"):
        S.segment(fm, t)                                    # no decoder: the text must have C channels
    with pytest.raises(ValueError, match="channels"):
        S.segment(fm, torch.rand(5, 32), weight=w, bias=b)
    with pytest.raises(ValueError, match="size"):
        S.segment(fm, torch.rand(5, 32), size=(4,))
    with pytest.raises(ValueError, match="negative"):
        S.segment(fm, torch.rand(5, 32), size=(-1, 4))
    with pytest.raises(ValueError, match="weight"):
        S.segment(fm, t, weight=torch.rand(128, 16), bias=b)
    with pytest.raises(ValueError, match="weight"):
        S.segment(fm, t, weight=torch.rand(128, 32, 3, 3), bias=b)
    with pytest.raises(ValueError, match="bias"):
        S.segment(fm, t, weight=w, bias=torch.rand(64))
    with pytest.raises(ValueError, match="bias without weight"):
        S.segment(fm, torch.rand(5, 32), bias=b)
    with pytest.raises(ValueError, match="supported"):
        S.segment(torch.rand(48, 6, 7), torch.rand(5, 96), weight=torch.rand(96, 48))         # decoder width 48
    with pytest.raises(ValueError, match="supported"):
        S.segment(fm, torch.rand(5, 100), weight=torch.rand(100, 32))                          # Cout % 32 != 0
    before = t.clone()
    with pytest.raises(RuntimeError, match="HIP device"):          # well-formed, but there is no CPU path
        S.segment(fm, t, weight=w.reshape(128, 32, 1, 1), bias=b)
    assert torch.equal(t, before)
    with pytest.raises(ValueError, match="channels"):
        S.segment_reference_chain(fm, t, (400, 500))
    for n in ("segment", "segment_reference_chain", "label_agreement"):
        assert callable(getattr(S, n))


def _lib():
    so = os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(so)
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_segment.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 4
    lib.f3dgs_segment_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_segment_scratch_bytes.argtypes = [ctypes.c_int] * 6
    return lib


def test_c_abi_segment_rejects_bad_arguments():
    lib = _lib()
    lib.f3dgs_version.restype = ctypes.c_int
    assert lib.f3dgs_version() >= 30800
    dummy = (ctypes.c_float * 64)()
    p = ctypes.addressof(dummy)

    def call(C=32, H=8, W=8, Cout=128, Hs=4, Ws=4, K=5, fm=p, w=p, b=p, t=p, flags=1, lab=p, sc=None, scratch=p):
        return lib.f3dgs_segment(C, H, W, Cout, Hs, Ws, K, fm, w, b, t, flags, lab, sc, scratch, None)

    err = lambda: lib.f3dgs_last_error()
    for kw in (dict(C=0), dict(H=0), dict(Cout=0), dict(Hs=-1), dict(K=0)):
        assert call(**kw) < 0 and b"bad sizes" in err()
    assert call(flags=0x4) < 0 and b"flag" in err()
    assert call(b=None) < 0 and b"go together" in err()
    assert call(w=None, b=None) < 0 and b"without a decoder" in err()              # Cout != C
    rc_invalid = call(flags=0x4)
    rc_k = call(K=257)
    assert rc_k < 0 and rc_k != rc_invalid and b"limit" in err()                   # F3DGS_ERR_UNSUPPORTED
    assert call(C=48, Cout=96) == rc_k and b"supported" in err()
    assert call(Cout=100) == rc_k and b"supported" in err()
    for kw in (dict(fm=None), dict(t=None), dict(lab=None)):
        assert call(**kw) == rc_invalid and b"null" in err()
    assert call(scratch=None) == rc_invalid and b"scratch" in err()
    # an empty output is a success without any pointer
    assert call(Hs=0, fm=None, t=None, lab=None, scratch=None) == 0
    assert call(Ws=0, C=512, Cout=512, K=256, w=None, b=None, fm=None, t=None, lab=None, scratch=None) == 0
    # scratch: the resized map (with a decoder) and the text padded to 32 rows
    n = lib.f3dgs_segment_scratch_bytes(128, 512, 360, 480, 150, 1)
    assert 4 * (360 * 480 * 128 + 160 * 512) <= n <= 4 * (360 * 480 * 128 + 160 * 512) + 1024
    assert 4 * 160 * 512 <= lib.f3dgs_segment_scratch_bytes(512, 512, 360, 480, 150, 0) <= 4 * 160 * 512 + 512
    assert lib.f3dgs_segment_scratch_bytes(0, 512, 360, 480, 150, 0) == 0


def _np_metric(teacher, student, num_classes):
    """encoders/lseg_encoder/segmentation_metric.py:58-61, 76-90, restated"""
    acc = np.sum(teacher == student) / np.prod(teacher.shape)
    labels, counts = np.unique(np.concatenate((teacher, student)), return_counts=True)
    iou = []
    for i in labels[np.argsort(-counts, kind="stable")][:num_classes]:
        a, b = teacher == i, student == i
        iou.append(np.sum(np.logical_and(a, b)) / np.sum(np.logical_or(a, b)))
    return acc, np.nanmean(iou)


def test_label_agreement_equals_the_reference_metric():
    g = np.random.default_rng(5)
    teacher = g.integers(0, 12, size=(40, 50))
    teacher[teacher == 7] = 8                                  # class 7 is absent from both maps
    student = np.where(g.random((40, 50)) < 0.8, teacher, g.integers(0, 12, size=(40, 50)))
    student[student == 7] = 3
    for nc in (1, 5, 11, 12, 150):
        acc, iou = S.label_agreement(torch.from_numpy(teacher), torch.from_numpy(student), nc)
        wa, wi = _np_metric(teacher, student, nc)
        assert abs(acc - wa) < 1e-12 and abs(iou - wi) < 1e-12, (nc, acc, wa, iou, wi)
    # a label only one map holds has IoU 0 and counts; identical maps agree fully
    a, b = torch.tensor([[0, 0, 1, 1]]), torch.tensor([[0, 0, 2, 2]])
    acc, iou = S.label_agreement(a, b, 3)
    assert acc == 0.5 and abs(iou - 1.0 / 3.0) < 1e-12
    assert S.label_agreement(a, a, 150) == (1.0, 1.0)
    with pytest.raises(ValueError):
        S.label_agreement(a, torch.tensor([[0, 1]]), 2)


@pytest.mark.parametrize("family", O.FAMILIES)
@pytest.mark.parametrize("name", [c[0] for c in O.CASES])
def test_reference_chain_in_float32_meets_the_cap(name, family):
    """The precondition of the GPU cases: on these inputs the reference's own float32 arithmetic differs from the float64
    judge on at most MAX_SHARE of the pixels, each within tau."""
    d = O.make_inputs(name, family)
    l64 = O.chain(d["fm"], d["text"], d["size"], d["weight"], d["bias"], torch.float64)
    l32 = O.chain(d["fm"], d["text"], d["size"], d["weight"], d["bias"], torch.float32)
    assert torch.isfinite(l64).all()
    tau = O.tau_of(l32, l64)
    assert 0.0 < tau < 1e-2 or l64.shape[1] == 1
    O.judge(O.labels_of(l32), l64, tau)


def test_region_inputs_have_regions_and_boundaries():
    d = O.make_inputs("dec32_k20", "regions")
    lab = O.labels_of(O.chain(d["fm"], d["text"], d["size"], d["weight"], d["bias"])).reshape(d["size"])
    same = float((lab[:, 1:] == lab[:, :-1]).to(torch.float64).mean())
    assert 0.5 < same < 0.999 and len(torch.unique(lab)) >= 10


def test_special_pixels_in_the_judge():
    """torch.max's rule on the judge's side: a zero pixel, an inf, a NaN and an fp16 overflow have all-NaN logits and label 0."""
    d = O.make_inputs("nodec48_k20", "random")
    fm = O.add_special_pixels(d["fm"])
    l64 = O.chain(fm, d["text"], None)
    bad = ~torch.isfinite(l64).all(dim=1)
    W = fm.shape[2]
    for y, x in ((3, 4), (10, 11), (20, 5), (30, 30)):
        assert bad[y * W + x]
    assert 4 <= int(bad.sum()) <= 16                          # 0 * inf in the resize reaches a neighbour or two
    assert torch.isnan(l64[bad]).all() and (O.labels_of(l64)[bad] == 0).all()
