"""CPU checks of the language-guided selection: the numpy restatement (tests/edit_oracle.py) against the masks the
reference's own functions returned (tests/golden/reference_edit_vectors.npz), every quirk of the decision pinned on a
hand-made case, and the C-ABI entry point's argument validation (no device work)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import edit_oracle as O
from util import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_edit_vectors.npz")


def _cases():
    z = np.load(GOLDEN)
    return sorted({k.split("/")[0] for k in z.files})


@pytest.mark.parametrize("name", _cases())
def test_oracle_equals_the_reference_fixture_on_every_row(name):
    z = np.load(GOLDEN)
    ran = 0
    for variant in ("select", "delete"):
        if f"{name}/mask_{variant}" not in z.files:
            continue
        # the fixture was made on CPU, where torch rounds the threshold to fp16 before it compares
        r = O.select(z[f"{name}/features"], z[f"{name}/text"], float(z[f"{name}/threshold"]), list(z[f"{name}/positive_ids"]),
                     variant, scalar="fp16")
        want = z[f"{name}/mask_{variant}"]
        assert r["mask"].shape == want.shape and np.array_equal(r["mask"], want.astype(np.float32)), \
            (name, variant, int((r["mask"] != want).sum()))
        assert 0.02 < want.mean() < 0.98, "a fixture case that selects (almost) all or nothing shows little"
        # the device-style comparison may differ from it on borderline rows only
        d = O.select(z[f"{name}/features"], z[f"{name}/text"], float(z[f"{name}/threshold"]), list(z[f"{name}/positive_ids"]),
                     variant, scalar="fp32")
        assert np.all(d["margin"][d["mask"] != r["mask"]] <= 1.0)
        # the in-place side effect on query_features: fp32 norm and divide
        tn = z[f"{name}/text_normalized"]
        assert np.all(np.abs(r["text_normalized"] - tn) <= 2 * np.spacing(np.abs(tn)))
        ran += 1
    assert ran


def test_fixture_is_small_and_has_the_special_rows():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 768 * 1024
    f = z["k5_c16_thr0198/features"]
    assert not f[0].any() and np.isinf(f[1, 0]) and np.isnan(f[2, -1])
    assert not z["k5_c16_thr0198/mask_select"][:3].any()          # NaN rows: every >= is false
    assert {int(z[f"{c}/text"].shape[0]) for c in _cases()} >= {1, 2, 5}


def _row(values, C=8):
    """One feature row along `values` and len(values) orthonormal text rows: the scores are the normalised values."""
    f = np.zeros((1, C), np.float32)
    f[0, :len(values)] = values
    return f, np.eye(len(values), C, dtype=np.float32)


def test_quirk_delete_counts_the_other_positives_twice():
    f, t = _row([0.1, 0.3, 0.9])
    p = O.softmax_fp16(O.scores_fp16(f, t)[0])[0].astype(np.float64)
    assert abs(p[0] - 0.22) < 0.01 and abs(p[1] - 0.27) < 0.01 and abs(p[2] - 0.51) < 0.01
    q = np.float16(p[0] + p[1])                                   # ~0.49: below p_2, so the argmax is NOT a positive column
    q2 = np.float16(np.float64(q) + p[1])                         # ~0.76: p_1 counted twice
    sel, dele = O.select(f, t, 0.6, [0, 1], "select"), O.select(f, t, 0.6, [0, 1], "delete")
    assert sel["decided"][0] == np.float32(q) and sel["mask"][0] == 0.0
    assert dele["decided"][0] == np.float32(q2) and dele["mask"][0] == 1.0          # selected by the double count alone
    assert O.select(f, t, None, [0, 1], "delete")["mask"][0] == 0.0                 # m itself is false
    # with positives [1, 0] the FIRST id is 1: column 1 is replaced, and p_0 is the one counted twice
    assert O.select(f, t, 0.6, [1, 0], "delete")["decided"][0] == np.float32(np.float16(np.float64(q) + p[0]))


def test_quirk_only_the_first_positive_column_is_replaced():
    f, t = _row([0.5, 0.5, 0.6, 0.6])                   # p ~ (0.2385, 0.2385, 0.2615, 0.2615)
    # positives [0, 1]: q ~ 0.477 goes into column 0 and wins the argmax; positives [0] alone: q = p_0 loses to column 2
    assert O.select(f, t, None, [0, 1], "select")["mask"][0] == 1.0
    assert O.select(f, t, None, [0], "select")["mask"][0] == 0.0
    r = O.select(f, t, None, [1, 0], "select")          # column 1 replaced instead: same answer, decided quantity q
    assert r["mask"][0] == 1.0 and abs(float(r["decided"][0]) - 0.477) < 2e-3 and r["margin"][0] > 100
    # a tie across the boundary has margin 0, and argmax takes the first of the equal columns
    f2, t2 = _row([1.0, 1.0])
    r2 = O.select(f2, t2, None, [1], "select")
    assert r2["margin"][0] == 0.0 and r2["mask"][0] == 0.0
    assert O.select(f2, t2, None, [0], "select")["mask"][0] == 1.0


def test_quirk_nan_rows():
    t = np.eye(3, 8, dtype=np.float32)
    f = np.zeros((3, 8), np.float32)
    f[1, 2], f[2, 0] = np.inf, np.nan
    for variant in ("select", "delete"):
        r = O.select(f, t, 0.0, [1], variant)            # every >= is false, even against 0; argmax = column 0, not positive
        assert not r["mask"].any() and np.isnan(r["decided"]).all() and np.isinf(r["margin"]).all()
        r = O.select(f, t, None, [0, 2], variant)        # argmax = column 0 (the first NaN), which is positive
        assert r["mask"].all()
    assert not O.select(f, t[:1], -1.0, [0], "select")["mask"].any()        # K = 1: NaN >= anything is false
    assert np.isnan(O.normalize_fp32(f)).any(axis=1).all()


def test_return_dtypes_per_branch():
    f, t = O.make_inputs(50, 8, 3, 1)
    assert O.select(f, t, None, [0], "delete")["is_bool"]                  # the reference returns the bool `m` there
    for variant, thr, k in (("select", None, 3), ("select", 0.3, 3), ("delete", 0.3, 3), ("select", 0.3, 1), ("delete", 0.3, 1)):
        r = O.select(f, t[:k], thr, [0], variant)
        assert not r["is_bool"] and r["mask"].dtype == np.float32 and set(np.unique(r["mask"])) <= {0.0, 1.0}
    with pytest.raises(AssertionError):
        O.select(f, t[:1], None, [0], "select")


def test_gap_inputs_are_off_the_boundary():
    for variant, thr, pos in (("select", 0.3, [0]), ("delete", 0.6, [2, 0]), ("select", None, [1, 3])):
        f, t = O.make_gap_inputs(300, 16, 5, 7, thr, pos, variant)
        r = O.select(f, t, thr, pos, variant)
        assert r["margin"].min() >= 8.0 and 0.05 < r["mask"].mean() < 0.95


def _lib():
    so = os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(so)
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_edit_select.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                                                                   ctypes.c_int, ctypes.c_float] + [ctypes.c_void_p] * 5
    return lib


def test_version_is_3_7():
    lib = _lib()
    lib.f3dgs_version.restype = ctypes.c_int
    assert lib.f3dgs_version() >= 30700


def test_c_abi_edit_select_rejects_bad_arguments():
    lib = _lib()
    assert hasattr(lib, "f3dgs_edit_select")
    dummy = (ctypes.c_float * 64)()
    p = ctypes.addressof(dummy)

    def call(P=4, C=8, K=2, f=p, nout=None, t=p, pm=1, first=0, variant=0, has_thr=1, thr=0.5, m=p, s=None, oi=None, oo=None):
        return lib.f3dgs_edit_select(P, C, K, f, nout, t, pm, first, variant, has_thr, thr, m, s, oi, oo, None)

    err = lambda: lib.f3dgs_last_error()
    for kw in (dict(P=-1), dict(C=0), dict(K=0)):
        assert call(**kw) < 0 and b"bad sizes" in err()
    for kw in (dict(f=None), dict(t=None), dict(m=None)):
        assert call(**kw) < 0 and b"null" in err()
    assert call(pm=0) < 0 and b"empty positive mask" in err()
    assert call(pm=0b100, first=2) < 0 and b"at or above K" in err()
    assert call(pm=0b10, first=0) < 0 and b"first_positive" in err()
    assert call(pm=0b01, first=5) < 0 and b"first_positive" in err()
    assert call(K=65, C=4) < 0 and b"limit" in err()
    assert call(K=64, C=1024) < 0 and b"limit" in err()              # K * C = 65536 > 32768
    assert call(K=1, has_thr=0) < 0 and b"threshold" in err()
    assert call(variant=0x40) < 0 and b"variant" in err()
    assert call(oi=p) < 0 and b"opacity" in err()
    # P = 0 is a success without any pointer
    assert call(P=0, f=None, t=None, m=None) == 0
    assert call(P=0, K=64, C=512, pm=(1 << 64) - 1, first=63, f=None, t=None, m=None) == 0     # the documented maximum


def test_public_surface_refuses_bad_arguments_before_any_device_work():
    import edit
    f, t = torch.rand(10, 8), torch.rand(3, 8)
    with pytest.raises(ValueError, match="duplicate"):
        edit.selection_mask(f, t, 0.3, positive_ids=(1, 1))
    with pytest.raises(ValueError, match="out of range"):
        edit.selection_mask(f, t, 0.3, positive_ids=(3,))
    with pytest.raises(ValueError, match="score_threshold"):
        edit.selection_mask(f, t[:1])
    with pytest.raises(ValueError, match="limit"):
        edit.selection_mask(torch.rand(4, 2), torch.rand(65, 2), 0.3)
    with pytest.raises(ValueError, match="limit"):
        edit.calculate_selection_score(torch.rand(4, 1024), torch.rand(33, 1024), 0.3)
    with pytest.raises(ValueError, match="variant"):
        edit.selection_mask(f, t, 0.3, variant="extract")
    with pytest.raises(ValueError, match="expected"):
        edit.selection_mask(torch.rand(10, 2, 8), t, 0.3)
    before = t.clone()
    with pytest.raises(RuntimeError, match="HIP device"):          # no CPU path, and nothing was normalised on the way
        edit.selection_mask(f, t, 0.3)
    assert torch.equal(t, before)
    for n in ("selection_mask", "calculate_selection_score", "calculate_selection_score_delete", "apply_edit", "render_edit", "install"):
        assert callable(getattr(edit, n))


def test_apply_edit_on_cpu_tensors():
    """apply_edit is plain torch: the reference's three operations for a given mask."""
    import edit
    op, shs = torch.ones(4, 1), torch.arange(4 * 2 * 3, dtype=torch.float32).reshape(4, 2, 3)
    mask = torch.tensor([1.0, 0.0, 1.0, 0.0])
    o, _ = edit.apply_edit(op.clone(), shs.clone(), mask, {"deletion": True})
    assert o[:, 0].tolist() == [0, 1, 0, 1]
    o, _ = edit.apply_edit(op.clone(), shs.clone(), mask.bool(), {"extraction": True})
    assert o[:, 0].tolist() == [1, 0, 1, 0]
    _, s = edit.apply_edit(op.clone(), shs.clone(), mask, {"color_func": lambda c: c * 0 + 7})
    assert torch.equal(s[0, 0], torch.full((3,), 7.0)) and torch.equal(s[1], shs[1]) and torch.equal(s[:, 1], shs[:, 1])
    with pytest.raises(AttributeError):
        edit.install(torch)
