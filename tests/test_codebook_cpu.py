"""The judge of the feature codebooks (tests/codebook_oracle.py) tested by itself, the seeds of the GPU cases checked against the
judge's own conditions in float32 numpy, and what the C ABI and codebook.py refuse before any device work.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import codebook_oracle as co
from util import ROOT


# ---- the judge ------------------------------------------------------------------------------------------------------------

def test_judge_assign_ties_and_bad_rows():
    cent = np.array([[0, 0], [4, 0], [4, 0], [0, 4]], np.float32)          # 1 and 2 are duplicates
    x = np.array([[4, 0], [2, 0], [2, 2], [0, 3], [np.nan, 0], [np.inf, 1]], np.float32)
    assert co.assign(x, cent).tolist() == [1, 0, 0, 3, -1, -1]            # the duplicate's lower index, equidistant rows: the lowest k
    bad = cent.copy()
    bad[0, 1] = np.nan
    assert co.assign(x, bad).tolist() == [1, 1, 1, 3, -1, -1]             # a non-finite centroid never wins
    assert co.assign(x, np.full((2, 2), np.inf, np.float32)).tolist() == [-1] * 6
    # cosine: the direction decides, a zero centroid scores 0 and beats every negative cosine
    cent = np.array([[0, 0], [10, 0], [0, 0.1]], np.float32)
    x = np.array([[1, 0.5], [0.5, 1], [-1, -1], [0, 0]], np.float32)
    assert co.assign(x, cent, "cosine").tolist() == [1, 2, 0, 0]
    right, differs = co.adjudicate(np.array([1, 2, 0, 0]), x, cent, "cosine")
    assert right.all() and not differs.any()
    right, differs = co.adjudicate(np.array([2, 2, 1, 5]), x, cent, "cosine")
    assert right.tolist() == [False, True, False, False] and differs.tolist() == [True, False, True, True]


def test_judge_allowance_decides_near_ties_only():
    x = np.array([[1.0, 0.0]], np.float32)
    near = np.array([[0.5, 0.0], [1.5, np.float32(1e-9)]], np.float32)     # equidistant up to 1e-18
    assert co.adjudicate(np.array([1]), x, near)[0].all() and not co.clear_of_rounding(x, near).all()
    far = np.array([[0.5, 0.0], [1.6, 0.0]], np.float32)
    assert not co.adjudicate(np.array([1]), x, far)[0].any() and co.clear_of_rounding(x, far).all()


def test_judge_dist2_update_and_reseed():
    x = np.array([[0, 0], [2, 0], [0, 2], [9, 9], [np.nan, 1]], np.float32)
    cent = np.array([[1, 1], [8, 8], [5, 5]], np.float32)
    codes = np.array([0, 0, 0, 1, -1], np.int32)
    d, bound = co.dist2(x, cent, codes)
    assert d.tolist() == [2, 2, 2, 2, 0] and (bound[:4] == 2.0 ** -23 + 16 * 2.0 ** -53).all() and bound[4] < 1e-44
    d, _ = co.dist2(np.array([[1, 0], [0, 0]], np.float32), np.array([[0, 2]], np.float32), np.array([0, 0]), "cosine")
    assert d.tolist() == [1, 1]
    w = np.array([1, 1, 0, np.inf, 1], np.float32)
    new, count, _, _ = co.update(x, codes, cent, w=w)
    assert count.tolist() == [2, 0, 0] and new.tolist() == [[1, 0], [8, 8], [5, 5]]                # empty clusters keep their rows
    new = co.update(x, codes, cent, w=w, reseed=True, iteration=3)[0]
    rows = [(k * co.MUL + 3 * co.ADD) % 5 for k in (1, 2)]
    for k, row in zip((1, 2), rows):
        assert np.array_equal(new[k], x[row] if np.isfinite(x[row]).all() else cent[k])
    assert co.inertia(np.array([2, 2, 2, 2, 0], np.float32), codes, 3, w) == 4.0
    new, _, _, bound = co.update(x[:4], codes[:4], cent, "cosine")
    assert np.allclose(new[0], np.array([1, 1]) / np.sqrt(2)) and (bound[0] < 1e-7).all()


def test_judge_lloyd_converges_on_blobs_and_refuses_what_it_cannot_decide():
    x, centres, which = co.integer_blobs(300, 5, 8, seed=1)
    res = co.lloyd(x, 5, 4, init=centres)
    assert np.array_equal(res["codes"], which) and res["count"].sum() == 300 and res["moved"].tolist() == [300, 0, 0, 0]
    res = co.lloyd(x, 5, 3, fit_stride=3)
    assert res["codes"].shape == (300,) and res["moved"][0] == 100
    with pytest.raises(AssertionError, match="cannot decide"):
        co.lloyd(np.array([[1.0], [2.0]], np.float32), 2, 1, init=np.array([[1.5 - 1e-8], [1.5 + 1e-8]], np.float32))


@pytest.mark.parametrize("metric", co.METRICS)
def test_the_seeds_of_the_gpu_cases_stay_inside_the_conditions(metric):
    """the same scores in float32 numpy: every code adjudicated right, at most 1 % of the rows off k*"""
    for P, K, C in co.SHAPES:
        if P == 0:
            continue
        x, cent = co.random_case(P, K, C)
        codes = np.argmin(co.scores32(x, cent, metric), axis=1)
        right, differs = co.adjudicate(codes, x, cent, metric)
        assert right.all(), (P, K, C)
        assert differs.sum() <= co.MAX_DIFFERENT * P, (P, K, C, int(differs.sum()))


def test_shapes_cover_every_listed_size():
    Ps, Ks, Cs = (set(s[i] for s in co.SHAPES) for i in range(3))
    assert {0, 1, 31, 32, 33, 127, 128, 129, 257, 1000} <= Ps and {1, 2, 31, 32, 33, 127, 128, 129, 300} <= Ks
    assert {1, 3, 16, 31, 32, 33, 64, 128, 129, 512} <= Cs and (64, 65536, 4) in co.SHAPES and (33, 2, 4096) in co.SHAPES


# ---- the C ABI: what is refused before any device work ---------------------------------------------------------------------

def _lib():
    so = os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import torch  # noqa: F401  (its bundled HIP runtime must be the one the library binds to)
    lib = ctypes.CDLL(so)
    vp, ci, sz, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int64
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_version.restype = ci
    for name in ("f3dgs_codebook_workspace_bytes", "f3dgs_codebook_update_scratch_bytes"):
        getattr(lib, name).restype = sz
        getattr(lib, name).argtypes = [ci, ci]
    lib.f3dgs_codebook_assign.argtypes = [ci, ci, ci, vp, i64, vp, ci, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.f3dgs_codebook_update.argtypes = [ci, ci, ci, vp, i64, vp, vp, ci, ci, vp, vp, vp, sz, vp]
    return lib


def test_c_abi_refuses_bad_arguments_without_gpu():
    lib = _lib()
    assert lib.f3dgs_version() >= 32200
    A, B, D, S = 0x10000, 0x20000, 0x30000, 0x50000                      # aligned, never dereferenced addresses
    INV, UNS, BIG = -1, -4, 1 << 40
    err = lib.f3dgs_last_error

    def assign(P=10, K=4, C=8, x=A, stride=8, cent=B, flags=0, prev=None, w=None, codes=D, dist2=None, inertia=None, moved=None, ws=S,
               nbytes=BIG):
        return lib.f3dgs_codebook_assign(P, K, C, x, stride, cent, flags, prev, w, codes, dist2, inertia, moved, ws, nbytes, None)

    need = lib.f3dgs_codebook_workspace_bytes(4096, 32)
    assert 4096 * 32 * 4 <= need <= 4096 * 33 * 4 + 64
    assert lib.f3dgs_codebook_workspace_bytes(65536, 4096) >= 65536 * 4096 * 4                   # (no 32-bit overflow)
    assert assign(P=-1) == INV and b"P < 0" in err()
    for K in (0, 65537):
        assert assign(K=K) == INV and b"1 .. 65536" in err()
    for C in (0, 4097):
        assert assign(C=C) == INV and b"1 .. 4096" in err()
    assert assign(flags=2) == INV and b"flags" in err()
    assert assign(stride=7) == INV and b"feature_stride" in err()
    for kw in (dict(x=None), dict(cent=None), dict(codes=None)):
        assert assign(**kw) == INV and b"null" in err(), kw
    assert assign(moved=D) == INV and b"prev_codes" in err()
    assert assign(P=(1 << 31) - 100) == UNS
    assert assign(ws=None) == INV and b"workspace" in err()
    assert assign(nbytes=lib.f3dgs_codebook_workspace_bytes(4, 8) - 1) == INV and b"workspace" in err()
    assert assign(ws=S + 8) == INV and b"16-byte" in err()
    assert assign(inertia=D + 4) == INV and b"8-byte" in err()

    def update(P=10, K=4, C=8, x=A, stride=8, codes=D, w=None, flags=0, it=0, cent=B, count=None, scratch=S, nbytes=BIG):
        return lib.f3dgs_codebook_update(P, K, C, x, stride, codes, w, flags, it, cent, count, scratch, nbytes, None)

    assert lib.f3dgs_codebook_update_scratch_bytes(300, 32) >= 300 * 33 * 8
    assert update(P=-1) == INV and b"P < 0" in err()
    assert update(K=0) == INV and b"1 .. 65536" in err()
    assert update(C=4097) == INV and b"1 .. 4096" in err()
    assert update(flags=4) == INV and b"flags" in err()
    assert update(it=-1) == INV and b"iteration" in err()
    assert update(stride=3) == INV and b"feature_stride" in err()
    for kw in (dict(x=None), dict(cent=None), dict(codes=None)):
        assert update(**kw) == INV and b"null" in err(), kw
    assert update(scratch=None) == INV and b"scratch" in err()
    assert update(nbytes=lib.f3dgs_codebook_update_scratch_bytes(4, 8) - 1) == INV and b"scratch" in err()
    assert update(scratch=S + 4) == INV and b"8-byte" in err()


def test_module_has_no_cpu_path():
    import torch
    _lib()
    import codebook
    x = torch.zeros(10, 4)
    for call in (lambda: codebook.assign(x, x[:2]), lambda: codebook.kmeans(x, 2), lambda: codebook.quantize(x, 2),
                 lambda: codebook.update(x, torch.zeros(10, dtype=torch.int32), x[:2])):
        with pytest.raises(ValueError, match=r"HIP device.*\(10, 4\)"):
            call()
    assert "split_labels" in codebook.__doc__ and "rewrite_semantic_feature" in codebook.__doc__
