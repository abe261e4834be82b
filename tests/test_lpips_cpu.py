"""CPU checks of the LPIPS test apparatus and of lpips_vgg.py's surface (no GPU): the independent oracle (tests/lpips_oracle.py)
in float32 and float64 against the reference's recorded float64 results (tests/golden/reference_lpips.npz) under the bars the GPU
tests use - every tap element within 4 gap_tap[l] of float64, every layer term and total within 4 gap_rel relative -, the names,
and the errors the Python layer raises before any device work."""
import os

import numpy as np
import pytest
import torch

import lpips_cases as cases
import lpips_oracle as oracle
from util import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_lpips.npz")
NAMES = [c.name for c in cases.CASES]
_Z, _W, _O = {}, {}, {}


def golden():
    if not _Z:
        _Z.update(np.load(GOLDEN))
    return _Z


def lv():
    import lpips_vgg
    return lpips_vgg


def weights_of(name):
    key = (int(golden()[f"{name}/params"][3]), cases.BY_NAME[name].dead)
    if key not in _W:
        _W[key] = cases.make_weights(*key)
    return _W[key]


def oracle_of(name, dtype):
    """(taps of cat(x, y), terms, totals) of the oracle as numpy float64, computed once per (case, dtype)"""
    if (name, dtype) not in _O:
        c = cases.BY_NAME[name]
        x, y = cases.make_pairs(c, int(golden()[f"{name}/params"][3]))
        w = weights_of(name)
        terms, totals = oracle.layer_terms(w, x, y, dtype)
        taps = [t.double().reshape(-1).numpy() for t in oracle.taps(w, np.concatenate([x, y]), dtype)]
        _O[(name, dtype)] = (taps, terms.double().numpy(), totals.double().numpy())
    return _O[(name, dtype)]


def check_against_golden(name, taps, terms, totals):
    """the bars of the issue; taps: five flattened tensors of cat(x, y)"""
    z, c = golden(), cases.BY_NAME[name]
    gap_tap, gap_rel = z[f"{name}/gap_tap"], float(z[f"{name}/gap_rel"])
    for l, t in enumerate(taps):
        shape = cases.tap_shapes(c)[l]
        assert t.size == int(np.prod(shape)), (l, t.size, shape)
        ref = z[f"{name}/tap64_{l}"]
        err = np.abs(t[cases.sample_index(t.size, c.samples, l)] - ref).max()
        print(f"{name} tap {l}: max error {err:.3g}, bar {4 * gap_tap[l]:.3g}")
        assert err <= 4 * gap_tap[l], (name, l, err, gap_tap[l])
    t64, tot64 = z[f"{name}/terms64"], z[f"{name}/total64"]
    print(f"{name}: term error {np.abs(terms - t64).max():.3g} of {t64.max():.3g}, relative bar {4 * gap_rel:.3g}")
    assert (np.abs(terms - t64) <= 4 * gap_rel * t64).all(), (name, terms, t64, gap_rel)
    assert (np.abs(totals - tot64) <= 4 * gap_rel * tot64).all(), (name, totals, tot64, gap_rel)


def test_golden_file_matches_the_recipe():
    z = golden()
    for c in cases.CASES:
        H, W, N, seed, dead, samples = z[f"{c.name}/params"].tolist()
        assert (H, W, N, bool(dead), samples) == (c.H, c.W, len(c.kinds), c.dead, c.samples) and seed == cases.SEED
        assert z[f"{c.name}/gap_rel"] > 0 and (z[f"{c.name}/gap_tap"][:4] > 0).all()
        for k, kind in enumerate(c.kinds):
            if kind == "same":
                assert (z[f"{c.name}/terms64"][k] == 0).all() and (z[f"{c.name}/terms32"][k] == 0).all()
    assert (z["dead/terms64"][:, 4] == 0).all() and (z["dead/terms32"][:, 4] == 0).all() and z["dead/gap_tap"][4] == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_the_reference(name, dtype):
    check_against_golden(name, *oracle_of(name, dtype))


def test_dropin_sums_over_the_batch():
    z = golden()
    for name in ("batch3", "odd"):
        c = cases.BY_NAME[name]
        x, y = cases.make_pairs(c, cases.SEED)
        v = oracle.lpips(weights_of(name), x, y, torch.float64)
        assert tuple(v.shape) == (1, 1, 1, 1) and z[f"{name}/dropin64"].shape == (1, 1, 1, 1)
        assert abs(v.item() - z[f"{name}/dropin64"].item()) <= 4 * float(z[f"{name}/gap_rel"]) * z[f"{name}/dropin64"].item()
        assert abs(z[f"{name}/dropin64"].item() - z[f"{name}/total64"].sum()) <= 1e-12


def test_parameter_table_against_the_recorded_names():
    z = golden()
    recorded = {str(n): tuple(int(d) for d in str(s).split(",")) for n, s in zip(z["names"], z["shapes"]) if str(s)}
    named = lv().canonical_names({k: np.empty(s, np.float32) for k, s in recorded.items()})      # the reference's LPIPS.state_dict()
    table = lv().parameter_table()
    assert len(table) == 31 and list(named) == [n for n, _ in table]
    assert all(tuple(named[n].shape) == s for n, s in table)
    assert sorted(weights_of("odd")) == sorted(n for n, _ in table) and all(weights_of("odd")[n].shape == s for n, s in table)


def test_canonical_names_spellings():
    w = weights_of("odd")
    conv = {k: v for k, v in w.items() if k.startswith("features.")}
    heads = [w[f"lin.{i}.weight"] for i in range(5)]
    spell_conv = (lambda k: k, lambda k: k[len("features."):], lambda k: "net.layers." + k[len("features."):])
    spell_head = (lambda i: f"lin{i}.model.1.weight", lambda i: f"{i}.1.weight", lambda i: f"lin.{i}.1.weight", lambda i: f"lin.{i}.weight")
    for sc in spell_conv:
        for sh in spell_head:
            sd = {sc(k): v for k, v in conv.items()}
            sd.update({sh(i): v for i, v in enumerate(heads)})
            sd["classifier.0.weight"] = np.zeros((4, 4), np.float32)          # ignored
            named = lv().canonical_names(sd)
            assert list(named) == [n for n, _ in lv().parameter_table()] and all(named[k] is w[k] for k in named)


def test_canonical_names_errors():
    w = dict(weights_of("odd"))
    missing = {k: v for k, v in w.items() if k != "features.17.bias"}
    with pytest.raises(KeyError, match="features.17.bias"):
        lv().canonical_names(missing)
    wrong = dict(w)
    wrong["features.5.weight"] = np.zeros((128, 64, 3, 2), np.float32)
    with pytest.raises(ValueError, match="features.5.weight"):
        lv().canonical_names(wrong)
    alex = dict(w)
    for i, ch in enumerate((64, 192, 384, 256, 256)):
        alex[f"lin.{i}.weight"] = np.zeros((1, ch, 1, 1), np.float32)
    with pytest.raises(NotImplementedError, match="lin.0.weight"):
        lv().canonical_names(alex)
    alex_conv = dict(w)
    alex_conv["features.0.weight"] = np.zeros((64, 3, 11, 11), np.float32)
    with pytest.raises(NotImplementedError, match="features.0.weight"):
        lv().canonical_names(alex_conv)
    squeeze = {f"lin{i}.model.1.weight": np.zeros((1, ch, 1, 1), np.float32) for i, ch in enumerate((64, 128, 256, 384, 384, 512, 512))}
    with pytest.raises(NotImplementedError, match="lin0.model.1.weight"):
        lv().canonical_names({**w, **squeeze})


REFUSALS = [
    ("below16_h", lambda t: (t(1, 3, 15, 40), t(1, 3, 15, 40)), {}, ValueError, "16"),
    ("below16_w", lambda t: (t(3, 40, 12), t(3, 40, 12)), {}, ValueError, "16"),
    ("channels", lambda t: (t(1, 4, 32, 32), t(1, 4, 32, 32)), {}, ValueError, "3 channels"),
    ("shapes", lambda t: (t(2, 3, 32, 32), t(1, 3, 32, 32)), {}, ValueError, "differ"),
    ("dims", lambda t: (t(32, 32), t(32, 32)), {}, ValueError, "expected"),
    ("dtype", lambda t: (t(1, 3, 32, 32).double(), t(1, 3, 32, 32).double()), {}, ValueError, "float32 or uint8"),
    ("quantize_u8", lambda t: (t(1, 3, 32, 32).to(torch.uint8), t(1, 3, 32, 32)), {"quantize": True}, ValueError, "quantize"),
    ("quantize_pair", lambda t: (t(1, 3, 32, 32), t(1, 3, 32, 32)), {"quantize": (True, False, True)}, ValueError, "quantize"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_without_a_device(case):
    _, make, kwargs, exc, match = case
    x, y = make(lambda *s: torch.zeros(s))
    with pytest.raises(exc, match=match):
        lv().lpips_views(x, y, None, **kwargs)


def test_other_refusals_without_a_device():
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="alex"):
        lv().lpips(x, x, net_type="alex")
    with pytest.raises(NotImplementedError, match="squeeze"):
        lv().lpips(x, x, net_type="squeeze")
    with pytest.raises(ValueError, match="no CPU path"):                       # CPU tensors
        lv().lpips_views(x, x, None)
    with pytest.raises(ValueError, match="no CPU path"):
        lv().lpips(x, x, net_type="vgg")
    with pytest.raises(ValueError, match="LpipsWeights"):
        lv().lpips_views(x, x, weights="vgg.pth")
    with pytest.raises(ValueError, match="LpipsWeights"):
        lv().vgg_taps(None, x)
    with pytest.raises(ValueError, match="renders"):
        lv().evaluate_views([x[0]], [], None)
    with pytest.raises(ValueError, match="no CPU path"):
        lv().evaluate_views([x[0]], [x[0]], None)
    with pytest.raises(AttributeError, match="lpips"):
        lv().install(os, None)
