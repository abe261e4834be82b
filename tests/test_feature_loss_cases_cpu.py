"""CPU: the case lists of tests/feature_loss_cases.py.  Every case's margin ground truth keeps every float64 residual at least
0.2 from zero (a condition on the reference alone, under which no L1 sign can differ in fp32), and the lists reach every tile,
list and store-path edge of csrc/feature_loss.hip - recomputed here from the launch arithmetic, with the per-axis list lengths
taken from the NumPy restatement of csrc/resize_taps.h (tests/test_resize_taps.py)."""
import pytest

import feature_loss_cases as flc


@pytest.mark.parametrize("case", flc.LOSS_CASES, ids=flc.case_id)
def test_every_case_has_its_margin(case):
    c = flc.build_case(case)            # asserts min |decoded64 - gt| >= 0.2 itself
    C, H, W, Cout, Hg, Wg, dec = case
    assert c["margin"] >= 0.2
    assert c["gt"].dtype.is_floating_point and c["gt"].shape == (Cout, Hg, Wg) and c["fm"].shape == (C, H, W)
    r = c["want"]["decoded"] - c["gt"].double()
    assert float(r.abs().max()) <= 1.0 + 1e-6
    # both signs occur (a gradient of one sign everywhere would not tell a sign error from a scale error), unless one element
    assert r.numel() < 8 or (bool((r > 0).any()) and bool((r < 0).any()))
    assert float(c["want"]["d_feature_map"].abs().max()) > 0


def test_case_ids_are_unique_and_the_decode_list_is_a_subset():
    assert len(set(flc.LOSS_CASES)) == len(flc.LOSS_CASES)
    assert set(flc.DECODE_CASES) <= set(flc.LOSS_CASES)
    assert len({flc.case_id(c) for c in flc.LOSS_CASES}) == len(flc.LOSS_CASES)


def test_k3_cases_have_empty_ranges():
    """fl_dweight_kernel's early return in front of its barrier: both cases launch ranges without a tile."""
    (a, b) = flc.K3_CASES
    assert flc.k3_ranges(a[4] * a[5], a[3]) == (512, 2, 512 - 257)          # 513 tiles, cblocks = 1
    assert flc.k3_ranges(b[4] * b[5], b[3]) == (102, 2, 102 - 52)           # 103 tiles, cblocks = 5
    # ... and nothing else in the suite's older list does (tests/test_feature_loss.py: CASES)
    for C, H, W, Cout, Hg, Wg in [(32, 54, 96, 128, 18, 32), (64, 40, 72, 256, 23, 41), (128, 45, 80, 512, 30, 40),
                                  (32, 16, 16, 128, 40, 56), (32, 33, 47, 96, 1, 1)]:
        assert flc.k3_ranges(Hg * Wg, Cout)[2] == 0


def _required():
    need = set()
    # pixel count against the three tilings: K1 / K3 64-pixel tiles, K2 / decode 128-pixel workgroups, 32-pixel half-waves
    need |= {f"N%64={r}" for r in (0, 1, 31, 32, 33, 63)}
    need |= {f"N%128={r}" for r in (0, 1, 31, 32, 33, 63, 64, 65, 127)}
    need |= {f"N%32={r}" for r in (0, 1, 31)}
    need |= {"ntiles64=1", "ntiles64=2", "ntiles64=3"}
    need |= {"k3-upper-half-all-pad", "k3-upper-half-part-pad", "k3-upper-half-no-pad"}
    # decoder output width: the ragged 32-row W tile of K2 / decode, the ragged 128-row block of K3 - for every C
    need |= {f"C={C}:Cout%32={r}" for C in (32, 64, 128) for r in (0, 1, 4, 31)}
    need |= {f"C={C}:Cout%128={r}" for C in (32, 64, 128) for r in (1, 31, 32, 33, 100)}
    need |= {f"C={C}:N={N}" for C in (32, 64, 128) for N in flc.N_EDGES}
    need |= {"k3-ragged-later-cblock", "k3-empty-ranges:cblocks=1", "k3-empty-ranges:cblocks=5"}
    # no decoder
    need |= {f"plainC%32={r}" for r in (1, 5, 8, 31)} | {"plain-two-channel-blocks"}
    need |= {f"plainC={C}:N={N}" for C in (1, 5, 31, 33, 40) for N in flc.N_EDGES}
    need |= {"form-1xN", "form-Nx1", "form-rect", "form-one"}
    # resize geometry and K4
    need |= {"source-H=1", "source-W=1", "scale0-rows-only", "scale0-cols-only", "identity",
             "k4-ny-overflow-nx-list", "k4-ny-list-nx-overflow", "k4-both-overflow", "k4-list-full",
             "k4-store-vec4", "k4-store-scalar", "k4-zero-row-vec4", "k4-zero-row-scalar", "k4-vec4-and-scalar-in-one-row",
             "k4-narrow-W%4==0", "k4-ragged-last-block", "k4-empty-column-list"}
    return need


@pytest.mark.parametrize("name", ["LOSS_CASES", "DECODE_CASES"])
def test_the_lists_reach_every_edge(name):
    cases = getattr(flc, name)
    got = set()
    for c in cases:
        got |= flc.describe(c)
    need = _required()
    if name == "DECODE_CASES":          # forward only: no K3, no K4
        need = {n for n in need if not n.startswith(("k3-", "k4-"))}
    assert need - got == set(), sorted(need - got)


def test_each_geometry_reaches_what_it_is_listed_for():
    want = {
        ((1, 50), (7, 17)): {"source-H=1"},
        ((30, 1), (12, 5)): {"source-W=1"},
        ((30, 50), (1, 17)): {"scale0-rows-only"},
        ((30, 50), (12, 1)): {"scale0-cols-only"},
        ((40, 16), (13, 56)): {"k4-ny-list-nx-overflow"},
        ((16, 40), (56, 13)): {"k4-ny-overflow-nx-list"},
        ((4, 4), (64, 64)): {"k4-both-overflow"},
        ((16, 16), (40, 40)): set(),
        ((8, 9), (23, 26)): {"k4-list-full"},
        ((24, 68), (8, 23)): {"k4-vec4-and-scalar-in-one-row", "k4-zero-row-vec4", "k4-zero-row-scalar"},
        ((24, 128), (8, 43)): {"k4-zero-row-vec4", "k4-store-vec4"},
        ((24, 60), (8, 20)): {"k4-narrow-W%4==0"},
        ((24, 67), (24, 67)): {"identity"},
    }
    assert set(want) == set(flc.GEOMETRIES)
    for ((H, W), (Hg, Wg)), need in want.items():
        for case in ((5, H, W, 5, Hg, Wg, False), (32, H, W, 33, Hg, Wg, True)):
            assert case in flc.GEOMETRY_CASES
            assert need <= flc.describe(case), (case, sorted(need - flc.describe(case)))
    # (24, 128) -> (8, 43) has no scalar block at all; (16, 16) -> (40, 40) and the full lists of (8, 9) -> (23, 26) overflow nowhere
    assert "k4-store-scalar" not in flc.describe((5, 24, 128, 5, 8, 43, False))
    for case in ((5, 16, 16, 5, 40, 40, False), (5, 8, 9, 5, 23, 26, False)):
        assert not any("overflow" in k for k in flc.describe(case))
    assert max(flc.axis_lists(16, 40)) == 5 and max(flc.axis_lists(8, 23)) == 6 and max(flc.axis_lists(9, 26)) == 6


def test_a_one_row_source_feeds_every_output_row():
    """in = 1, out > 1: scale is 0 and EVERY output reads source index 0 with weight 1 (F.interpolate, align_corners=True) - the
    list of source index 0 is all outputs, not just output 0 (which is right only for out == 1)."""
    from test_resize_taps import build, scale_of
    for n_out in (1, 2, 5, 7, 12):
        lst = build(0, scale_of(1, n_out), 1, n_out)
        assert [o for o, _ in lst] == list(range(n_out)) and all(float(w) == 1.0 for _, w in lst)
    # out == 1 from a longer source: only source index 0 is read
    assert build(0, scale_of(30, 1), 30, 1) == [(0, 1.0)] and build(3, scale_of(30, 1), 30, 1) == []
