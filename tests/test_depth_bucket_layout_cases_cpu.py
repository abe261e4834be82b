"""CPU: the designed keys of tests/depth_bucket_layout_cases.py, proven by the scalar oracle alone, as
tests/test_depth_order_cases_cpu.py proves its own: the alive set, the float bits as depths, the shift, the group's single bucket
above the capacity, its ODD first pair index, the pass count, and the oracle's lists in `expected_order`.  Plus the arithmetic of
the sizes tests/test_gpu_depth_bucket_layout.py runs at: rows of the histogram matrix and the column scan's sweeps."""
import numpy as np
import pytest

import depth_bucket_layout_cases as lay_cases
import depth_order_cases as doc
from test_depth_order_cases_cpu import _assert_lists_follow_the_order


def _oracle(name):
    from util import run_oracle
    o, out, _ = run_oracle(lay_cases.designed_scene(name), backward=False)
    return dict(n=out["num_rendered"], radii=out["radii"].copy(), depths=o.read("depths").copy(),
                tiles_touched=o.read("tiles_touched").copy(), point_list=o.read("point_list").copy(),
                ranges=o.read("ranges").copy())


def test_the_sizes_of_the_gpu_cases():
    rows = lay_cases.matrix_rows
    assert rows(16385) == 9 and 16385 - 8 * lay_cases.SORT_CHUNK == 1 and doc.depth_bucket_count(16385) == 32
    assert [rows(P) for P in (18431, 18432, 18433)] == [9, 9, 10] and 18432 == 9 * lay_cases.SORT_CHUNK
    sweep = lay_cases.COLSCAN_SWEEP_ROWS
    P = sweep * lay_cases.SORT_CHUNK + 1         # the smallest P with one row more than the first sweep takes
    assert rows(P) == sweep + 1 and rows(P - 1) == sweep and P == 1048577
    assert doc.depth_bucket_bits(P) == 10 and doc.depth_bucket_count(P) == 1024          # (the 10-bit pass: 1,024 bins)
    assert rows(1000000) == 489 <= sweep < rows(2000000) == 977


@pytest.mark.parametrize("name", lay_cases.CASES)
def test_a_layout_case_is_what_its_name_claims(name):
    d, want = lay_cases.design(name), _oracle(name)
    P, keys, group = d["P"], d["keys"], d["group"]
    near, far = d["outliers"]
    alive = want["radii"] > 0
    assert np.array_equal(alive, ~d["culled"]) and int(alive.sum()) == d["n"] + 2 + d["leads"].size
    assert np.array_equal(want["depths"].view(np.uint32)[alive], keys[alive])
    oracle_keys = np.where(alive, want["depths"].view(np.uint32), doc.CULLED_KEY).astype(np.uint32)
    lay = doc.bucket_layout(oracle_keys, P)
    assert lay["count"] == 32 and lay["kmin"] == d["kmin"] == keys[near] and lay["kmax"] == d["kmax"] == keys[far]
    assert lay["shift"] == d["shift"] == 23
    bucket = np.full(P, -1, np.int64)
    bucket[alive] = lay["bucket"]
    j = d["bucket"]
    assert np.all(bucket[group] == j) and bucket[near] == 0 and np.all((bucket[d["leads"]] > 0) & (bucket[d["leads"]] < j))
    assert group.size == d["n"] == int(lay["sizes"][j]) == lay["largest"] == doc.CAPACITY + 1 and lay["oversized"] == 1
    # the bucket's first pair index: the alive keys of the buckets in front - odd, and so is n: the scratch's id half starts on an odd word
    offset = int(lay["sizes"][:j].sum())
    assert offset == d["offset"] == 3 and offset % 2 == 1 and d["n"] % 2 == 1
    real = doc.sort_passes(oracle_keys[group], lay["kmin"], lay["shift"])
    assert real == d["real_passes"] == (d["m"] + 7) // 8 and d["passes"] == doc.stream_passes(real)
    assert (d["real_passes"], d["passes"]) == ((0, 1) if name == "equal-8065" else (2, 3))
    if name == "equal-8065":
        assert np.unique(keys[group]).size == 1
    else:
        assert np.unique(keys[group]).size < d["n"]          # ties: 8,065 draws from 4,096 values
    # equal keys stay in id order
    order = doc.expected_order(oracle_keys)
    if name == "equal-8065":
        assert np.array_equal(order[offset:offset + d["n"]], group.astype(np.uint32))
    _assert_lists_follow_the_order(want, oracle_keys)
