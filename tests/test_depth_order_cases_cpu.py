"""CPU: the designed depth-key cases of tests/depth_order_cases.py, proven by the scalar oracle alone.

For every case the oracle's forward must report exactly the designed alive set, the designed float bits as depths, and - through
the restated bucket arithmetic of common.h - the shift, the single bucket, its size and the pass count the case's name claims.
The oracle's own tile lists must follow `expected_order`: the stable argsort IS the reference of the depth sort.  Only then is a
GPU run of such a case (tests/test_gpu_depth_order.py) a run of the path it names."""
import numpy as np
import pytest

import depth_order_cases as doc


def test_the_bucket_arithmetic_is_the_headers():
    """The values of common.h's own static_asserts."""
    assert doc.depth_bucket_count(16385) == 32 and doc.depth_bucket_count(16384) == 16 and doc.depth_bucket_count(1) == 16
    assert doc.depth_bucket_count(1000000) == 1024 and doc.depth_bucket_count(1250000) == 1024
    assert doc.depth_bucket_count(1250001) == 2048 and doc.depth_bucket_count(5000000) == 2048
    assert doc.depth_bucket_bits(1250000) == 10 and doc.depth_bucket_bits(1250001) == 11
    assert doc.depth_bucket_shift(5, 5, 16) == 0 and doc.depth_bucket_shift(0xFFFFFFFF, 0, 16) == 0
    assert doc.depth_bucket_shift(0, 14, 16) == 0 and doc.depth_bucket_shift(0, 15, 16) == 1
    assert doc.depth_bucket_shift(0x40000000, 0x41200000, 1024) == 15
    assert doc.depth_bucket_shift(0, 0xFFFFFFFE, 16) == 29 and (0xFFFFFFFE >> 29) <= 14
    assert doc.depth_bucket_count(doc.P_DESIGNED) == 32


def test_expected_order_is_stable_and_puts_the_culled_last():
    keys = np.array([7, 0xFFFFFFFF, 3, 7, 0xFFFFFFFF, 3, 0x80000000], np.uint32)       # (unsigned: 0x80000000 above 7)
    assert doc.expected_order(keys).tolist() == [2, 5, 0, 3, 6, 1, 4]


def test_names_and_lists():
    assert len(set(doc.DESIGNED)) == len(doc.DESIGNED) == 15
    assert set(doc.ORACLE_LIST_CASES) <= set(doc.DESIGNED) and set(doc.OTHER_FLAVOUR_CASES) <= set(doc.DESIGNED)
    sizes = {doc.design(n)["n"] for n in doc.GROUP_CASES}
    # the kernel's own edges: steps = ceil(n / 512) from 1 to 2, a wave's partial step, the capacity and the first size beyond
    assert {64, 65, 512, 513, doc.CAPACITY - 1, doc.CAPACITY, doc.CAPACITY + 1, 2 * doc.STREAM_CHUNK,
            2 * doc.STREAM_CHUNK + 1} <= sizes
    assert {doc.design(n)["passes"] for n in doc.GROUP_CASES if not doc.design(n)["stream"]} == {0, 1, 2, 3, 4}
    assert {(doc.design(n)["real_passes"], doc.design(n)["passes"]) for n in doc.GROUP_CASES if doc.design(n)["stream"]} == \
        {(1, 1), (2, 3), (3, 3), (4, 5)}


@pytest.mark.parametrize("name", doc.GROUP_CASES)
def test_a_designed_case_is_what_its_name_claims(name):
    d, want = doc.design(name), doc.designed_oracle(name)
    P, keys = d["P"], d["keys"]
    (group,) = d["groups"]
    near, far = d["outliers"]
    # the alive set is the designed one, every radius finite and positive there
    alive = want["radii"] > 0
    assert np.array_equal(alive, ~d["culled"]) and int(alive.sum()) == d["n"] + 2
    assert want["radii"][alive].max() < 100000
    # the oracle's view depths are the designed float bits
    assert np.array_equal(want["depths"].view(np.uint32)[alive], keys[alive])
    oracle_keys = np.where(alive, want["depths"].view(np.uint32), doc.CULLED_KEY).astype(np.uint32)
    # shift, bucket, size - from the oracle's keys through the restated arithmetic
    lay = doc.bucket_layout(oracle_keys, P)
    assert lay["count"] == 32 and lay["kmin"] == d["kmin"] == keys[near] and lay["kmax"] == d["kmax"] == keys[far]
    assert lay["shift"] == d["shift"] == (25 if name in ("lds-4pass-5000", "stream-5pass-12289") else 23)
    bucket = np.full(P, -1, np.int64)
    bucket[alive] = lay["bucket"]
    (j,) = d["group_buckets"]
    assert np.all(bucket[group] == j) and bucket[near] == 0 and bucket[far] not in (j, 0) and bucket[far] <= 30
    assert group.size == d["n"] and int(lay["sizes"][j]) == d["n"] == lay["largest"]
    assert lay["oversized"] == d["oversized"] == int(d["n"] > doc.CAPACITY)
    assert sorted(np.flatnonzero(lay["sizes"]).tolist()) == sorted({0, j, int(bucket[far])})
    # the pass count: the bits in which the bucket's keys differ, in digits of eight
    real = doc.sort_passes(oracle_keys[group], lay["kmin"], lay["shift"])
    assert real == d["real_passes"] == (d["m"] + 7) // 8
    assert d["passes"] == (doc.stream_passes(real) if d["stream"] else real)
    assert d["chunks"] == (-(-d["n"] // doc.STREAM_CHUNK) if d["stream"] else 0)
    if d["m"]:
        assert np.unique(keys[group]).size < d["n"] or d["m"] > 16        # ties wherever 2^m is not far above n
    _assert_lists_follow_the_order(want, oracle_keys)


def test_the_mixed_case_has_two_oversized_buckets_beside_ordinary_ones():
    d, want = doc.design("mixed"), doc.designed_oracle("mixed")
    P, keys = d["P"], d["keys"]
    alive = want["radii"] > 0
    assert np.array_equal(alive, ~d["culled"]) and int(alive.sum()) == 2 * doc.MIXED_N + doc.MIXED_SPREAD
    assert np.array_equal(want["depths"].view(np.uint32)[alive], keys[alive])
    oracle_keys = np.where(alive, want["depths"].view(np.uint32), doc.CULLED_KEY).astype(np.uint32)
    lay = doc.bucket_layout(oracle_keys, P)
    assert lay["count"] == 32 and lay["kmin"] == d["kmin"] and lay["kmax"] == d["kmax"] and lay["shift"] == d["shift"] == 20
    bucket = np.full(P, -1, np.int64)
    bucket[alive] = lay["bucket"]
    for g, j in zip(d["groups"], d["group_buckets"]):
        assert g.size == doc.MIXED_N and np.all(bucket[g] == j) and lay["sizes"][j] > doc.CAPACITY
        own = oracle_keys[np.flatnonzero(bucket == j)]          # (id order; the spread's share of the bucket included)
        assert np.unique(oracle_keys[g]).size > 3000 and doc.sort_passes(own, lay["kmin"], lay["shift"]) >= 2
    assert d["group_buckets"] == (4, 14) and lay["oversized"] == 2
    ordinary = np.delete(lay["sizes"], d["group_buckets"])
    assert (ordinary > 0).sum() >= 15 and ordinary.max() <= doc.CAPACITY
    _assert_lists_follow_the_order(want, oracle_keys)


def _assert_lists_follow_the_order(want, keys):
    """The oracle's point_list holds every tile's Gaussians in expected_order: the rank in that order rises strictly inside
    every tile's range."""
    order = doc.expected_order(keys)
    rank = np.empty(order.size, np.int64)
    rank[order] = np.arange(order.size)
    pl, rg = want["point_list"], want["ranges"].reshape(-1, 2)
    assert pl.size == want["n"] == int(want["tiles_touched"].sum()) > 0
    r = rank[pl]
    rising = np.ones(pl.size, bool)
    rising[1:] = r[1:] > r[:-1]
    starts = rg[rg[:, 1] > rg[:, 0], 0]
    rising[starts] = True                                           # (a tile's first entry has no predecessor)
    assert rising.all(), f"{int((~rising).sum())} entries out of order"
    assert int((rg[:, 1] - rg[:, 0]).sum()) == pl.size
    assert np.array_equal(np.bincount(pl, minlength=keys.size), want["tiles_touched"])
