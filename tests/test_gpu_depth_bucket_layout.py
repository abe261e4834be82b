"""The bucket depth sort at the edges of its two intermediates' layouts (binning.hip): the row-major histogram matrix with its
column scan, and the B side as (key, id) pairs.

Every case runs one forward with depth_sort_buckets = 1 and pins `depth_key`, `order` and `order_counts` against
`np.argsort(keys, kind="stable")`, through the checks of tests/test_gpu_depth_order.py (272 x 256 image, C = 0, SH degree 0,
small splats):

  P = 16,385                    9 matrix rows of 32 bins, the last row holding ONE key
  P = 18,431 / 18,432 / 18,433  nine full rows - 1, exactly, + 1 (a tenth row of one key)
  P = 1,048,576 / 1,048,577     512 rows: all the column scan's first sweep takes; 513: its loop goes round again for one row
  tied keys, 18,433 / 200,001   every key at least twice: the fused pair store keeps a copy behind its original
  equal-8065, scratch-8065      a bucket above the capacity whose pairs start at pair index 3 (tests/depth_bucket_layout_cases.py,
                                proven on the CPU by tests/test_depth_bucket_layout_cases_cpu.py): the streaming sort reads pairs
                                in its first pass and, with three passes, ping-pongs through its own 2 n words of the B side
"""
import numpy as np
import pytest
import torch

import depth_bucket_layout_cases as lay_cases
import depth_order_cases as doc
import test_gpu_depth_order as tdo
from test_gpu_parity import _scene

pytestmark = pytest.mark.gpu

SWEEP_P = lay_cases.COLSCAN_SWEEP_ROWS * lay_cases.SORT_CHUNK        # 1,048,576 keys: 512 rows


def _plain(P, seed):
    return _scene(P=P, C=0, seed=seed, sh_degree=0, **doc.IMG, **doc.SMALL)


@pytest.mark.parametrize("P", [16385, 18431, 18432, 18433])
def test_matrix_rows_at_their_edges(P, option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 1)
    _res, info, keys, _want = tdo._check_order(f"rows P={P}", _plain(P, seed=300 + P % 7), "buckets")
    lay = doc.bucket_layout(keys, P)
    assert info["buckets"] == lay["count"] == 32 and lay_cases.matrix_rows(P) == (10 if P == 18433 else 9)
    assert info["largest"] == lay["largest"] and info["oversized"] == lay["oversized"]
    assert (keys != doc.CULLED_KEY).sum() > P // 2 and (lay["sizes"] > 0).sum() > 8


@pytest.fixture(scope="module")
def sweep_scenes():
    """One scene of 1,048,577 Gaussians (513 matrix rows) and its cut to 1,048,576 (512 rows)."""
    P = SWEEP_P + 1
    full = _scene(P=P, C=0, seed=310, sh_degree=0, **doc.IMG, scale_lo=0.002, scale_hi=0.006)
    cut = dict(full, P=SWEEP_P, **{k: v[:SWEEP_P].contiguous() for k, v in full.items()
                                   if torch.is_tensor(v) and v.dim() and v.shape[0] == P})
    return {SWEEP_P + 1: full, SWEEP_P: cut}


@pytest.mark.parametrize("P", [SWEEP_P + 1, SWEEP_P])
def test_column_scan_past_its_first_sweep(P, sweep_scenes, option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 1)
    scene = sweep_scenes[P]
    assert scene["P"] == P and lay_cases.matrix_rows(P) == lay_cases.COLSCAN_SWEEP_ROWS + (P > SWEEP_P)
    _res, info, keys, _want = tdo._check_order(f"sweep P={P}", scene, "buckets")
    lay = doc.bucket_layout(keys, P)
    assert info["buckets"] == lay["count"] == 1024
    assert info["largest"] == lay["largest"] and info["oversized"] == lay["oversized"] == 0
    # the last row's keys are alive and spread: its counts matter to the order
    assert (keys[SWEEP_P - 2048:] != doc.CULLED_KEY).any() and (lay["sizes"] > 0).sum() > 256


@pytest.mark.parametrize("P", [18433, 200001])
def test_tied_keys_through_the_pair_store(P, option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 1)
    scene = doc.ties_scene(P, seed=320 + P % 5)
    _res, info, keys, want = tdo._check_order(f"ties P={P}", scene, "buckets")
    assert info["buckets"] == doc.depth_bucket_count(P)
    h = P // 2
    assert np.array_equal(keys[:h], keys[h:2 * h]) and (keys != doc.CULLED_KEY).sum() > P // 2
    rank = np.empty(P, np.int64)
    rank[want] = np.arange(P)
    alive = np.flatnonzero(keys[:h] != doc.CULLED_KEY)
    twins = rank[alive + h] - rank[alive]
    assert np.all(twins >= 1) and (twins == 1).sum() > alive.size // 2      # (apart only where more than two keys tie)


@pytest.mark.parametrize("name", lay_cases.CASES)
def test_oversized_bucket_at_an_odd_pair_index(name, option):
    option("tile_cull", 0)
    option("depth_sort_buckets", 1)
    d = lay_cases.design(name)
    _res, info, _keys, want = tdo._check_order(name, lay_cases.designed_scene(name), "buckets", d["keys"])
    lay = doc.bucket_layout(d["keys"], d["P"])
    assert info["buckets"] == 32 and info["capacity"] == doc.CAPACITY
    assert info["largest"] == lay["largest"] == d["n"] and info["oversized"] == lay["oversized"] == 1
    off = d["offset"]
    assert off % 2 == 1 and int(lay["sizes"][:d["bucket"]].sum()) == off
    if name == "equal-8065":
        assert np.array_equal(want[off:off + d["n"]], d["group"].astype(np.uint32))       # equal keys: id order
