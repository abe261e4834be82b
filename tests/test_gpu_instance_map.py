"""The painter's instance map of packed masks on the GPU (csrc/sam_masks.hip: instance_map_kernel; sam_masks.instance_map)
against the numpy painter of tests/label_maps.py, exactly; and the map as the labels of the label vote."""
import numpy as np
import pytest
import torch

import label_maps as lm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _masks(K, FH, FW, seed):
    """K overlapping random rectangles; the last but one is noise, the last one empty (where K allows)."""
    rng = np.random.default_rng(seed)
    m = np.zeros((K, FH, FW), bool)
    for k in range(K):
        y0, x0 = rng.integers(0, FH), rng.integers(0, FW)
        m[k, y0:y0 + rng.integers(1, FH), x0:x0 + rng.integers(1, FW)] = True
    if K >= 2:
        m[K - 2] = rng.random((FH, FW)) < 0.3
    if K >= 3:
        m[K - 1] = False
    return m


@pytest.mark.parametrize("K", [0, 1, 33, 70])
@pytest.mark.parametrize("FH,FW", [(37, 45), (64, 64), (300, 33)])          # (300, 33): more than one tile each way
def test_instance_map_equals_the_numpy_painter(FH, FW, K):
    import sam_masks as sm
    masks = _masks(K, FH, FW, seed=100 * K + FH)
    packed = sm.pack_masks(torch.from_numpy(masks).to(DEV))
    got = sm.instance_map(packed)
    assert got.dtype == torch.int32 and tuple(got.shape) == (FH, FW) and got.device.type == "cuda"
    assert np.array_equal(got.cpu().numpy(), lm.painter(masks))
    if K == 0:
        assert (got == -1).all()
        assert (sm.instance_map(packed, torch.zeros(0, dtype=torch.int32, device=DEV)) == -1).all()
        return
    # a permuted index with a repeated row, int64 and int32; the values are positions in the index
    rng = np.random.default_rng(K)
    order = rng.permutation(K)
    order = np.concatenate([order, order[:1], order[K // 2:K // 2 + 1]])
    for dtype in (torch.int64, torch.int32):
        got = sm.instance_map(packed, torch.from_numpy(order).to(DEV).to(dtype))
        assert np.array_equal(got.cpu().numpy(), lm.painter(masks, order))
    # a part of the masks only, and show_anns' order: the small masks on top
    few = order[:max(1, K // 3)]
    assert np.array_equal(sm.instance_map(packed, torch.from_numpy(few).to(DEV)).cpu().numpy(), lm.painter(masks, few))
    areas = masks.reshape(K, -1).sum(1)
    by_area = sm.paint_order(torch.from_numpy(areas).to(DEV))
    assert by_area.device.type == "cuda" and by_area.tolist() == sorted(range(K), key=lambda j: areas[j], reverse=True)
    assert np.array_equal(sm.instance_map(packed, by_area).cpu().numpy(), lm.painter(masks, by_area.tolist()))


def test_instance_map_feeds_the_label_vote():
    """A view's instance map goes into label_votes as it is (int32, -1 = no instance: counted in the total alone), and gives
    what the grouped route gives for the same map."""
    import contrib
    import sam_masks as sm
    from test_gpu_contrib import CASES
    from test_gpu_label_votes import _bar, _np, _wrapper_inputs
    sc = CASES["chunks"]()
    W, H, P, K = sc["image_width"], sc["image_height"], sc["P"], 33
    masks = _masks(K, H, W, seed=5)
    packed = sm.pack_masks(torch.from_numpy(masks).to(DEV))
    ids = sm.instance_map(packed, sm.paint_order(torch.from_numpy(masks.reshape(K, -1).sum(1)).to(DEV)))
    assert (ids == -1).any() and int(ids.max()) >= 8
    st, kw = _wrapper_inputs(sc)
    out = contrib.label_votes(st, labels=ids, num_classes=K, **kw)
    grouped = contrib.contributions(st, masks=contrib.MaskLifter.from_label_map(ids, K), pixel_outputs=False, **kw)["acc"]
    torch.cuda.synchronize()
    assert out["acc"].shape == (P, K + 1) and out["acc"][:, :K].any()
    _bar(_np(out["acc"]), _np(grouped), "the instance map's votes against the grouped route")
