"""GPU tests of the fused open-vocabulary segmentation (csrc/segment.hip, segment.py) against the reference chain restated
in torch (tests/segment_oracle.py).

The rule everywhere: the judge is the chain in float64 with the fp16 store applied, never the kernel's output.  A pixel may
differ from the float64 label only if the float64 logit of the label it got lies within tau of the float64 maximum, at most
1e-3 of a case's pixels may differ, and the score is within tau of the float64 maximum on every finite pixel.  tau is 4 x the
largest |logit_fp32 - logit_fp64| of the LIVE torch float32 chain on this GPU, and every case first proves that this chain
itself meets the cap on its inputs.
"""
import pytest
import torch

import segment_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(d):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}


def _judge_case(d, half=True, text_normalized=False):
    """Runs segment() on the inputs `d` and judges labels and score; returns (labels, score, figures)."""
    from segment import segment
    l64 = O.chain(d["fm"], d["text"], d["size"], d["weight"], d["bias"], torch.float64, half=half)
    l32 = O.chain(d["fm"], d["text"], d["size"], d["weight"], d["bias"], torch.float32, half=half)
    tau = O.tau_of(l32, l64)
    print("torch float32 chain:")
    O.judge(O.labels_of(l32), l64, tau)          # the precondition (pixels with non-finite logits are not judged): re-seed a case that fails HERE
    text = d["text"]
    before = text.clone()
    if text_normalized:
        text = text / text.norm(dim=-1, keepdim=True)
    labels, score = segment(d["fm"], text, size=d["size"], weight=d["weight"], bias=d["bias"], half=half,
                            text_normalized=text_normalized, return_score=True)
    assert torch.equal(d["text"], before), "text_features was modified"
    Hs, Ws = d["size"] if d["size"] is not None else d["fm"].shape[1:]
    assert labels.shape == (Hs, Ws) and labels.dtype == torch.int64 and score.shape == (Hs, Ws) and score.dtype == torch.float32
    print("segment():")
    return labels, score, O.judge(labels, l64, tau, score)


@pytest.mark.parametrize("family", O.FAMILIES)
@pytest.mark.parametrize("name", [c[0] for c in O.CASES])
def test_labels_and_score_against_the_float64_chain(name, family):
    _judge_case(_dev(O.make_inputs(name, family)))


@pytest.mark.parametrize("name", ["dec32_k150", "nodec48_k20"])
def test_without_the_fp16_store(name):
    _judge_case(_dev(O.make_inputs(name, "random")), half=False)


@pytest.mark.parametrize("name,family", [("dec32_k150", "random"), ("nodec512_k150", "regions"), ("nodec3_k5", "random")])
def test_normalised_text_gives_the_same_labels(name, family):
    """text_normalized=True on torch's own t / ||t||: the same labels, bit for bit, as the raw text"""
    from segment import segment
    d = _dev(O.make_inputs(name, family))
    kw = dict(size=d["size"], weight=d["weight"], bias=d["bias"])
    raw = segment(d["fm"], d["text"], **kw)
    tn = d["text"] / d["text"].norm(dim=-1, keepdim=True)
    pre = segment(d["fm"], tn, text_normalized=True, **kw)
    assert torch.equal(raw, pre), int((raw != pre).sum())
    _judge_case(d, text_normalized=True)


def test_special_pixels_follow_the_nan_and_tie_rule():
    """A zero pixel, an inf, a NaN and a value that overflows fp16: label 0 and score NaN, as torch.max gives; every other
    pixel is judged as usual."""
    from segment import segment
    d = _dev(O.make_inputs("nodec48_k20", "random"))
    d["fm"] = O.add_special_pixels(d["fm"])
    d["size"] = None
    labels, score, fig = _judge_case(d)
    l64 = O.chain(d["fm"], d["text"], None)
    bad = ~torch.isfinite(l64).all(dim=1)
    assert int(bad.sum()) >= 4 and fig["pixels"] == l64.shape[0] - int(bad.sum())
    assert int(torch.isnan(score).sum()) == int(bad.sum())
    assert torch.isnan(score.reshape(-1)[bad]).all()
    assert torch.equal(labels.reshape(-1)[bad], O.labels_of(l64)[bad]) and (labels.reshape(-1)[bad] == 0).all()
    # ties: two equal text rows - the lower index wins on every pixel where they lead
    t2 = torch.cat((d["text"][:3], d["text"][1:2], d["text"][3:]))          # row 3 == row 1
    lab = segment(d["fm"], t2)
    assert not (lab == 3).any() and (lab == 1).any()
    # the label does not depend on whether the score is asked for
    assert torch.equal(lab, segment(d["fm"], t2, return_score=True)[0])


@pytest.mark.parametrize("gt_size", [(90, 120), (100, 500)])
def test_reference_chain_narrower_and_wider_than_the_segmentation_size(gt_size):
    """segment_reference_chain: one call when the stored map is not wider than 480, the second resize composed when it is"""
    from segment import segment_reference_chain
    d = _dev(O.make_inputs("dec32_k20", "regions"))
    wide = gt_size[1] > 480
    second = (360, 480) if wide else None
    args = (d["fm"], d["text"], gt_size, d["weight"], d["bias"])
    l64 = O.chain(*args, torch.float64, second_size=second)
    l32 = O.chain(*args, torch.float32, second_size=second)
    tau = O.tau_of(l32, l64)
    O.judge(O.labels_of(l32), l64, tau)
    labels = segment_reference_chain(d["fm"], d["text"], gt_size, d["weight"], d["bias"])
    assert labels.shape == ((360, 480) if wide else gt_size)
    O.judge(labels, l64, tau)


@pytest.mark.parametrize("name", ["dec32_k20", "dec64_k1", "dec128_k150"])
def test_decoded_map_gives_exactly_the_fused_labels(name):
    """segment() on the stored map of fused_feature_decode(half=True) == segment() with the decoder fused: the same decode,
    the same rounding, the same contraction order"""
    from feature_loss import fused_feature_decode
    from segment import segment
    d = _dev(O.make_inputs(name, "random"))
    fused_l, fused_s = segment(d["fm"], d["text"], size=d["size"], weight=d["weight"], bias=d["bias"], half=True, return_score=True)
    stored = fused_feature_decode(d["fm"], d["size"], d["weight"], d["bias"], half=True)
    assert stored.dtype == torch.float16
    two_l, two_s = segment(stored.to(torch.float32), d["text"], return_score=True)
    assert torch.equal(fused_l, two_l) and torch.equal(fused_s, two_s)
    # and without a decoder: resize inside segment() == the resize of fused_feature_decode
    n = _dev(O.make_inputs("nodec48_k20", "random"))
    a = segment(n["fm"], n["text"], size=n["size"], return_score=True)
    b = segment(fused_feature_decode(n["fm"], n["size"], half=True).to(torch.float32), n["text"], return_score=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graph_capture_replays_to_identical_labels():
    from segment import segment
    d = _dev(O.make_inputs("dec32_k150", "regions"))
    kw = dict(size=d["size"], weight=d["weight"], bias=d["bias"], return_score=True)
    want_l, want_s = segment(d["fm"], d["text"], **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got_l, got_s = segment(d["fm"], d["text"], **kw)
    got_l.zero_()
    got_s.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got_l, want_l) and torch.equal(got_s, want_s)
    # new contents in the captured input: the replay follows them
    other = _dev(O.make_inputs("dec32_k150", "random"))
    d["fm"].copy_(other["fm"])
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got_l, segment(d["fm"], d["text"], **kw)[0])


def test_the_decoded_map_is_never_formed():
    """128 -> 512, K = 150, 360 x 480: the call's peak memory stays under labels + score + the resized input + the text
    block + 1 MiB - about half of the fp16 decoded map the reference writes"""
    from segment import segment
    C, Cout, K, Hs, Ws = 128, 512, 150, 360, 480
    g = torch.Generator().manual_seed(7)
    fm = torch.randn(C, 240, 320, generator=g).to(DEV)
    w = (torch.randn(Cout, C, generator=g) / C ** 0.5).to(DEV)
    b = (0.1 * torch.randn(Cout, generator=g)).to(DEV)
    t = torch.randn(K, Cout, generator=g).to(DEV)
    segment(fm, t, size=(Hs, Ws), weight=w, bias=b, return_score=True)        # (first-call allocations of the runtime)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    labels, score = segment(fm, t, size=(Hs, Ws), weight=w, bias=b, return_score=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    bound = 4 * Hs * Ws * (C + 3) + 4 * 256 * Cout + (1 << 20)
    print(f"peak rise {rise} bytes, bound {bound}, fp16 decoded map {2 * Cout * Hs * Ws}")
    assert rise <= bound and bound < 0.6 * 2 * Cout * Hs * Ws
    l64 = O.chain(fm, t, (Hs, Ws), w, b, torch.float64)
    l32 = O.chain(fm, t, (Hs, Ws), w, b, torch.float32)
    O.judge(labels, l64, O.tau_of(l32, l64), score)
