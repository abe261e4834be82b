"""numpy restatement of the language-guided selection (reference gaussian_renderer/__init__.py:21-55), in the reference's
number formats, the yardstick for csrc/edit.hip:

  n = ||f||_2 and f^ = f / n in fp32; f^ and the fp32-normalised text rows rounded to fp16; s_k = f^ . t^_k of the fp16
  values (summed in fp64: the exact value of what any fp32 accumulation order approximates) rounded to fp16; for K > 1 the
  softmax over the fp16 scores (fp64 here, rounded once) with every probability rounded to fp16; the decision on those fp16
  values (sums of fp16 probabilities are exact in fp64).

For every row: the mask, the decided quantity (s_0, q or q2: what was compared; q in the pure argmax branches) and a MARGIN
in fp16 ulps of the decided quantity: the distance of the compared value from the threshold, or - for an argmax decision -
the gap between the best positive and the best non-positive column (0 for a tie across the boundary).  Where both a
threshold and an argmax take part (delete with a threshold) the margin is the smaller of the two.  A row with margin <= 1
is BORDERLINE: only there may another accumulation order, another exp, or a host-versus-device scalar comparison
legitimately change the answer.  NaN rows (zero norm, non-finite elements) are decided with certainty: every >= is false
and torch's argmax takes the first NaN column, which is column 0 because the whole row is NaN."""
import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64


def _fma32(a, acc):
    """fp32 fma(a, a, acc): a * a is exact in fp64"""
    return (a.astype(F64) * a.astype(F64) + acc.astype(F64)).astype(F32)


def sum_squares_fp32(x, vector=True):
    """Row sums of squares in fp32 in the order of the device: torch's row reduction, which csrc/edit.hip follows (measured
    bit-equal to `features.norm(dim=-1)` on MI355X at C = 16, 32, 128, 512).  Rows with C % 4 == 0 (vector=True): every lane
    owns float4 pieces 64 apart and keeps one fma accumulator per component; the four are added pairwise for C < 128, else
    left to right; the lanes are then added as a tree of neighbours.  Other rows, and the text rows: one accumulator per lane
    over elements 64 apart, then the same tree."""
    x = np.asarray(x, F32)
    P, C = x.shape
    pow2 = lambda n: 1 << max(0, int(n - 1).bit_length())
    if vector and C % 4 == 0 and C <= 2048:
        C4 = C // 4
        L = min(64, pow2(C4))
        NV = -(-C4 // L)
        xs = np.zeros((P, NV * L, 4), F32)
        xs[:, :C4] = x.reshape(P, C4, 4)
        acc = np.zeros((P, L, 4), F32)
        for j in range(NV):
            acc = _fma32(xs[:, j * L:(j + 1) * L], acc)
        if C < 128:
            lane = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
        else:
            lane = ((acc[..., 0] + acc[..., 1]) + acc[..., 2]) + acc[..., 3]
    else:
        L = min(64, pow2(C)) if vector else 64
        J = -(-C // L)
        xs = np.zeros((P, J * L), F32)
        xs[:, :C] = x
        lane = np.zeros((P, L), F32)
        for j in range(J):
            lane = _fma32(xs[:, j * L:(j + 1) * L], lane)
    while lane.shape[1] > 1:
        lane = lane[:, 0::2] + lane[:, 1::2]
    return lane.astype(F32)


def normalize_fp32(x, order="device", vector=True):
    """x / ||x||_2 per row, norm and quotient in fp32.  order "device": the sum of squares as sum_squares_fp32 adds it;
    "exact": the exactly rounded sum (what any order approximates; the two quotients differ by at most 2 ulps)."""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        ss = sum_squares_fp32(x, vector) if order == "device" else (x.astype(F64) ** 2).sum(-1, keepdims=True).astype(F32)
        return (x / np.sqrt(ss)).astype(F32)


def scores_fp16(features, text, text_normalized=False, order="device"):
    """(P, K) fp16 scores of the half GEMM, (P, C) fp32 normalised features, (K, C) fp32 normalised text."""
    fn = normalize_fp32(features, order)
    tn = np.asarray(text, F32) if text_normalized else normalize_fp32(text, order, vector=False)
    with np.errstate(all="ignore"):
        s = (fn.astype(F16).astype(F64) @ tn.astype(F16).astype(F64).T).astype(F16)
    return s, fn, tn


def softmax_fp16(s):
    """softmax over the fp16 scores, every probability the fp16 neighbour of its exact value (fp64 here; the reference's fp32
    evaluation lands on the other neighbour on about 1 row in 10^4, which is why rows near a decision are borderline)"""
    with np.errstate(all="ignore"):
        x = s.astype(F64)
        e = np.exp(x - x.max(-1, keepdims=True))        # a NaN or +inf score: the whole row becomes NaN
        return (e / e.sum(-1, keepdims=True)).astype(F16)


def _ulp(x):
    """fp16 spacing at |x| (the subnormal spacing at 0)."""
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(x.astype(F16))).astype(F64)


def _threshold_margin(q, thr):
    with np.errstate(all="ignore"):
        m = np.abs(q.astype(F64) - F64(thr)) / _ulp(q)
    return np.where(np.isnan(q.astype(F64)), np.inf, m)


def _argmax_margin(v, pos):
    """gap between the best positive and the best non-positive column in ulps of the larger; inf when a side is empty or the
    row is NaN"""
    K = v.shape[1]
    neg = [k for k in range(K) if k not in set(pos)]
    if not neg:
        return np.full(v.shape[0], np.inf)
    a, b = v[:, list(pos)].astype(F64).max(-1), v[:, neg].astype(F64).max(-1)
    with np.errstate(all="ignore"):
        m = np.abs(a - b) / _ulp(np.maximum(a, b))
    return np.where(np.isnan(a) | np.isnan(b), np.inf, m)


def select(features, text, threshold=None, positive_ids=(0,), variant="select", scalar="fp32", text_normalized=False, scores=None):
    """The reference's two functions.  `scalar`: how the threshold meets the fp16 value - "fp32" (the value widened, the
    threshold rounded to fp32: the kernel, and torch's device comparison) or "fp16" (the threshold rounded to fp16: torch's
    CPU comparison).  The two differ only on rows of margin < 1.  `scores`: what scores_fp16 returned for these inputs, to
    spare the contraction when one input is decided several times.
    Returns dict(mask float32 0/1, decided float32, margin float64, is_bool, features_normalized, text_normalized)."""
    assert variant in ("select", "delete") and scalar in ("fp32", "fp16")
    pos = [int(k) for k in positive_ids]
    s, fn, tn = scores if scores is not None else scores_fp16(features, text, text_normalized)
    P, K = s.shape
    assert len(set(pos)) == len(pos) and all(0 <= k < K for k in pos) and pos
    thr = None if threshold is None else (F64(F16(threshold)) if scalar == "fp16" else F64(F32(threshold)))
    ge = lambda q: q.astype(F64) >= thr             # False for NaN
    is_bool = False
    if K == 1:
        assert thr is not None, "K = 1 needs a threshold"
        decided = s[:, 0]
        mask, margin = ge(decided), _threshold_margin(decided, thr)
    else:
        p = softmax_fp16(s)
        with np.errstate(all="ignore"):
            q = p[:, pos].astype(F64).sum(-1).astype(F16)
        v = p.copy()
        v[:, pos[0]] = q
        m = np.isin(np.argmax(v.astype(F64), -1), pos)       # NaN is the maximum, the first column wins a tie
        if variant == "select" and thr is not None:
            decided, mask, margin = q, ge(q), _threshold_margin(q, thr)
        elif variant == "delete" and thr is not None:
            with np.errstate(all="ignore"):
                q2 = v[:, pos].astype(F64).sum(-1).astype(F16)
            decided, mask = q2, m | ge(q2)
            margin = np.minimum(_threshold_margin(q2, thr), _argmax_margin(v, pos))
        else:
            decided, mask, margin = q, m, _argmax_margin(v, pos)
            is_bool = variant == "delete"
    return dict(mask=mask.astype(F32), decided=decided.astype(F32), margin=margin, is_bool=is_bool,
                features_normalized=fn, text_normalized=tn)


def make_inputs(P, C, K, seed, noise=0.6, common=1.0, decades=3.0):
    """Clustered features f = a * t[label] + noise + a shared component, the row scale spread over 2 * decades orders of
    magnitude; the text rows share a CLIP-like common direction, which pulls the softmax towards 1 / K.  fp32 arrays."""
    g = np.random.default_rng(seed)
    shared = g.standard_normal(C)
    text = g.standard_normal((K, C)) + common * shared
    label = g.integers(0, K, P)
    f = text[label] * g.uniform(0.5, 2.0, (P, 1)) + noise * g.standard_normal((P, C)) * np.sqrt(1.0 + common) \
        + 0.3 * common * shared
    f *= 10.0 ** g.uniform(-decades, decades, (P, 1))
    return f.astype(F32), text.astype(F32)


def make_gap_inputs(P, C, K, seed, threshold, positive_ids, variant, min_margin=8.0, special_rows=True):
    """Inputs on which every row's margin is >= min_margin ulps: weak noise makes the positive-class probability bimodal, and
    the rows that still land near the decision are dropped and redrawn.  special_rows: row 0 is all zero, row 1 holds an
    inf, row 2 a NaN (decided with certainty, see the module docstring)."""
    g = np.random.default_rng(seed)
    text = (g.standard_normal((K, C)) + 0.5 * g.standard_normal(C)).astype(F32)
    rows = np.zeros((0, C), F32)
    for _ in range(50):
        n = 2 * (P - len(rows)) + 16
        label = g.integers(0, K, n)
        sign = g.choice([-1.0, 1.0], (n, 1)) if K == 1 else 1.0        # one text: the cosine is near -1 or near +1
        f = (sign * text[label] * g.uniform(0.5, 2.0, (n, 1)) + 0.15 * g.standard_normal((n, C))) * 10.0 ** g.uniform(-2, 2, (n, 1))
        f = f.astype(F32)
        keep = select(f, text, threshold, positive_ids, variant)["margin"] >= min_margin
        rows = np.concatenate([rows, f[keep]])[:P]
        if len(rows) == P:
            break
    assert len(rows) == P, "could not draw enough rows off the decision boundary"
    if special_rows and P >= 3:
        rows[0] = 0.0
        rows[1, 0] = np.inf
        rows[2, C - 1] = np.nan
    return rows, text
