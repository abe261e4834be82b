"""The feature codebooks on the GPU (csrc/codebook.hip; codebook.py).  The judge is tests/codebook_oracle.py in numpy fp64: a code
is adjudicated against the DERIVED allowance of the fp32 fmaf chain, (C + 2) 2^-24 (2 sum|x c| + |c|^2), and at most 1 % of the
rows of a random-normal case may differ from the fp64 arg-min; dist2 and the centroids against ulp32 / 2 + 4 n 2^-53 sum|terms|;
count and moved exactly; on integer data - where every product and sum is exact - everything bit for bit."""
import numpy as np
import pytest
import torch

import codebook_oracle as co

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_codes(codes, x, cent, metric, what, share=co.MAX_DIFFERENT):
    right, differs = co.adjudicate(codes, x, cent, metric)
    print(f"{what}: {int((~right).sum())} wrong, {int(differs.sum())} of {len(codes)} off the fp64 arg-min")
    assert right.all(), f"{what}: {int((~right).sum())} codes beyond the allowance, the first at row {int(np.argmin(right))}"
    assert differs.sum() <= share * len(codes), f"{what}: {int(differs.sum())} of {len(codes)} rows differ from the fp64 arg-min"


@pytest.mark.parametrize("metric", co.METRICS)
@pytest.mark.parametrize("P,K,C", co.SHAPES)
def test_assign_against_the_judge(P, K, C, metric):
    import codebook
    x, cent = co.random_case(P, K, C)
    g = np.random.default_rng(P + K + C)
    prev = g.integers(-1, K, P).astype(np.int32)
    w = g.random(P).astype(np.float32)
    res = codebook.assign(_t(x), _t(cent), metric=metric, prev_codes=_t(prev, torch.int32), weight=_t(w), return_dist2=True)
    torch.cuda.synchronize()
    assert isinstance(res, codebook.Assignment) and res.codes.dtype == torch.int32 and tuple(res.codes.shape) == (P,)
    assert res.dist2.dtype == torch.float32 and tuple(res.dist2.shape) == (P,)
    assert res.inertia.dtype == torch.float64 and res.inertia.dim() == 0 and res.moved.dtype == torch.int32 and res.moved.dim() == 0
    codes, d = _n(res.codes), _n(res.dist2)
    _check_codes(codes, x, cent, metric, f"{(P, K, C)} {metric}")
    want, bound = co.dist2(x, cent, codes, metric)
    miss = np.abs(d.astype(np.float64) - want) > bound
    assert not miss.any(), f"dist2: {int(miss.sum())} of {P} beyond the bound"
    assert int(res.moved) == int((codes != prev).sum())
    total = co.inertia(d, codes, K, w)
    assert abs(float(res.inertia) - total) <= 1e-12 * abs(total)
    plain = codebook.assign(_t(x), _t(cent), metric=metric)                        # codes alone: the same bits
    assert torch.is_tensor(plain) and np.array_equal(_n(plain), codes)


def test_exact_codes_on_integer_data():
    """every product and sum is exact in fp32: the codes are the judge's, bit for bit - duplicated centroids (the lower index
    wins) and rows equidistant from two centroids included"""
    import codebook
    for P, K, C, seed in ((257, 33, 8, 0), (1000, 130, 64, 1), (129, 5, 3, 2), (33, 2, 1, 3)):
        g = np.random.default_rng(seed)
        x = g.integers(-8, 9, (P, C)).astype(np.float32)
        cent = g.integers(-8, 9, (K, C)).astype(np.float32)
        cent[K - 1] = cent[0]                                                      # a duplicate: the lower index wins
        x[0] = cent[0]
        if K >= 8:
            cent[K // 2] = cent[1]                                                 # another, beyond a sub-tile's edge
            x[1] = cent[1]
            x[2], cent[3], cent[4] = 0, 0, 0                                       # equidistant: +-2 in one channel
            cent[3, 0], cent[4, 0] = 2, -2
        want = co.assign(x, cent)
        got = _n(codebook.assign(_t(x), _t(cent)))
        assert np.array_equal(got, want), (P, K, C, int((got != want).sum()))
        assert got[0] == 0 and (K < 8 or (got[1] == 1 and got[2] == 3))
        ties = (co.scores(x, cent)[0] == co.scores(x, cent)[0].min(1, keepdims=True)).sum(1) > 1
        assert ties.sum() >= (3 if K >= 8 else 1)                                  # the case holds what it is about


def _same_book(a, b, what):
    for name in ("centroids", "codes", "count", "moved"):
        x, y = _n(getattr(a, name)), _n(getattr(b, name)) if not isinstance(b, dict) else b[name]
        same = np.array_equal(_bits(x), _bits(y)) if x.dtype == np.float32 else np.array_equal(x, y)
        assert same, f"{what}: {name} differs"


@pytest.mark.parametrize("P,K,C,stride,chain", [(1000, 7, 8, 1, True), (1200, 35, 10, 1, True), (900, 5, 4, 3, True), (800, 40, 16, 1, False)])
def test_kmeans_on_integer_data_equals_chained_steps_and_the_judge(P, K, C, stride, chain):
    """chain: a case without empty clusters - the reseeding rule takes the iteration number, and a single step is iteration 0 of
    its own.  The last case has empty clusters that are reseeded: against the judge's loop alone."""
    import codebook
    x, centres, _ = co.integer_blobs(P, K, C, seed=P)
    n = 4
    want = co.lloyd(x, K, n, fit_stride=stride)
    assert chain == np.array_equal(co.lloyd(x, K, n, fit_stride=stride, reseed=False)["centroids"], want["centroids"])
    xt = _t(x)
    full = codebook.kmeans(xt, K, iterations=n, fit_stride=stride)
    torch.cuda.synchronize()
    assert full.count.dtype == torch.int64 and full.inertia.dtype == torch.float64 and tuple(full.inertia.shape) == (n,)
    assert full.moved.dtype == torch.int32 and tuple(full.moved.shape) == (n,)
    _same_book(full, want, "kmeans against the judge's Lloyd loop")
    inert = _n(full.inertia)                                                       # every dist2 is within 2^-24 of its exact value
    assert np.isfinite(inert).all() and (np.diff(inert) <= 2.0 ** -23 * inert[:-1]).all()
    if not chain:
        return
    cent, moved = None, []
    for it in range(n):                                                            # n single steps, each from the last centroids
        if it == 0:
            step = codebook.kmeans(xt, K, iterations=1, fit_stride=stride)
        else:
            step = codebook.kmeans(xt, K, iterations=1, init=cent, fit_stride=stride, reseed_empty=False)
        cent = step.centroids
        moved.append(int(step.moved[0]))
    for name in ("centroids", "codes", "count"):
        a, b = _n(getattr(step, name)), _n(getattr(full, name))
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), name
    assert moved[0] == int(full.moved[0]) and moved[1:] == [len(x[::stride])] * (n - 1)          # (a step of its own starts from -1)


@pytest.mark.parametrize("metric", co.METRICS)
def test_kmeans_step_by_step_on_real_data(metric):
    """kmeans driven one iteration at a time: the codes of every step adjudicated, the centroids against the judge's fp64 mean of
    the DEVICE's codes, and (L2, unit weights) an inertia that does not rise by more than the roundings allow"""
    import codebook
    P, K, C = 1000, 12, 33
    g = np.random.default_rng(5)
    centres = g.normal(0, 2, (K, C))
    x = (centres[g.integers(0, K, P)] + g.normal(0, 1, (P, C))).astype(np.float32)
    xt = _t(x)
    cent = x[co.init_rows(P, K)].copy()
    last = None
    for it in range(4):
        codes = _n(codebook.assign(xt, _t(cent), metric=metric))
        _check_codes(codes, x, cent, metric, f"step {it} {metric}")
        step = codebook.kmeans(xt, K, iterations=1, metric=metric, init=_t(cent), reseed_empty=False)
        torch.cuda.synchronize()
        _, count, want, bound = co.update(x, codes, cent, metric)
        got = _n(step.centroids)
        miss = np.abs(got.astype(np.float64) - want) > bound
        assert not miss.any(), f"step {it}: {int(miss.sum())} centroid elements beyond the bound"
        assert int(step.moved[0]) == int((codes >= 0).sum())
        d, dbound = co.dist2(x, cent, codes, metric)
        inertia = float(step.inertia[0])
        assert abs(inertia - d.sum()) <= dbound.sum() + 1e-12 * d.sum()
        if metric == "l2" and last is not None:
            # Lloyd's argument holds for the fp64 arg-min; a device code may be worse than it by both allowances, once per row
            s, e = co.scores(x, cent, metric)
            slack = 2 * e[np.arange(P), codes].sum() + 2 * dbound.sum() + 1e-12 * last
            assert inertia <= last + slack, f"step {it}: the inertia rose from {last} to {inertia}"
        last = inertia
        cent = got


def test_views_are_read_in_place():
    """the model's (P, 1, C) tensor, a column slice and a row-strided view: the bits of their contiguous copies, and no copy"""
    import codebook
    P, K = 4001, 9
    g = np.random.default_rng(11)
    wide = _t(g.normal(0, 1, (P, 64)).astype(np.float32))
    views = {"(P, 1, C)": wide.reshape(P, 1, 64), "[:, 16:48]": wide[:, 16:48], "[::3]": wide[::3], "[::3, 5:36]": wide[::3, 5:36]}
    for name, v in views.items():
        flat = v.reshape(v.shape[0], -1) if v.dim() == 3 else v
        cent = flat[:K].contiguous()
        copy = flat.contiguous()
        assert name == "(P, 1, C)" or not flat.is_contiguous()
        want = codebook.assign(copy, cent, return_dist2=True)
        book = codebook.kmeans(copy, K, iterations=2)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        got = codebook.assign(v, cent, return_dist2=True)
        book_v = codebook.kmeans(v, K, iterations=2)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - before
        assert extra < copy.numel() * 4 // 2, f"{name}: {extra} bytes allocated, the features are {copy.numel() * 4}"
        assert torch.equal(got.codes, want.codes) and np.array_equal(_bits(_n(got.dist2)), _bits(_n(want.dist2))), name
        assert torch.equal(book_v.codes, book.codes) and torch.equal(book_v.count, book.count), name
        # the centroids are sums of fp64 atomics in a varying order: equal up to the last bit of the rounding
        assert np.abs(_n(book_v.centroids).astype(np.float64) - _n(book.centroids)).max() <= co.ulp32(_n(book.centroids)).max(), name


def test_assign_never_holds_a_score_matrix():
    import codebook
    from simple_knn import _C
    P, K, C = 20000, 4096, 32
    x, cent = (torch.randn(n, C, device=DEV) for n in (P, K))
    codebook.assign(x[:256], cent)                                                 # (the allocator's and the runtime's first-call state)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    codes = codebook.assign(x, cent)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before - codes.numel() * 4
    assert extra <= _C.codebook_workspace_bytes(K, C) + 65536, f"{extra} bytes above the inputs and outputs"
    assert extra < P * K * 4 // 100
    xs, cs = _n(x[:500]), _n(cent)
    _check_codes(_n(codes[:500]), xs, cs, "l2", "20000 x 4096 x 32, the first 500 rows")


def test_rows_and_centroids_that_are_not_finite():
    import codebook
    x, cent = co.random_case(300, 40, 19, seed=2)
    x[5, 3], x[77, 18], x[128, 0], x[299, 7] = np.nan, np.inf, -np.inf, np.nan
    cent[0, 2], cent[33, 18] = np.inf, np.nan
    for metric in co.METRICS:
        res = codebook.assign(_t(x), _t(cent), metric=metric, return_dist2=True)
        codes = _n(res.codes)
        assert (codes[[5, 77, 128, 299]] == -1).all() and (_n(res.dist2)[[5, 77, 128, 299]] == 0).all()
        assert not np.isin(codes, (0, 33)).any() and (np.delete(codes, [5, 77, 128, 299]) >= 0).all()
        _check_codes(codes, x, cent, metric, f"non-finite {metric}")
        assert np.isfinite(float(res.inertia))
        none = codebook.assign(_t(x), _t(np.full((3, 19), np.nan, np.float32)), metric=metric)
        assert (_n(none) == -1).all()
        new, count = codebook.update(_t(x), res.codes, _t(cent), metric=metric)    # -1 belongs to no centroid
        assert int(count.sum()) == 296 and count[0] == 0 and count[33] == 0
        assert np.array_equal(_bits(_n(new)[[0, 33]]), _bits(cent[[0, 33]]))       # empty: kept, bit for bit


@pytest.mark.parametrize("metric", co.METRICS)
def test_weights_and_empty_clusters(metric):
    """weights of 0, inf and NaN exclude a row from the update and from the inertia, never from assign; an empty cluster keeps its
    centroid or takes the judge's row"""
    import codebook
    P, K, C = 500, 24, 10
    x, cent = co.random_case(P, K, C, seed=3)
    cent[20:] = cent[:4] * 50 + 100                                                # far away: nobody's nearest under L2
    x[(7 * co.MUL + 2 * co.ADD) % P, 1] = np.nan                                   # a reseeding row that is not finite
    g = np.random.default_rng(4)
    w = (g.random(P) + 0.5).astype(np.float32)
    w[::7], w[3::11], w[5::13], w[1::17] = 0, np.inf, np.nan, -1
    plain = codebook.assign(_t(x), _t(cent), metric=metric)
    res = codebook.assign(_t(x), _t(cent), metric=metric, weight=_t(w), return_dist2=True)
    assert torch.equal(res.codes, plain)
    codes, d = _n(res.codes), _n(res.dist2)
    total = co.inertia(d, codes, K, w)
    assert np.isfinite(total) and abs(float(res.inertia) - total) <= 1e-12 * total
    codes = codes.copy()
    codes[np.isin(codes, (2, 7))] = 3                                              # two clusters emptied by hand, 7 with a bad row
    for reseed, it in ((False, 0), (True, 2)):
        new, count = codebook.update(_t(x), _t(codes, torch.int32), _t(cent), metric=metric, weight=_t(w), reseed_empty=reseed, iteration=it)
        want, wcount, want64, bound = co.update(x, codes, cent, metric, w, reseed, it)
        assert count.dtype == torch.int64 and np.array_equal(_n(count), wcount) and (wcount == 0).sum() >= 2
        got = _n(new)
        empty = wcount == 0
        assert np.array_equal(_bits(got[empty]), _bits(want[empty])), "an empty cluster: the judge's row, bit for bit"
        assert np.array_equal(_bits(got[7]), _bits(cent[7]))                       # its reseeding row is not finite: kept
        assert reseed == (not np.array_equal(got[2], cent[2]))
        miss = np.abs(got.astype(np.float64) - want64) > bound
        assert not miss[~empty].any(), f"{int(miss.sum())} centroid elements beyond the bound"


def test_prev_codes_aliased_with_the_output():
    import codebook
    x, cent = co.random_case(777, 50, 12, seed=6)
    want = codebook.assign(_t(x), _t(cent))
    prev = want.clone()
    prev[::5] = -1
    prev[1::9] = 49
    expect = int((prev != want).sum())
    buf = prev.clone()
    res = codebook.assign(_t(x), _t(cent), prev_codes=buf, out=buf)
    assert res.codes.data_ptr() == buf.data_ptr() and torch.equal(buf, want) and int(res.moved) == expect and res.dist2 is None
    again = codebook.assign(_t(x), _t(cent), prev_codes=buf, out=buf)
    assert int(again.moved) == 0


def test_fit_stride_and_quantize():
    import codebook
    x, _, _ = co.integer_blobs(1200, 6, 16, seed=9)                                # integer data: bit for bit
    xt = _t(x)
    by_hand = codebook.kmeans(xt[::4], 6, iterations=3)
    strided = codebook.kmeans(xt, 6, iterations=3, fit_stride=4)
    assert np.array_equal(_bits(_n(strided.centroids)), _bits(_n(by_hand.centroids)))
    assert torch.equal(strided.moved, by_hand.moved) and tuple(strided.codes.shape) == (1200,)
    assert torch.equal(strided.codes, codebook.assign(xt, strided.centroids)) and torch.equal(strided.codes[::4], by_hand.codes)
    for M in (1, 4, 8):
        q = codebook.quantize(xt, 5, subspaces=M, iterations=2)
        d = 16 // M
        assert tuple(q.codebooks.shape) == (M, 5, d) and tuple(q.codes.shape) == (1200, M) and q.codes.dtype == torch.int32
        assert tuple(q.count.shape) == (M, 5) and tuple(q.inertia.shape) == (M, 2)
        for m in range(M):
            part = codebook.kmeans(xt[:, m * d:(m + 1) * d], 5, iterations=2)
            assert np.array_equal(_bits(_n(q.codebooks[m])), _bits(_n(part.centroids))) and torch.equal(q.codes[:, m], part.codes)
        back = codebook.dequantize(q)
        want = np.concatenate([_n(q.codebooks)[m][_n(q.codes)[:, m]] for m in range(M)], axis=1)
        assert back.dtype == torch.float32 and np.array_equal(_bits(_n(back)), _bits(want))
        small = codebook.quantize(xt, 5, subspaces=M, iterations=2, narrow=True)
        assert small.codes.dtype == torch.uint8 and torch.equal(small.codes.int(), q.codes) and torch.equal(codebook.dequantize(small), back)
    bad = xt.clone()
    bad[3, 9] = float("nan")
    q = codebook.quantize(bad, 5, subspaces=4, iterations=1, narrow=True)
    assert q.codes[3].tolist()[2] == 255 and (q.codes[3].int() != 255).sum() == 3 and (codebook.dequantize(q)[3, 8:12] == 0).all()
    assert codebook.quantize(xt, 300, subspaces=2, iterations=1, narrow=True).codes.dtype == torch.int16


def test_bad_arguments():
    import codebook
    x = torch.zeros(10, 6, device=DEV)
    cent = torch.zeros(3, 6, device=DEV)
    cases = [
        (lambda: codebook.assign(x.double(), cent), r"\(10, 6\)"),
        (lambda: codebook.assign(x.reshape(10, 2, 3), cent), r"\(10, 2, 3\)"),
        (lambda: codebook.assign(x, cent[:, :5]), r"\(3, 5\)"),
        (lambda: codebook.assign(x, cent.cpu()), r"\(3, 6\)"),
        (lambda: codebook.assign(x, cent[:0]), r"\(0, 6\)"),
        (lambda: codebook.assign(x, cent, metric="l1"), "l1"),
        (lambda: codebook.assign(x, cent, prev_codes=torch.zeros(9, dtype=torch.int32, device=DEV)), r"\(9,\)"),
        (lambda: codebook.assign(x, cent, prev_codes=torch.zeros(10, dtype=torch.int64, device=DEV)), r"int64 \(10,\)"),
        (lambda: codebook.assign(x, cent, weight=torch.zeros(10, 1, device=DEV)), r"\(10, 1\)"),
        (lambda: codebook.assign(x, cent, out=torch.zeros(11, dtype=torch.int32, device=DEV)), r"\(11,\)"),
        (lambda: codebook.kmeans(x, 0), "k = 0"),
        (lambda: codebook.kmeans(x, 65537), "k = 65537"),
        (lambda: codebook.kmeans(x, 3, iterations=-1), "iterations = -1"),
        (lambda: codebook.kmeans(x, 3, fit_stride=0), "fit_stride = 0"),
        (lambda: codebook.kmeans(x, 3, init=cent[:2]), r"\(2, 6\)"),
        (lambda: codebook.kmeans(x[:0], 3), r"\(0, 6\)"),
        (lambda: codebook.quantize(x, 3, subspaces=4), r"\(10, 6\)"),
        (lambda: codebook.quantize(x, 3, subspaces=2, init=cent), r"\(3, 6\)"),
        (lambda: codebook.update(x, torch.zeros(10, dtype=torch.int64, device=DEV), cent), r"int64 \(10,\)"),
        (lambda: codebook.update(x, torch.zeros(10, dtype=torch.int32, device=DEV), cent, iteration=-2), "iteration = -2"),
        (lambda: codebook.dequantize(codebook.Quantized(cent, torch.zeros(10, 2, dtype=torch.int32, device=DEV), None, None, None)), r"\(3, 6\)"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError, match=text):
            call()
    empty = codebook.kmeans(x[:0], 3, init=cent)                                   # no rows: nothing to do, nothing breaks
    assert tuple(empty.codes.shape) == (0,) and torch.equal(empty.centroids, cent) and int(empty.count.sum()) == 0


def test_determinism_and_capture():
    """two assigns: identical bits; kmeans(iterations=3) on integer data captured in a graph and replayed twice: the eager bits"""
    import codebook
    x, cent = co.random_case(1000, 300, 129)
    a = codebook.assign(_t(x), _t(cent), return_dist2=True)
    b = codebook.assign(_t(x), _t(cent), return_dist2=True)
    assert torch.equal(a.codes, b.codes) and np.array_equal(_bits(_n(a.dist2)), _bits(_n(b.dist2)))
    xi, _, _ = co.integer_blobs(1500, 9, 12, seed=4)
    xt = _t(xi)
    eager = codebook.kmeans(xt, 9, iterations=3)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                  # one stream, no parallel branches
        captured = codebook.kmeans(xt, 9, iterations=3)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        _same_book(captured, eager, "replay")
        assert np.allclose(_n(captured.inertia), _n(eager.inertia), rtol=1e-12, atol=0)        # (fp64 atomics in a varying order)
