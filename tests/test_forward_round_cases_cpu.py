"""CPU: every designed case of tests/forward_round_cases.py, proven with the scalar oracle alone - the designed tile's list has
exactly L entries in construction order, and its positions reach the quadrants the placement says (read off the oracle's
n_contrib and final T planes)."""
import numpy as np
import pytest

import forward_round_cases as fr
from util import run_oracle


def _oracle(sc):
    o, out, _ = run_oracle(sc, backward=False)
    return dict(ranges=o.read("ranges").reshape(-1, 2).astype(np.int64), point_list=o.read("point_list").astype(np.int64),
                n_contrib=o.read("n_contrib").astype(np.int64), final_T=o.read("final_T").astype(np.float64))


@pytest.mark.parametrize("placement", fr.PLACEMENTS)
@pytest.mark.parametrize("L", fr.LENGTHS)
def test_design_holds_on_the_oracle(L, placement):
    C = (5, 16, 32)[fr.LENGTHS.index(L) % 3]           # the geometry differs by image size only: every size is visited
    sc = fr.scene(L, placement, C)
    st = _oracle(sc)
    lo, hi = st["ranges"][sc["case"]["tile_index"]]
    assert hi - lo == L
    assert np.array_equal(st["point_list"][lo:hi], np.arange(L))          # list position i = Gaussian i
    nq = [int(q.max()) for q in fr.quadrants(fr.tile_block(st["n_contrib"], sc))]
    Tq = [q for q in fr.quadrants(fr.tile_block(st["final_T"], sc))]
    if placement == "quad":
        assert nq == [L, 0, 0, 0]
    elif placement == "alt":
        # the last position of each parity is the last contributor of its quadrant
        last_even, last_odd = (L - 1) // 2 * 2 + 1 if L else 0, L // 2 * 2 if L > 1 else 0
        assert nq == [last_even, 0, 0, last_odd]
    elif placement == "full":
        assert (fr.tile_block(st["n_contrib"], sc) == L).all()            # every entry blended at every pixel
        assert all((t > 1e-3).all() for t in Tq) or L == 0
    else:
        f = fr.front_start(L)
        n = fr.tile_block(st["n_contrib"], sc)
        if L >= 8:
            # every pixel ends inside the front: behind at least one opaque entry, in front of the front's last one (the entry that
            # would take T below 1e-4 is not blended)
            assert (n > f).all() and (n < f + fr.FRONT).all()
            assert all((t < 1e-2).all() for t in Tq)
        else:
            assert (n == L).all()


def test_placements_differ_where_they_should():
    """The case table itself: lengths on both sides of every round and chunk edge, and hit counts of both parities."""
    assert {31, 32, 33, 63, 64, 65, 95, 96, 97}.issubset(fr.LENGTHS)
    hits0 = [(L + 1) // 2 for L in fr.LENGTHS]
    assert any(h % 2 for h in hits0) and any(h % 2 == 0 for h in hits0 if h)
