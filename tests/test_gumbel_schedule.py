"""CPU: the Sequential Halving schedule of the Gumbel root search (liuzhou_amd/gumbel.py)."""
import itertools

import numpy as np
import pytest

from liuzhou_amd.gumbel import considered_table, considered_visits, gumbel_on

BUDGETS = (1, 2, 5, 16, 50, 200, 800)


def test_known_answers():
    assert considered_visits(4, 16) == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert considered_visits(4, 10) == [0, 0, 0, 0, 1, 1, 2, 2, 3, 3]
    assert considered_visits(3, 7) == [0, 0, 0, 1, 1, 2, 2]
    assert considered_visits(2, 5) == [0, 0, 1, 1, 2]
    want = [0] * 16 + [1] * 8 + [2] * 4 + [3] * 4 + [4] * 4
    for v in range(5, 12):
        want += [v, v]
    assert len(want) == 50 and considered_visits(16, 50) == want
    assert considered_visits(1, 6) == [0, 1, 2, 3, 4, 5] and considered_visits(0, 3) == [0, 1, 2]


@pytest.mark.parametrize("n", BUDGETS)
def test_every_row_has_length_n(n):
    for m in range(0, 33):
        assert len(considered_visits(m, n)) == n
    tab = considered_table(32, n)
    assert tab.shape == (33, n) and tab.dtype == np.int32
    for j in range(33):
        assert tab[j].tolist() == considered_visits(j, n)


def _runs(row):
    return [(v, len(list(grp))) for v, grp in itertools.groupby(row)]


@pytest.mark.parametrize("n", BUDGETS)
def test_fresh_root_simulation(n):
    """A fresh root with fixed random scores, driven by the selection rule (candidates: visits == the schedule's entry,
    largest score first): a candidate always exists; when a round of c entries ends, exactly c children hold the most
    visits, one more than the round's entry; the rounds' lengths never grow."""
    rng = np.random.default_rng(1234 + n)
    for m in range(1, 33):
        for ne in sorted({1, 2, max(1, m - 1), m, m + 3, 72, 128}):
            j = min(m, ne)
            row = considered_visits(j, n)
            runs = _runs(row)
            lengths = [c for _v, c in runs[:-1]]              # (the last round may be cut by the budget)
            assert all(a >= b for a, b in zip(lengths, lengths[1:])), (m, n, ne, lengths)
            if len(runs) > 1:
                assert runs[-1][1] <= runs[-2][1]
            score = rng.standard_normal(ne)
            visits = np.zeros(ne, np.int64)
            picks = []
            ends = set(itertools.accumulate(c for _v, c in runs))
            full = dict(zip(itertools.accumulate(c for _v, c in runs), runs))
            for s in range(n):
                cand = np.nonzero(visits == row[s])[0]
                assert cand.size > 0, (m, n, ne, s)
                picks.append(int(cand[np.argmax(score[cand])]))
                visits[picks[-1]] += 1
                if (s + 1) in ends and (s + 1 < n or len(runs) == 1 or runs[-1][1] == runs[-2][1]):
                    v, c = full[s + 1]
                    assert visits.max() == v + 1 and int((visits == v + 1).sum()) == min(c, ne), (m, n, ne, s)
            assert int(visits.sum()) == n
            first = min(n, j)                                 # the first j simulations: the top-j by score, in that order
            assert picks[:first] == np.argsort(-score, kind="stable")[:first].tolist(), (m, n, ne)


def test_validation():
    assert gumbel_on(0) is False and gumbel_on(0, 50.0, 1.0) is False
    assert gumbel_on(16) is True and gumbel_on(72, 0.0, 0.0) is True and gumbel_on(1, 50, 0.1) is True
    for m in (-1, 73, 1000, 2.5, True):
        with pytest.raises(ValueError):
            gumbel_on(m)
    for bad in (-1.0, -1e-9, float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError):
            gumbel_on(16, bad, 1.0)
        with pytest.raises(ValueError):
            gumbel_on(16, 50.0, bad)
