"""CPU: the visit-offset / value-cutoff move pick as the checker states it (tests/move_pick.py), the temperature table
and the parameter validation of liuzhou_amd/move_pick.py."""
import math

import numpy as np
import pytest

from liuzhou_amd import move_pick as M
from tests import move_pick as chk

RNG = np.random.default_rng(20260119)


def _roots(n=200):
    for _ in range(n):
        ne = int(RNG.integers(1, 37))
        N = RNG.integers(0, 40, size=ne)
        if RNG.random() < 0.3:
            N[RNG.integers(0, ne)] = N.max()                     # ties for k*
        W = N * RNG.integers(-8, 9, size=ne) / 8.0
        q = chk.child_q(W, N, RNG.integers(0, 2, size=ne).astype(bool), 1)
        yield N, q, float(RNG.choice([1.0, 0.5, 2.0])), float(RNG.uniform(0.001, 0.999))


def test_off_at_zero_and_validation():
    assert M.move_pick_on() is False and M.move_pick_on(0.0, 0.0) is False and M.move_pick_on(0, 0) is False
    assert M.move_pick_on(0.5, 0.0) and M.move_pick_on(0.0, 0.125) and M.move_pick_on(1e6, 2.0)
    assert M.move_pick_kwargs() == {} and M.move_pick_kwargs(0.0, 0.0, 0.0) == {}
    assert M.move_pick_kwargs(3, 0) == {"move_visit_offset": 3.0, "move_value_cutoff": 0.0}
    assert M.move_pick_kwargs(0, 0.25, 6) == {"move_visit_offset": 0.0, "move_value_cutoff": 0.25, "temperature_halflife": 6.0}
    assert M.move_pick_kwargs(0, 0, 6) == {"temperature_halflife": 6.0}
    assert not chk.applies(terminal=False, sample_moves=True, temperature=1.0, force_uniform=False, offset=0.0, cutoff=0.0)
    for key, bads in (("move_visit_offset", (True, math.nan, math.inf, -math.inf, -0.5, "x", None)),
                      ("move_value_cutoff", (False, math.nan, math.inf, -0.125, 2.0000001, "x", None)),
                      ("temperature_halflife", (True, math.nan, math.inf, -1.0, "x", None))):
        for bad in bads:
            with pytest.raises(ValueError, match=key):
                M.move_pick_kwargs(**{key: bad})


def test_refusals_without_a_device():
    from liuzhou_amd.search_rules import SearchRules
    on = SearchRules.parse(32, move_visit_offset=1.0)
    assert on.refusal() is None
    assert "Gumbel" in SearchRules.parse(32, move_visit_offset=1.0, gumbel_considered=16).refusal()
    assert "sample_moves" in on.refusal(sample_moves=False)
    SearchRules.parse(32).refuse(search_backend="cuda_root")
    on.refuse(search_backend="tree")
    on.refuse(search_backend="portable")
    with pytest.raises(ValueError, match="tree backend"):
        on.refuse(search_backend="cuda_root")


def test_where_the_rule_applies():
    on = dict(terminal=False, sample_moves=True, temperature=1.0, force_uniform=False, offset=1.0, cutoff=0.0)
    assert chk.applies(**on)
    assert chk.applies(**{**on, "offset": 0.0, "cutoff": 0.5})
    for k, v in (("terminal", True), ("sample_moves", False), ("temperature", 1e-7), ("temperature", 1e-6),
                 ("temperature", 0.0), ("force_uniform", True)):
        assert not chk.applies(**{**on, k: v})
    assert chk.applies(**{**on, "temperature": 2e-6})


def test_large_offset_gives_the_most_visited_child():
    for N, q, T, u in _roots():
        for o in (float(N.max()), N.max() + 0.5, 1e6):
            r = chk.pick(N, q, T, u, o, 0.0)
            assert r["pick"] == r["kstar"] == int(np.argmax(N))
            assert r["eligible"].sum() == 1


def test_eligible_set_is_monotone_and_holds_kstar():
    for N, q, T, u in _roots():
        prev = None
        for o in (0.0, 0.5, 1.0, 3.0, 10.0, 1e6):
            e = chk.pick(N, q, T, u, o, 0.0 if o else 2.0)["eligible"]     # (o = 0 alone is off: cutoff 2 cuts nothing)
            assert e[int(np.argmax(N))]
            if prev is not None:
                assert not np.any(e & ~prev)                                  # shrinks in o
            prev = e
        prev = None
        for c in (0.125, 0.5, 1.0, 2.0):
            r = chk.pick(N, q, T, u, 0.5, c)
            e = r["eligible"]
            assert e[r["kstar"]] and r["weights"][r["kstar"]] == 1.0
            if prev is not None:
                assert not np.any(prev & ~e)                                  # grows in c
            prev = e
        full = chk.pick(N, q, T, u, 0.5, 0.0)["eligible"]                    # c = 0: no value test at all
        assert not np.any(prev & ~full)
        assert np.array_equal(chk.pick(N, q, T, u, 0.5, 2.0)["eligible"], full)   # |q| <= 1: a cutoff of 2 cuts nothing


def test_pick_is_eligible_and_counters_add_up():
    for N, q, T, u in _roots():
        for o, c in ((1.0, 0.0), (0.0, 0.25), (3.0, 0.5)):
            r = chk.pick(N, q, T, u, o, c)
            assert r["eligible"][r["pick"]]
            others = int((N > 0).sum()) - (1 if N[r["kstar"]] > 0 else 0)     # visited children other than k*
            assert r["cut_visits"] + r["cut_value"] + int(r["eligible"].sum()) - 1 == others
            first, last = (int(x) for x in np.nonzero(r["eligible"])[0][[0, -1]])
            assert chk.pick(N, q, T, 0.0, o, c)["pick"] == first                # weights of eligible children are > 0
            assert chk.pick(N, q, T, 1.0, o, c)["pick"] == last                 # no C_k exceeds S: the last eligible child


def test_offset_zero_cutoff_two_samples_the_visit_distribution():
    """With nothing cut the weights are the finish's own softmax(log N / T) up to the common factor."""
    N = np.array([5, 0, 20, 3, 12])
    r = chk.pick(N, np.zeros(5), 0.5, 0.4, 0.0, 2.0)
    want = (N / 20.0) ** 2.0
    assert np.allclose(r["weights"], want, rtol=1e-14, atol=0)
    assert r["pick"] == int(np.searchsorted(np.cumsum(want), 0.4 * want.sum(), side="right"))


def test_temperature_table():
    t = M.temperature_table(1.0, 0.1, 10, 4.0, 64)
    assert t.dtype == np.float32 and t.shape == (65,)
    assert t[0] == np.float32(1.0)                                           # T(0) = t_init
    assert t[4] == np.float32(0.1 + 0.9 * 0.5)                               # the excess halves at p = h
    assert t[8] == np.float32(0.1 + 0.9 * 0.25)
    assert np.all(t[10:] == np.float32(0.1))                                 # t_final from the threshold on
    assert np.all(np.diff(t[:10].astype(np.float64)) < 0)
    for p in range(10):
        assert t[p] == np.float32(0.1 + (1.0 - 0.1) * math.pow(0.5, p / 4.0))
    step = M.temperature_table(1.0, 0.1, 10, 0.0, 64)                        # h = 0: the step
    assert np.array_equal(step, np.where(np.arange(65) < 10, np.float32(1.0), np.float32(0.1)).astype(np.float32))
    assert M.temperature_table(1.0, 0.1, 0, 4.0, 3).tolist() == [np.float32(0.1)] * 4
    assert M.temperature_table(0.7, 0.7, 5, 2.0, 8).tolist() == [np.float32(0.7)] * 9
    with pytest.raises(ValueError, match="temperature_halflife"):
        M.temperature_table(1.0, 0.1, 10, -1.0, 64)


def test_meta_and_counter_names():
    assert M.move_pick_meta(M.move_pick_kwargs(3, 0.25, 6)) == {"visit_offset": 3.0, "value_cutoff": 0.25,
                                                                 "temperature_halflife": 6.0}
    assert M.move_pick_meta(M.move_pick_kwargs(0, 0, 6)) == {"visit_offset": 0.0, "value_cutoff": 0.0,
                                                              "temperature_halflife": 6.0}
    assert M.counters_from_block([4, 3, 2, 1]) == {"move_pick_applied": 4, "move_pick_cut_visits": 3,
                                                   "move_pick_cut_value": 2, "move_pick_changed": 1}
