"""CPU: the checker of the Gumbel root search tests (tests/gumbel_tree.py).

1. With the mode off the Python tree equals oracle.OracleTree bit for bit (the checker is checked first), on the cases
   tests/test_forced_tree_cpu.py uses.
2. With it on, under tree_parity.hash_evaluator: the Gumbel-top-k order of the first simulations, the pick, the target,
   the prior as the target of a search that learns nothing, and selection on N - N0 at a kept root."""
import numpy as np
import pytest

from oracle import lz_oracle as O
from tests import forced_tree as FT
from tests import gumbel_tree as GT
from tests.tree_parity import hash_evaluator


# ---- 1. the checker against the C oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("with_noise", [False, True])
def test_mode_off_equals_the_c_oracle_tree(with_noise):
    """40 positions of g1_rules.npz, 64 simulations, 3 moves with advance: the same pending state at every step, root
    child visits and priors bit-exact, value sums equal as doubles."""
    from oracle.selfplay_oracle import deterministic_pick
    B, sims, eps = 40, 64, 0.25
    states, _ = FT.parity_inputs(False, num_games=B, seed=5)
    rng = np.random.default_rng(17)
    cur = [O.state_from_batch(states, i) for i in range(B)]
    ref = [O.OracleTree(cur[i], 1.0) for i in range(B)]
    make = lambda cs: GT.GumbelTree(cs, 1.0, considered=0, sims=sims)
    got = [make(cur[i]) for i in range(B)]

    def step(is_root, noise):
        pa = [t.prepare_root() if is_root else t.select() for t in ref]
        pb = [t.prepare_root() if is_root else t.select() for t in got]
        assert pa == pb
        need = [i for i, p in enumerate(pa) if p]
        if need:
            sa = O.batch_from_states([ref[i].pending_state() for i in need])
            sb = O.batch_from_states([got[i].pending_state() for i in need])
            for f in sa:
                assert np.array_equal(np.asarray(sa[f]), np.asarray(sb[f])), f
            pri, val = hash_evaluator(sa)
            for j, i in enumerate(need):
                nz = noise[i] if (is_root and noise is not None) else None
                ref[i].complete(pri[j], float(val[j]), nz, eps)
                got[i].complete(pri[j], float(val[j]), nz, eps)
        if is_root:
            for i in range(B):
                if noise is not None and not pa[i] and not ref[i].root_terminal():
                    ref[i].root_noise(noise[i], eps)
                    got[i].root_noise(noise[i], eps)
                got[i].root_step(pb[i], g=np.zeros(80, np.float32))      # m = 0: records nothing, changes nothing
                assert not got[i].active()

    kept = 0
    for mv in range(3):
        noise = (rng.gamma(0.3, 1.0, size=(B, 80)).astype(np.float32) + np.float32(1e-6)) if with_noise else None
        step(True, noise)
        for _ in range(sims):
            step(False, None)
        for i in range(B):
            assert ref[i].root_terminal() == got[i].root_terminal()
            a, b = ref[i].root_children(), got[i].root_children()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4]), (mv, i)
            assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)), (mv, i, "value sums differ")
            assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32)), (mv, i, "priors differ")
            assert ref[i].root_visits() == got[i].root_visits()
            assert ref[i].root_value_sum() == got[i].root_value_sum()
            assert ref[i].root_player() == got[i].root_player()
            if ref[i].root_terminal():
                ref[i], got[i] = O.OracleTree(cur[i], 1.0), make(cur[i])
                continue
            pick = deterministic_pick(*a, ref[i].root_player())
            cur[i] = O.apply_index(cur[i], pick)
            ka, kb = ref[i].advance(pick), got[i].advance(pick)
            assert ka == kb
            kept += int(ka)
            if not ka:
                ref[i], got[i] = O.OracleTree(cur[i], 1.0), make(cur[i])
    assert kept > B                                                         # subtrees were carried over


# ---- 2. the rule ------------------------------------------------------------------------------------------------------
def _trees(m, sims, num_games=32, seed=23, **kw):
    states, g = GT.parity_inputs(num_games=num_games, seed=seed)
    return states, g, [GT.GumbelTree(O.state_from_batch(states, i), 1.0, considered=m, sims=sims, **kw)
                       for i in range(num_games)]


@pytest.mark.parametrize("m", [16, 4])
def test_top_m_order_pick_and_target(m):
    sims = 64
    states, g, trees = _trees(m, sims)
    GT.search_alone(trees, sims, g)
    live = more_than_m = 0
    for i, t in enumerate(trees):
        if t.root_terminal():
            continue
        live += 1
        idx, vis, _vs, pr, _pl = t.root_children()
        ne = len(idx)
        more_than_m += int(ne > m)
        assert int(vis.sum()) == sims == t.root_visits(), i
        assert t.no_candidate == 0, i                                       # a fresh root never lacks a candidate
        # the first min(m, ne) simulations visit the top-m children by gl = g + log P, in that order
        first = min(m, ne, sims)
        want = sorted(range(ne), key=lambda k: (-float(t.gl[k]), k))[:first]
        assert t.root_order[:first] == want, i
        assert set(np.nonzero(vis)[0].tolist()) == set(want) or ne <= m, i  # Sequential Halving never leaves the sample
        # the pick is among the most visited of this search, and the best of them by score
        pick, target, score, vmix = t.gumbel_finish()
        L = vis - np.array(t.base)
        assert L[pick] == L.max(), i
        assert all(score[pick] >= score[k] for k in range(ne) if L[k] == L.max()), i
        assert -1.0 <= vmix <= 1.0
        # the target: a distribution on the legal set
        legal = np.zeros(220, bool)
        legal[O.legal_indices_py(O.state_from_batch(states, i))] = True
        assert abs(float(target.sum(dtype=np.float64)) - 1.0) < 1e-6, i
        assert not target[~legal].any() and np.all(target[legal] > 0), i
    assert live >= 16 and more_than_m > 0


def test_target_equals_the_prior_when_the_search_learns_nothing():
    """All g = 0, n = m = ne and an evaluator that returns one constant value: every child is visited once, every
    completed value is that constant as the root's mover sees it, so sigma is the same for every child and
    softmax(log P + sigma) = P.  (Roots whose children are all non-terminal and moved by one player: a terminal child
    backs up its own value, and a child moved by the other player has the opposite sign.)"""
    const = np.float32(0.375)

    def evaluator(states):
        pri, val = hash_evaluator(states)
        return pri, np.full_like(val, const)

    states, _g = GT.parity_inputs(num_games=48, seed=31)
    checked = 0
    for i in range(48):
        cs = O.state_from_batch(states, i)
        ne = len(O.legal_indices_py(cs))
        if ne < 2 or ne > 72:
            continue
        t = GT.GumbelTree(cs, 1.0, considered=ne, sims=ne)
        GT.search_alone([t], ne, np.zeros((1, 80), np.float32), evaluator=evaluator)
        idx, vis, _vs, pr, pl = t.root_children()
        if np.any(vis != 1) or len(set(pl.tolist())) != 1 or any(t.nodes[t.nodes[t.root].first_child + k].terminal
                                                                   for k in range(ne)):
            continue
        _pick, target, _score, _vmix = t.gumbel_finish()
        np.testing.assert_allclose(target[idx], pr, atol=1e-6, rtol=0)
        checked += 1
    assert checked >= 8


def test_kept_root_selects_on_visits_of_this_search():
    """Two consecutive moves: the second search starts from a kept subtree whose children bring visits along; its
    candidates are the children with N - N0 equal to the schedule's entry."""
    m, sims = 8, 48
    states, g, trees = _trees(m, sims, num_games=24, seed=41)
    GT.search_alone(trees, sims, g)
    g2 = np.random.default_rng(99).gumbel(size=g.shape).astype(np.float32)
    kept = []
    for i, t in enumerate(trees):
        if t.root_terminal():
            continue
        pick, _target, _score, _vmix = t.gumbel_finish()
        action = int(t.root_children()[0][pick])
        if t.advance(action) and not t.root_terminal() and t.nodes[t.root].expanded and t.nodes[t.root].n_children > 1:
            kept.append(i)
    assert len(kept) >= 8
    carried = 0
    for i in kept:
        t = trees[i]
        assert not t.prepare_root()                                         # a kept root needs no evaluation
        t.root_step(False, g=g2[i])
        assert t.active() and t.root_base == t.root_visits()
        carried += int(sum(t.base) > 0)
        ne = t.nodes[t.root].n_children
        table = t.table[min(m, ne)]
        for s in range(sims):
            before = t.root_children()[1].copy()
            assert t.root_visits() - t.root_base == s
            pend = t.select()
            k = t.last_root_child
            L = before - np.array(t.base)
            cand = np.nonzero(L == table[s])[0]
            assert k in (cand if cand.size else range(ne)), (i, s)
            if pend:
                pri, val = hash_evaluator(O.batch_from_states([t.pending_state()]))
                t.complete(pri[0], float(val[0]))
            assert t.root_children()[1][k] == before[k] + 1
        pick, _target, _score, _vmix = t.gumbel_finish()
        L = t.root_children()[1] - np.array(t.base)
        assert L[pick] == L.max() and int(L.sum()) == sims
    assert carried >= 4                                                     # N0 was not all zero: the test saw kept visits
