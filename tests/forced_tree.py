"""Pure-Python variant-P tree with forced playouts and policy target pruning (Wu 2019, "Accelerating Self-Play Learning in
Go", section 3.2): the checker of the `forced_playouts_k` tests.

`oracle/lz_oracle.c` holds the reference tree of every other parity test and cannot be extended, so this module restates
it in Python and adds the two rules.  It keeps `OracleTree`'s method surface (prepare_root, select, pending_state,
complete, root_noise, root_children, root_visits, root_value_sum, root_player, root_terminal, advance), so the helpers
of tests/tree_parity.py drive it unchanged.  With k = 0 it must equal `OracleTree` bit for bit
(tests/test_forced_tree_cpu.py checks that first).

Arithmetic: value sums and scores in Python floats (doubles; one addition per edge and simulation in path order),
priors and the noise mix in numpy.float32 exactly as lzo_tree_complete / lzo_tree_root_noise do them; rules through the
oracle's legal_indices_py / apply_index / game_status.

Forced playouts (root level of a descent; n = the root's visit count, not clamped):
    child c is due  <=>  N(c) > 0  and  float(N) * float(N) < (k * float(P)) * float(n)
and the descent takes the due child with the lowest index; otherwise PUCT as in lzo_tree_select.
Policy target pruning: `prune_targets()` (see its docstring).  A tree whose `forced_on` is False (a fast search of the
playout cap) is neither forced nor pruned."""
import math

import numpy as np

from oracle import lz_oracle as O
from tests import readout_ref as R


class _Node:
    __slots__ = ("state", "parent", "first_child", "n_children", "action_index", "prior", "visit_count", "value_sum",
                 "player", "terminal", "expanded", "no_legal_terminal", "initial_value")

    def __init__(self, state, parent, action, prior):
        self.state = state
        self.parent = parent
        self.first_child = -1
        self.n_children = 0
        self.action_index = action
        self.prior = prior                      # a numpy.float32 value widened to a Python float
        self.visit_count = 0
        self.value_sum = 0.0
        self.player = int(state.player)
        self.terminal = O.game_status(state) != 0
        self.expanded = False
        self.no_legal_terminal = False
        self.initial_value = 0.0


def _terminal_value(state) -> float:
    st = O.game_status(state)
    if st in (1, -1):
        return 1.0 if st == int(state.player) else -1.0
    return 0.0


class ForcedTree:
    def __init__(self, cs, exploration_weight: float = 1.0, forced_k: float = 0.0):
        self.nodes = [_Node(cs, -1, -1, 1.0)]
        self.root = 0
        self.c = float(exploration_weight)
        self.k = float(forced_k)
        self.forced_on = True                   # the game's root-noise switch (False: a fast search of the playout cap)
        self.path = []
        self.pending = -1
        self.pending_is_root = False
        self.forced_count = 0                   # descents that took a due child
        self.last_due = []                      # child offsets that were due at the last select() (empty: PUCT decided)
        self.last_root_child = -1               # child offset the last select() took at the root (-1: none)

    # ---- the protocol of OracleTree ----
    def prepare_root(self) -> bool:
        r = self.nodes[self.root]
        self.pending = -1
        if O.game_status(r.state) != 0:
            r.terminal = True
            return False
        if r.expanded:
            return False
        self.pending = self.root
        self.pending_is_root = True
        return True

    def _backup(self, leaf_value: float) -> None:
        value = leaf_value
        for off in range(len(self.path) - 1, -1, -1):
            n = self.nodes[self.path[off]]
            n.visit_count += 1
            n.value_sum += value
            if off > 0 and self.nodes[self.path[off - 1]].player != n.player:
                value = -value

    def due_children(self):
        """Offsets of the root children that are due for a forced playout right now (ascending)."""
        r = self.nodes[self.root]
        if not (self.k > 0.0 and self.forced_on):
            return []
        n = float(r.visit_count)
        out = []
        for j in range(r.n_children):
            ch = self.nodes[r.first_child + j]
            N = float(ch.visit_count)
            if ch.visit_count > 0 and N * N < (self.k * float(ch.prior)) * n:
                out.append(j)
        return out

    def select(self) -> bool:
        self.pending = -1
        self.last_due, self.last_root_child = [], -1
        root = self.nodes[self.root]
        if root.terminal:
            return False
        cur = self.root
        self.path = [cur]
        while True:
            n = self.nodes[cur]
            if not (n.expanded and n.n_children > 0 and not n.terminal):
                break
            best_child = -1
            if cur == self.root:
                due = self.due_children()
                if due:
                    self.last_due = due
                    best_child = n.first_child + due[0]
                    self.forced_count += 1
            if best_child < 0:
                sqrt_total = math.sqrt(float(n.visit_count if n.visit_count > 1 else 1))
                best = -math.inf
                for j in range(n.n_children):
                    ch = self.nodes[n.first_child + j]
                    q = 0.0
                    if ch.visit_count > 0:
                        mv = ch.value_sum / float(ch.visit_count)
                        q = mv if n.player == ch.player else -mv
                    u = self.c * ch.prior * sqrt_total / (1.0 + float(ch.visit_count))
                    score = q + u
                    if score > best:
                        best, best_child = score, n.first_child + j
            if best_child < 0:
                break
            if cur == self.root:
                self.last_root_child = best_child - n.first_child
            cur = best_child
            self.path.append(cur)
        leaf = self.nodes[cur]
        if leaf.terminal:
            self._backup(-1.0 if leaf.no_legal_terminal else _terminal_value(leaf.state))
            return False
        if leaf.expanded and leaf.n_children == 0:
            leaf.terminal = True
            leaf.no_legal_terminal = True
            self._backup(-1.0)
            return False
        self.pending = cur
        self.pending_is_root = False
        return True

    def pending_state(self):
        return self.nodes[self.pending if self.pending >= 0 else self.root].state

    def complete(self, priors220, value, noise=None, epsilon: float = 0.25) -> None:
        ni = self.pending
        if ni < 0:
            return
        self.pending = -1
        st = self.nodes[ni].state
        idx = O.legal_indices_py(st)
        n = len(idx)
        nd = self.nodes[ni]
        if n == 0:
            nd.expanded = True
            nd.terminal = True
            nd.no_legal_terminal = O.game_status(st) == 0
            nd.initial_value = -1.0 if nd.no_legal_terminal else _terminal_value(st)
            ret = nd.initial_value
        else:
            p220 = np.asarray(priors220, np.float32)
            pr = [np.float32(p220[a]) for a in idx]
            eps = np.float32(epsilon)
            if self.pending_is_root and noise is not None and n > 1:
                keep = np.float32(1.0 - float(eps))
                nz = np.asarray(noise, np.float32)
                pr = [np.float32(np.float32(keep * pr[j]) + np.float32(eps * nz[j])) for j in range(n)]
            s = np.float32(0.0)
            for j in range(n):
                s = np.float32(s + pr[j])
            if not np.isfinite(s) or s <= np.float32(0.0):
                pr = [np.float32(np.float32(1.0) / np.float32(n))] * n
            else:
                pr = [np.float32(pr[j] / s) for j in range(n)]
            first = len(self.nodes)
            for j in range(n):
                self.nodes.append(_Node(O.apply_index(st, idx[j]), ni, idx[j], float(pr[j])))
            nd.first_child, nd.n_children, nd.expanded = first, n, True
            nd.initial_value = float(np.float32(value))
            ret = nd.initial_value
        if not self.pending_is_root:
            self._backup(ret)

    def root_noise(self, noise, epsilon: float) -> None:
        r = self.nodes[self.root]
        if not r.expanded or r.n_children <= 1:
            return
        eps = np.float32(epsilon)
        keep = np.float32(1.0 - float(eps))
        nz = np.asarray(noise, np.float32)
        pr, s = [], np.float32(0.0)
        for j in range(r.n_children):
            v = np.float32(np.float32(keep * np.float32(self.nodes[r.first_child + j].prior)) + np.float32(eps * nz[j]))
            pr.append(v)
            s = np.float32(s + v)
        denom = np.float32(1e-8) if s < np.float32(1e-8) else s
        for j in range(r.n_children):
            self.nodes[r.first_child + j].prior = float(np.float32(pr[j] / denom))

    def root_terminal(self) -> bool:
        r = self.nodes[self.root]
        return bool(r.terminal or r.n_children == 0)

    def root_children(self):
        r = self.nodes[self.root]
        ch = [self.nodes[r.first_child + j] for j in range(r.n_children)]
        return (np.array([c.action_index for c in ch], np.int32), np.array([c.visit_count for c in ch], np.int32),
                np.array([c.value_sum for c in ch], np.float64), np.array([c.prior for c in ch], np.float32),
                np.array([c.player for c in ch], np.int32))

    def root_visits(self) -> int:
        return int(self.nodes[self.root].visit_count)

    def root_value_sum(self) -> float:
        return float(self.nodes[self.root].value_sum)

    def root_player(self) -> int:
        return int(self.nodes[self.root].player)

    def advance(self, action_index: int) -> bool:
        r = self.nodes[self.root]
        for j in range(r.n_children):
            if self.nodes[r.first_child + j].action_index == int(action_index):
                self.root = r.first_child + j
                self.nodes[self.root].parent = -1
                self.pending = -1
                return True
        return False

    def node_count(self) -> int:
        return len(self.nodes)

    # ---- policy target pruning ----
    def prune_targets(self) -> np.ndarray:
        """Visits N' of the root children that form the training target (int32, in child order).

        Not forced (k = 0, `forced_on` False) or a terminal root: N.  Otherwise, with T = root visits,
        sq = sqrt(max(T, 1)), Q(c) the root mover's mean value of c (0 when N = 0):
          c* = most visits, lowest index;  S* = Q(c*) + c_puct * P(c*) * sq / (1 + N(c*));  N'(c*) = N(c*)
          every other child with N > 0:
            F = the smallest integer m >= 0 with m * m >= (k * P) * max(T, 1)
            L = N if S* - Q <= 0, else x = (c_puct * P * sq) / (S* - Q) - 1, L = 0 if x < 0 else floor(x) + 1
            N' = min(N, max(N - F, L)), and N' <= 1 -> 0."""
        r = self.nodes[self.root]
        ch = [self.nodes[r.first_child + j] for j in range(r.n_children)]
        N = [int(c.visit_count) for c in ch]
        if not (self.k > 0.0 and self.forced_on) or self.root_terminal():
            return np.array(N, np.int32)
        q = [0.0] * len(ch)
        for j, c in enumerate(ch):
            if c.visit_count > 0:
                mv = c.value_sum / float(c.visit_count)
                q[j] = mv if c.player == r.player else -mv
        return R.prune_targets(N, [float(c.prior) for c in ch], q, int(r.visit_count), self.k, self.c)


def target_policy(tree: ForcedTree, temperature: float, prior_pseudocount: float = 0.0) -> np.ndarray:
    """The 220-d training target of `tree`'s root: O.policy_from_visits over the pruned visits."""
    idx, _vis, _vs, pr, _pl = tree.root_children()
    out = np.zeros(220, np.float32)
    out[idx] = O.policy_from_visits(tree.prune_targets(), temperature, pr, prior_pseudocount)
    return out


# ---- the inputs of the injected-evaluator parity test (tests/test_gpu_forced_playouts.py) and of the CPU test that shows
# ---- they are not vacuous (tests/test_forced_tree_cpu.py): one definition, so that both look at the same roots
PARITY_GAMES, PARITY_SIMS, PARITY_SEED, PARITY_K, PARITY_EPS = 64, 64, 11, 2.0, 0.25


def parity_inputs(with_noise: bool, num_games: int = PARITY_GAMES, seed: int = PARITY_SEED):
    """(states dict of numpy arrays, noise float32[num_games, 80] or None) drawn from g1_rules.npz."""
    from tests.golden_utils import FIELDS, load, states as gstates
    st_all = gstates(load("g1_rules.npz"), "s")
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, st_all["board"].shape[0], num_games)
    states = {f: np.ascontiguousarray(np.asarray(st_all[f])[idx]) for f in FIELDS}
    noise = (rng.gamma(0.3, 1.0, size=(num_games, 80)).astype(np.float32) + np.float32(1e-6)) if with_noise else None
    return states, noise


def search_alone(trees, sims: int, noise=None, eps: float = PARITY_EPS, on_select=None):
    """One search of every tree under tree_parity.hash_evaluator, no GPU: prepare / (re-noise) / `sims` x select +
    complete.  `on_select(i, tree)` is called after every select of tree i.  Returns the forced descents per tree."""
    from tests.tree_parity import hash_evaluator
    before = [t.forced_count for t in trees]

    def complete(pend, is_root):
        need = [i for i, p in enumerate(pend) if p]
        if not need:
            return
        pri, val = hash_evaluator(O.batch_from_states([trees[i].pending_state() for i in need]))
        for j, i in enumerate(need):
            trees[i].complete(pri[j], float(val[j]), noise[i] if (is_root and noise is not None) else None, eps)

    pend = [t.prepare_root() for t in trees]
    complete(pend, True)
    if noise is not None:
        for i, t in enumerate(trees):
            if not pend[i] and not t.root_terminal():
                t.root_noise(noise[i], eps)
    for _ in range(sims):
        pend = []
        for i, t in enumerate(trees):
            pend.append(t.select())
            if on_select is not None:
                on_select(i, t)
        complete(pend, False)
    return [t.forced_count - b for t, b in zip(trees, before)]
