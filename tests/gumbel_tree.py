"""Pure-Python variant-P tree with the Gumbel root search and Sequential Halving (Danihelka, Guez, Schrittwieser, Silver:
"Policy improvement by planning with Gumbel", ICLR 2022): the checker of the `gumbel_considered` tests.

Node, backup, expansion and advance are tests/forced_tree.py's (with k = 0 that tree equals oracle.OracleTree bit for bit,
and so does this one with the mode off: tests/test_gumbel_tree_cpu.py checks that first); this module adds the root rule
of include/liuzhou_hip.h (LzTreeDesc.gumbel_*) and keeps `OracleTree`'s method surface, so the helpers of
tests/tree_parity.py drive it unchanged.

The rule takes its transcendental inputs as data: `gl` (g + log P in fp32), `v0` (the root's own value) and the table.
GPU parity runs hand over the device's buffers (`root_step(gl=..., v0=...)`), CPU tests let numpy form them
(`root_step(g=...)`).  Everything after that is Python float (IEEE double) arithmetic of + - * / and comparisons in the
order the header documents: a sum over the children is the per-lane sum of children l and l + 64 (a missing term is
+0.0) followed by an xor butterfly over 64 lanes with offsets 32, 16, 8, 4, 2, 1.  Python does not contract a product and
a sum into one rounding, which the bit-for-bit comparison with the device relies on."""
import math

import numpy as np

from liuzhou_amd.gumbel import considered_table
from tests import readout_ref as R
from tests.forced_tree import ForcedTree, _terminal_value


butterfly_sum = R.butterfly_sum          # the one definition: tests/readout_ref.py


class GumbelTree(ForcedTree):
    def __init__(self, cs, exploration_weight: float = 1.0, considered: int = 0, sims: int = 1, c_visit: float = 50.0,
                 c_scale: float = 1.0, table=None):
        super().__init__(cs, exploration_weight, 0.0)
        self.m, self.n = int(considered), max(1, int(sims))
        self.c_visit, self.c_scale = float(c_visit), float(c_scale)
        self.table = considered_table(self.m, self.n) if table is None else np.asarray(table)
        self.gumbel_on = True                   # the game's root-noise switch (False: a fast search of the playout cap)
        self.gl = None                          # float32 per root child, set by root_step()
        self.base = None                        # N0 per root child
        self.root_base = 0
        self.v0 = 0.0
        self.root_order = []                    # child offsets the descents of this search took at the root, in order
        self.no_candidate = 0                   # descents that found no candidate (fell back to all children)
        self.searches = 0                       # searches whose root step ran the rule
        self._due = None                        # (fresh, inputs) of a root step still to be taken: see feed()
        self._fresh = False

    def active(self) -> bool:
        return self.m > 0 and self.gumbel_on and self.gl is not None

    def prepare_root(self) -> bool:
        self._fresh = super().prepare_root()
        return self._fresh

    def feed(self, g=None, gl=None, v0=None) -> None:
        """Inputs of the NEXT root step, for drivers that know nothing of it (tree_parity.replay_part_in_oracle): the step
        is taken lazily by the first select() after prepare_root() / complete(), i.e. on the root as the root step left
        it."""
        self.gl = None
        self._due = dict(g=g, gl=gl, v0=v0)

    # ---- the root step's snapshot ----
    def root_step(self, fresh: bool, g=None, gl=None, v0=None) -> None:
        """After the root step of a search (`fresh`: the root was expanded in it, else it is a kept root).  Either `g`
        (standard Gumbel variates per child rank; gl is then formed in numpy fp32) or the device's own `gl` row; `v0`
        defaults to the definition: the network value of a fresh root, the mean value of a kept one (0 without visits),
        rounded to fp32."""
        self.gl, self.root_order, self._due = None, [], None
        r = self.nodes[self.root]
        if self.m <= 0 or not self.gumbel_on or r.terminal or not r.expanded or r.n_children <= 0:
            return
        ch = [self.nodes[r.first_child + j] for j in range(r.n_children)]
        if gl is None:
            with np.errstate(divide="ignore"):
                gl = (np.asarray(g, np.float32)[: len(ch)] +
                      np.log(np.array([c.prior for c in ch], np.float32))).astype(np.float32)
        self.gl = np.asarray(gl, np.float32)[: len(ch)].copy()
        self.base = [int(c.visit_count) for c in ch]
        self.root_base = int(r.visit_count)
        if v0 is None:
            v0 = r.initial_value if fresh else (r.value_sum / float(r.visit_count) if r.visit_count > 0 else 0.0)
        self.v0 = float(np.float32(v0))
        self.searches += 1

    # ---- the completed values ----
    def scores(self):
        """(score, sigma, vmix, L) of the root children as the statistics stand: lists in child order, vmix a float."""
        r = self.nodes[self.root]
        ch = [self.nodes[r.first_child + j] for j in range(r.n_children)]
        N = [int(c.visit_count) for c in ch]
        P = [float(c.prior) for c in ch]
        q = []
        for c in ch:
            if c.visit_count > 0:
                mv = c.value_sum / float(c.visit_count)
                q.append(mv if c.player == r.player else -mv)
            else:
                q.append(0.0)
        return R.gumbel_scores(N, P, q, self.gl, self.base, self.v0, self.c_visit, self.c_scale)

    _argmax = staticmethod(R.gumbel_argmax)

    def root_choice(self) -> int:
        """The child offset the Gumbel rule takes at the root right now."""
        r = self.nodes[self.root]
        score, _sigma, _vmix, L = self.scores()
        s = int(r.visit_count) - self.root_base
        j = min(self.m, r.n_children)
        cv = int(self.table[j][min(max(s, 0), self.n - 1)])
        cand = [k for k in range(r.n_children) if L[k] == cv]
        if not cand:
            self.no_candidate += 1
            cand = list(range(r.n_children))
        return self._argmax(score, cand)

    def select(self) -> bool:
        if self._due is not None:
            self.root_step(self._fresh, **self._due)
        if not self.active():
            return super().select()
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
                k = self.root_choice()
                if k >= 0:
                    best_child = n.first_child + k
            else:
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
                self.root_order.append(self.last_root_child)
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

    def advance(self, action_index: int) -> bool:
        self.gl = None                           # the next search's root step sets it again
        return super().advance(action_index)

    # ---- finish ----
    def gumbel_finish(self):
        """(pick child offset, target float32[220], score float64[ne], vmix) of a Gumbel game with a live root."""
        r = self.nodes[self.root]
        ch = [self.nodes[r.first_child + k] for k in range(r.n_children)]
        q = [(c.value_sum / float(c.visit_count)) * (1.0 if c.player == r.player else -1.0) if c.visit_count > 0 else 0.0
             for c in ch]
        pick, probs, score, vmix = R.gumbel_finish([int(c.visit_count) for c in ch], [float(c.prior) for c in ch], q, self.gl,
                                                   self.base, self.v0, self.c_visit, self.c_scale)
        target = np.zeros(220, np.float32)
        for k, c in enumerate(ch):
            target[c.action_index] = probs[k]
        return pick, target, score, vmix


def rng_gumbel(seed: int, game, ply, count: int):
    """(u, g) float32[B, count]: lz_rng.h::gumbel_draw restated over oracle/rng_oracle.draw -- the first word of the block
    (purpose 3, index 1 + k, attempt 0), u = ((float)(x >> 9) + 0.5f) * 2^-23 in fp32, g = -log(-log(u)) with both logarithms
    in double, rounded to fp32 once."""
    from oracle import rng_oracle as R
    game = np.asarray(game, np.int64).reshape(-1)
    ply = np.broadcast_to(np.asarray(ply, np.int64), game.shape)
    k = np.arange(int(count), dtype=np.int64)
    x = R.draw(seed, game[:, None], ply[:, None], 3, 1 + k[None, :], 0)[:, 0].reshape(game.shape[0], int(count))
    u = ((x >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    g = (-np.log(-np.log(u.astype(np.float64)))).astype(np.float32)
    return u.astype(np.float32), g.astype(np.float32)


# ---- the inputs of the injected-evaluator parity test (tests/test_gpu_gumbel.py) and of the CPU tests: one definition
PARITY_GAMES, PARITY_SIMS, PARITY_SEED = 64, 64, 11


def parity_inputs(num_games: int = PARITY_GAMES, seed: int = PARITY_SEED):
    """(states dict of numpy arrays, g float32[num_games, 80] standard Gumbel variates) drawn from g1_rules.npz."""
    from tests.forced_tree import parity_inputs as forced_inputs
    states, _ = forced_inputs(False, num_games=num_games, seed=seed)
    g = np.random.default_rng(seed + 1000).gumbel(size=(num_games, 80)).astype(np.float32)
    return states, g


def search_alone(trees, sims: int, g, evaluator=None, fresh_only: bool = False):
    """One search of every tree under `evaluator` (default tree_parity.hash_evaluator), no GPU: prepare / root step /
    `sims` x select + complete."""
    from oracle import lz_oracle as O
    from tests.tree_parity import hash_evaluator
    evaluate = evaluator or hash_evaluator

    def complete(pend):
        need = [i for i, p in enumerate(pend) if p]
        if not need:
            return
        pri, val = evaluate(O.batch_from_states([trees[i].pending_state() for i in need]))
        for j, i in enumerate(need):
            trees[i].complete(pri[j], float(val[j]))

    pend = [t.prepare_root() for t in trees]
    complete(pend)
    for i, t in enumerate(trees):
        t.root_step(pend[i], g=g[i])
    for _ in range(sims):
        complete([t.select() for t in trees])
