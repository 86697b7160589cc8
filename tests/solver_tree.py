"""Pure-Python variant-P tree with the MCTS-Solver (Winands, Bjornsson, Saito 2008): the checker of the `solver` tests.

`oracle/lz_oracle.c` holds the reference tree of every other parity test and cannot be extended, so this module builds on
the Python restatement of it in tests/forced_tree.py (same method surface as `OracleTree`, forced playouts included, so the
helpers of tests/tree_parity.py drive it unchanged) and adds the solver's three parts.  With `solver=False` (and k = 0) it
must equal `OracleTree` bit for bit (tests/test_solver_tree_cpu.py checks that first).

Notation (LzTreeDesc.solver in include/liuzhou_hip.h).  A node c stands for the edge from its parent X to it.  c is DECIDED
when it is terminal (the game is over there, or it was found to have no legal move) or PROVEN; d(c) in {-1, 0, +1} is its
value for its own mover, x(c) = d(c) if c's mover is X's mover, else -d(c).
    R(X): a decided child with x = +1 -> X is proven +1; otherwise every child decided -> X is proven max x; else undecided.
Marking (`complete`): a leaf expanded into a node X evaluates R(X); a proven X -- or a leaf that turns out to have no legal
move -- is a new decision, and the climb evaluates R on the node above it along the path, marks it if it is proven, and goes
on until a node stays undecided or the root result is set.  The value a simulation backs up is what it is without the solver.
Selection: a child decided with x = +1 is taken (lowest index); otherwise the children decided with x = -1 are no candidates
(unless all are) and a decided child scores with q = x at any visit count; a descent that takes a decided child ends there.
A root level on which the forced-playout rule has a due child keeps that rule.
Pick (`solver_pick`): a proven win is played -- the most visited one, lowest index; a pick that is a proven loss is replaced
by the most visited child that is not one, if there is any.
`solver_count` counts every node the expand step decides (proven, or terminal for want of a legal move) and every root result
it sets."""
import math

import numpy as np

from oracle import lz_oracle as O
from tests import readout_ref as R
from tests.forced_tree import ForcedTree, _terminal_value

INFO_WHITE, INFO_TERMINAL, INFO_PROVEN = 1, 2, 16


class SolverTree(ForcedTree):
    def __init__(self, cs, exploration_weight: float = 1.0, solver: bool = True, forced_k: float = 0.0):
        super().__init__(cs, exploration_weight, forced_k)
        self.solver = bool(solver)
        self.proven = {}                        # node index -> proven value d for the node's own mover
        self.root_proven = 0                    # 0 unknown, 1 lost, 2 drawn, 3 won for the root's mover
        self.solver_count = 0

    # ---- the rule ----
    def decided(self, ni: int) -> bool:
        return bool(self.nodes[ni].terminal) or ni in self.proven

    def d(self, ni: int) -> int:
        n = self.nodes[ni]
        if n.terminal:
            return -1 if n.no_legal_terminal else int(_terminal_value(n.state))
        return int(self.proven[ni])

    def x(self, parent: int, ni: int) -> int:
        d = self.d(ni)
        return d if self.nodes[parent].player == self.nodes[ni].player else -d

    def rule(self, ni: int):
        """R(node): its proven value for its own mover (+1, 0, -1) or None.  Only for an expanded node with children."""
        n = self.nodes[ni]
        kids = range(n.first_child, n.first_child + n.n_children)
        xs = [self.x(ni, c) if self.decided(c) else None for c in kids]
        if any(v == 1 for v in xs):
            return 1
        if any(v is None for v in xs):
            return None
        return max(xs)

    def info_byte(self, ni: int) -> int:
        """The edge info byte the device keeps for this node (bit 0 white, bit 1 terminal, bits 2..3 d + 1, bit 4 proven)."""
        n = self.nodes[ni]
        b = INFO_WHITE if n.player < 0 else 0
        if n.terminal:
            b |= INFO_TERMINAL | (0 if n.no_legal_terminal else (int(_terminal_value(n.state)) + 1) << 2)
        elif ni in self.proven:
            b |= INFO_PROVEN | (int(self.proven[ni]) + 1) << 2
        return b

    def root_infos(self) -> np.ndarray:
        r = self.nodes[self.root]
        return np.array([self.info_byte(r.first_child + j) for j in range(r.n_children)], np.uint8)

    def _root_step(self) -> None:
        r = self.nodes[self.root]
        if self.solver and r.expanded and r.n_children > 0 and not r.terminal:
            p = self.rule(self.root)
            if p is not None:
                self.root_proven = p + 2
                self.solver_count += 1

    # ---- the protocol of OracleTree ----
    def prepare_root(self) -> bool:
        self.root_proven = 0                    # a new search: begin / advance clear the result
        pend = super().prepare_root()
        if not pend:
            self._root_step()                   # a kept root: R over its existing children
        return pend

    def select(self) -> bool:
        if not self.solver:
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
            if cur != self.root and self.decided(cur):
                break                           # a descent that takes a decided edge ends there
            if not (n.expanded and n.n_children > 0 and not n.terminal):
                break
            kids = list(range(n.first_child, n.first_child + n.n_children))
            best_child = -1
            if cur == self.root:
                due = self.due_children()
                if due:
                    self.last_due = due
                    best_child = n.first_child + due[0]
                    self.forced_count += 1
            if best_child < 0:
                xs = [self.x(cur, c) if self.decided(c) else None for c in kids]
                wins = [c for c, v in zip(kids, xs) if v == 1]
                if wins:
                    best_child = wins[0]
                else:
                    cand = [c for c, v in zip(kids, xs) if v != -1] or kids
                    sqrt_total = math.sqrt(float(n.visit_count if n.visit_count > 1 else 1))
                    best = -math.inf
                    for c, v in zip(kids, xs):
                        if c not in cand:
                            continue
                        ch = self.nodes[c]
                        q = 0.0
                        if v is not None:
                            q = float(v)
                        elif ch.visit_count > 0:
                            mv = ch.value_sum / float(ch.visit_count)
                            q = mv if n.player == ch.player else -mv
                        u = self.c * ch.prior * sqrt_total / (1.0 + float(ch.visit_count))
                        score = q + u
                        if score > best:
                            best, best_child = score, c
            if best_child < 0:
                break
            if cur == self.root:
                self.last_root_child = best_child - n.first_child
            cur = best_child
            self.path.append(cur)
        leaf = self.nodes[cur]
        if cur != self.root and self.decided(cur):
            self._backup(float(self.d(cur)))
            return False
        if leaf.expanded and leaf.n_children == 0:
            leaf.terminal = True
            leaf.no_legal_terminal = True
            self._backup(-1.0)
            return False
        self.pending = cur
        self.pending_is_root = False
        return True

    def complete(self, priors220, value, noise=None, epsilon: float = 0.25) -> None:
        ni, is_root, path = self.pending, self.pending_is_root, list(self.path)
        super().complete(priors220, value, noise, epsilon)
        if ni < 0 or not self.solver:
            return
        nd = self.nodes[ni]
        if is_root:
            self._root_step()
            return
        if nd.n_children == 0:
            if not nd.no_legal_terminal:
                return
        else:
            p = self.rule(ni)
            if p is None:
                return
            self.proven[ni] = p
        self.solver_count += 1
        # the climb: path[j] has just been decided; its owner is path[j - 1]
        j = len(path) - 1
        assert path[j] == ni
        while True:
            owner = path[j - 1]
            p = self.rule(owner)
            if p is None:
                return
            if owner == self.root:
                if self.root_proven == 0:
                    self.root_proven = p + 2
                    self.solver_count += 1
                return
            if self.decided(owner):
                return
            self.proven[owner] = p
            self.solver_count += 1
            j -= 1

    def advance(self, action_index: int) -> bool:
        ok = super().advance(action_index)
        if ok:
            self.root_proven = 0
        return ok

    def drop_subtree(self, ni: int) -> None:
        """What a pruning advance does to a kept node: its subtree goes, the marks on the node itself stay."""
        n = self.nodes[ni]
        n.first_child, n.n_children, n.expanded = -1, 0, False

    # ---- the pick ----
    def solver_pick(self, picked_action: int, force_uniform: bool = False) -> int:
        """The action played after lz_tree_solver_pick, given the one the finish picked."""
        r = self.nodes[self.root]
        if not self.solver or force_uniform or self.root_terminal() or not r.expanded:
            return int(picked_action)
        kids = list(range(r.first_child, r.first_child + r.n_children))
        xs = [self.x(self.root, c) if self.decided(c) else None for c in kids]
        return R.solver_pick([self.nodes[c].action_index for c in kids], [self.nodes[c].visit_count for c in kids], xs,
                             picked_action)


# ---- exact values by brute force, and the test positions --------------------------------------------------------------
def brute_value(cs, depth: int):
    """Depth-limited minimax over the oracle's rules: the exact value of `cs` for its mover (+1, 0, -1) as far as `depth`
    edges decide it, else None.  The same three-way rule, applied to the whole game tree instead of a search tree."""
    if O.game_status(cs) != 0:
        return int(_terminal_value(cs))
    idx = O.legal_indices_py(cs)
    if not idx:
        return -1
    if depth <= 0:
        return None
    best, unknown = -2, False
    for a in idx:
        c = O.apply_index(cs, a)
        v = brute_value(c, depth - 1)
        if v is None:
            unknown = True
            continue
        xv = v if int(c.player) == int(cs.player) else -v
        if xv == 1:
            return 1
        best = max(best, xv)
    return None if unknown else best


def winning_children(cs, depth: int):
    """Action indices of `cs` whose child is a proven win for cs's mover within `depth` edges below the child."""
    out = []
    for a in O.legal_indices_py(cs):
        c = O.apply_index(cs, a)
        v = brute_value(c, depth)
        if v is not None and (v if int(c.player) == int(cs.player) else -v) == 1:
            out.append(a)
    return out


POSITION_SEED, POSITION_PLAYOUTS, POSITION_DEPTH = 20261018, 400, 3
_positions_cache = {}


def _winning_move(cs):
    """A removal (or any move) that ends the game in the mover's favour at once, if there is one."""
    for a in O.legal_indices_py(cs):
        c = O.apply_index(cs, a)
        st = O.game_status(c)
        if st in (1, -1) and st == int(cs.player):
            return a
    return None


def solver_positions(seed: int = POSITION_SEED, playouts: int = POSITION_PLAYOUTS, depth: int = POSITION_DEPTH):
    """Positions from seeded random playouts that take a winning move when there is one: the states 1 to 4 plies before an
    elimination and 1 to 3 plies before a draw by the move or no-capture limit, each classified by brute_value(depth):
        "win":  the root is a forced win within `depth` edges and has at least one child that does not win,
        "decided": the root is a proven draw or loss,
        "open": nothing is provable within `depth` edges.
    Returns {"win": [...], "decided": [...], "open": [...]} of CStates (at most 12 / 6 / 6, in playout order)."""
    key = (seed, playouts, depth)
    if key in _positions_cache:
        return _positions_cache[key]
    rng = np.random.default_rng(seed)
    start = O.state_from_batch(O.initial_states(1), 0)
    out = {"win": [], "decided": [], "open": []}
    seen = set()
    for _ in range(playouts):
        cs, hist = start, []
        while O.game_status(cs) == 0:
            idx = O.legal_indices_py(cs)
            if not idx:
                break
            hist.append(cs)
            a = _winning_move(cs)
            if a is None:
                a = idx[int(rng.integers(0, len(idx)))]
            cs = O.apply_index(cs, a)
        st = O.game_status(cs)
        back = range(1, 5) if st in (1, -1) else range(1, 4)
        for b in back:
            if b > len(hist):
                break
            s = hist[-b]
            sig = (tuple(s.board[:]), tuple(s.mb[:]), tuple(s.mw[:]), s.phase, s.player, s.pm_rem, s.pc_rem, s.move_count, s.msc)
            if sig in seen or len(O.legal_indices_py(s)) < 2:
                continue
            seen.add(sig)
            v = brute_value(s, depth)
            if v == 1:
                if len(out["win"]) < 12 and len(winning_children(s, depth - 1)) < len(O.legal_indices_py(s)):
                    out["win"].append(s)
            elif v is not None:
                if len(out["decided"]) < 6:
                    out["decided"].append(s)
            elif len(out["open"]) < 6:
                out["open"].append(s)
        if len(out["win"]) >= 12 and len(out["decided"]) >= 6 and len(out["open"]) >= 6:
            break
    _positions_cache[key] = out
    return out
