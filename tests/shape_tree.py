"""Pure-Python variant-P tree with first-play urgency and the visit-scaled exploration constant: the checker of the
`puct_shape` tests (LzTreeDesc.puct_shape in include/liuzhou_hip.h).

Builds on tests/solver_tree.py (and through it on tests/forced_tree.py), so it has the method surface of `OracleTree`, the
forced playouts and the solver, and the helpers of tests/tree_parity.py drive it unchanged.  With the shape off it must equal
`SolverTree` and `ForcedTree` bit for bit (tests/test_shape_tree_cpu.py checks that first).

On a level at node v that PUCT decides (a forced root level and a child the solver takes outright are decided before):
    n_v  = v's visit count (the root's, or the count on the edge that leads to v)
    c    = table[min(n_v, len - 1)] with table = liuzhou_amd.puct_shape.cpuct_table(...) -- the same function the engine
           uploads the result of -- or c_puct while cpuct_log == 0
    V    = W_v / n_v, or v's network value (as float32) while n_v == 0
    S    = sum over the children with n > 0 of int(float(P) * 2^30)
    f    = max(V - r * sqrt(S / 2^30), -1.0), r = fpu_root_reduction at the root, fpu_reduction below it
    q(k) = x(k) for a child the solver has decided, +-W/n for a visited one, f for an unvisited one (0 while FPU is off)
    score = q + c * P * sqrt(max(n_v, 1)) / (1 + n), lowest index among equals.
`prune_targets` is ForcedTree's rule with c(T), T = the root's visit count, wherever that has c_puct."""
import math

import numpy as np

from liuzhou_amd.puct_shape import CPUCT_TABLE_LEN, cpuct_table, parse_puct_shape
from tests.solver_tree import SolverTree

FIX = float(1 << 30)

# the three settings of the issue's table; the base is small because with 19652 the table hardly moves within 64 visits
SETTINGS = {
    "fpu": dict(fpu_reduction=0.2, fpu_root_reduction=0.1),
    "table": dict(cpuct_log=1.0, cpuct_base=8.0),
    "both": dict(fpu_reduction=0.2, fpu_root_reduction=0.1, cpuct_log=1.0, cpuct_base=8.0),
}
# both clamps: the FPU value at -1 and the table at its last entry
CLAMPS = dict(fpu_reduction=1.5, fpu_root_reduction=1.5, cpuct_log=1.0, cpuct_base=8.0, table_len=16)

_tables = {}


def shared_table(c_puct, cpuct_log, cpuct_base, length):
    key = (float(c_puct), float(cpuct_log), float(cpuct_base), int(length))
    if key not in _tables:
        _tables[key] = cpuct_table(*key)
    return _tables[key]


class ShapedTree(SolverTree):
    def __init__(self, cs, exploration_weight: float = 1.0, solver: bool = False, forced_k: float = 0.0,
                 fpu_reduction=None, fpu_root_reduction=None, cpuct_log: float = 0.0, cpuct_base: float = 19652.0,
                 table_len: int = CPUCT_TABLE_LEN):
        super().__init__(cs, exploration_weight, solver, forced_k)
        self.shape = parse_puct_shape(fpu_reduction, fpu_root_reduction, cpuct_log, cpuct_base)
        self.table = shared_table(self.c, cpuct_log, cpuct_base, table_len) if self.shape.table else None
        self.fpu_clamped = 0                    # levels whose f was clamped at -1
        self.table_clamped = 0                  # levels whose n_v lay beyond the table's last entry

    def c_of(self, n_v: int) -> float:
        if self.table is None:
            return self.c
        return self.table[min(max(int(n_v), 0), len(self.table) - 1)]

    def fpu_value(self, ni: int) -> float:
        """f of node ni as its statistics stand."""
        n = self.nodes[ni]
        V = n.value_sum / float(n.visit_count) if n.visit_count > 0 else float(np.float32(n.initial_value))
        S = 0
        for c in range(n.first_child, n.first_child + n.n_children):
            ch = self.nodes[c]
            if ch.visit_count > 0:
                S += int(float(ch.prior) * FIX)
        r = self.shape.fpu_root_reduction if ni == self.root else self.shape.fpu_reduction
        red = r * math.sqrt(float(S) / FIX)
        f = V - red
        if f < -1.0:
            f = -1.0
            self.fpu_clamped += 1
        return f

    def select(self) -> bool:
        if not self.shape.on:
            return super().select()
        dec = self.decided if self.solver else (lambda c: False)
        self.pending = -1
        self.last_due, self.last_root_child = [], -1
        root = self.nodes[self.root]
        if root.terminal:
            return False
        cur = self.root
        self.path = [cur]
        while True:
            n = self.nodes[cur]
            if cur != self.root and dec(cur):
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
                xs = [self.x(cur, c) if dec(c) else None for c in kids]
                wins = [c for c, v in zip(kids, xs) if v == 1]
                if wins:
                    best_child = wins[0]
                else:
                    cand = set(c for c, v in zip(kids, xs) if v != -1) or set(kids)
                    c_level = self.c_of(n.visit_count)
                    if self.table is not None and n.visit_count > len(self.table) - 1:
                        self.table_clamped += 1
                    sqrt_total = math.sqrt(float(n.visit_count if n.visit_count > 1 else 1))
                    f = None
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
                        elif self.shape.fpu:
                            if f is None:
                                f = self.fpu_value(cur)
                            q = f
                        u = c_level * ch.prior * sqrt_total / (1.0 + float(ch.visit_count))
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
        if cur != self.root and dec(cur):
            self._backup(float(self.d(cur)))
            return False
        if leaf.terminal:
            from tests.forced_tree import _terminal_value
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

    def prune_targets(self) -> np.ndarray:
        """ForcedTree.prune_targets with c(T) for c_puct, T = the root's visit count (not clamped at 1); first-play urgency
        does not enter: the rule only looks at visited children."""
        if self.table is None:
            return super().prune_targets()
        keep = self.c
        self.c = self.c_of(int(self.nodes[self.root].visit_count))
        try:
            return super().prune_targets()
        finally:
            self.c = keep


def make_trees(states, setting, c=1.0, solver=False, forced_k=0.0):
    """One ShapedTree per row of a state dict (`setting`: keyword arguments of ShapedTree, e.g. SETTINGS["fpu"])."""
    from oracle import lz_oracle as O
    n = np.asarray(states["board"]).shape[0]
    return [ShapedTree(O.state_from_batch(states, i), c, solver=solver, forced_k=forced_k, **setting) for i in range(n)]


def root_visit_vectors(trees):
    return [tuple(int(v) for v in t.root_children()[1]) if not t.root_terminal() else None for t in trees]
