"""Hand-built launches for lz_tree_select / lz_tree_expand: real skeletons with hand statistics
(tests/hand_arenas.py StepGame), seeded and tagged.  Every launch is a mix -- deep and shallow games, one inactive game, one
game with root_terminal set and one whose descent ends on an all-NaN level -- and B is never a multiple of 4, so the waves of
a workgroup differ and the last workgroup is partly filled.

A launch is a dict: name, img, opts (tests/step_ref.options), steps.  A step is ("select",), ("expand", rows, is_root) or
("hand", f) with f(image) -> image, applied to what the previous step left (on the restatement's side in the CPU tests, on
the device's in the GPU tests).  `plain`: the descent is plain PUCT, so the launch is rerun with LZ_TREE_F32SEL=1."""
import functools

import numpy as np

from tests import hand_arenas as H
from tests.step_ref import options

F32 = np.float32
DEEP_SEEDS = (3, 5, 6, 7)           # 144-ply lines with same-mover edges on both sides of entry 64
WIN_SEED = 10                       # a line that ends in a win after 126 plies; every child of its ply 125 is finished
PATH_LENS = (1, 2, 63, 64, 65, 66, 127, 128, 129, 143)
VALUES = (1.0, -1.0, 0.0, 0.3, -0.0)


@functools.lru_cache(maxsize=None)
def line_of(seed):
    return H.playout(seed)


def position(seed, ply, need=4):
    """The first open position of the line at or after `ply` with at least `need` legal moves."""
    from oracle import lz_oracle as O
    line = line_of(seed)[0]
    return next(c for c in line[ply:-1] if len(O.legal_indices_py(c)) >= need)


class StepGame(H.StepGame):
    """H.StepGame plus what the evaluator rows of this game hold: `value`, `row` (None, or how the prior row is spoilt)."""

    def __init__(self, tag, root, fresh=False, value=0.3, row=None, **scalars):
        super().__init__(tag, root, fresh=fresh, **scalars)
        self.value, self.row = value, row


def decorate(g, levels, rng):
    """Off-path statistics: on every level one other child with a visit and a poor mean, so that W of both signs and
    visited siblings are on the way."""
    for node, slot in levels:
        n = len(g.nodes[node]["act"])
        if n > 1:
            o = (slot + 1 + int(rng.integers(n - 1))) % n
            if not g.nodes[node]["info"][o] & H.INFO_TERMINAL:
                g.steer(node, o, q=-0.5, n=1)


def deep_game(tag, seed, L, end="expand", value=0.3, d=0, rng=None):
    """A chain of L edges along the line of `seed`.  end: 'expand' (the last edge has no node), 'terminal' / 'decided' (the
    last edge carries a terminal / proven mark with value d, set by hand), 'real' (L is the whole line: the last child is
    finished and the edge carries what the expand step wrote)."""
    line, acts = line_of(seed)
    g = StepGame(tag, line[0], value=value)
    lv = g.line(acts[:L])
    decorate(g, lv[:-1], rng or np.random.default_rng(L))
    node, slot = lv[-1]
    if end == "terminal":
        g.nodes[node]["info"][slot] |= H.INFO_TERMINAL | ((d + 1) << 2)
    elif end == "decided":
        g.nodes[node]["info"][slot] |= H.INFO_PROVEN | ((d + 1) << 2)
    elif end == "real":
        assert L == len(acts) and g.nodes[node]["info"][slot] & H.INFO_TERMINAL
    g.levels = lv
    return g


def decide(g, node, slot, x, proven=True):
    """Mark (node, slot) decided with value x for the node's mover."""
    nd = g.nodes[node]
    same = (-1 if nd["info"][slot] & H.INFO_WHITE else 1) == nd["cs"].player
    d = x if same else -x
    nd["info"][slot] = (nd["info"][slot] & H.INFO_WHITE) | (H.INFO_PROVEN if proven else H.INFO_TERMINAL) | ((d + 1) << 2)


def extras(seed):
    """The three games every mix holds."""
    a = StepGame("extra:inactive", position(1, 20), active=0, root_terminal=1)
    a.line(line_of(1)[1][20:23])
    b = StepGame("extra:root_terminal", position(2, 30), root_terminal=1)
    b.line(line_of(2)[1][30:32])
    c = StepGame("extra:nan_depth3", position(4, 10))
    lv = c.line(line_of(4)[1][10:14])
    node = lv[3][0]
    c.nodes[node]["P"][:] = np.nan
    c.nodes[node]["N"][:], c.nodes[node]["W"][:] = 0, 0.0
    return [a, b, c]


def rows_for(img, specs, seed, heads=False, noise=False, epsilon=0.25):
    """Evaluator rows of a launch: seeded positive priors (or normal head logits), per game its value and its spoilt row."""
    rng = np.random.default_rng(seed)
    B = img["B"]
    r = dict(values=np.array([s[0] for s in specs], F32), epsilon=epsilon)
    pri = (rng.random((B, 220)) + 0.01).astype(F32)
    hd = [rng.normal(0, 2, (B, 36)).astype(F32) for _ in range(3)]
    for g, (_, row) in enumerate(specs):
        if row == "zero":
            pri[g] = 0
        elif isinstance(row, tuple) and row[0] == "nan":              # one NaN among good values, on a legal action
            pri[g, row[1]] = np.nan
        elif row == "inf":
            pri[g, ::5] = np.inf
        elif row == "negative":
            pri[g] = -pri[g]
        elif row == "minus_inf":
            for h in hd:
                h[g] = -np.inf
        elif row == "huge":
            for h in hd:
                h[g] *= F32(1e37)
        elif row == "very_negative":
            for h in hd:
                h[g] = -np.abs(h[g]) * F32(1e30)
        elif row == "one_hot":
            hd[0][g, 7] = hd[1][g, 7] = hd[2][g, 7] = F32(3e4)
    if heads:
        r["heads"] = tuple(hd)
    else:
        r["priors220"] = pri
    if noise:
        r["noise"] = rng.dirichlet(np.full(72, 0.3), B).astype(F32)
    return r


def make(name, games, node_cap, chunk, seed, opts=None, plain=False, spare=8):
    assert len(games) % 4 != 0, name
    img = H.build_step_image(games, node_cap, chunk, seed, spare_chunks=spare + len(games))   # a chunk for every game and more
    img["hand_index"] = set()
    return dict(name=name, img=img, opts=opts or options(), specs=[(g.value, g.row) for g in games], plain=plain, steps=[])


def step_pair(L, seed, **kw):
    return [("select",), ("expand", rows_for(L["img"], L["specs"], seed, **kw), False)]


# ---- deep lines -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deep(solver=False):
    rng = np.random.default_rng(5 if solver else 4)
    games = []
    for i, L in enumerate(PATH_LENS):
        seed = DEEP_SEEDS[i % len(DEEP_SEEDS)]
        if solver:
            end = ("decided", "expand", "terminal")[i % 3]
        else:
            end = ("expand", "terminal")[i % 2]
        if L == 143:                      # the leaf at ply 143: every child finished and drawn, movers of both colours
            seed, end = DEEP_SEEDS[3], "expand"
        games.append(deep_game(f"deep:{L}:{end}", seed, L, end, value=VALUES[i % len(VALUES)], d=(i % 3) - 1, rng=rng))
    # whole lines: a real finished child at the end (a draw after 144 plies, a win after 126), and the leaf one ply before
    # the end, whose children are all finished
    games.append(deep_game("deep:144:real", DEEP_SEEDS[1], 144, "real", rng=rng))
    games.append(deep_game("deep:126:real", WIN_SEED, 126, "real", rng=rng))
    games.append(deep_game("deep:125:all_children_finished", WIN_SEED, 125, "expand", value=-0.0, rng=rng))
    games.append(deep_game("deep:100:expand", DEEP_SEEDS[3], 100, "expand", value=-1.0, rng=rng))
    games += extras(1)
    L = make("deep_solver" if solver else "deep", games, 300, 128, 17, options(solver=solver), plain=not solver)
    L["steps"] = step_pair(L, 21) + step_pair(L, 22, heads=True) + step_pair(L, 23)
    return L


# ---- descent decisions ------------------------------------------------------------------------------------------------
def wide_game(tag, tie, seed=3, ply=40, n=72, **kw):
    """A synthetic run of n edges below the root's steered edge; the edges `tie` share the best score."""
    line, acts = line_of(seed)
    g = StepGame(tag, line[ply], **kw)
    s = g.slot_of(0, acts[ply])
    g.steer(0, s)
    w = g.synthetic(0, s, n, terminal_values=(-1, 0, 1))
    g.nodes[w]["P"][:] = F32(0.001)
    for k in tie:
        g.nodes[w]["P"][k] = F32(0.25)
    g.wide = w
    return g


def tie_game(tag, tie, seed, ply):
    g = StepGame(tag, position(seed, ply))
    nd = g.nodes[0]
    assert len(nd["act"]) > max(tie)
    nd["P"][:] = F32(0.01)
    for k in tie:
        nd["P"][k] = F32(0.3)
    return g


@functools.lru_cache(maxsize=None)
def descent():
    games = [tie_game("tie:0,1", (0, 1), 3, 50), wide_game("tie:5,63", (5, 63)), wide_game("tie:63,64", (63, 64)),
             wide_game("tie:64,71", (64, 71), n=72), wide_game("tie:64,70:of71", (64, 70), n=71),
             wide_game("wide:65:last", (64,), n=65)]
    # W of -0.0 against +0.0 at equal counts and priors: equal scores, the lower index wins; the backup adds to -0.0
    g = tie_game("negzero", (1, 2), 5, 60)
    g.nodes[0]["N"][1] = g.nodes[0]["N"][2] = 2
    g.nodes[0]["W"][1], g.nodes[0]["W"][2] = -0.0, 0.0
    g.value = -0.0
    games.append(g)
    games.append(tie_game("tie:2,3", (2, 3), 6, 70))
    # a NaN level at depth 0; a level with one NaN score among real ones (the NaN is never the maximum)
    g = StepGame("nan_depth0", position(7, 33))
    g.nodes[0]["P"][:] = np.nan
    games.append(g)
    g = tie_game("one_nan", (2,), 7, 44)
    g.nodes[0]["P"][0] = np.nan
    games.append(g)
    # the single-precision argmax: a lead just inside and just outside its 1e-4 (1 + |s|) margin, |W / n| > 1, one child
    for tag, lead in (("f32:inside", 0.9e-4), ("f32:outside", 1.2e-4)):
        g = StepGame(tag, position(5, 52))
        nd = g.nodes[0]
        nd["P"][:] = F32(0.0)
        nd["N"][0] = nd["N"][1] = 1
        same = [(-1 if nd["info"][k] & H.INFO_WHITE else 1) == nd["cs"].player for k in (0, 1)]
        nd["W"][0], nd["W"][1] = (0.5 if same[0] else -0.5), (1 if same[1] else -1) * (0.5 + lead * 1.5)
        games.append(g)
    g = tie_game("f32:off_scale", (0,), 6, 58)
    g.nodes[0]["N"][1], g.nodes[0]["W"][1] = 1, 1.5
    games.append(g)
    line, acts = line_of(0)
    g = StepGame("single_child", line[36])
    assert len(g.nodes[0]["act"]) == 1
    games.append(g)
    games += extras(2)
    L = make("descent", games, 220, 1024, 31, plain=True)
    L["steps"] = step_pair(L, 32) + step_pair(L, 33) + step_pair(L, 34)
    return L


@functools.lru_cache(maxsize=None)
def big_n():
    """N = 2^24 - 2 under every info bit a live edge can carry, with the solver off (the proven mark is then only carried
    along).  One step: a second visit would carry into the info byte."""
    games = []
    for k, bits in enumerate((0, H.INFO_PROVEN | (2 << 2), H.INFO_PROVEN | (1 << 2))):
        g = StepGame(f"bigN:{bits}", position(6, 70 + k), value=VALUES[k + 2])
        g.steer(0, 0, q=0.9, n=(1 << 24) - 2)
        g.nodes[0]["info"][0] |= bits
        games.append(g)
    games.append(tie_game("tie:0,1", (0, 1), 3, 50))
    games += extras(11)
    L = make("big_n", games, 220, 1024, 35, plain=True)
    L["steps"] = step_pair(L, 36)
    return L


@functools.lru_cache(maxsize=None)
def forced():
    """k = 2, root visits 16, N = 4: N * N == (k * P) * n at P = 0.5 exactly (not due), one float32 ulp above 0.5 due, one
    below not due.  The due child has a poor mean, so PUCT alone would not take it."""
    games = []
    for tag, P in (("forced:equal", F32(0.5)), ("forced:ulp_above", np.nextafter(F32(0.5), F32(1))),
                   ("forced:ulp_below", np.nextafter(F32(0.5), F32(0))), ("forced:unvisited", F32(0.9))):
        g = StepGame(tag, position(3, 48), root_visits=16)
        assert len(g.nodes[0]["act"]) >= 3
        g.steer(0, 0, q=0.9, n=3)
        g.steer(0, 2, q=-0.9, n=0 if tag.endswith("unvisited") else 4)
        g.nodes[0]["P"][2] = P
        games.append(g)
    w = wide_root("forced:wide:due_at_66", kept_root=False, root_visits=16)   # the upper ballot: nothing due below edge 64
    w.nodes[0]["N"][66] = w.nodes[0]["N"][70] = 4
    w.nodes[0]["P"][66] = w.nodes[0]["P"][70] = F32(0.9)
    games.append(w)
    games += extras(3)
    games.append(tie_game("tie:0,1", (0, 1), 3, 50))
    L = make("forced", games, 220, 1024, 41, options(forced_k=2.0))
    L["steps"] = step_pair(L, 42) + step_pair(L, 43)
    return L


@functools.lru_cache(maxsize=None)
def solver():
    games = []
    g = StepGame("solver:win_in_slot1", position(5, 50))               # a win in slot 1 behind losses
    decide(g, 0, 0, -1)
    decide(g, 0, 1, +1)
    g.nodes[0]["P"][0] = F32(0.9)
    games.append(g)
    g = StepGame("solver:every_child_lost", position(5, 51))
    for k in range(len(g.nodes[0]["act"])):
        decide(g, 0, k, -1, proven=k % 2 == 0)
        g.nodes[0]["N"][k] = 1 + k % 3
    games.append(g)
    g = StepGame("solver:draw_vs_open", position(6, 53))                # a decided draw (q = 0 at any count) against q = 0.3
    decide(g, 0, 0, 0)
    g.nodes[0]["N"][0], g.nodes[0]["W"][0] = 5, 4.0
    g.steer(0, 1, q=0.3, n=2)
    games.append(g)
    g = StepGame("solver:draw_wins", position(6, 54))                   # ... and against q = -0.3
    decide(g, 0, 0, 0)
    g.steer(0, 1, q=-0.3, n=2)
    g.nodes[0]["P"][:] = F32(0.0)
    games.append(g)
    games.append(wide_game("solver:wide:win_at_70", (5,)))              # the upper ballot of the win test
    w = games[-1]
    for k in range(72):
        decide(w, w.wide, k, -1 if k < 64 else 0, proven=False)
    decide(w, w.wide, 70, +1, proven=False)
    games.append(wide_game("solver:wide:losses_below_64", (3, 66)))     # candidates only in the upper slot
    w = games[-1]
    for k in range(64):
        decide(w, w.wide, k, -1, proven=False)
    for k in range(64, 72):
        decide(w, w.wide, k, 0, proven=False)
    games.append(leaf_game("nolegal:below_root", 20, value=0.5))
    games += extras(4)
    L = make("solver", games, 220, 1024, 51, options(solver=True))
    first = step_pair(L, 52)
    L["steps"] = [first[0], ("hand", _block), first[1]] + step_pair(L, 53)
    return L


@functools.lru_cache(maxsize=None)
def shape():
    """fpu 0.5 below the root and 0.25 at it, a c(n_v) table of four entries (1 + ln((n_v + 3) / 2): 1.41 .. 2.10)."""
    games = []
    g = StepGame("shape:n_v=0", position(3, 45), root_visits=0, root_init_value=F32(-0.4), root_w=0.0)   # V = root_init_value
    g.nodes[0]["N"][1], g.nodes[0]["W"][1] = 1, -0.45
    games.append(g)
    g = StepGame("shape:clamp", position(3, 46), root_visits=9, root_w=-8.5)      # V = -0.944, f < -1: clamped
    nd = g.nodes[0]
    nd["P"][:] = F32(0.001)
    nd["N"][0], nd["P"][0] = 9, F32(0.9)                                        # S = 0.9: f = -0.944 - 0.25 * 0.949 < -1
    same = (-1 if nd["info"][0] & H.INFO_WHITE else 1) == nd["cs"].player
    nd["W"][0] = -14.4 if same else 14.4        # scores -1.06: under the clamped -0.99 of an unvisited child, over the raw -1.17
    games.append(g)
    g = StepGame("shape:table_last", position(3, 47), root_visits=1000, root_w=100.0)
    g.steer(0, 1, q=0.2, n=400)
    games.append(g)
    g = wide_game("shape:wide_S", (), root_visits=5, root_w=1.0)               # S from members of both slots
    nd = g.nodes[g.wide]
    nd["P"][:] = F32(1.0 / 72)
    for k in (3, 40, 66, 70):
        nd["N"][k], nd["W"][k] = 2, (0.2 if k < 64 else -0.2)
    games.append(g)
    games.append(deep_game("shape:deep", DEEP_SEEDS[2], 20, "expand"))
    games.append(tie_game("shape:tie:0,1", (0, 1), 3, 50))
    games += extras(5)
    L = make("shape", games, 220, 1024, 61, options(fpu=0.5, fpu_root=0.25, cpuct=(1.0, 2.0, 4)))
    L["steps"] = step_pair(L, 62) + step_pair(L, 63)
    return L


# ---- expansion --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def leaf_with(n):
    """(state, action) whose successor is an open position with exactly n legal moves."""
    from oracle import lz_oracle as O
    for seed in range(40):
        line, acts = line_of(seed)
        for j in range(len(acts)):
            if O.game_status(line[j + 1]) == 0 and len(O.legal_indices_py(line[j + 1])) == n:
                return line[j], acts[j]
    raise AssertionError(n)


def leaf_game(tag, n, **kw):
    st, a = leaf_with(n)
    from oracle import lz_oracle as O
    g = StepGame(tag, st, **kw)
    g.steer(0, g.slot_of(0, a))
    g.leaf_slot = g.slot_of(0, a)
    if g.row == "nan":                                                # the middle one of the leaf's legal actions
        g.row = ("nan", O.legal_indices_py(O.apply_index(st, a))[n // 2])
    return g


def ballast_game(tag, n, cursor, **kw):
    """A leaf with n legal moves below a root whose other edges carry synthetic ballast runs, so that the game's edge
    cursor stands at `cursor` (inside its first chunk) when the leaf expands."""
    g = leaf_game(tag, n, **kw)
    left = cursor - len(g.nodes[0]["act"])
    slots = [k for k in range(len(g.nodes[0]["act"])) if k != g.leaf_slot and not g.nodes[0]["info"][k] & H.INFO_TERMINAL]
    assert left >= 0
    while left > 0:
        m = min(left, 72)
        g.synthetic(0, slots.pop(), m, terminal_values=(1, -1, 0))
        left -= m
    return g


@functools.lru_cache(maxsize=None)
def expansion(heads=False):
    games = []
    rows = ("minus_inf", "huge", "very_negative", "one_hot") if heads else ("zero", "inf", "nan", "negative")
    for n, row in zip((1, 2, 35, 20), rows):
        games.append(leaf_game(f"leaf:n={n}:{row}", n, row=row, value=VALUES[n % 5]))
    games.append(leaf_game("leaf:n=2:good", 2))
    games.append(leaf_game("leaf:n=35:good", 35))
    n = 20
    games.append(ballast_game("alloc:exact_fit", n, 128 - n))
    games.append(ballast_game("alloc:one_over", n, 128 - n + 1))
    games.append(ballast_game("alloc:off_zero", n, 128))
    games.append(ballast_game("alloc:one_under", n, 128 - n - 1))
    games.append(leaf_game("nolegal:below_root", 20, value=0.5))
    games += extras(6)
    L = make("expansion_heads" if heads else "expansion", games, 200, 128, 71, plain=True, spare=12)
    first = step_pair(L, 72, heads=heads)
    L["steps"] = [first[0], ("hand", _block), first[1]] + step_pair(L, 73, heads=heads) + step_pair(L, 74, heads=heads)
    return L


def _drain(img):
    """Every free chunk taken away by hand: the expansions that need a new chunk are refused."""
    out = H.copy_image(img)
    out["saved_top"] = int(out["pool_top"][0])
    out["pool_top"][0] = int(out["pool_stats"][2])
    return out


def _refill(img):
    out = H.copy_image(img)
    out["pool_top"][0] = out.pop("saved_top")
    return out


@functools.lru_cache(maxsize=None)
def refusal():
    """Pool empty: the games that need a chunk are refused (the value is still backed up, pool_stats[0] counts them), the
    one whose run fits its open chunk expands; after the chunks are back the same leaves expand on the next visit."""
    n = 20
    games = [ballast_game("refused:one_over", n, 128 - n + 1), ballast_game("refused:off_zero", n, 128),
             ballast_game("fits:exact_fit", n, 128 - n, value=-1.0), ballast_game("refused:one_over:b", 2, 127)]
    games += extras(7)
    L = make("refusal", games, 200, 128, 81, plain=True)
    L["steps"] = [("hand", _drain)] + step_pair(L, 82) + [("hand", _refill)] + step_pair(L, 83)
    return L


@functools.lru_cache(maxsize=None)
def blocked_position():
    """A position without a legal move and not finished.  The rules offer none that play reaches (none in the random
    playouts of 60 seeds; a blocked mover of the movement phase removes a piece instead), so this one is made by hand, the
    nearest there is: the placement phase on a full board.  The step only enumerates its legal moves; nothing is applied."""
    from oracle import lz_oracle as O
    c = O.CState.from_buffer_copy(line_of(3)[0][30])
    for i in range(36):
        c.board[i], c.mb[i], c.mw[i] = (1 if (i // 6 + i % 6) % 2 == 0 else -1), 0, 0
    c.phase, c.player, c.move_count = 1, 1, 36
    c.pm_req = c.pm_rem = c.pc_req = c.pc_rem = c.forced = 0
    assert O.game_status(c) == 0 and O.legal_indices_py(c) == []
    return c


def _block(img):
    """The leaf of the games tagged nolegal replaced by the blocked position, as if the descent had reached it."""
    out = H.copy_image(img)
    for g, tag in enumerate(img["tags"]):
        if tag.startswith("nolegal") and int(out["leaf_kind"][g]) == H.LEAF_EXPAND:
            out["leaf_state"][g] = H.packed_from_cs(blocked_position())
    return out


def _share(img):
    """What the descent of a search leaves for a leaf whose position the tree already holds (the look-ups are off in
    lz_tree_select): leaf_kind shared and the source node, for the games tagged shared."""
    out = H.copy_image(img)
    for g, tag in enumerate(img["tags"]):
        if tag.startswith("shared") and int(out["leaf_kind"][g]) == H.LEAF_EXPAND:
            nn = int(out["n_nodes"][g])
            src = [i for i in range(1, nn) if (out["nodes"][g, i]["state"] == out["leaf_state"][g]).all()]
            if src:
                out["leaf_kind"][g], out["leaf_src"][g] = H.LEAF_SHARED, src[0]
    return out


def _fill_window(img):
    """The 64-slot window of the leaf's position filled by hand with entries in [1, n_nodes)."""
    from tests.advance_ref import pos_hash
    out = H.copy_image(img)
    for g, tag in enumerate(img["tags"]):
        if tag.startswith("full_window"):
            h, mask = pos_hash(out["leaf_state"][g]), out["pos_slots"] - 1
            for p in range(H.WAVE):
                out["pos_index"][g, (h + p) & mask] = 1
            out["hand_index"] = out["hand_index"] | {g}
    return out


def shared_game(tag, n=20, **kw):
    """A leaf whose position another node of the tree holds: the twin hangs from a synthetic run below another root edge
    and carries priors and a node_value of its own."""
    from oracle import lz_oracle as O
    g = leaf_game(tag, n, **kw)
    st, a = leaf_with(n)
    other = next(k for k in range(len(g.nodes[0]["act"])) if k != g.leaf_slot and not g.nodes[0]["info"][k] & H.INFO_TERMINAL)
    s = g.synthetic(0, other, 3, terminal_values=(0,))
    t = g.attach(s, 1, O.apply_index(st, a), value=F32(0.7123))
    rng = np.random.default_rng(n)
    p = rng.random(n).astype(F32)
    g.nodes[t]["P"][:] = p / p.sum(dtype=F32)
    return g


@functools.lru_cache(maxsize=None)
def sharing(solver=False):
    games = [shared_game("shared:n=20", 20), shared_game("shared:n=2", 2, value=-1.0),
             shared_game("full_window:n=20", 20), leaf_game("plain:n=20", 20)]
    games += extras(8)
    L = make("sharing_solver" if solver else "sharing", games, 200, 128, 91, options(solver=solver))
    L["steps"] = [("select",), ("hand", _share), ("hand", _fill_window), ("expand", rows_for(L["img"], L["specs"], 92), False)]
    L["steps"] += step_pair(L, 93)
    return L


# ---- the root step ----------------------------------------------------------------------------------------------------
def kept(g):
    g.kept = True
    return g


@functools.lru_cache(maxsize=None)
def root_step(noise=True, solver=False, heads=False):
    from oracle import lz_oracle as O
    initial = O.state_from_batch(O.initial_states(1), 0)
    games = [StepGame("fresh:n=36", initial, fresh=True, value=0.25), StepGame("fresh:n=35", position(3, 1, 35), fresh=True, value=-0.5),
             StepGame("fresh:n=1", O.apply_index(*leaf_with(1)), fresh=True),
             StepGame("fresh:bad_row", position(5, 2), fresh=True, row="minus_inf" if heads else "zero"),
             StepGame("fresh:no_legal_move", blocked_position(), fresh=True, value=0.5),
             StepGame("fresh:n=2", O.apply_index(*leaf_with(2)), fresh=True)]
    g = kept(StepGame("kept:ne=1", O.apply_index(*leaf_with(1))))
    g.nodes[0]["P"][0] = F32(0.8)
    games.append(g)
    g = kept(StepGame("kept:ne=2", O.apply_index(*leaf_with(2))))
    games.append(g)
    g = kept(StepGame("kept:ne=36", initial))
    g.nodes[0]["P"][:] = np.random.default_rng(3).dirichlet(np.ones(36)).astype(F32)
    games.append(g)
    g = kept(StepGame("kept:tiny_sum", position(3, 2)))               # the mixed sum stays below 1e-8: the divisor is clamped
    g.nodes[0]["P"][:] = F32(1e-12)
    g.row = "tiny_noise"
    games.append(g)
    # solver: R(root) over existing edges -- won, drawn, lost, undecided
    for tag, xs in (("kept:R=won", (-1, 1)), ("kept:R=drawn", (-1, 0)), ("kept:R=lost", (-1, -1)), ("kept:R=open", (-1, None))):
        g = kept(StepGame(tag, position(6, 60)))
        for k in range(len(g.nodes[0]["act"])):
            x = xs[0] if k != 2 else xs[1]
            if x is not None:
                decide(g, 0, k, x, proven=k % 2 == 1)
        games.append(g)
    games += extras(9)
    name = "root" + ("_noise" if noise else "") + ("_solver" if solver else "") + ("_heads" if heads else "")
    L = make(name, games, 200, 128, 101, options(solver=solver))
    img = L["img"]
    for gi, g in enumerate(games):
        if getattr(g, "kept", False):
            img["leaf_kind"][gi] = H.LEAF_REUSED_ROOT
    rows = rows_for(img, L["specs"], 102, heads=heads, noise=noise)
    if noise:
        for gi, g in enumerate(games):
            if g.row == "tiny_noise":
                rows["noise"][gi] = F32(1e-12)
    L["steps"] = [("expand", rows, True)] + step_pair(L, 103, heads=heads) + step_pair(L, 104, heads=heads)
    return L


def wide_root(tag="kept:ne=72", kept_root=True, **kw):
    """A root of 72 edges cannot be a real position; its run is synthetic (every edge terminal)."""
    line, acts = line_of(3)
    g = StepGame(tag, line[40], **kw)
    nd = g.nodes[0]
    n = 72
    nd["act"], nd["succ"] = np.array([(7 + 3 * k) % 220 for k in range(n)], np.uint8), [None] * n
    nd["W"], nd["N"], nd["child"] = np.zeros(n), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    nd["P"] = np.random.default_rng(9).dirichlet(np.ones(n)).astype(F32)
    nd["info"] = np.array([(k % 2) | H.INFO_TERMINAL | ((k % 3) << 2) for k in range(n)], np.uint8)
    nd["synthetic"] = True
    return kept(g) if kept_root else g


@functools.lru_cache(maxsize=None)
def root_wide():
    games = [wide_root(), StepGame("fresh:n=36", position(3, 0, 36), fresh=True)] + extras(10)
    L = make("root_wide", games, 200, 128, 111)
    L["img"]["leaf_kind"][0] = H.LEAF_REUSED_ROOT
    L["steps"] = [("expand", rows_for(L["img"], L["specs"], 112, noise=True), True)] + step_pair(L, 113)
    return L


LAUNCHES = {
    "deep": deep, "deep_solver": lambda: deep(True), "descent": descent, "big_n": big_n, "forced": forced, "solver": solver, "shape": shape,
    "expansion": expansion, "expansion_heads": lambda: expansion(True), "refusal": refusal, "sharing": sharing,
    "sharing_solver": lambda: sharing(True), "root_noise": lambda: root_step(True), "root": lambda: root_step(False),
    "root_noise_solver": lambda: root_step(True, True), "root_noise_heads": lambda: root_step(True, False, True),
    "root_wide": root_wide,
}
NAMES = tuple(LAUNCHES)


def launch(name):
    return LAUNCHES[name]()
