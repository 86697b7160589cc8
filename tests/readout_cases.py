"""Seeded hand-built roots for the tree read-out kernels: the inputs of tests/test_gpu_readout.py and
of the CPU test that counts their classes (tests/test_readout_ref_cpu.py).  Root dicts as tests/readout_ref.ref_finish reads
them, grouped into launches (one engine, one call of the kernel under test each).

Every row is tagged by what it actually holds (`tags`), not by what its generator meant, and the CPU test asserts at least
three rows of every tag of `REQUIRED`.

Why the visit counts of the softmax rows are what they are: the kernel forms log(score) / T in float32, whose rounding is
half an ulp of the quotient; at 1 / T = 10 and N = 40 that is 1.9e-6 of the exponent, which the 2e-6 cap of the bound
(tests/test_gpu_readout.py) still covers, at N = 4000 it would not.  So rows with a temperature below 0.5 keep N <= 40 unless
one child dominates (then every other probability is below 1e-5 and the dominant one is exp(0) / (1 + tiny)), rows at
T >= 0.5 keep N <= 4000.  At the float32 next above 1e-6f only exact ties and clear gaps occur: there a difference of one
visit in 2^24 would be a 0.06 difference of the exponent that float32 cannot see."""
import numpy as np

from tests.golden_utils import load, states
from tests.hand_roots import root_from_state
from tests import readout_ref as R

F32 = np.float32
NE = (1, 2, 35, 36, 37, 59, 60, 63, 64, 65, 71, 72)
BATCHES = (1, 3, 4, 5, 257)
T_ABOVE = np.nextafter(F32(1e-6), F32(1))
TEMPS = (F32(1), F32(0.5), F32(2), F32(0.1), F32(1e-6), T_ABOVE, F32(0), F32(-1))
NMAX = (1 << 24) - 1
U_TOP = np.nextafter(F32(1), F32(0))
SEGMENTS = ((0, 36), (36, 180), (180, 216), (216, 220))

_FIX = {}


def fixture():
    if "st" not in _FIX:
        _FIX["st"] = states(load("g1_rules.npz"), "s")
    return _FIX["st"]


def _state_pool():
    """Fixture rows by (phase, mover), open positions only (game_status 0)."""
    st = fixture()
    ph, pl = np.asarray(st["phase"]), np.asarray(st["current_player"])
    pool = {}
    for i in range(len(ph)):
        key = (int(ph[i]), int(pl[i]))
        if len(pool.get(key, ())) < 8 and root_from_state(st, i)["status"] == 0:
            pool.setdefault(key, []).append(i)
    return pool


def _actions(rng, ne):
    """`ne` distinct action bytes from all four segments of the 220, 216-219 included when there is room."""
    must = [int(rng.integers(lo, hi)) for lo, hi in SEGMENTS][:ne]
    if ne >= 8:
        must = list({*must, 216, 217, 218, 219})
    rest = [a for a in rng.permutation(220).tolist() if a not in must][:ne - len(must)]
    acts = np.array(must + rest)
    return acts[rng.permutation(ne)]


def _w(N, j8, white, player):
    """W (child mover's frame) such that q = j8 / 8 exactly in the root mover's frame."""
    sign = np.where(np.where(white, -1, 1) == player, 1.0, -1.0)
    return sign * (np.asarray(N, np.float64) * (np.asarray(j8, np.float64) / 8.0))


STAT_KINDS = ("random", "dominant", "allbits_small", "allbits_large", "single_0", "single_63", "single_64", "single_last",
              "all_zero", "tied_slots", "tie_q", "tie_p", "tie_index", "zero_runs", "priors_zero", "tie_q_fine")


def make_root(rng, st_idx, ne, kind, lowN, root_visits_kind=2):
    st = fixture()
    base = root_from_state(st, st_idx)
    player = base["player"]
    n = max(ne, 0)
    cap = 40 if lowN else 4000
    N = rng.integers(0, cap + 1, n).astype(np.int64)
    P = rng.dirichlet(np.full(max(n, 1), 0.5))[:n].astype(F32) if n else np.zeros(0, F32)
    j8 = rng.integers(-8, 9, n)
    info = rng.integers(0, 2, n).astype(np.int64)                       # child mover white / black
    k = int(rng.integers(0, n)) if n else 0
    hi = int(rng.integers(64, n)) if n > 64 else max(n - 1, 0)
    fine = None
    if n and N.max() == 0:
        N[k] = 1
    if kind == "dominant" and n:
        N = np.minimum(N, 40); N[k] = NMAX
    elif kind == "allbits_small" and n:
        info[:] = 0xFF; N = np.minimum(N, 40); N[k] = max(N[k], 1)
    elif kind == "allbits_large" and n:
        info[:] = 0xFF; N = np.minimum(N, 40); N[hi] = NMAX
    elif kind.startswith("single") and n:
        at = {"single_0": 0, "single_63": 63, "single_64": 64, "single_last": n - 1}[kind]
        at = at if at < n else n - 1
        N[:] = 0; N[at] = int(rng.integers(1, cap + 1))
    elif kind == "all_zero":
        N[:] = 0
    elif kind == "tied_slots" and n:
        N = np.minimum(N, cap - 1); N[[k, hi]] = cap
        j8[[k, hi]] = 3; P[[k, hi]] = P[k]                              # equal down to the index
    elif kind in ("tie_q", "tie_p", "tie_index") and n:
        tied = sorted({k, hi, int(rng.integers(0, n))})
        if n > 64 and rng.random() < 0.4:                               # the whole tie in the second slot
            tied = sorted({hi, 64, n - 1})
        N = np.minimum(N, cap - 1); N[tied] = cap
        if kind == "tie_q":                                             # Q decides: eighths differ by 0.125 >> 4e-6
            j8[tied] = -2; j8[tied[int(rng.integers(0, len(tied)))]] = 5
        else:
            j8[tied] = 4
            P[tied] = F32(0.0078125)
            if kind == "tie_p":                                         # P decides: 2^-7 against 2^-6
                P[tied[int(rng.integers(0, len(tied)))]] = F32(0.015625)
    elif kind == "tie_q_fine" and n > 1:                                # Q decides by 6e-6: above 4 x its tolerance, below 1e-5
        a, b = (0, n - 1) if rng.random() < 0.5 else (n - 1, 0)
        N = np.minimum(N, cap - 1); N[[a, b]] = cap
        P[a], P[b] = F32(0.25), F32(0.5)                                # (the prior would take the other one)
        fine = (a, b)
    elif kind == "zero_runs" and n:
        N = np.minimum(N, 8)
        N[rng.random(n) < 0.5] = 0
        if N.max() == 0:
            N[k] = 2
    elif kind == "priors_zero":
        P[:] = 0
    white = (info & 1) != 0
    j8 = np.where(N > 0, j8, 0)
    W = _w(N, j8, white, player)
    if fine is not None:
        sign = np.where(np.where(white, -1, 1) == player, 1.0, -1.0)
        W[fine[0]] = sign[fine[0]] * (N[fine[0]] * (0.5 + 6e-6))
        W[fine[1]] = sign[fine[1]] * (N[fine[1]] * 0.5)
    total = int(N.sum())
    rv = (0, 1, total)[root_visits_kind]
    root = dict(base, ne=ne, act=_actions(rng, n), N=N, P=P, W=W, info=info, kind=kind, root_visits=rv,
                root_w=float(rng.integers(-8, 9)) / 8.0 * max(rv, 1), root_init_value=F32(rng.integers(-8, 9) / 16.0),
                root_terminal=0, st_idx=int(st_idx))
    return root


def _terminal_states():
    """Fixture rows edited into finished games: a draw by the no-capture limit, and a movement position whose black side
    is down to three pieces (white has won).  The kernels read the status from the root's packed state."""
    st = fixture()
    pool = _state_pool()
    out = []
    for key in ((4, 1), (4, -1), (5, 1)):
        i = pool[key][0]
        s = {f: np.asarray(st[f][i:i + 1]).copy() for f in st}
        s["moves_since_capture"][0] = 36
        out.append(root_from_state(s, 0))
        s = {f: np.asarray(st[f][i:i + 1]).copy() for f in st}
        b = s["board"][0].reshape(-1)
        own = np.nonzero(b == 1)[0]
        b[own[3:]] = 0
        out.append(root_from_state(s, 0))
    assert {r["status"] for r in out} == {2, -1}
    return out


def _dead_root(rng, base, ne, root_terminal):
    r = dict(base, ne=ne, act=np.zeros(0, int), N=np.zeros(0, int), P=np.zeros(0, F32), W=np.zeros(0), info=np.zeros(0, int),
             kind="dead", root_visits=int(rng.integers(0, 3)), root_w=0.5, root_init_value=F32(0.25),
             root_terminal=root_terminal, st_idx=-1)
    return r


def finish_launch(seed, B, *, mode, beta, target, out_cap):
    """One launch of lz_tree_finish.  mode: "det" | "sampled"; target: None | "equal" | "different"."""
    rng = np.random.default_rng(seed)
    pool = _state_pool()
    keys = sorted(pool)
    dead = _terminal_states()
    roots, temps, ttemps = [], [], []
    for g in range(B):
        key = keys[(g + seed) % len(keys)]
        st_idx = pool[key][(g // len(keys)) % len(pool[key])]
        ne = NE[(g * 5 + seed) % len(NE)]
        kind = STAT_KINDS[(g + seed // 3) % len(STAT_KINDS)]
        T = TEMPS[(g * 3 + seed) % len(TEMPS)]
        Tt = T if target != "different" else TEMPS[(g * 5 + 1 + seed) % len(TEMPS)]
        if kind == "all_zero":                                   # no mass: only where the contract defines the row
            if mode == "sampled" or not beta > 0:
                T = (F32(1e-6), F32(0), F32(-1))[g % 3]
            if not beta > 0:
                Tt = T
        if T == T_ABOVE or (target is not None and Tt == T_ABOVE):
            if kind not in ("tied_slots", "tie_index", "single_0", "single_63", "single_64", "single_last", "all_zero"):
                kind = "tied_slots" if ne > 1 else "single_0"    # at the float32 above 1e-6f: exact ties and clear gaps only
        lowN = min(float(T), float(Tt)) < 0.5 or mode == "sampled"
        r = make_root(rng, st_idx, ne, kind, lowN, root_visits_kind=(g + seed) % 3)
        while Tt <= R.T_EDGE and beta > 0 and not onehot_margin_ok(r, beta):        # a one-hot target needs a clear leader
            r = make_root(rng, st_idx, ne, kind, lowN, root_visits_kind=(g + seed) % 3)
        if mode == "sampled":                                    # intervals wider than 1e-3: few visits per child
            r["N"] = np.minimum(r["N"], 8) if kind not in ("dominant", "allbits_large") else r["N"]
            if r["N"].max() == 0 and kind != "all_zero":
                r["N"][0] = 1
            white = (np.asarray(r["info"]) & 1) != 0
            r["W"] = _w(r["N"], np.where(r["N"] > 0, 2, 0), white, r["player"])
        roots.append(r); temps.append(T); ttemps.append(Tt)
    # finished games, a stuck mover and root_terminal = 1 in the first, a middle and the last slot
    slots = sorted({0, B // 2, B - 1})
    specials = [(_dead_root(rng, dead[(seed + i) % len(dead)], (-1, 0, -1)[i % 3], 0)) for i in range(3)]
    if B >= 5:
        for i, g in enumerate(slots):
            if (seed + i) % 3 == 0:
                roots[g] = specials[i]
            elif (seed + i) % 3 == 1:
                roots[g] = dict(roots[g], root_terminal=1)       # edges present, root marked terminal
            else:                                                # a stuck mover: an open position without a legal move
                roots[g] = _dead_root(rng, root_from_state(fixture(), roots[g]["st_idx"]), 0, 0)
        roots[1] = specials[(seed + 1) % 3]
    elif seed % 4 == 0 and B >= 3:
        roots[0] = dict(roots[0], root_terminal=1)
    elif seed % 2:
        roots[B - 1] = specials[seed % 3] if seed % 4 == 1 else dict(roots[B - 1], root_terminal=1)
    L = dict(name=f"finish B={B} {mode} beta={beta} target={target} cap={out_cap}", B=B, roots=roots, mode=mode,
             temps=np.array(temps, F32), target_temps=None if target is None else np.array(ttemps, F32), beta=F32(beta),
             out_cap=out_cap, sample_moves=mode == "sampled", uniforms=None, force=None)
    if mode == "sampled":
        force = np.array([1 if g % 7 == 3 else 0 for g in range(B)], np.uint8)
        u = np.zeros(B, F32)
        for g, r in enumerate(roots):
            u[g] = _uniform_for(rng, r, temps[g], bool(force[g]), g)
        L["force"], L["uniforms"] = force, u
    for g, r in enumerate(roots):
        r["tags"] = row_tags(L, g)
    return L


def onehot_margin_ok(r, beta):
    """The largest float32 target score is exactly tied or leads by 1e-5 of itself (80 float32 ulps)."""
    top = np.sort(np.unique(R.target_scores(r["N"], r["P"], beta).astype(F32)))[::-1]
    return len(top) < 2 or top[0] - top[1] > 1e-5 * top[0]


def live(r):
    return not (r["root_terminal"] or r["ne"] <= 0)


def _uniform_for(rng, r, T, forced, g):
    """Target child first, then u (section 23): the midpoint of the target's interval, u = 0, or the float32 below 1."""
    if not live(r):
        return F32(rng.uniform(0.05, 0.95))
    ne = r["ne"]
    if forced:
        how = g % 3
        return F32(0) if how == 0 else U_TOP if how == 1 else F32((int(rng.integers(0, ne)) + 0.5) / ne)
    pol = R.policy(r["N"], T)
    cum = np.concatenate([[0.0], np.cumsum(pol)])
    wide = [k for k in range(ne) if pol[k] > 1e-3]
    lives = np.nonzero(pol > 0)[0]
    assert wide, (r["kind"], ne)
    want = g % 7
    if want == 0 and lives[0] in wide:
        return F32(0)                                                         # the first live child
    if want == 1 and lives[-1] in wide:
        return U_TOP                                                          # the last live child, by prefix or by fall-back
    cands = {2: [k for k in wide if k == lives[0]], 3: [k for k in wide if k == lives[-1]], 4: [k for k in wide if k == 63],
             5: [k for k in wide if k == 64],
             6: [k for k in wide if k >= 2 and r["N"][k - 1] == 0 and r["N"][k - 2] == 0]}.get(want, [])
    k = cands[0] if cands else wide[int(rng.integers(0, len(wide)))]
    return F32(0.5 * (cum[k] + cum[k + 1]))


def row_tags(L, g):
    r = L["roots"][g]
    T = L["temps"][g]
    Tt = T if L["target_temps"] is None else L["target_temps"][g]
    tags = {f"B={L['B']}", f"cap={L['out_cap']}", f"beta={float(L['beta'])}",
            "target_" + ("null" if L["target_temps"] is None else "equal" if Tt == T else "different")}
    if r["ne"] == -1:
        tags.add("nedges=-1")
    if r["ne"] == 0:
        tags.add("stuck" if r["status"] == 0 else "nedges=0_finished")
    if r["root_terminal"]:
        tags.add("root_terminal_" + ("first" if g == 0 else "last" if g == L["B"] - 1 else "middle"))
    if not live(r):
        tags.add(f"dead_status={r['status']}")
        return tags
    ne, N, P = r["ne"], np.asarray(r["N"]), np.asarray(r["P"], F32)
    tags |= {f"ne={ne}", f"phase={r['phase']}", f"mover={r['player']}", f"T={float(T)!r}", f"stats_{r['kind']}"}
    tags |= {f"segment{i}" for i, (lo, hi) in enumerate(SEGMENTS) if ((r["act"] >= lo) & (r["act"] < hi)).any()}
    white = (np.asarray(r["info"]) & 1) != 0
    tags |= {f"child_{'white' if w else 'black'}_root_{r['player']}" for w in set(white.tolist())}
    tags.add(f"root_visits_{'0' if r['root_visits'] == 0 else '1' if r['root_visits'] == 1 else 'sum'}")
    if N.max() == NMAX:
        tags.add("N=2^24-1")
    if (np.asarray(r["info"]) == 0xFF).all():
        tags.add("allbits_" + ("large" if N.max() == NMAX else "small"))
    if (N > 0).sum() == 1:
        at = int(np.argmax(N))
        tags |= {f"single_slot{at}" for _ in [0] if at in (0, 63, 64)} | ({"single_last"} if at == ne - 1 else set())
    if N.max() == 0:
        tags.add("allzero_" + ("both" if T <= R.T_EDGE and L["beta"] > 0 else "coldT" if T <= R.T_EDGE else "beta"))
    if ne > 64 and (N[:64] == N.max()).any() and (N[64:] == N.max()).any():
        tags.add("max_tied_across_slots")
    if not (P > 0).any() and L["beta"] > 0:
        tags.add("priors_sum_0")
    if L["mode"] == "det":
        q = R.child_q(r["W"], N, white, r["player"]).astype(F32)
        c0 = np.nonzero(N == N.max())[0]
        c1 = c0[np.abs(q[c0] - q[c0].max()) <= F32(1e-6)]
        c2 = c1[np.abs(P[c1] - P[c1].max()) <= F32(1e-8)]
        stage = "N" if len(c0) == 1 else "Q" if len(c1) == 1 else "P" if len(c2) == 1 else "index"
        tags.add(f"det_{stage}_slot{int(c2.min() >= 64)}")
    elif L["force"][g]:
        u = L["uniforms"][g]
        tags.add("forced_u0" if u == 0 else "forced_utop" if u == U_TOP else "forced_mid")
    else:
        u = L["uniforms"][g]
        pol = R.policy(N, T)
        k = R.sampled_pick(pol, u)
        lives = np.nonzero(pol > 0)[0]
        tags.add("sampled_u0" if u == 0 else "sampled_utop" if u == U_TOP else "sampled_mid")
        tags |= {t for t, on in (("sampled_first_live", k == lives[0]), ("sampled_last_live", k == lives[-1]),
                                 ("sampled_lane63", k == 63), ("sampled_slot1_lane0", k == 64),
                                 ("sampled_after_zero_run", k >= 2 and N[k - 1] == 0 and N[k - 2] == 0)) if on}
    return tags


FINISH_SETTINGS = (
    (11, 257, dict(mode="det", beta=0.0, target=None, out_cap=72)),
    (12, 257, dict(mode="sampled", beta=0.0, target=None, out_cap=36)),
    (13, 257, dict(mode="det", beta=0.5, target="equal", out_cap=36)),
    (14, 257, dict(mode="det", beta=8.0, target="different", out_cap=72)),
    (15, 257, dict(mode="sampled", beta=8.0, target="different", out_cap=72)),
    (16, 1, dict(mode="det", beta=0.0, target=None, out_cap=72)), (17, 1, dict(mode="sampled", beta=0.5, target="equal", out_cap=36)),
    (18, 1, dict(mode="det", beta=8.0, target="different", out_cap=72)),
    (19, 3, dict(mode="det", beta=0.0, target=None, out_cap=36)), (20, 3, dict(mode="sampled", beta=0.0, target=None, out_cap=72)),
    (21, 3, dict(mode="det", beta=0.5, target="different", out_cap=72)),
    (22, 4, dict(mode="det", beta=0.0, target="equal", out_cap=72)), (23, 4, dict(mode="sampled", beta=0.0, target=None, out_cap=36)),
    (24, 4, dict(mode="det", beta=8.0, target=None, out_cap=36)),
    (25, 5, dict(mode="det", beta=0.0, target=None, out_cap=72)), (26, 5, dict(mode="sampled", beta=0.5, target="equal", out_cap=72)),
    (27, 5, dict(mode="det", beta=0.0, target="different", out_cap=36)),
)
_CACHE = {}


def finish_launches():
    if "finish" not in _CACHE:
        _CACHE["finish"] = [finish_launch(seed, B, **kw) for seed, B, kw in FINISH_SETTINGS]
    return _CACHE["finish"]


REQUIRED = tuple(
    [f"B={b}" for b in BATCHES] + [f"ne={n}" for n in NE] + [f"phase={p}" for p in range(1, 8)] + ["mover=1", "mover=-1"] +
    [f"segment{i}" for i in range(4)] + ["nedges=-1", "nedges=0_finished", "stuck", "root_terminal_first",
                                         "root_terminal_middle", "root_terminal_last"] +
    [f"stats_{k}" for k in STAT_KINDS] + ["N=2^24-1", "allbits_small", "allbits_large"] +
    [f"child_{c}_root_{p}" for c in ("white", "black") for p in (1, -1)] +
    ["root_visits_0", "root_visits_1", "root_visits_sum", "single_slot0", "single_slot63", "single_slot64", "single_last",
     "allzero_coldT", "allzero_beta", "allzero_both", "max_tied_across_slots", "priors_sum_0"] +
    [f"T={float(t)!r}" for t in TEMPS] + ["target_null", "target_equal", "target_different", "beta=0.0", "beta=0.5", "beta=8.0"] +
    [f"det_{s}_slot{k}" for s in ("N", "Q", "P", "index") for k in (0, 1)] +
    ["sampled_u0", "sampled_utop", "sampled_mid", "sampled_first_live", "sampled_last_live", "sampled_lane63",
     "sampled_slot1_lane0", "sampled_after_zero_run", "forced_u0", "forced_utop", "forced_mid", "cap=72", "cap=36"])


# ---- policy target pruning (lz_tree_finish_pruned) ---------------------------------------------------------------------------
# Dyadic everywhere: forced_k in {2, 0.5}, P = m / 128, T = root visits in {0, 1, 64, 65, 66, 256}, q in eighths, table entries
# in quarters, so that every threshold (forced_k P) max(T, 1) is exact in double and the classes below are what they say.
PRUNE_TABLE = np.array([1.0 + 0.25 * (i % 5) for i in range(66)], np.float64)        # len - 1 = 65
PRUNE_T = (64, 64, 64, 256, 0, 1, 65, 66)


def prune_trace(N, P, q, T, k, c):
    """The rule's intermediate quantities per child (for tagging only; tests/readout_ref.prune_targets is the checker)."""
    tm = float(max(T, 1)); sq = np.sqrt(tm)
    star = max(range(len(N)), key=lambda j: (N[j], -j))
    s_star = q[star] + c * float(P[star]) * sq / (1.0 + N[star])
    rows = []
    for j in range(len(N)):
        if j == star or N[j] <= 0:
            continue
        thr = (k * float(P[j])) * tm
        gap = s_star - q[j]
        x = (c * float(P[j]) * sq) / gap - 1.0 if gap > 0 else None
        rows.append(dict(j=j, n2=float(N[j]) ** 2, thr=thr, gap=gap, x=x, N=N[j]))
    return star, rows


def prune_launch(seed, B, *, forced_k, table, outputs):
    rng = np.random.default_rng(seed)
    pool = _state_pool()
    keys = sorted(pool)
    roots = []
    for g in range(B):
        key = keys[(g + seed) % len(keys)]
        ne = NE[(g * 7 + seed) % len(NE)]
        base = root_from_state(fixture(), pool[key][g % len(pool[key])])
        T = PRUNE_T[(g + seed) % len(PRUNE_T)]
        kf = forced_k if forced_k > 0 else 2.0
        N = rng.integers(0, 13, ne).astype(np.int64)
        m = rng.integers(0, 33, ne)                                         # P = m / 128
        how = g % 6
        for j in range(ne):                                                 # N * N equal to, one below and one above thr
            if N[j] > 0 and how < 3 and T in (64, 256) and j % 2 == 0:
                want = N[j] * N[j] + (0, 1, -1)[how]                         # thr = kf * m / 128 * T
                mm = want * 128.0 / (kf * T)
                if mm == int(mm) and 0 <= mm <= 128:
                    m[j] = int(mm)
        star = int(rng.integers(0, ne)) if g % 5 else (int(rng.integers(64, ne)) if ne > 64 else ne - 1)
        N[star] = (15, 31, 63)[g % 3]
        if g % 4 == 1 and ne > 2:
            N[(star + 1) % ne] = N[star]                                    # c* tied: the lowest index takes it
        if g % 5 == 0 and ne > 64:
            N[:64] = np.minimum(N[:64], 12)                                 # c* in slot 1
        j8 = rng.integers(-8, 9, ne)
        if how == 4:
            j8[:] = np.maximum(j8, 6)                                       # gap <= 0 for many
        if how == 5:
            m = np.minimum(m, 2)                                            # tiny priors: x < 0
        info = rng.integers(0, 2, ne)
        white = info != 0
        j8 = np.where(N > 0, j8, 0)
        P = (m / 128.0).astype(F32)
        roots.append(dict(base, ne=ne, act=_actions(rng, ne), N=N, P=P, W=_w(N, j8, white, base["player"]), info=info,
                          kind="prune", root_visits=T, root_w=float(rng.integers(-8, 9)) / 8.0 * max(T, 1),
                          root_init_value=F32(0.5), root_terminal=0, st_idx=-1))
    if B >= 5:
        roots[B // 2] = dict(roots[B // 2], root_terminal=1)
        roots[B - 1] = _dead_root(rng, _terminal_states()[seed % 6], -1, 0)
    noise = np.array([0 if g % 9 == 4 else 1 for g in range(B)], np.uint8)
    temps = np.array([(F32(1), F32(0.5), F32(1e-6), F32(2))[g % 4] for g in range(B)], F32)
    L = dict(name=f"prune B={B} k={forced_k} table={table} outputs={outputs}", B=B, roots=roots, mode="det", temps=temps,
             target_temps=None, beta=F32(0), out_cap=72, sample_moves=False, uniforms=None, force=None, forced_k=forced_k,
             root_noise=noise, table=PRUNE_TABLE if table else None, outputs=outputs, c_puct=1.25)
    for g, r in enumerate(roots):
        r["tags"] = prune_tags(L, g)
    return L


def prune_c(L, g):
    return R.table_c(L["table"], L["roots"][g]["root_visits"]) if L["table"] is not None else L["c_puct"]


def prune_on(L, g):
    return L["forced_k"] > 0 and L["root_noise"][g] != 0 and live(L["roots"][g])


def prune_tags(L, g):
    r = L["roots"][g]
    tags = {f"pruneB={L['B']}", "outputs_given" if L["outputs"] else "outputs_null",
            "prune_table" if L["table"] is not None else "prune_plain"}
    if L["forced_k"] == 0:
        tags.add("forced_k=0")
    if not live(r):
        return tags
    if L["root_noise"][g] == 0:
        tags.add("root_noise=0")
    if not prune_on(L, g):
        return tags
    T, N = r["root_visits"], np.asarray(r["N"])
    white = (np.asarray(r["info"]) & 1) != 0
    q = R.child_q(r["W"], N, white, r["player"])
    star, rows = prune_trace(N, r["P"], q, T, L["forced_k"], prune_c(L, g))
    out = R.prune_targets(N, r["P"], q, T, L["forced_k"], prune_c(L, g))
    tags |= {f"pruneT={'0' if T == 0 else '1' if T == 1 else 'big'}", f"prune_ne={r['ne']}"}
    if L["table"] is not None:
        n = len(L["table"])
        tags.add("table_at_end" if T == n - 1 else "table_beyond" if T > n - 1 else "table_inside")
    if (N == N.max()).sum() > 1:
        tags.add("cstar_tied")
    if star >= 64:
        tags.add("cstar_slot1")
    for t in rows:
        tags.add("sq_equal" if t["n2"] == t["thr"] else "sq_one_above" if t["n2"] == t["thr"] + 1 else
                 "sq_one_below" if t["n2"] == t["thr"] - 1 else "sq_other")
        tags.add("gap<=0" if t["gap"] <= 0 else "x<0" if t["x"] < 0 else "x>=N" if t["x"] >= t["N"] else "x_inside")
    raw = [min(int(N[t["j"]]), max(int(N[t["j"]]) - _F(t["thr"]), _L(t))) for t in rows]
    tags |= {f"nprime_raw={v}" for v in raw if v in (1, 2)}
    if (out != N).any():
        tags.add("pruned_something")
    return tags


def _F(thr):
    m = 0
    while float(m) * float(m) < thr:
        m += 1
    return m


def _L(t):
    if t["gap"] <= 0:
        return int(t["N"])
    return 0 if t["x"] < 0 else int(t["N"]) if t["x"] >= t["N"] else int(np.floor(t["x"])) + 1


PRUNE_SETTINGS = ((31, 257, dict(forced_k=2.0, table=False, outputs=True)), (32, 257, dict(forced_k=0.5, table=True, outputs=True)),
                  (33, 257, dict(forced_k=2.0, table=True, outputs=False)), (34, 5, dict(forced_k=0.0, table=False, outputs=True)),
                  (35, 3, dict(forced_k=2.0, table=False, outputs=False)), (36, 4, dict(forced_k=0.0, table=True, outputs=True)),
                  (37, 1, dict(forced_k=0.0, table=False, outputs=False)))
PRUNE_REQUIRED = ("sq_equal", "sq_one_above", "sq_one_below", "gap<=0", "x<0", "x>=N", "x_inside", "nprime_raw=1", "nprime_raw=2",
                  "cstar_tied", "cstar_slot1", "pruneT=0", "pruneT=1", "pruneT=big", "table_at_end", "table_beyond",
                  "table_inside", "root_noise=0", "forced_k=0", "outputs_null", "outputs_given", "prune_plain", "prune_table",
                  "pruned_something")


def prune_launches():
    if "prune" not in _CACHE:
        _CACHE["prune"] = [prune_launch(seed, B, **kw) for seed, B, kw in PRUNE_SETTINGS]
    return _CACHE["prune"]


# ---- MCTS-Solver pick (lz_tree_solver_pick behind a deterministic lz_tree_finish) --------------------------------------------------
SOLVER_KINDS = ("win_terminal", "win_proven", "wins_tied", "picked_lost_other", "picked_lost_alone", "all_lost", "none_decided",
                "draws_only")


def _decided(white, player, x, proven):
    """Info byte of a child decided with value x for the ROOT's mover."""
    d = x if (-1 if white else 1) == player else -x
    return (1 if white else 0) | (R.INFO_PROVEN if proven else R.INFO_TERMINAL) | ((d + 1) << 2)


def solver_launch(seed, B, *, overrides):
    rng = np.random.default_rng(seed)
    pool = _state_pool()
    keys = sorted(pool)
    roots = []
    for g in range(B):
        key = keys[(g + seed) % len(keys)]
        ne = NE[(g * 5 + seed) % len(NE)]
        kind = SOLVER_KINDS[g % len(SOLVER_KINDS)]
        r = make_root(rng, pool[key][g % len(pool[key])], ne, "random", True)
        N, info, player = r["N"], r["info"] & 1, r["player"]
        white = info != 0
        top = int(np.argmax(N))                                          # what the finish picks, ties apart
        N[top] += 1
        dec = lambda k, x, proven: _decided(bool(white[k]), player, x, proven)
        others = [k for k in range(ne) if k != top]
        if kind in ("win_terminal", "win_proven") and others:
            k = others[int(rng.integers(0, len(others)))]
            info[k] = dec(k, 1, kind == "win_proven")
        elif kind == "wins_tied" and ne > 2:
            ks = sorted({others[0], others[-1], others[len(others) // 2]})
            for k in ks:
                info[k] = dec(k, 1, bool(k % 2)); N[k] = 7
        elif kind == "picked_lost_other" and others:
            info[top] = dec(top, -1, bool(g % 2))
            for k in others[::3][1:]:
                info[k] = dec(k, -1, True)
        elif kind == "picked_lost_alone":
            ne = 1
            r = make_root(rng, r["st_idx"], 1, "random", True)
            N, info, white = r["N"], r["info"] & 1, (r["info"] & 1) != 0
            info[0] = _decided(bool(white[0]), player, -1, bool(g % 2))
        elif kind == "all_lost":
            for k in range(ne):
                info[k] = dec(k, -1, bool((k + g) % 2))
        elif kind == "draws_only":
            for k in others[::2]:
                info[k] = dec(k, 0, bool(k % 2))
        r["N"], r["info"] = N, info
        r["W"] = _w(N, np.where(N > 0, rng.integers(-8, 9, len(N)), 0), (info & 1) != 0, player)
        r["kind"] = kind
        roots.append(r)
    if B >= 5:
        roots[B // 2] = dict(roots[B // 2], root_terminal=1)
        roots[B - 1] = _dead_root(rng, _terminal_states()[seed % 6], 0, 0)
    force = np.array([1 if g % 10 == 6 else 0 for g in range(B)], np.uint8)
    L = dict(name=f"solver B={B} overrides={overrides}", B=B, roots=roots, mode="det", temps=np.full(B, 1, F32),
             target_temps=None, beta=F32(0), out_cap=72, sample_moves=False, force=force,
             uniforms=np.array([F32((g % 13 + 0.5) / 13) for g in range(B)], F32), overrides=overrides)
    for g, r in enumerate(roots):
        r["tags"] = solver_tags(L, g)
    return L


def solver_xs(r):
    return [R.solver_x(b, r["player"]) if int(b) & (R.INFO_TERMINAL | R.INFO_PROVEN) else None for b in r["info"]]


def solver_tags(L, g):
    r = L["roots"][g]
    tags = {f"solverB={L['B']}", "overrides_given" if L["overrides"] else "overrides_null"}
    if not live(r):
        return tags | {"solver_dead"}
    if L["force"][g]:
        return tags | {"solver_force_uniform"}
    xs, N, info = solver_xs(r), np.asarray(r["N"]), np.asarray(r["info"])
    fin = R.ref_finish(r, temperature=L["temps"][g])
    wins = [k for k, x in enumerate(xs) if x == 1]
    tags |= {f"solver_mover={r['player']}"} | {f"solver_child_{'white' if b & 1 else 'black'}" for b in info if b & 18}
    if any(info[k] & R.INFO_TERMINAL for k in wins):
        tags.add("win_by_terminal")
    if any(info[k] & R.INFO_PROVEN for k in wins):
        tags.add("win_by_proven")
    if len(wins) > 1 and (N[wins] == N[wins].max()).sum() > 1 and min(wins) < 64 <= max(wins):
        tags.add("wins_tied_across_slots")
    lost = [k for k, x in enumerate(xs) if x == -1]
    if not wins and fin["pick"] in lost:
        tags.add("picked_lost_" + ("no_other" if len(lost) == r["ne"] else "with_other"))
    if len(lost) == r["ne"]:
        tags.add("every_child_lost")
    if all(x is None for x in xs):
        tags.add("no_decided_child")
    played = R.solver_pick(r["act"], N, xs, fin["chosen_index"])
    tags.add("solver_changed" if played != fin["chosen_index"] else "solver_kept")
    return tags


SOLVER_SETTINGS = ((41, 257, dict(overrides=True)), (42, 257, dict(overrides=False)), (43, 5, dict(overrides=True)),
                   (44, 3, dict(overrides=True)), (45, 1, dict(overrides=False)))
SOLVER_REQUIRED = ("win_by_terminal", "win_by_proven", "wins_tied_across_slots", "picked_lost_with_other", "picked_lost_no_other",
                   "every_child_lost", "no_decided_child", "solver_force_uniform", "overrides_null", "overrides_given",
                   "solver_mover=1", "solver_mover=-1", "solver_child_white", "solver_child_black", "solver_changed",
                   "solver_kept", "solver_dead")


def solver_launches():
    if "solver" not in _CACHE:
        _CACHE["solver"] = [solver_launch(seed, B, **kw) for seed, B, kw in SOLVER_SETTINGS]
    return _CACHE["solver"]


# ---- Gumbel finish (lz_tree_finish_gumbel) -------------------------------------------------------------------------------------------
GUMBEL_M = 40
GUMBEL_KINDS = ("random", "p_zero", "all_n_zero", "pv_zero", "l_tie_score", "l_tie_index", "random")


def gumbel_launch(seed, B):
    rng = np.random.default_rng(seed)
    pool = _state_pool()
    keys = sorted(pool)
    roots = []
    gl, base = np.zeros((B, 80), F32), np.zeros((B, 80), np.int32)
    v0 = (rng.integers(-8, 9, B) / 16.0).astype(F32)
    for g in range(B):
        key = keys[(g + seed) % len(keys)]
        ne = NE[(g * 5 + seed) % len(NE)]
        kind = GUMBEL_KINDS[g % len(GUMBEL_KINDS)]
        r = make_root(rng, pool[key][g % len(pool[key])], ne, "random", True)
        N, P = r["N"], r["P"]
        j8 = rng.integers(-8, 9, ne)
        row = rng.gumbel(size=ne).astype(F32)
        b = np.minimum(rng.integers(0, 5, ne), N)
        if kind == "p_zero":
            P[rng.random(ne) < 0.4] = 0
            if ne > 1:
                P[0] = F32(0.25)
        elif kind == "all_n_zero":
            N[:] = 0; b[:] = 0
        elif kind == "pv_zero":
            P[N > 0] = 0
            if (N == 0).any():
                P[N == 0] = F32(1.0 / 64)
            else:
                N[0] = 0; b[0] = 0; P[0] = F32(0.5)
        elif kind in ("l_tie_score", "l_tie_index") and ne > 1:
            ks = sorted({0, ne - 1, ne // 2})
            N[:] = np.minimum(N, 20); b[:] = np.minimum(b, N)
            for k in ks:
                N[k] = 30; b[k] = 5; j8[k] = 2; row[k] = F32(0.5); P[k] = F32(0.03125)
            if kind == "l_tie_score":
                row[ks[-1]] = F32(0.75)
        with np.errstate(divide="ignore"):
            gl[g, :ne] = (row + np.log(P.astype(F32))).astype(F32)
        base[g, :ne] = b
        r["N"], r["P"] = N, P
        r["W"] = _w(N, np.where(N > 0, j8, 0), (r["info"] & 1) != 0, r["player"])
        r["kind"], r["root_visits"] = kind, int(N.sum())
        roots.append(r)
    if B >= 5:
        roots[B // 2] = dict(roots[B // 2], root_terminal=1)
        roots[B - 1] = _dead_root(rng, _terminal_states()[seed % 6], -1, 0)
    noise = np.array([0 if g % 8 == 5 else 1 for g in range(B)], np.uint8)
    force = np.array([1 if g % 11 == 7 else 0 for g in range(B)], np.uint8)
    # (a root without visits has no selection policy at T > 1e-6: the plain finish under the Gumbel rule runs it at 1e-6f)
    temps = np.array([F32(1e-6) if live(r) and np.asarray(r["N"]).sum() == 0 else F32(1) for r in roots], F32)
    L = dict(name=f"gumbel B={B}", B=B, roots=roots, mode="det", temps=temps, target_temps=None, beta=F32(0),
             out_cap=72, sample_moves=False, force=force, uniforms=np.array([F32((g % 13 + 0.5) / 13) for g in range(B)], F32),
             root_noise=noise, gl=gl, base=base, v0=v0, m=GUMBEL_M, c_visit=50.0, c_scale=1.0)
    for g, r in enumerate(roots):
        r["tags"] = gumbel_tags(L, g)
    return L


def gumbel_row(L, g):
    r = L["roots"][g]
    N = np.asarray(r["N"])
    q = R.child_q(r["W"], N, (np.asarray(r["info"]) & 1) != 0, r["player"])
    return N, q, R.gumbel_finish(N, r["P"], q, L["gl"][g], L["base"][g], L["v0"][g], L["c_visit"], L["c_scale"])


def gumbel_tags(L, g):
    r = L["roots"][g]
    tags = {f"gumbelB={L['B']}"}
    if not live(r):
        return tags | {"gumbel_dead"}
    if L["root_noise"][g] == 0:
        return tags | {"gumbel_switch_off"}
    if L["force"][g]:
        tags.add("gumbel_force_uniform")
    N, q, (pick, target, score, vmix) = gumbel_row(L, g)
    P = np.asarray(r["P"])
    tags.add("gumbel_ne_below_m" if r["ne"] < L["m"] else "gumbel_ne_above_m" if r["ne"] > L["m"] else "gumbel_ne_is_m")
    if (P == 0).any() and (P > 0).any():
        tags.add("gumbel_p_zero")
    if N.max() == 0:
        tags.add("gumbel_all_n_zero")
    elif not (P[N > 0] > 0).any():
        tags.add("gumbel_pv_zero")
    Lk = N - L["base"][g][:r["ne"]]
    cand = np.nonzero(Lk == Lk.max())[0]
    if len(cand) > 1:
        best = [k for k in cand if score[k] == max(score[c] for c in cand)]
        tags.add("gumbel_L_tie_by_index" if len(best) > 1 else "gumbel_L_tie_by_score")
        if cand.min() < 64 <= cand.max():
            tags.add("gumbel_L_tie_across_slots")
    return tags


GUMBEL_SETTINGS = ((51, 257), (52, 5), (53, 4), (54, 3), (55, 1))
GUMBEL_REQUIRED = ("gumbel_p_zero", "gumbel_all_n_zero", "gumbel_pv_zero", "gumbel_L_tie_by_score", "gumbel_L_tie_by_index",
                   "gumbel_L_tie_across_slots", "gumbel_force_uniform", "gumbel_switch_off", "gumbel_ne_below_m",
                   "gumbel_ne_above_m", "gumbel_dead")


def gumbel_launches():
    if "gumbel" not in _CACHE:
        _CACHE["gumbel"] = [gumbel_launch(seed, B) for seed, B in GUMBEL_SETTINGS]
    return _CACHE["gumbel"]


# ---- move pick and KLD check on wide roots ---------------------------------------------------------------------------------------------
WIDE_NE = (37, 60, 64, 65, 72)


def wide_launch(seed, B=40):
    """Roots of 37, 60, 64, 65 and 72 children with few visits per child (the existing checkers' rules need nothing else)."""
    rng = np.random.default_rng(seed)
    pool = _state_pool()
    keys = sorted(pool)
    roots = []
    for g in range(B):
        key = keys[(g + seed) % len(keys)]
        r = make_root(rng, pool[key][g % len(pool[key])], WIDE_NE[g % len(WIDE_NE)], ("random", "zero_runs", "tied_slots")[g % 3],
                      True)
        roots.append(r)
    roots[B // 2] = dict(roots[B // 2], root_terminal=1)
    temps = np.array([(F32(1), F32(0.5), F32(2), F32(1e-7))[g % 4] for g in range(B)], F32)
    force = np.array([1 if g % 11 == 3 else 0 for g in range(B)], np.uint8)
    u = rng.uniform(0.001, 0.999, B).astype(F32)
    u[[g for g in range(B) if roots[g]["ne"] > 64 and g % 2 == 0]] = F32(0.995)      # picks in the second slot
    return dict(name=f"wide B={B}", B=B, roots=roots, mode="sampled", temps=temps, target_temps=None, beta=F32(0), out_cap=72,
                sample_moves=True, force=force, uniforms=u)


def g22_rows():
    """The finish rows the fixture g22_finish_edges.npz holds the reference's answers for: every live row of the small
    launches and every fourth one of the 257-game launches, as (launch index, game)."""
    for i, L in enumerate(finish_launches()):
        for g, r in enumerate(L["roots"]):
            if live(r) and (L["B"] < 257 or g % 4 == 0):
                yield i, g


def g22_inputs(L, g):
    """(visits, priors, float32 Q, target temperature, beta) of a finish row: what the reference's two functions take."""
    r = L["roots"][g]
    N = np.asarray(r["N"], np.int64)
    q = R.child_q(r["W"], N, (np.asarray(r["info"]) & 1) != 0, r["player"]).astype(F32)
    Tt = L["temps"][g] if L["target_temps"] is None else L["target_temps"][g]
    return N, np.asarray(r["P"], F32), q, float(Tt), float(L["beta"])


def oracle_distance(launches):
    """The float32 oracle (oracle.lz_oracle.policy_from_visits) against the float64 restatement over the live rows of
    `launches`, in probabilities: {1 / T (0.0: one-hot): the largest distance}."""
    from oracle import lz_oracle as O
    worst = {}
    for L in launches:
        for g, r in enumerate(L["roots"]):
            if not live(r):
                continue
            N, P = np.asarray(r["N"]), np.asarray(r["P"], F32)
            Tt = L["temps"][g] if L["target_temps"] is None else L["target_temps"][g]
            scores = R.target_scores(N, P, L["beta"])
            if scores.sum() <= 0 and Tt > R.T_EDGE:
                continue
            got = O.policy_from_visits(N, float(Tt), P, float(L["beta"]))
            key = 0.0 if Tt <= R.T_EDGE else float(1.0 / np.float64(Tt))
            worst[key] = max(worst.get(key, 0.0), float(np.abs(got.astype(np.float64) - R.policy(scores, Tt)).max()))
    return worst


def all_rows():
    for fn in (finish_launches, prune_launches, solver_launches, gumbel_launches):
        for L in fn():
            for g, r in enumerate(L["roots"]):
                yield L, g, r
