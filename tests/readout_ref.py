"""Per-root numpy restatements of the tree read-out stage (csrc/lz_engine.hip: lz_tree_finish, lz_tree_finish_pruned,
lz_tree_finish_gumbel, lz_tree_solver_pick; lz_tree_move_pick and lz_tree_kld_check are tests/move_pick.py and
tests/kld_stop.py as they are), written from the contract of include/liuzhou_hip.h and the reference's
portable_mcts.py:150-261, :690-727.  Arithmetic is float64 unless the contract names a float32 (the temperature test, the
clamp of the priors, Q and P of the deterministic pick, the inclusive prefix of the sampled pick, the forced-uniform
product, root_value).  Checkers of the tests: they do nothing else.

The array-level functions `prune_targets`, `gumbel_scores`, `gumbel_finish` and `solver_pick` are the one definition of
their rules: tests/forced_tree.py, tests/gumbel_tree.py and tests/solver_tree.py call them."""
import math

import numpy as np

F32 = np.float32
T_EDGE = F32(1e-6)                       # temperatures at or below it take the one-hot argmax
INFO_WHITE, INFO_TERMINAL, INFO_PROVEN = 1, 2, 16
PHASE_MARK, PHASE_MOVE, PHASE_CAPTURE, PHASE_FORCED, PHASE_COUNTER = 2, 4, 5, 6, 7


def index_to_code(phase, a):
    """index_to_code of csrc/lz_rules.h."""
    if a < 0:
        return [0, -1, -1, -1]
    if a < 36:
        return [1, a, -1, -1]
    if a < 180:
        p, s = (a - 36) >> 2, (a - 36) & 3
        return [2, p, s, p + (-6, 6, -1, 1)[s]]
    if a < 216:
        return [{2: 3, 5: 4, 6: 5, 7: 6, 4: 7}.get(int(phase), 0), a - 180, -1, -1]
    return [8 if a == 216 else 0, -1, -1, -1]


def game_status(phase, blacks, whites, move_count, moves_since_capture):
    """game_status of csrc/lz_rules.h: -1 / +1 the winner (white / black), 2 a draw by the limits, 0 open."""
    if phase in (PHASE_MOVE, PHASE_CAPTURE, PHASE_COUNTER):
        if blacks < 4:
            return -1
        if whites < 4:
            return 1
    return 2 if (move_count >= 144 or moves_since_capture >= 36) else 0


def child_q(W, N, white, root_player):
    """q_k as the read-out forms it: double W / N in the root mover's frame (white: info bit 0), 0 at N = 0."""
    q = np.zeros(len(N), np.float64)
    for k in range(len(N)):
        if N[k] > 0:
            mv = np.float64(W[k]) / np.float64(N[k])
            q[k] = mv if (-1 if white[k] else 1) == root_player else -mv
    return q


def policy(scores, temperature):
    """portable_mcts.py:188-205 in float64: one-hot on the first maximum where the float32 temperature is <= 1e-6f, else the
    softmax of log(score) / max(T, 1e-6f) over score > 0.  No mass at T > 1e-6 is 0 / 0 (the reference raises)."""
    s = np.asarray(scores, np.float64)
    out = np.zeros(len(s), np.float64)
    if F32(temperature) <= T_EDGE:
        out[int(np.argmax(s))] = 1.0
        return out
    tt = np.float64(max(F32(temperature), T_EDGE))
    pos = s > 0
    if not pos.any():
        return np.full(len(s), np.nan)
    lg = np.log(s[pos]) / tt
    e = np.exp(lg - lg.max())
    out[pos] = e / e.sum()
    return out


def target_scores(N, P, beta):
    """visits + beta * normalised priors: float32 clamp at 1e-8, 1 / ne when the clamped sum is not a positive finite
    number (it always is: the fall-back is the reference's own dead branch, kept for the `bad` case of the kernel)."""
    s = np.asarray(N, np.float64).copy()
    if F32(beta) > 0:
        c = np.maximum(np.asarray(P, F32), F32(1e-8)).astype(np.float64)
        tot = c.sum()
        s = s + np.float64(F32(beta)) * (c / tot if (tot > 0 and np.isfinite(tot)) else np.full(len(s), 1.0 / len(s)))
    return s


def deterministic_pick(N, qf, P):
    """portable_mcts.py:208-261: N, then float32 Q within 1e-6 of the maximum, then P within 1e-8, then the lowest index."""
    N, qf, P = np.asarray(N), np.asarray(qf, F32), np.asarray(P, F32)
    c = np.nonzero(N == N.max())[0]
    c = c[np.abs(qf[c] - qf[c].max()) <= F32(1e-6)]
    c = c[np.abs(P[c] - P[c].max()) <= F32(1e-8)]
    return int(c.min())


def sampled_pick(pol, u):
    """The first child with pol > 0 whose float32 inclusive prefix exceeds u, else the last child with pol > 0 (-1: none)."""
    cum = np.cumsum(np.asarray(pol, np.float64)).astype(F32)
    live = np.nonzero(np.asarray(pol) > 0)[0]
    for k in live:
        if cum[k] > F32(u):
            return int(k)
    return int(live[-1]) if len(live) else -1


def uniform_pick(u, ne):
    return int(min(max(int(math.floor(float(F32(u) * F32(ne)))), 0), ne - 1))


def prune_targets(N, P, q, root_visits, k, c):
    """Policy target pruning (lz_tree_finish_pruned; the rule of ForcedTree.prune_targets): the visits N' of the target.
    N int, P float, q float64 (root mover's frame, 0 at N = 0), `c` the exploration constant in force (c_puct, or c(T) of
    the visit-scaled table)."""
    N = [int(v) for v in N]
    T = max(int(root_visits), 1)
    sq = math.sqrt(float(T))
    star = max(range(len(N)), key=lambda j: (N[j], -j))
    s_star = float(q[star]) + float(c) * float(P[star]) * sq / (1.0 + float(N[star]))
    out = list(N)
    for j in range(len(N)):
        if j == star or N[j] <= 0:
            continue
        thr = (float(k) * float(P[j])) * float(T)
        F = max(0, int(math.isqrt(int(min(thr, 1e30)))) - 1)
        while float(F) * float(F) < thr:
            F += 1
        while F > 0 and float(F - 1) * float(F - 1) >= thr:
            F -= 1
        gap = s_star - float(q[j])
        if gap > 0.0:
            x = (float(c) * float(P[j]) * sq) / gap - 1.0
            L = 0 if x < 0.0 else (N[j] if x >= float(N[j]) else int(math.floor(x)) + 1)
        else:
            L = N[j]
        n2 = min(N[j], max(N[j] - F, L))
        out[j] = 0 if n2 <= 1 else n2
    return np.array(out, np.int32)


def table_c(table, root_visits):
    """c(T) of the visit-scaled table: entry min(max(T, 0), len - 1)."""
    return float(table[min(max(int(root_visits), 0), len(table) - 1)])


def butterfly_sum(terms) -> float:
    """Sum of up to 128 doubles in the device's order: children l and l + 64 per lane, then an xor butterfly."""
    ne = len(terms)
    x = [(float(terms[l]) if l < ne else 0.0) + (float(terms[l + 64]) if l + 64 < ne else 0.0) for l in range(64)]
    for o in (32, 16, 8, 4, 2, 1):
        x = [x[l] + x[l ^ o] for l in range(64)]
    return x[0]


def gumbel_scores(N, P, q, gl, base, v0, c_visit, c_scale):
    """(score, sigma, vmix, L) of the root children (LzTreeDesc.gumbel_*): lists in child order, vmix a float."""
    n = len(N)
    Pv = butterfly_sum([float(P[k]) if N[k] > 0 else 0.0 for k in range(n)])
    Pq = butterfly_sum([float(P[k]) * float(q[k]) if N[k] > 0 else 0.0 for k in range(n)])
    T = int(sum(int(v) for v in N))
    tm = float(T)
    vmix = float(v0) if (T == 0 or Pv <= 0.0) else (float(v0) + tm * (Pq / Pv)) / (1.0 + tm)
    scale = (float(c_visit) + float(max(N))) * float(c_scale)
    sigma = [scale * (0.5 * (float(q[k]) if N[k] > 0 else vmix)) for k in range(n)]
    score = [float(gl[k]) + sigma[k] for k in range(n)]
    L = [int(N[k]) - int(base[k]) for k in range(n)]
    return score, sigma, vmix, L


def gumbel_argmax(score, cand):
    best, best_k = -math.inf, -1
    for k in cand:
        if best_k < 0 or score[k] > best:
            best, best_k = score[k], k
    if best_k >= 0 and best != best:          # NaN
        return -1
    return best_k


def gumbel_finish(N, P, q, gl, base, v0, c_visit, c_scale):
    """(pick child offset, target probabilities float32[ne] or None when no child has P > 0, score float64[ne], vmix)."""
    score, sigma, vmix, L = gumbel_scores(N, P, q, gl, base, v0, c_visit, c_scale)
    lmax = max(L)
    pick = gumbel_argmax(score, [k for k in range(len(N)) if L[k] == lmax])
    lg = [math.log(float(P[k])) + sigma[k] if float(P[k]) > 0.0 else -math.inf for k in range(len(N))]
    mx = max(lg)
    if mx == -math.inf:
        return pick, None, np.array(score, np.float64), float(vmix)
    ex = [0.0 if x == -math.inf else math.exp(x - mx) for x in lg]
    tot = butterfly_sum(ex)
    return pick, np.array([F32(e / tot) for e in ex], F32), np.array(score, np.float64), float(vmix)


def solver_x(info, owner_player):
    """Value of a decided edge for the mover of the node that owns it (info bits 2..3 hold d + 1 for the child's mover)."""
    d = ((int(info) >> 2) & 3) - 1
    return d if (-1 if int(info) & INFO_WHITE else 1) == owner_player else -d


def solver_pick(acts, N, xs, picked_action):
    """lz_tree_solver_pick on a live root: `xs[k]` the value x of child k when it is decided, else None.  Returns the
    action played, given the one the finish picked."""
    kids = range(len(acts))
    most = lambda cs: max(cs, key=lambda k: (int(N[k]), -k))
    wins = [k for k in kids if xs[k] is not None and xs[k] > 0]
    if wins:
        return int(acts[most(wins)])
    lost = {int(acts[k]) for k in kids if xs[k] is not None and xs[k] < 0}
    rest = [k for k in kids if not (xs[k] is not None and xs[k] < 0)]
    if int(picked_action) in lost and rest:
        return int(acts[most(rest)])
    return int(picked_action)


def ref_finish(root, *, temperature, target_temperature=None, beta=0.0, force_uniform=False, sample_moves=False,
               uniform=None, out_cap=72, target_visits=None):
    """One root of lz_tree_finish.  `root`: a dict with ne, act, N, P, W, info, player, phase, status (game_status of the
    root state), root_visits, root_w, root_init_value, root_terminal.  `target_visits`: the pruned N' when the pruning rule
    is in force for this game.  Returns a dict: terminal, chosen_valid, chosen_index, chosen_code, child_count, root_value
    (float32), and for a live root policy (float64[220]), pol (the selection policy, float64[ne]), pick (edge index),
    child_action / child_visits / child_prior (the first min(ne, out_cap) children)."""
    ne = int(root["ne"])
    term = bool(root["root_terminal"]) or ne <= 0
    out = dict(terminal=term, chosen_valid=not term, chosen_index=-1, chosen_code=[-1, -1, -1, -1],
               child_count=0 if term else ne)
    if term:
        st = int(root["status"])
        out["root_value"] = F32(-1.0) if (ne == 0 and st == 0) else \
            F32((1.0 if st == int(root["player"]) else -1.0) if st in (1, -1) else 0.0)
        return out
    rv = int(root["root_visits"])
    out["root_value"] = F32(np.float64(root["root_w"]) / np.float64(rv)) if rv > 0 else F32(root["root_init_value"])
    N = np.asarray(root["N"], np.int64)
    P = np.asarray(root["P"], F32)
    act = np.asarray(root["act"], np.int64)
    white = (np.asarray(root["info"], np.int64) & INFO_WHITE) != 0
    q = child_q(root["W"], N, white, int(root["player"]))
    pol = policy(N, temperature)
    plain = target_temperature is None and not F32(beta) > 0 and target_visits is None
    tpol = pol if plain else policy(target_scores(N if target_visits is None else target_visits, P, beta),
                                    temperature if target_temperature is None else target_temperature)
    dense = np.zeros(220, np.float64)
    dense[act] = tpol
    if force_uniform and uniform is not None:
        pick = uniform_pick(uniform, ne)
    elif sample_moves and uniform is not None:
        pick = sampled_pick(pol, uniform)
    else:
        pick = deterministic_pick(N, q.astype(F32), P)
    m = min(ne, int(out_cap))
    out.update(policy=dense, pol=pol, pick=pick, q=q, child_action=act[:m], child_visits=N[:m], child_prior=P[:m])
    if pick >= 0:
        out["chosen_index"] = int(act[pick])
        out["chosen_code"] = index_to_code(int(root["phase"]), int(act[pick]))
    return out
