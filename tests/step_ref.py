"""lz_tree_select / lz_tree_expand restated: `ref_select` and `ref_expand` are sequential Python
written from the contract of include/liuzhou_hip.h (the LzTreeDesc comments), one game after the other on an image of
tests/hand_arenas.py, and `diff_step` is the whole-image byte comparison with the few bytes the contract leaves open
masked out.  Rules come from the oracle (legal actions, successors, game status).

Everything on the priors220 path is + * / sqrt and comparisons on IEEE types and is compared bit for bit.  The heads path
contains expf: its priors are a float64 softmax here and are compared under HEADS_TOL (`settle_heads`), every other field
of a heads case exactly.

`flaw` names one deliberate mistake (FLAWS): tests/test_step_ref_cpu.py shows that each one changes compared bytes."""
import math

import numpy as np

from tests.advance_ref import pos_hash
from tests.hand_arenas import (BUFFERS, INFO_DECIDED, INFO_PROVEN, INFO_TERMINAL, INFO_WHITE, LEAF_EXPAND, LEAF_INACTIVE,
                               LEAF_REUSED_ROOT, LEAF_SHARED, LEAF_TERMINAL, PATH_FLIP, SIDE, WAVE, copy_image,
                               cs_from_packed, edge_info_for, packed_from_cs)

F32 = np.float32
FIX = 1073741824.0                                                   # 2^30: the fixed point of S
# Largest |P(device) - P(float64 softmax)| over every heads case, measured on an MI355X: 1.192e-7.
# Four times that; below the 1e-6 tests/tree_parity.replay_part_in_oracle grants production priors.
HEADS_MEASURED = 1.192e-7
HEADS_TOL = 4 * HEADS_MEASURED
FLAWS = ("parity_not_carried", "last_index_on_ties", "forced_le", "uniform_fallback_omitted", "fpu_clamp_omitted",
         "mix_at_one", "source_value_not_taken", "run_straddles_chunk", "root_w_unflipped", "terminal_bits_off_by_one",
         "nan_level_descends", "shared_leaf_indexed", "refusal_not_counted")


def options(c_puct=1.0, forced_k=0.0, solver=False, fpu=None, fpu_root=None, cpuct=None):
    """The search options of a launch.  `cpuct`: None or (cpuct_log, cpuct_base, table length) of TreeEngine.set_puct_shape;
    `table` is then the float64 c(n_v) table the host builds from them and uploads -- an input of the step, not restated."""
    from liuzhou_amd.puct_shape import cpuct_table
    table = None if cpuct is None else np.array(cpuct_table(float(c_puct), cpuct[0], cpuct[1], cpuct[2]), np.float64)
    return dict(c_puct=float(c_puct), forced_k=float(forced_k), solver=bool(solver), fpu=fpu,
                fpu_root=fpu if fpu_root is None else fpu_root, cpuct=cpuct, table=table)


def _info(ni):
    return int(ni) >> 24


def _x(info, owner_player):
    """Value of a decided edge for the mover of the node that owns it."""
    d = ((info >> 2) & 3) - 1
    return d if (-1 if info & INFO_WHITE else 1) == owner_player else -d


def node_rule(infos, owner_player):
    """R(X): 0 undecided, else the proven value for X's mover + 2."""
    dec = [(i & INFO_DECIDED) != 0 for i in infos]
    xs = [_x(i, owner_player) for i in infos]
    if any(d and x > 0 for d, x in zip(dec, xs)):
        return 3
    if not all(dec):
        return 0
    return 2 if any(x == 0 for x in xs) else 1


def _player(packed):
    return -1 if (int(packed[0]) >> 53) & 1 else 1


# ---- select -----------------------------------------------------------------------------------------------------------
def choose(run, n_v, player, depth, node_W, init_v, opts, flaw=None):
    """Index of the child a descent takes on one level, or None (no score compares greater than -inf), and whether the
    forced rule took it."""
    ne = len(run)
    N = (run["n_info"] & 0xFFFFFF).astype(np.int64)
    info = (run["n_info"] >> 24).astype(np.int64)
    P = run["P"].astype(np.float64)
    W = run["W"]
    if depth == 0 and opts["forced_k"] > 0.0:
        for k in range(ne):
            n = float(N[k])
            lhs, rhs = n * n, (opts["forced_k"] * P[k]) * float(n_v)
            if n > 0.0 and (lhs <= rhs if flaw == "forced_le" else lhs < rhs):
                return k, True
    cand = [True] * ne
    solver = opts["solver"]
    if solver:
        x = [_x(int(i), player) if i & INFO_DECIDED else None for i in info]
        for k in range(ne):
            if x[k] is not None and x[k] > 0:
                return k, False
        keep = [not (v is not None and v < 0) for v in x]
        if any(keep):
            cand = keep
    sq = math.sqrt(float(max(n_v, 1)))
    c = opts["c_puct"]
    if opts["table"] is not None:
        c = float(opts["table"][min(max(n_v, 0), len(opts["table"]) - 1)])
    f = 0.0
    if opts["fpu"] is not None:
        S = sum(int(P[k] * FIX) for k in range(ne) if N[k] > 0)
        with np.errstate(all="ignore"):
            V = float(np.float64(node_W) / np.float64(n_v)) if n_v > 0 else float(init_v)
        red = (opts["fpu_root"] if depth == 0 else opts["fpu"]) * math.sqrt(float(S) / FIX)
        f = V - red
        if f < -1.0 and flaw != "fpu_clamp_omitted":
            f = -1.0
    best, best_k = -math.inf, None
    with np.errstate(all="ignore"):
        for k in range(ne):
            if not cand[k]:
                continue
            n = int(N[k])
            q = 0.0
            if solver and info[k] & INFO_DECIDED:
                q = float(_x(int(info[k]), player))
            elif n > 0:
                mv = float(np.float64(W[k]) / np.float64(n))
                q = mv if (-1 if info[k] & INFO_WHITE else 1) == player else -mv
            elif opts["fpu"] is not None:
                q = f
            sc = q + c * P[k] * sq / (1.0 + float(n))
            if sc > best or (flaw == "last_index_on_ties" and sc == best and best_k is not None):
                best, best_k = sc, k
    return best_k, False


def ref_select(img, opts, flaw=None):
    """The image lz_tree_select leaves (the look-ups of shared positions are off in this entry point)."""
    from oracle import lz_oracle as O
    out = copy_image(img)
    cap = img["path_cap"]
    for g in range(img["B"]):
        if img["root_terminal"][g]:
            out["leaf_kind"][g] = LEAF_INACTIVE
            continue
        nodes = img["nodes"][g]
        ne, e0 = int(nodes[0]["nedges"]), int(nodes[0]["edge_begin"])
        node, depth, n_v = 0, 0, int(img["root_visits"][g])
        player = _player(nodes[0]["state"])
        node_W, init_v = float(img["root_w"][g]), float(img["root_init_value"][g])
        kind, term, leaf_edge, action = LEAF_INACTIVE, 0.0, -1, 0
        while ne > 0:
            run = img["edges"][e0:e0 + ne]
            k, forced = choose(run, n_v, player, depth, node_W, init_v, opts, flaw)
            if k is None:
                if flaw == "nan_level_descends":
                    k = 0
                else:
                    break
            if forced:
                out["forced_count"][g] += 1
            info = _info(run["n_info"][k])
            child_player = -1 if info & INFO_WHITE else 1
            leaf_edge = e0 + k
            out["path"][g * cap + depth] = np.uint32(leaf_edge | (PATH_FLIP if child_player != player else 0)).astype(np.int32)
            depth += 1
            if info & (INFO_DECIDED if opts["solver"] else INFO_TERMINAL):
                kind, term = LEAF_TERMINAL, float(((info >> 2) & 3) - 1)
                break
            if int(run["child"][k]) < 0:
                kind, action = LEAF_EXPAND, int(run["act"][k])
                break
            node_W, n_v, player = float(run["W"][k]), int(run["n_info"][k]) & 0xFFFFFF, child_player
            node, e0, ne = int(run["child"][k]), int(run["cbegin"][k]), int(run["cn"][k])
            assert depth < cap - 1, "a chain as long as path_cap: out of scope"
        out["path_len"][g], out["leaf_kind"][g], out["leaf_value"][g] = depth, kind, term
        out["leaf_edge"][g], out["leaf_parent"][g] = leaf_edge, node
        if kind == LEAF_EXPAND:
            out["leaf_state"][g] = packed_from_cs(O.apply_index(cs_from_packed(nodes[node]["state"]), action))
    return out


# ---- expand + backup --------------------------------------------------------------------------------------------------
def heads_logits(lp1, lp2, lpm, legal):
    """Logit of every legal action from the three 36-wide heads, float32: p1[cell] for a placement, p2[from] + p1[dest]
    (one float32 addition) for a move, pm[cell] for a selection, 0 for the process action."""
    out = []
    with np.errstate(all="ignore"):
        for a in legal:
            if a < 36:
                x = F32(lp1[a])
            elif a < 180:
                frm, d = (a - 36) >> 2, (a - 36) & 3
                dest = frm + (-6, 6, -1, 1)[d]
                x = F32(lp2[frm]) + F32(lp1[dest])
            elif a < 216:
                x = F32(lpm[a - 180])
            else:
                x = F32(0.0)
            out.append(x)
    return np.array(out, F32)


def priors_for(legal, g, rows, is_root, flaw=None):
    """(priors float32[n], exact): the priors a new run gets.  exact is False where expf is involved (heads path, a row
    that is not `bad`): those are a float64 softmax, to be compared under HEADS_TOL."""
    n = len(legal)
    noise, eps = rows.get("noise"), F32(rows.get("epsilon", 0.25))
    mix = is_root and noise is not None and (n > 1 or flaw == "mix_at_one")
    keep = F32(1.0 - float(eps))
    uniform = np.full(n, F32(1.0) / F32(n), F32)
    with np.errstate(all="ignore"):
        if rows.get("priors220") is not None:
            val = np.asarray(rows["priors220"], F32)[g, legal]
            if mix:
                val = (keep * val).astype(F32) + (eps * np.asarray(noise, F32)[g, :n]).astype(F32)
            psum = F32(0.0)
            for v in val:
                psum = F32(psum + v)
            bad = not (psum > 0) or not np.isfinite(psum)
            if bad and flaw != "uniform_fallback_omitted":
                return uniform, True
            return (val / psum).astype(F32), True
        lp1, lp2, lpm = (np.asarray(h, F32)[g] for h in rows["heads"])
        x = heads_logits(lp1, lp2, lpm, legal).astype(np.float64)
        e = np.exp(x - np.max(x[~np.isnan(x)]) if (~np.isnan(x)).any() else x)
        p = e / e.sum()
        if not np.isfinite(p).all():                                  # every such row ends in the uniform fallback, exactly
            if mix:                                                   # (the mix of NaN priors stays NaN)
                pass
            return uniform, True
        if mix:
            p = (1.0 - float(eps)) * p + float(eps) * np.asarray(noise, np.float64)[g, :n]
            p = p / p.sum()
        return p.astype(F32), False


def take_chunk(out, g, for_root, taken, flaw=None):
    """The first pool index of a new chunk for game g, or -1 (refused and counted)."""
    nc = int(out["n_chunks"][g])
    if nc >= out["chunk_cap"]:
        out["pool_stats"][0] += 1
        return -1
    top = int(out["pool_top"][0]) - 1
    reserved = 0 if for_root else int(out["pool_stats"][2])
    if top < reserved:
        if flaw != "refusal_not_counted":
            out["pool_stats"][0] += 1
        return -1
    pending = int(out["n_nodes"][g]) == 1 and int(out["nodes"][g, 0]["nedges"]) < 0 and int(out["root_terminal"][g]) == 0
    if for_root and pending:
        out["pool_stats"][2] -= 1
    out["pool_top"][0] = top
    out["pool_stats"][1] = min(int(out["pool_stats"][1]), top)
    cid = int(out["free_chunks"][top]) if taken is None else int(taken[g])
    out["chunk_list"][g, nc] = cid
    out["n_chunks"][g] = nc + 1
    return cid * out["chunk"]


def _mark(out, e, bits):
    out["edges"]["n_info"][e] |= np.uint32(bits << 24)


def ref_expand(img, rows, opts, is_root, taken=None, flaw=None):
    """(image lz_tree_expand leaves, [(first edge, n)] of the runs whose priors are a float64 softmax).  `taken`: per game
    the chunk id it took in this launch -- which of the free chunks goes to which game follows the order of an atomic, so
    the device's own assignment is passed in after `chunk_assignment` has checked it; None: in game order."""
    from oracle import lz_oracle as O
    out = copy_image(img)
    soft = []
    cap, chunk = img["path_cap"], img["chunk"]
    edges = out["edges"]
    solver = opts["solver"]
    values = np.asarray(rows["values"], F32)
    for g in range(img["B"]):
        kind = int(img["leaf_kind"][g])
        nodes = out["nodes"][g]
        if kind == LEAF_INACTIVE:
            continue
        if kind == LEAF_REUSED_ROOT:
            if not is_root:
                continue
            ne, e0 = int(nodes[0]["nedges"]), int(nodes[0]["edge_begin"])
            noise = rows.get("noise")
            if noise is not None and (ne > 1 or (flaw == "mix_at_one" and ne == 1)):
                eps = F32(rows.get("epsilon", 0.25))
                keep = F32(1.0 - float(eps))
                with np.errstate(all="ignore"):
                    pr = (keep * edges["P"][e0:e0 + ne]).astype(F32) + (eps * np.asarray(noise, F32)[g, :ne]).astype(F32)
                    psum = F32(0.0)
                    for v in pr:
                        psum = F32(psum + v)
                    denom = F32(1e-8) if psum < F32(1e-8) else psum
                    edges["P"][e0:e0 + ne] = (pr / denom).astype(F32)
            if solver and ne > 0:
                p = node_rule([_info(v) for v in edges["n_info"][e0:e0 + ne]], _player(nodes[0]["state"]))
                if p:
                    out["root_proven"][g] = p
                    out["solver_count"][g] += 1
            continue
        plen = 0 if is_root else int(img["path_len"][g])
        leaf_edge = int(img["leaf_edge"][g])
        sol, sol_terminal, leaf_player = 0, False, 1
        if kind == LEAF_TERMINAL:
            v = float(img["leaf_value"][g])
        else:
            shared = (not is_root) and kind == LEAF_SHARED
            out["share_count" if shared else "eval_count"][g] += 1
            leaf = cs_from_packed(img["leaf_state"][g])
            leaf_player = leaf.player
            legal = O.legal_indices_py(leaf)
            n = len(legal)
            src = int(img["leaf_src"][g]) if shared else -1
            value = F32(img["node_value"][g, src]) if shared and flaw != "source_value_not_taken" else values[g]
            if n == 0:
                v = -1.0
                if is_root:
                    if int(out["n_nodes"][g]) == 1 and int(nodes[0]["nedges"]) < 0 and int(out["root_terminal"][g]) == 0:
                        out["pool_stats"][2] -= 1
                    nodes[0]["nedges"], out["root_terminal"][g], out["root_init_value"][g] = 0, 1, -1.0
                else:
                    _mark(out, leaf_edge, INFO_TERMINAL | (4 if flaw == "terminal_bits_off_by_one" else 0))
                    if solver:
                        sol, sol_terminal = 1, True
            else:
                if shared:
                    sb = int(nodes[src]["edge_begin"])
                    pri, exact = edges["P"][sb:sb + n].copy(), True
                else:
                    pri, exact = priors_for(legal, g, rows, is_root, flaw)
                e0 = int(out["n_edges"][g])
                off = e0 & (chunk - 1)
                if off == 0 or (off + n > chunk and flaw != "run_straddles_chunk"):
                    e0 = take_chunk(out, g, is_root, taken, flaw)
                if e0 >= 0:
                    out["n_edges"][g] = e0 + n
                    if is_root:
                        nid = 0
                    else:
                        nid = int(out["n_nodes"][g])
                        out["n_nodes"][g] = nid + 1
                        edges["child"][leaf_edge], edges["cbegin"][leaf_edge], edges["cn"][leaf_edge] = nid, e0, n
                        nodes[nid]["state"], nodes[nid]["parent"] = img["leaf_state"][g], int(img["leaf_parent"][g])
                        out["node_value"][g, nid] = value
                        if not shared or flaw == "shared_leaf_indexed":
                            tab, mask = out["pos_index"][g], img["pos_slots"] - 1
                            h = pos_hash(img["leaf_state"][g])
                            for p in range(WAVE):
                                t = int(tab[(h + p) & mask])
                                if t < 1 or t >= nid:
                                    tab[(h + p) & mask] = nid
                                    break
                    nodes[nid]["edge_begin"], nodes[nid]["nedges"] = e0, n
                    infos = []
                    for k, a in enumerate(legal):
                        info = edge_info_for(O.apply_index(leaf, a))
                        if flaw == "terminal_bits_off_by_one" and info & INFO_TERMINAL:
                            info ^= 4
                        infos.append(info)
                        rec = edges[e0 + k:e0 + k + 1]
                        rec.view(np.uint8)[:] = 0
                        rec["P"], rec["n_info"], rec["child"], rec["act"] = pri[k], info << 24, -1, a
                    if not exact:
                        soft.append((e0, n))
                    if solver:
                        sol = node_rule(infos, leaf.player)
                if is_root:
                    out["root_init_value"][g] = value
                v = float(value)
        if is_root:
            if solver and sol:
                out["root_proven"][g] = sol
                out["solver_count"][g] += 1
            continue
        if plen <= 0:
            continue
        # backup: one addition per edge; the sign of entry j is the parity of the flip bits above it
        path = img["path"][g * cap:g * cap + plen].astype(np.int64) & 0xFFFFFFFF
        flips = 0
        for j in range(plen - 1, -1, -1):
            e = int(path[j]) & 0x7FFFFFFF
            par = flips
            if flaw == "parity_not_carried":                         # only the flips inside the entry's own block of 64
                hi = plen - WAVE * ((plen - 1 - j) // WAVE)
                par = sum(1 for i in range(j + 1, hi) if path[i] & PATH_FLIP)
            edges["n_info"][e] += np.uint32(1)
            edges["W"][e] = np.float64(edges["W"][e]) + np.float64(-v if par & 1 else v)
            flips += 1 if path[j] & PATH_FLIP else 0
        out["root_visits"][g] += 1
        rv = -v if flips & 1 and flaw != "root_w_unflipped" else v
        out["root_w"][g] = np.float64(img["root_w"][g]) + np.float64(rv)
        if solver and sol:
            marks = 1
            if not sol_terminal:
                _mark(out, leaf_edge, INFO_PROVEN | ((sol - 1) << 2))
            j = plen - 1
            while True:
                if j == 0:
                    ye0, yne, yp = int(nodes[0]["edge_begin"]), int(nodes[0]["nedges"]), _player(nodes[0]["state"])
                else:
                    e_up = int(path[j - 1]) & 0x7FFFFFFF
                    up = edges[e_up]
                    if _info(up["n_info"]) & INFO_DECIDED or int(up["child"]) < 0:
                        break
                    ye0, yne, yp = int(up["cbegin"]), int(up["cn"]), (-1 if _info(up["n_info"]) & INFO_WHITE else 1)
                p = node_rule([_info(x) for x in edges["n_info"][ye0:ye0 + yne]], yp)
                if p == 0:
                    break
                if j == 0:
                    if int(out["root_proven"][g]) == 0:
                        out["root_proven"][g] = p
                        marks += 1
                    break
                _mark(out, e_up, INFO_PROVEN | ((p - 1) << 2))
                marks += 1
                j -= 1
            out["solver_count"][g] += marks
    return out, soft


# ---- comparison -------------------------------------------------------------------------------------------------------
def chunk_assignment(before, got):
    """Per game the chunk id it took in the launch between `before` and `got` (None where it took none), after asserting
    that the chunks taken are exactly the top entries of the free stack, each once."""
    taken, ids = {}, []
    for g in range(before["B"]):
        a, b = int(before["n_chunks"][g]), int(got["n_chunks"][g])
        assert b in (a, a + 1), (g, "n_chunks")
        if b == a + 1:
            taken[g] = int(got["chunk_list"][g, a])
            ids.append(taken[g])
    t0, t1 = int(before["pool_top"][0]), int(got["pool_top"][0])
    assert t0 - t1 == len(ids), ("pool_top", t0, t1, len(ids))
    assert sorted(ids) == sorted(before["free_chunks"][t1:t0].tolist()), "the chunks taken are not the top of the stack"
    return taken


def settle_heads(want, got, soft):
    """Largest |P(got) - P(want)| over the runs whose priors are a float64 softmax; asserts it under HEADS_TOL and then
    takes the device's priors into `want`, so that the byte comparison covers every other field of those records."""
    worst = 0.0
    for e0, n in soft:
        a, b = want["edges"]["P"][e0:e0 + n].astype(np.float64), got["edges"]["P"][e0:e0 + n].astype(np.float64)
        assert np.isfinite(b).all(), (e0, "a prior of a good heads row is not finite")
        worst = max(worst, float(np.abs(a - b).max()))
        want["edges"]["P"][e0:e0 + n] = got["edges"]["P"][e0:e0 + n]
    print(f"heads priors: largest |device - float64 softmax| = {worst:.3e} (bound {HEADS_TOL:.3e})")
    assert worst <= HEADS_TOL, worst
    return worst


def diff_step(want, got):
    """Names (with the first differing places) of the buffers and side arrays in which `got` differs from `want`.  Every
    byte is compared: other games, the 0xA5 filler, records beyond n_nodes, path entries beyond path_len, chunk lists, the
    free stack.  No mask: the only freedoms of the contract (which free chunk a game gets, expf) are settled before the
    comparison by `chunk_assignment` and `settle_heads`."""
    bad = []
    for name in tuple(BUFFERS) + SIDE:
        a = np.ascontiguousarray(want[name]).view(np.uint8).reshape(-1)
        b = np.ascontiguousarray(got[name]).view(np.uint8).reshape(-1)
        ne = np.flatnonzero(a != b)
        if len(ne):
            item = want[name].dtype.itemsize
            first = int(ne[0] // item)
            bad.append((name, (ne[:6] // item).tolist(), (ne[:6] % item).tolist(),
                        f"want {want[name].reshape(-1)[first]!r} got {got[name].reshape(-1)[first]!r}"))
    return bad
