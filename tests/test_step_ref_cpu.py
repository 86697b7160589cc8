"""No GPU: the hand-built launches of tests/step_cases.py on the restatement of tests/step_ref.py alone (DESIGN.md section
33).  Three things: every case has the property it was built for (the restatement really walks the branch); the arena
check accepts every launch and rejects broken arenas; the comparison has teeth -- each deliberately wrong restatement
(step_ref.FLAWS) differs from the right one in compared bytes."""
import functools

import numpy as np
import pytest

from tests import hand_arenas as H
from tests import step_cases as K
from tests import step_ref as R


@functools.lru_cache(maxsize=None)
def trace(name, flaw=None):
    """Every step of a launch on the restatement: [(kind of step, image before, image after)]."""
    L = K.launch(name)
    img, out = L["img"], []
    for st in L["steps"]:
        if st[0] == "hand":
            img = st[1](img)
            continue
        step = "select" if st[0] == "select" else "root" if st[2] else "expand"
        if flaw is None:
            assert H.check_step_arena(img, step)
        after = R.ref_select(img, L["opts"], flaw) if step == "select" else R.ref_expand(img, st[1], L["opts"], st[2], flaw=flaw)[0]
        out.append((step, img, after))
        img = after
    return out


def game(img, tag):
    return img["tags"].index(tag)


def flips(img, g):
    cap, n = img["path_cap"], int(img["path_len"][g])
    return (img["path"][g * cap:g * cap + n].astype(np.int64) & H.PATH_FLIP) != 0


@pytest.mark.parametrize("name", K.NAMES)
def test_every_launch_is_a_mix_the_arena_check_accepts(name):
    t = trace(name)
    img = K.launch(name)["img"]
    assert img["B"] % 4 != 0 and 200 <= img["node_cap"] <= 520 and img["chunk"] in (128, 1024)
    sel = next(a for s, b, a in t if s == "select")
    assert int(sel["leaf_kind"][game(img, "extra:nan_depth3")]) == H.LEAF_INACTIVE
    assert int(sel["path_len"][game(img, "extra:nan_depth3")]) == 3
    for tag in ("extra:inactive", "extra:root_terminal"):
        g = game(img, tag)
        last = t[-1][2]
        assert last["root_terminal"][g] == 1 and (last["nodes"][g] == img["nodes"][g]).all()
    assert img["active"][game(img, "extra:inactive")] == 0
    # the side arrays are preset to values of their own, so that += 1 is told apart from = 1
    assert all(int(img[k][0]) == H.SIDE_PRESET[k] for k in H.SIDE)


def test_deep_lines_cross_the_blocks_of_64_with_both_kinds_of_edges():
    step, before, sel = trace("deep")[0]
    lens = sel["path_len"].tolist()
    for L in K.PATH_LENS + (144, 126, 125):
        assert L in lens, L
    kinds = {t.split(":")[2]: int(sel["leaf_kind"][g]) for g, t in enumerate(before["tags"]) if t.startswith("deep")}
    assert kinds["expand"] == H.LEAF_EXPAND and kinds["terminal"] == H.LEAF_TERMINAL and kinds["real"] == H.LEAF_TERMINAL
    odd_above_a_seam = same_both_sides = 0
    for g, t in enumerate(before["tags"]):
        n = int(sel["path_len"][g])
        if not t.startswith("deep") or n <= H.WAVE:
            continue
        f = flips(sel, g)
        if n >= 72:
            same_both_sides += int(not f[56:64].all() and not f[64:72].all())     # same-mover edges next to entry 64
        for seam in range(n - H.WAVE, 0, -H.WAVE):                   # the backup works down from the leaf in blocks of 64
            odd_above_a_seam += int(f[seam:].sum()) & 1
    assert odd_above_a_seam >= 3 and same_both_sides >= 6
    # the entry on top of a full block (lane 63) sits below an odd number of flips of its own block somewhere
    top = 0
    for g, t in enumerate(before["tags"]):
        n = int(sel["path_len"][g])
        if t.startswith("deep") and n >= H.WAVE:
            top += int(flips(sel, g)[n - H.WAVE:].sum()) & 1
    assert top >= 2
    # backed-up values: +1, -1, 0, a non-dyadic float32 and -0.0
    vals = {float(v) for v in K.launch("deep")["steps"][1][1]["values"]}
    assert {1.0, -1.0, 0.0, float(np.float32(0.3))} <= vals and any(np.signbit(v) and v == 0 for v in K.launch("deep")["steps"][1][1]["values"])
    # the leaf one ply before the end of the won line: every child finished
    exp = trace("deep")[1][2]
    g = game(before, "deep:125:all_children_finished")
    nd = exp["nodes"][g, int(exp["n_nodes"][g]) - 1]
    run = exp["edges"][int(nd["edge_begin"]):int(nd["edge_begin"]) + int(nd["nedges"])]
    assert ((run["n_info"] >> 24) & H.INFO_TERMINAL).all()
    # the leaf at ply 143: every child finished and DRAWN, with movers of both colours; with the won children above, the
    # terminal marks the expansions write hold value bits 1 and 2 and both white bits (a finished child that is lost for
    # its own mover, bits 0, appears nowhere in the playouts of 40 seeds)
    g143 = game(before, "deep:143:expand")
    nd = exp["nodes"][g143, int(exp["n_nodes"][g143]) - 1]
    info = exp["edges"]["n_info"][int(nd["edge_begin"]):int(nd["edge_begin"]) + int(nd["nedges"])] >> 24
    assert int(nd["nedges"]) >= 10 and (info & H.INFO_TERMINAL).all() and (((info >> 2) & 3) == 1).all()
    assert set((info & H.INFO_WHITE).tolist()) == {0, 1}
    assert ((run["n_info"] >> 26) & 3 == 2).all()
    # ... which the solver proves, and carries upward: R = drawn from the new run of the leaf at ply 143
    tags_s = K.launch("deep_solver")["img"]["tags"]
    s143 = tags_s.index("deep:143:expand")
    sel0, exp0 = trace("deep_solver")[0][2], trace("deep_solver")[1][2]
    e = int(sel0["leaf_edge"][s143])
    assert int(sel0["path_len"][s143]) == 143 and int(sel0["leaf_kind"][s143]) == H.LEAF_EXPAND
    assert (int(exp0["edges"]["n_info"][e]) >> 24) & ~H.INFO_WHITE == H.INFO_PROVEN | (1 << 2)
    assert int(exp0["solver_count"][s143]) >= H.SIDE_PRESET["solver_count"] + 1
    exp_s = trace("deep_solver")[1][2]
    assert int(exp_s["solver_count"][g]) > H.SIDE_PRESET["solver_count"]
    sel_s = trace("deep_solver")[0][2]
    tags_s = K.launch("deep_solver")["img"]["tags"]
    deep_decided = [g for g, t in enumerate(tags_s) if t.endswith("decided") and int(sel_s["path_len"][g]) > H.WAVE]
    assert deep_decided and all(int(sel_s["leaf_kind"][g]) == H.LEAF_TERMINAL for g in deep_decided)


def chosen(sel, g, depth):
    """Index inside its run of the edge a descent took at `depth`."""
    cap = sel["path_cap"]
    e = int(sel["path"][g * cap + depth]) & 0x7FFFFFFF
    node = 0
    for d in range(depth):
        node = int(sel["edges"]["child"][int(sel["path"][g * cap + d]) & 0x7FFFFFFF])
    return e - int(sel["nodes"][g, node]["edge_begin"])


def test_descent_cases_decide_what_they_were_built_to_decide():
    _, img, sel = trace("descent")[0]
    for tag, depth, want in (("tie:0,1", 0, 0), ("tie:5,63", 1, 5), ("tie:63,64", 1, 63), ("tie:64,71", 1, 64),
                             ("tie:64,70:of71", 1, 64), ("wide:65:last", 1, 64), ("negzero", 0, 1), ("one_nan", 0, 2),
                             ("single_child", 0, 0), ("f32:inside", 0, 1), ("f32:outside", 0, 1)):
        assert chosen(sel, game(img, tag), depth) == want, tag
    g = game(img, "nan_depth0")
    assert int(sel["leaf_kind"][g]) == H.LEAF_INACTIVE and int(sel["path_len"][g]) == 0 and int(sel["leaf_edge"][g]) == -1
    after = trace("descent")[1][2]
    assert (after["nodes"][g] == img["nodes"][g]).all() and int(after["eval_count"][g]) == H.SIDE_PRESET["eval_count"]
    g = game(img, "negzero")
    e = int(sel["path"][g * sel["path_cap"]]) & 0x7FFFFFFF
    assert np.signbit(img["edges"]["W"][e]) and np.signbit(after["edges"]["W"][e])        # -0.0 + -0.0
    _, img, sel = trace("big_n")[0]
    after = trace("big_n")[1][2]
    for g in range(3):
        e = int(sel["path"][g * sel["path_cap"]]) & 0x7FFFFFFF
        assert int(after["edges"]["n_info"][e]) & 0xFFFFFF == (1 << 24) - 1
        assert int(after["edges"]["n_info"][e]) >> 24 == int(img["edges"]["n_info"][e]) >> 24


def test_forced_solver_and_shape_cases():
    _, img, sel = trace("forced")[0]
    want = {"forced:equal": (0, 0), "forced:ulp_above": (2, 1), "forced:ulp_below": (0, 0), "forced:unvisited": (2, 0),
            "forced:wide:due_at_66": (66, 1)}                        # (edge taken, by the forced rule)
    for tag, (k, by_rule) in want.items():
        g = game(img, tag)
        assert chosen(sel, g, 0) == k, tag
        assert int(sel["forced_count"][g]) - H.SIDE_PRESET["forced_count"] == by_rule, tag
    _, img, sel = trace("solver")[0]
    for tag, depth, k in (("solver:win_in_slot1", 0, 1), ("solver:draw_vs_open", 0, 1), ("solver:draw_wins", 0, 0),
                          ("solver:wide:win_at_70", 1, 70), ("solver:wide:losses_below_64", 1, 66)):
        assert chosen(sel, game(img, tag), depth) == k, tag
    g = game(img, "solver:every_child_lost")
    assert int(sel["leaf_kind"][g]) == H.LEAF_TERMINAL and float(sel["leaf_value"][g]) in (-1.0, 1.0)
    _, img, sel = trace("shape")[0]
    assert chosen(sel, game(img, "shape:clamp"), 0) != 0                 # the clamp lets an unvisited child win
    flawed = trace("shape", "fpu_clamp_omitted")[0][2]
    assert chosen(flawed, game(img, "shape:clamp"), 0) == 0
    assert int(img["root_visits"][game(img, "shape:n_v=0")]) == 0 and int(img["root_visits"][game(img, "shape:table_last")]) > 3


def test_expansion_cases():
    t = trace("expansion")
    img, sel, exp = t[0][1], t[0][2], t[1][2]
    rows = K.launch("expansion")["steps"][2][1]
    for g, tag in enumerate(img["tags"]):
        if not tag.startswith("leaf:") or tag.endswith("good"):
            continue
        n = int(tag.split("=")[1].split(":")[0])
        nd = exp["nodes"][g, int(exp["n_nodes"][g]) - 1]
        assert int(nd["nedges"]) == n
        run = exp["edges"][int(nd["edge_begin"]):int(nd["edge_begin"]) + n]
        assert (run["P"] == np.float32(1.0) / np.float32(n)).all(), tag        # the uniform fallback
        legal = run["act"].astype(int)
        s = rows["priors220"][g, legal].sum()
        assert not (s > 0 and np.isfinite(s)), tag
    chunk = img["chunk"]
    off = lambda im, tag: int(im["n_edges"][game(img, tag)]) % chunk
    nch = lambda im, tag: int(im["n_chunks"][game(img, tag)])
    assert off(exp, "alloc:exact_fit") == 0 and nch(exp, "alloc:exact_fit") == nch(img, "alloc:exact_fit")
    assert nch(exp, "alloc:one_over") == nch(img, "alloc:one_over") + 1 and off(exp, "alloc:one_over") == 20
    assert off(img, "alloc:off_zero") == 0 and nch(exp, "alloc:off_zero") == nch(img, "alloc:off_zero") + 1
    assert off(exp, "alloc:one_under") == chunk - 1
    exp2 = t[3][2]                                                   # the next expansion of the exact fit starts at off == 0
    assert nch(exp2, "alloc:exact_fit") == nch(img, "alloc:exact_fit") + 1
    # no legal move below the root: the terminal mark with value bits 0, -1 backed up, no node, no chunk
    g = game(img, "nolegal:below_root")
    before = t[1][1]
    e = int(before["leaf_edge"][g])
    assert int(exp["edges"]["n_info"][e]) >> 24 == (int(before["edges"]["n_info"][e]) >> 24) | H.INFO_TERMINAL
    assert (int(exp["edges"]["n_info"][e]) >> 26) & 3 == 0 and int(exp["n_nodes"][g]) == int(before["n_nodes"][g])
    flip = bool(int(before["path"][g * before["path_cap"]]) & H.PATH_FLIP)
    assert float(exp["root_w"][g]) - float(before["root_w"][g]) == (1.0 if flip else -1.0)
    assert int(t[2][2]["leaf_kind"][g]) == H.LEAF_TERMINAL and float(t[2][2]["leaf_value"][g]) == -1.0      # the next visit
    ts = trace("solver")
    gs = game(ts[0][1], "nolegal:below_root")
    won = bool(int(ts[1][1]["path"][gs * ts[1][1]["path_cap"]]) & H.PATH_FLIP)      # lost for the leaf's mover: won for the other
    assert int(ts[1][2]["root_proven"][gs]) == (3 if won else 0)                       # ... which the climb carries to the root
    assert int(ts[1][2]["solver_count"][gs]) == H.SIDE_PRESET["solver_count"] + (2 if won else 1)
    # heads: the all -inf row and the overflowing row end in the fallback, exactly; the others are a softmax
    th = trace("expansion_heads")
    soft = R.ref_expand(th[1][1], K.launch("expansion_heads")["steps"][2][1], K.launch("expansion_heads")["opts"], False)[1]
    assert len(soft) >= 6


def test_refusal_sharing_and_full_window_cases():
    t = trace("refusal")
    img, exp = t[0][1], t[1][2]
    assert int(exp["pool_stats"][0]) == 3 and int(exp["pool_top"][0]) == 0
    for tag in ("refused:one_over", "refused:off_zero", "refused:one_over:b"):
        g = game(img, tag)
        assert int(exp["n_nodes"][g]) == int(img["n_nodes"][g]) and int(exp["root_visits"][g]) == int(img["root_visits"][g]) + 1
    g = game(img, "fits:exact_fit")
    assert int(exp["n_nodes"][g]) == int(img["n_nodes"][g]) + 1
    retry = t[3][2]
    for tag in ("refused:one_over", "refused:off_zero", "refused:one_over:b"):
        g = game(img, tag)
        assert int(retry["n_nodes"][g]) == int(img["n_nodes"][g]) + 1
    for name in ("sharing", "sharing_solver"):
        t = trace(name)
        before, exp = t[1][1], t[1][2]
        for tag in ("shared:n=20", "shared:n=2"):
            g = game(before, tag)
            assert int(before["leaf_kind"][g]) == H.LEAF_SHARED
            src, new = int(before["leaf_src"][g]), int(exp["n_nodes"][g]) - 1
            a, b = exp["nodes"][g, src], exp["nodes"][g, new]
            pa = exp["edges"]["P"][int(a["edge_begin"]):int(a["edge_begin"]) + int(a["nedges"])]
            pb = exp["edges"]["P"][int(b["edge_begin"]):int(b["edge_begin"]) + int(b["nedges"])]
            assert (pa.view(np.uint32) == pb.view(np.uint32)).all()
            assert exp["node_value"][g, new] == exp["node_value"][g, src] == np.float32(0.7123)
            assert int(exp["share_count"][g]) == H.SIDE_PRESET["share_count"] + 1
            assert (exp["pos_index"][g] == before["pos_index"][g]).all()                  # a shared leaf is not indexed
        g = game(before, "full_window:n=20")
        assert int(exp["n_nodes"][g]) == int(before["n_nodes"][g]) + 1 and (exp["pos_index"][g] == before["pos_index"][g]).all()
        g = game(before, "plain:n=20")
        assert (exp["pos_index"][g] != before["pos_index"][g]).sum() == 1


def test_root_step_cases():
    t = trace("root_noise")
    img, out = t[0][1], t[0][2]
    P = lambda im, g: im["edges"]["P"][int(im["nodes"][g, 0]["edge_begin"]):int(im["nodes"][g, 0]["edge_begin"]) + int(im["nodes"][g, 0]["nedges"])]
    g = game(img, "kept:ne=1")
    assert (P(out, g) == P(img, g)).all()                               # no mix on a single edge
    assert (P(trace("root_noise", "mix_at_one")[0][2], g) != P(img, g)).all()
    g = game(img, "kept:tiny_sum")
    assert 1e-4 < float(P(out, g).sum()) < 0.01                        # divided by 1e-8, not by the sum
    g = game(img, "fresh:n=1")
    assert (P(out, g) == 1.0).all() and int(out["pool_stats"][2]) == 0 and int(img["pool_stats"][2]) == 6
    g = game(img, "fresh:no_legal_move")                                # a fresh root without a legal move
    assert int(out["nodes"][g, 0]["nedges"]) == 0 and out["root_terminal"][g] == 1 and out["root_init_value"][g] == -1.0
    assert int(out["n_chunks"][g]) == 0 and int(out["eval_count"][g]) == H.SIDE_PRESET["eval_count"] + 1
    quiet = trace("root")[0][2]
    g = game(img, "fresh:bad_row")
    assert len(set(P(quiet, g).tolist())) == 1 and len(set(P(out, g).tolist())) > 1    # (the noise mix mends an all-zero row)
    for tag in ("kept:ne=2", "kept:ne=36"):
        g = game(img, tag)
        assert (P(quiet, g) == P(img, g)).all() and (P(out, g) != P(img, g)).any()
    s = trace("root_noise_solver")[0][2]
    for tag, p in (("kept:R=won", 3), ("kept:R=drawn", 2), ("kept:R=lost", 1), ("kept:R=open", 0)):
        assert int(s["root_proven"][game(img, tag)]) == p, tag
    w = trace("root_wide")
    assert int(w[0][1]["nodes"][0, 0]["nedges"]) == 72 and (P(w[0][2], 0) != P(w[0][1], 0)).all()


BREAKS = {
    "act_not_legal": lambda im, g: im["edges"]["act"].__setitem__(int(im["nodes"][g, 0]["edge_begin"]), 219),
    "act_repeats": lambda im, g: im["edges"]["act"].__setitem__(int(im["nodes"][g, 0]["edge_begin"]) + 1,
                                                               im["edges"]["act"][int(im["nodes"][g, 0]["edge_begin"])]),
    "no_room_for_a_node": None,
    "cursor_not_greedy": lambda im, g: im["n_edges"].__setitem__(g, int(im["n_edges"][g]) + 1),
    "child_state_not_successor": lambda im, g: im["nodes"]["state"][g, 1].__setitem__(2, int(im["nodes"]["state"][g, 1][2]) ^ 1),
    "player_bit": lambda im, g: im["edges"]["n_info"].__setitem__(int(im["nodes"][g, 0]["edge_begin"]),
                                                                  int(im["edges"]["n_info"][int(im["nodes"][g, 0]["edge_begin"])]) ^ (1 << 24)),
    "index_entry_past_n_nodes": lambda im, g: im["pos_index"][g].__setitem__(0, int(im["n_nodes"][g])),
    "index_entry_in_wrong_window": None,
    "count_about_to_overflow": lambda im, g: im["edges"]["n_info"].__setitem__(int(im["nodes"][g, 0]["edge_begin"]), (1 << 24) - 1),
    "node_under_terminal_edge": None,
    "chunk_owned_twice": lambda im, g: im["chunk_list"][g].__setitem__(0, int(im["chunk_list"][g + 1, 0])),
    "cbegin_wrong": None,
    "pool_half_empty": lambda im, g: im["pool_top"].__setitem__(0, 2),
    "fresh_root_below_the_root_step": None,
}


@pytest.mark.parametrize("what", sorted(BREAKS))
def test_arena_check_rejects_broken_arenas(what):
    img = H.copy_image(trace("deep")[1][1])                             # the image the first expand step starts from
    g = game(img, "deep:63:expand")
    step = "expand"
    e0 = int(img["nodes"][g, 0]["edge_begin"])
    if what == "index_entry_in_wrong_window":
        tab = img["pos_index"][g]
        s = int(np.flatnonzero(tab >= 1)[0])
        tab[(s + 200) % len(tab)], tab[s] = tab[s], -1
    elif what == "node_under_terminal_edge":
        k = int(np.flatnonzero(img["edges"]["child"][e0:e0 + int(img["nodes"][g, 0]["nedges"])] >= 0)[0])
        img["edges"]["n_info"][e0 + k] |= np.uint32(H.INFO_TERMINAL << 24)
    elif what == "cbegin_wrong":
        k = int(np.flatnonzero(img["edges"]["child"][e0:e0 + int(img["nodes"][g, 0]["nedges"])] >= 0)[0])
        img["edges"]["cbegin"][e0 + k] += 1
    elif what == "fresh_root_below_the_root_step":
        img = H.copy_image(K.launch("root")["img"])
    elif what == "no_room_for_a_node":                                  # an arena whose game fills its node_cap
        full = K.StepGame("full", K.position(3, 50))
        full.line(K.line_of(3)[1][50:53])
        img = H.build_step_image([full], len(full.nodes), 128, 5)
        assert int(img["n_nodes"][0]) == img["node_cap"] and H.check_arena(img)
        with pytest.raises(AssertionError, match="no room for the node"):
            H.check_step_arena(img, step)
        return
    else:
        BREAKS[what](img, g)
    with pytest.raises(AssertionError):
        H.check_step_arena(img, step)


WHERE = {
    "parity_not_carried": "deep", "last_index_on_ties": "descent", "forced_le": "forced", "uniform_fallback_omitted": "expansion",
    "fpu_clamp_omitted": "shape", "mix_at_one": "root_noise", "source_value_not_taken": "sharing",
    "run_straddles_chunk": "expansion", "root_w_unflipped": "deep", "terminal_bits_off_by_one": "deep",
    "nan_level_descends": "descent", "shared_leaf_indexed": "sharing", "refusal_not_counted": "refusal",
}


@pytest.mark.parametrize("flaw", R.FLAWS)
def test_a_wrong_restatement_differs_in_compared_bytes(flaw):
    right, wrong = trace(WHERE[flaw]), trace(WHERE[flaw], flaw)
    assert any(R.diff_step(a[2], b[2]) for a, b in zip(right, wrong)), flaw
