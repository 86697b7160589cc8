"""lz_tree_advance restated: `ref_advance` is a sequential restatement written from the contract,
`verify_advance` an independent declarative check of an (image before, image after) pair that never calls it, and
`diff_images` the byte comparison of two images with exactly the bytes the contract leaves unspecified masked out.
Images: tests/hand_arenas.py.  Everything is integers and copied bits; no tolerance anywhere."""
import numpy as np

from tests.hand_arenas import BUFFERS, INFO_TERMINAL, WAVE, copy_image, packed_status, run_indices

M64 = (1 << 64) - 1
LEAF_INACTIVE, LEAF_EXPAND, LEAF_REUSED_ROOT = 0, 1, 3
FLAWS = ("rank_off_by_one", "cbegin_untranslated", "cn_kept_on_cut_child", "run_straddles_chunk", "cut_one_word_late",
         "budget_ge", "parent_unranked", "node_value_not_moved", "one_chunk_too_many", "stale_table_entry",
         "child_kept_on_cut_child", "root_w_negated", "terminal_bit_ignored")


def pos_hash(state):
    """pos_hash of csrc/lz_tree_dev.h with Python integers: the slot of a packed state before masking."""
    w0, w1, w2, w3 = (int(v) & M64 for v in state)
    h = (w0 * 0x9E3779B97F4A7C15) & M64
    h = ((h ^ (h >> 29) ^ w1) * 0xBF58476D1CE4E5B9) & M64
    h = ((h ^ (h >> 31) ^ w2) * 0x94D049BB133111EB) & M64
    h = ((h ^ (h >> 27) ^ w3) * 0x9E3779B97F4A7C15) & M64
    return h >> 32


def keep_decision(img, g, flaw=None):
    """(index of the played edge in the root's run, child id) if game g keeps a subtree, else None."""
    nd = img["nodes"][g, 0]
    ne, e0, played = int(nd["nedges"]), int(nd["edge_begin"]), int(img["played"][g]) if img["played"] is not None else -1
    if not img["active"][g] or (img["reset"] is not None and img["reset"][g]) or img["root_terminal"][g] or ne <= 0 or played < 0:
        return None
    run = img["edges"][e0:e0 + ne]
    hit = np.flatnonzero(run["act"] == played)
    if not len(hit):
        return None
    k = int(hit[0])
    child = int(run["child"][k])
    if child <= 0 or ((int(run["n_info"][k]) >> 24) & INFO_TERMINAL and flaw != "terminal_bit_ignored"):
        return None
    if not (img["nodes"][g, child]["state"] == img["root_state"][g]).all():
        return None
    return k, child


def begin_game_ref(out, g):
    """What lz_tree_begin leaves for game g's root state and active flag (lz_tree_dev.h begin_game), its chunks aside."""
    was = int(out["n_nodes"][g]) == 1 and int(out["nodes"][g, 0]["nedges"]) < 0 and int(out["root_terminal"][g]) == 0
    rs = out["root_state"][g]
    nd = out["nodes"][g]
    nd["state"][0], nd["edge_begin"][0], nd["nedges"][0], nd["parent"][0] = rs, 0, -1, -1
    out["n_nodes"][g], out["n_edges"][g], out["root_visits"][g], out["root_w"][g] = 1, 0, 0, 0.0
    out["root_init_value"][g], out["path_len"][g] = 0.0, 0
    dead = packed_status(rs[0], rs[1]) != 0 or not out["active"][g]
    out["root_terminal"][g] = 1 if dead else 0
    out["leaf_kind"][g] = LEAF_INACTIVE if dead else LEAF_EXPAND
    out["pool_stats"][2] += int(not dead) - int(was)
    out["leaf_state"][g], out["leaf_value"][g] = rs, 0.0


def _release(out, g, keep):
    nc = int(out["n_chunks"][g])
    if nc > keep:
        top = int(out["pool_top"][0])
        out["free_chunks"][top:top + nc - keep] = out["chunk_list"][g, keep:nc]
        out["pool_top"][0] = top + nc - keep
        out["n_chunks"][g] = keep


def _table(out, g, kept, clear=True):
    if clear:
        out["pos_index"][g] = -1
    tab = out["pos_index"][g].tolist()
    mask, room = len(tab) - 1, tab.count(-1)
    for i, s in enumerate(out["nodes"][g, :kept]["state"].tolist()):
        if i == 0:
            continue
        if room == 0:                                                # every window is full from here on
            break
        h = pos_hash(s)
        for p in range(WAVE):
            if tab[(h + p) & mask] == -1:
                tab[(h + p) & mask] = i
                room -= 1
                break
    out["pos_index"][g] = tab


def ref_advance(image, played=None, reset=None, next_sims=None, flaw=None):
    """The expected image after lz_tree_advance and (dropped, pruned).  The position index of a kept game is filled in
    node order (the device fills it in the order of an atomic: compare it with verify_advance, not bit for bit).
    `flaw`: one of FLAWS -- a deliberately wrong restatement (tests/test_advance_ref_cpu.py)."""
    assert flaw is None or flaw in FLAWS
    img = copy_image(image)
    if played is not None or reset is not None or next_sims is not None:
        img["played"], img["reset"], img["next_sims"] = played, reset, int(next_sims)
    out = copy_image(img)
    cap, chunk = img["node_cap"], img["chunk"]
    budget = cap - (img["next_sims"] + 1)
    assert budget >= 0
    dropped = pruned = 0
    out["info"] = info = []                     # per game, for the tag checks of the cases: what the restatement did
    for g in range(img["B"]):
        kd = keep_decision(img, g, flaw)
        nn = int(img["n_nodes"][g])
        old = None
        info.append(dict(fresh=True, dropped=False, pruned=False, kept=0, cut_word=None, ci=-1, k_played=-1, c=-1, old=None))
        if kd is not None:
            k_played, c = kd
            nodes = img["nodes"][g, :nn]
            par = nodes["parent"]
            ins = np.zeros(nn, bool)
            ins[c] = True
            for i in range(c + 1, nn):
                if ins[par[i]]:
                    ins[i] = True
            kept, cut = 0, False
            for w in range((nn + WAVE - 1) // WAVE):
                n_w = int(ins[w * WAVE:(w + 1) * WAVE].sum())
                over = kept + n_w >= budget if flaw == "budget_ge" else kept + n_w > budget
                if over:
                    cut = True
                    info[g]["cut_word"] = w
                    if flaw == "cut_one_word_late":
                        kept += n_w
                        w += 1
                    ins[w * WAVE:] = False
                    break
                kept += n_w
            info[g].update(k_played=k_played, c=c, dropped=kept == 0)
            if kept == 0:
                dropped += 1
            else:
                pruned += int(cut)
                old = np.flatnonzero(ins)
        if old is None:
            _release(out, g, 0)
            out["pos_index"][g] = -1
            begin_game_ref(out, g)
            continue
        # ---- nodes ----
        rank = np.cumsum(ins) - 1
        rec = nodes[old].copy()
        if flaw != "parent_unranked":
            rec["parent"] = np.where(old == c, -1, rank[np.maximum(nodes["parent"][old], 0)])
        if flaw != "node_value_not_moved":
            out["node_value"][g, :kept] = img["node_value"][g, old]
        # ---- runs: greedy along the game's own chunk list from its start ----
        lst = img["chunk_list"][g]
        n_chunks = int(img["n_chunks"][g])
        ci, off = 0, 0
        cnt = np.maximum(rec["nedges"], 0).astype(np.int64)
        new_begin = np.zeros(kept, np.int64)
        for i in range(kept):
            n = int(cnt[i])
            if n == 0:
                continue
            if off + n > chunk:
                if flaw == "run_straddles_chunk" and off < chunk and int(lst[ci]) + 1 < img["pool_chunks"]:
                    new_begin[i] = int(lst[ci]) * chunk + off
                    ci, off = ci + 1, 0
                    assert ci < n_chunks
                    continue
                ci, off = ci + 1, 0
                assert ci < n_chunks, (g, "the packing ran past the chunk list")
            new_begin[i] = int(lst[ci]) * chunk + off
            off += n
        old_begin = rec["edge_begin"].astype(np.int64)
        rec["edge_begin"] = new_begin
        out["nodes"][g, :kept] = rec
        # ---- edges ----
        src, _ = run_indices(old_begin, cnt)
        dst, _ = run_indices(new_begin, cnt)
        e = img["edges"][src].copy()
        ch = e["child"].astype(np.int64)
        has = ch >= 0
        stays = has & ins[np.where(has, ch, 0)]
        gone = has & ~stays
        r = rank[ch[stays]]
        e["child"][stays] = r + (1 if flaw == "rank_off_by_one" else 0)
        if flaw != "cbegin_untranslated":
            e["cbegin"][stays] = new_begin[r]
        if flaw != "child_kept_on_cut_child":
            e["child"][gone] = -1
        e["cbegin"][gone] = 0
        if flaw != "cn_kept_on_cut_child":
            e["cn"][gone] = 0
        out["edges"][dst] = e
        # ---- scalars, chunks, table ----
        keep = ci + 1 + (1 if flaw == "one_chunk_too_many" and ci + 1 < n_chunks else 0)
        _release(out, g, keep)
        root_run = img["edges"][int(nodes["edge_begin"][0]):int(nodes["edge_begin"][0]) + int(nodes["nedges"][0])]
        out["n_nodes"][g], out["n_edges"][g] = kept, int(lst[ci]) * chunk + off
        out["root_visits"][g] = int(root_run["n_info"][k_played]) & 0xFFFFFF
        out["root_w"][g] = -root_run["W"][k_played] if flaw == "root_w_negated" else root_run["W"][k_played]
        out["root_init_value"][g], out["path_len"][g], out["root_terminal"][g] = 0.0, 0, 0
        out["leaf_kind"][g], out["leaf_state"][g], out["leaf_value"][g] = LEAF_REUSED_ROOT, img["root_state"][g], 0.0
        _table(out, g, kept, clear=flaw != "stale_table_entry")
        info[g].update(fresh=False, pruned=cut, kept=kept, ci=ci, old=old)
    return out, (dropped, pruned)


# ---- comparison -------------------------------------------------------------------------------------------------------
def kept_games(after):
    return np.flatnonzero(after["leaf_kind"] == LEAF_REUSED_ROOT)


def diff_images(want, got, before, pos_index_of_kept=False):
    """Names (with the first differing places) of the buffers in which `got` differs from `want` in a compared byte.
    Not compared: old_begin of the records below a game's new n_nodes, edge_begin of a kept node without records and the
    cbegin of an edge to such a node, the pad bytes of the records inside the new runs, the order of the games' blocks
    among the released chunks, and (unless asked) the position index of a kept game."""
    bad = []
    B, cap = want["B"], want["node_cap"]
    kept = kept_games(want)
    for name in BUFFERS:
        a, b = want[name], got[name]
        ab = a.view(np.uint8).reshape(-1).copy()
        bb = b.view(np.uint8).reshape(-1).copy()
        if name == "nodes":
            m = np.zeros((B, cap, 48), bool)
            below = np.arange(cap)[None, :] < want["n_nodes"][:, None]
            m[:, :, 44:48] = below[:, :, None]
            for g in kept:
                empty = np.flatnonzero(want["nodes"][g, :want["n_nodes"][g]]["nedges"] <= 0)
                m[g, empty, 32:36] = True
            m = m.reshape(-1)
            ab[m] = 0
            bb[m] = 0
        elif name == "edges":
            m = np.zeros((len(a), 32), bool)
            for g in kept:
                nd = want["nodes"][g, :want["n_nodes"][g]]
                idx, _ = run_indices(nd["edge_begin"], nd["nedges"])
                m[idx, 26:] = True
                ch = want["edges"][idx]["child"].astype(np.int64)
                no_run = (ch >= 0) & (nd["nedges"][np.maximum(ch, 0)] <= 0)
                m[idx[no_run], 20:24] = True
            m = m.reshape(-1)
            ab[m] = 0
            bb[m] = 0
        elif name == "pos_index" and not pos_index_of_kept:
            m = np.zeros(a.shape, bool)
            m[kept] = True
            m = np.repeat(m.reshape(-1), 4)
            ab[m] = 0
            bb[m] = 0
        elif name == "free_chunks":
            t0, t1 = int(before["pool_top"][0]), int(want["pool_top"][0])
            wa, gb = a[t0:t1].copy(), b[t0:t1].copy()
            if sorted(wa.tolist()) != sorted(gb.tolist()):
                bad.append(("free_chunks", "released chunks differ as a multiset"))
            else:                                                    # each game's block contiguous and in list order
                where = {int(v): i for i, v in enumerate(gb.tolist())}
                for g in range(B):
                    rel = before["chunk_list"][g, int(want["n_chunks"][g]):int(before["n_chunks"][g])].tolist()
                    if rel and [where[int(v)] for v in rel] != list(range(where[int(rel[0])], where[int(rel[0])] + len(rel))):
                        bad.append(("free_chunks", f"game {g}'s released block is not contiguous in list order"))
            ab.view("<i4")[t0:t1] = 0
            bb.view("<i4")[t0:t1] = 0
        ne = np.flatnonzero(ab != bb)
        if len(ne):
            item = a.dtype.itemsize
            bad.append((name, (ne[:6] // item).tolist(), (ne[:6] % item).tolist()))
    return bad


# ---- the declarative verifier -----------------------------------------------------------------------------------------
def verify_advance(before, after):
    """Asserts that `after` is a correct outcome of lz_tree_advance on `before` (launch arguments inside `before`)
    without restating how it is computed: see DESIGN.md section 26 for the list of properties."""
    B, cap, chunk, slots = before["B"], before["node_cap"], before["chunk"], before["pos_slots"]
    budget = cap - (before["next_sims"] + 1)
    released = []
    pending = 0
    for g in range(B):
        kd = keep_decision(before, g)
        nn = int(before["n_nodes"][g])
        bn = before["nodes"][g, :nn]
        sel = None
        if kd is not None:
            k_played, c = kd
            # the subtree by pointer doubling: j[i] = an ancestor of i, ids <= c absorbing
            j = np.where(np.arange(nn) > c, bn["parent"].astype(np.int64), np.arange(nn))
            for _ in range(max(int(nn).bit_length(), 1)):
                j = j[j]
            full = j == c
            per_word = np.bincount(np.flatnonzero(full) >> 6, minlength=(nn + 63) >> 6)
            cum = np.cumsum(per_word)
            over = np.flatnonzero(cum > budget)
            cut_word = int(over[0]) if len(over) else len(per_word)
            sel = full & ((np.arange(nn) >> 6) < cut_word)
            if not sel.any():
                sel = None
        kept = int(after["n_nodes"][g])
        tab = after["pos_index"][g].astype(np.int64)
        if sel is None:                                               # a fresh root
            assert kept == 1 and int(after["n_chunks"][g]) == 0 and int(after["n_edges"][g]) == 0, (g, "fresh root")
            an = after["nodes"][g, 0]
            assert (an["state"] == before["root_state"][g]).all() and int(an["nedges"]) == -1 and int(an["parent"]) == -1
            assert (tab == -1).all(), (g, "table of a fresh root")
            assert int(after["leaf_kind"][g]) in (LEAF_INACTIVE, LEAF_EXPAND)
            pending += int(after["root_terminal"][g] == 0)
            released.append(before["chunk_list"][g, :int(before["n_chunks"][g])])
            assert (after["nodes"][g, 1:].view(np.uint8) == before["nodes"][g, 1:].view(np.uint8)).all()
            continue
        old = np.flatnonzero(sel)                                     # order-preserving bijection old[i] -> i
        assert kept == len(old), (g, "kept", kept, len(old))
        assert int(after["leaf_kind"][g]) == LEAF_REUSED_ROOT
        an = after["nodes"][g, :kept]
        assert (an["state"] == bn["state"][old]).all(), (g, "state")
        assert (an["nedges"] == bn["nedges"][old]).all(), (g, "nedges")
        want_parent = np.searchsorted(old, bn["parent"][old])
        want_parent[0] = -1
        assert sel[bn["parent"][old[1:]]].all(), (g, "the set is not parent-closed")
        assert (an["parent"] == want_parent).all(), (g, "parent")
        assert (after["node_value"][g, :kept].view(np.uint32) == before["node_value"][g, old].view(np.uint32)).all(), (g, "node_value")
        assert (after["node_value"][g, kept:].view(np.uint32) == before["node_value"][g, kept:].view(np.uint32)).all()
        assert (after["nodes"][g, kept:].view(np.uint8) == before["nodes"][g, kept:].view(np.uint8)).all(), (g, "records past n_nodes")
        # runs: inside one owned chunk, in list order, no overlap
        cnt = np.maximum(an["nedges"], 0).astype(np.int64)
        has = cnt > 0
        nb = an["edge_begin"].astype(np.int64)
        lst = before["chunk_list"][g].astype(np.int64)
        assert (after["chunk_list"][g] == before["chunk_list"][g]).all()
        nch = int(after["n_chunks"][g])
        assert 1 <= nch <= int(before["n_chunks"][g])
        b_, n_ = nb[has], cnt[has]
        ck = b_ // chunk
        assert ((b_ + n_ - 1) // chunk == ck).all(), (g, "a run straddles a chunk")
        lookup = {int(v): i for i, v in enumerate(lst[:nch].tolist())}
        assert all(int(v) in lookup for v in np.unique(ck)), (g, "a run lies in a chunk the game does not keep")
        li = np.array([lookup[int(v)] for v in ck], np.int64)
        key = li * chunk + (b_ - ck * chunk)
        assert (key[1:] >= key[:-1] + n_[:-1]).all(), (g, "runs overlap or leave list order")
        if len(key):
            assert li[-1] == nch - 1, (g, "a kept chunk behind the last run")
            assert int(after["n_edges"][g]) == int(b_[-1] + n_[-1]), (g, "n_edges")
        released.append(before["chunk_list"][g, nch:int(before["n_chunks"][g])])
        # run contents and links
        src, _ = run_indices(bn["edge_begin"][old], cnt)
        dst, _ = run_indices(nb, cnt)
        eo, en = before["edges"][src], after["edges"][dst]
        for f in ("W", "P", "n_info", "act"):
            assert (np.ascontiguousarray(eo[f]).view(np.uint8) == np.ascontiguousarray(en[f]).view(np.uint8)).all(), (g, f)
        ch = eo["child"].astype(np.int64)
        hasc = ch >= 0
        stays = hasc & sel[np.where(hasc, ch, 0)]
        gone = hasc & ~stays
        r = np.searchsorted(old, ch[stays])
        assert (en["child"][stays] == r).all(), (g, "child id")
        with_run = cnt[r] > 0
        assert (en["cbegin"][stays][with_run] == nb[r][with_run]).all(), (g, "cbegin")
        assert (en["cn"][stays] == eo["cn"][stays]).all(), (g, "cn")
        assert (en["child"][gone] == -1).all() and (en["cbegin"][gone] == 0).all() and (en["cn"][gone] == 0).all(), (g, "cut child")
        for f in ("child", "cbegin", "cn"):
            assert (en[f][~hasc] == eo[f][~hasc]).all(), (g, "edge without a child", f)
        # scalars
        e0 = int(bn["edge_begin"][0])
        pe = before["edges"][e0 + k_played]
        assert int(after["root_visits"][g]) == int(pe["n_info"]) & 0xFFFFFF
        assert after["root_w"][g:g + 1].view(np.uint64)[0] == np.array([pe["W"]]).view(np.uint64)[0], (g, "root_w")
        assert (int(after["path_len"][g]), int(after["root_terminal"][g])) == (0, 0)
        assert after["root_init_value"][g:g + 1].view(np.uint32)[0] == 0 and after["leaf_value"][g:g + 1].view(np.uint32)[0] == 0
        assert (after["leaf_state"][g] == before["root_state"][g]).all()
        # position index
        ent = np.flatnonzero(tab != -1)
        ids = tab[ent]
        assert ((ids >= 1) & (ids < kept)).all(), (g, "table entry outside [1, kept)")
        assert len(np.unique(ids)) == len(ids), (g, "a node twice in the table")
        mask = slots - 1
        h = np.array([pos_hash(s) & mask for s in an["state"]], np.int64) if kept > 1 else np.zeros(kept, np.int64)
        dist = (ent - h[ids]) & mask
        assert (dist < WAVE).all(), (g, "an entry outside the window of its hash")
        empty = tab == -1
        ecs = np.concatenate([[0], np.cumsum(np.concatenate([empty, empty[:WAVE]]))])     # empties before slot i (wrapped)
        assert (ecs[h[ids] + dist] - ecs[h[ids]] == 0).all(), (g, "an empty slot between a hash and its entry")
        in_tab = np.zeros(kept, bool)
        in_tab[ids] = True
        miss = np.flatnonzero(~in_tab[1:]) + 1
        for i in miss[ecs[h[miss] + WAVE] - ecs[h[miss]] > 0]:            # missing although its window has room: only a twin
            win = tab[(h[i] + np.arange(WAVE)) & mask]
            twin = any((an["state"][int(t)] == an["state"][i]).all() for t in win[win >= 0])
            assert twin or (win != -1).all(), (g, i, "a node missing from a table with room")
    # the pool
    t0, t1 = int(before["pool_top"][0]), int(after["pool_top"][0])
    rel = np.concatenate(released) if released else np.zeros(0, np.int32)
    assert t1 - t0 == len(rel), "pool_top"
    assert (after["free_chunks"][:t0] == before["free_chunks"][:t0]).all()
    assert sorted(after["free_chunks"][t0:t1].tolist()) == sorted(rel.tolist()), "released chunks"
    assert (after["free_chunks"][t1:] == before["free_chunks"][t1:]).all()
    assert int(after["pool_stats"][2]) == pending, "pool_stats[2]"
    # the edge pool outside the new runs
    touched = np.zeros(len(before["edges"]), bool)
    for g in kept_games(after):
        nd = after["nodes"][g, :int(after["n_nodes"][g])]
        touched[run_indices(nd["edge_begin"], nd["nedges"])[0]] = True
    assert (after["edges"][~touched].view(np.uint8) == before["edges"][~touched].view(np.uint8)).all(), "pool outside the runs"
    return True
