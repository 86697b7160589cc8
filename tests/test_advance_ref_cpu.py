"""CPU: the harness, the restatement and the verifier behind tests/test_gpu_advance.py -- the numpy
packer round-trips, `check_arena` accepts every case and rejects broken arenas, `verify_advance` accepts `ref_advance` on
every case, every case tag is really exercised (asserted on the restatement alone), and the verifier has teeth: every
deliberately wrong restatement is rejected by it and differs from the right one in the compared bytes."""
import numpy as np
import pytest

from tests import advance_cases as K
from tests import advance_ref as R
from tests import hand_arenas as H

ALL = [(s, i) for s in ("E1", "E2", "E3") for i in range(len(K.BUDGETS) if s != "E3" else 1)]
_REF = {}


def ref_of(shape, i):
    """(name, image, expected image, (dropped, pruned)) of launch i of a shape, computed once."""
    if (shape, i) not in _REF:
        name, img = K.launches(shape)[i]
        _REF[shape, i] = (name, img) + R.ref_advance(img)
    return _REF[shape, i]


def find(shape, launch, tag):
    for i in range(len(K.launches(shape))):
        name, img, out, _ = ref_of(shape, i)
        if name == launch:
            gs = [g for g, t in enumerate(img["tags"]) if t == tag]
            assert gs, (shape, launch, tag)
            return img, out, gs
    raise AssertionError((shape, launch))


def test_pack_states_round_trips_through_unpack_packed():
    from tests.tree_parity import unpack_packed
    st, packed, status = H.fixture_rows()
    back = unpack_packed(packed)
    for f in H.FIELDS:
        assert np.array_equal(np.asarray(back[f]).astype(np.int64), np.asarray(st[f]).astype(np.int64)), f
    assert np.array_equal(H.pack_states(back), packed)
    assert (packed[:, 2:] >> 36 == 0).all() and len(np.unique(packed, axis=0)) > 1000
    # the mark words of the hand-made states survive the trip too
    s = H.node_states(np.random.default_rng(1), 500, 3)
    assert len(np.unique(s, axis=0)) == 500 and np.array_equal(H.pack_states(unpack_packed(s)), s)


@pytest.mark.parametrize("shape,i", ALL)
def test_check_arena_accepts_every_case(shape, i):
    name, img = K.launches(shape)[i]
    assert img["B"] % 4 != 0
    assert (img["nodes"].view(np.uint8).reshape(img["B"], img["node_cap"], 48)[
        np.arange(img["node_cap"])[None, :] >= img["n_nodes"][:, None]] == H.FILL).all()
    used = np.zeros(len(img["edges"]), bool)
    for g in range(img["B"]):
        nd = img["nodes"][g, :img["n_nodes"][g]]
        used[H.run_indices(nd["edge_begin"], nd["nedges"])[0]] = True
    assert (img["edges"][~used].view(np.uint8) == H.FILL).all()
    assert H.check_arena(img, detached=[t == "fresh:no_child" for t in img["tags"]])


def _broken(kind):
    img = H.copy_image(K.launches("E1")[0][1])
    g = img["tags"].index("parent_places")
    nd, e0 = img["nodes"][g], int(img["nodes"][g, 0]["edge_begin"])
    first_child = int(np.flatnonzero(img["edges"][e0:e0 + nd[0]["nedges"]]["child"] > 0)[0]) + e0
    if kind == "parent_not_below":
        nd["parent"][7] = 7
    elif kind == "root_has_parent":
        nd["parent"][0] = 0
    elif kind == "child_out_of_range":
        img["edges"]["child"][first_child] = int(img["n_nodes"][g])
    elif kind == "parent_link":
        img["edges"]["child"][first_child] = int(img["n_nodes"][g]) - 1
    elif kind == "cn":
        img["edges"]["cn"][first_child] += 1
    elif kind == "cbegin":
        img["edges"]["cbegin"][first_child] += 1
    elif kind == "nedges_73":
        nd["nedges"][3] = 73
    elif kind == "slack_layout":
        nd["edge_begin"][1:int(img["n_nodes"][g])] += 1
    elif kind == "chunk_owned_twice":
        img["chunk_list"][g, 0] = img["chunk_list"][g + 1, 0]
    elif kind == "chunk_outside_pool":
        img["free_chunks"][0] = img["pool_chunks"]
    elif kind == "n_edges":
        img["n_edges"][g] += 1
    elif kind == "too_many_nodes":
        img["n_nodes"][g] = img["node_cap"] + 1
    elif kind == "n_chunks":
        img["n_chunks"][g] += 1
    elif kind == "pending_count":
        img["pool_stats"][2] += 1
    return img


@pytest.mark.parametrize("kind", ["parent_not_below", "root_has_parent", "child_out_of_range", "parent_link", "cn", "cbegin",
                                  "nedges_73", "slack_layout", "chunk_owned_twice", "chunk_outside_pool", "n_edges",
                                  "too_many_nodes", "n_chunks", "pending_count"])
def test_check_arena_rejects_a_broken_arena(kind):
    with pytest.raises((AssertionError, IndexError)):
        H.check_arena(_broken(kind))


@pytest.mark.parametrize("shape,i", ALL)
def test_verifier_accepts_the_restatement_on_every_case(shape, i):
    name, img, out, counts = ref_of(shape, i)
    assert R.verify_advance(img, out)
    assert R.diff_images(out, out, img, pos_index_of_kept=True) == []
    # what the case list promises of every launch
    for g, ex in enumerate(img["expect"]):
        if ex:
            inf = out["info"][g]
            assert inf["kept"] == ex["kept"] and ("cut" not in ex or inf["cut_word"] == ex["cut"]), (img["tags"][g], ex, inf)
    assert counts == (sum(i_["dropped"] for i_ in out["info"]), sum(i_["pruned"] for i_ in out["info"]))


def test_pos_hash_with_python_integers_matches_wrapping_uint64_arithmetic():
    """pos_hash with Python integers against the same formula in wrapping uint64 numpy arithmetic."""
    s = H.node_states(np.random.default_rng(5), 4000, 1).view(np.uint64)
    with np.errstate(over="ignore"):
        h = s[:, 0] * np.uint64(0x9E3779B97F4A7C15)
        h = (h ^ (h >> np.uint64(29)) ^ s[:, 1]) * np.uint64(0xBF58476D1CE4E5B9)
        h = (h ^ (h >> np.uint64(31)) ^ s[:, 2]) * np.uint64(0x94D049BB133111EB)
        h = (h ^ (h >> np.uint64(27)) ^ s[:, 3]) * np.uint64(0x9E3779B97F4A7C15)
    assert [R.pos_hash(r) for r in s.view(np.int64)] == (h >> np.uint64(32)).tolist()


# ---- every tag is really exercised ------------------------------------------------------------------------------------
def _kinds_in_run(img, out, g):
    """Per kept run of game g: does it hold a kept child, a cut child and an edge that never had a child?"""
    inf = out["info"][g]
    old, sel = inf["old"], np.zeros(int(img["n_nodes"][g]), bool)
    sel[old] = True
    nd = img["nodes"][g]
    for o in old:
        run = img["edges"][int(nd["edge_begin"][o]):int(nd["edge_begin"][o]) + max(int(nd["nedges"][o]), 0)]
        ch = run["child"].astype(np.int64)
        if (ch < 0).any() and (ch >= 0).any() and sel[ch[ch >= 0]].any() and (~sel[ch[ch >= 0]]).any():
            return True
    return False


def test_mark_cases_hold_what_their_tags_say():
    img, out, (g,) = find("E1", "largest", "chain130")
    assert (img["nodes"][g, 1:130]["parent"] == np.arange(129)).all() and out["info"][g]["kept"] == 129
    for tag, lane in (("c_lane0", 0), ("c_lane63", 63)):
        img, out, (g,) = find("E1", "largest", tag)
        assert out["info"][g]["c"] % 64 == lane and out["info"][g]["kept"] > 64
    img, out, (g,) = find("E1", "largest", "c_last")
    assert out["info"][g]["c"] == int(img["n_nodes"][g]) - 1 and out["info"][g]["kept"] == 1
    img, out, (g,) = find("E1", "largest", "interleaved")
    old = out["info"][g]["old"]
    assert (old % 2 == 1).all() and len(old) == 160 and (np.bincount(old >> 6) == 32).all()    # rank != id in every word
    for nn, words in ((2, 1), (64, 1), (65, 2), (128, 2), (129, 3), (256, 4), (257, 5), (320, 5)):
        img, out, (g,) = find("E1", "largest", f"nn{nn}")
        assert int(img["n_nodes"][g]) == nn and (nn + 63) // 64 == words and not out["info"][g]["fresh"]
    img, out, (g,) = find("E1", "largest", "parent_places")
    par = img["nodes"][g]["parent"]
    assert (par[64], par[70], par[130]) == (63, 65, 5) and out["info"][g]["kept"] == 199
    img, out, (g,) = find("E1", "largest", "twins")
    st = img["nodes"][g, out["info"][g]["old"]]["state"]
    assert len(np.unique(st, axis=0)) < len(st)


def test_cut_cases_hold_what_their_tags_say():
    img, out, gs = find("E1", "middle", "exact_fit")
    assert [(out["info"][g]["kept"], out["info"][g]["pruned"]) for g in gs] == [(200, False)]
    img, out, (g,) = find("E1", "largest", "exact_fit")
    assert (out["info"][g]["kept"], out["info"][g]["pruned"]) == (513, False)
    img, out, (g,) = find("E1", "middle", "one_over")
    assert (out["info"][g]["kept"], out["info"][g]["pruned"], out["info"][g]["cut_word"]) == (200, True, 4)
    residues = set()
    for tag in ("one_over", "cut_w1", "cut_w2", "cut_w3", "cut_last_word", "mixed_run"):
        img, out, (g,) = find("E1", "middle", tag)
        residues.add(out["info"][g]["cut_word"] % 4)
        assert out["info"][g]["pruned"]
    assert residues == {0, 1, 2, 3}
    img, out, (g,) = find("E1", "middle", "cut_last_word")
    assert out["info"][g]["cut_word"] == (int(img["n_nodes"][g]) + 63) // 64 - 1
    img, out, (g,) = find("E1", "middle", "mixed_run")
    assert _kinds_in_run(img, out, g)
    img, out, gs = find("E1", "one", "cut_own_word")
    assert all(out["info"][g]["dropped"] and out["info"][g]["cut_word"] == out["info"][g]["c"] // 64 for g in gs)
    img, out, (g,) = find("E1", "one", "budget1_alone")
    root = out["nodes"][g, 0]
    run = out["edges"][int(root["edge_begin"]):int(root["edge_begin"]) + int(root["nedges"])]
    before_run = img["edges"][int(img["nodes"][g, 127]["edge_begin"]):][:int(root["nedges"])]
    assert out["info"][g]["kept"] == 1 and (run["child"] == -1).all() and (before_run["child"] > 0).any()
    assert (run["cn"][before_run["child"] > 0] == 0).all()
    name, img, out, counts = ref_of("E1", 3)
    assert name == "zero" and counts[0] == sum(t == "budget0" for t in img["tags"]) == 4 and counts[1] == 0


def test_run_cases_hold_what_their_tags_say():
    img, out, (g,) = find("E1", "largest", "runs72_56")
    nd = out["nodes"][g, :out["n_nodes"][g]]
    assert int(out["n_edges"][g]) % 128 == 0 and ((nd["edge_begin"] + nd["nedges"]) % 128 == 0).sum() == 20
    img, out, (g,) = find("E1", "largest", "runs72")
    assert out["info"][g]["ci"] + 1 == out["info"][g]["kept"] == 59
    img, out, (g,) = find("E1", "largest", "kept130x64")
    assert out["info"][g]["ci"] >= 64 and out["info"][g]["kept"] == 130
    lst = img["chunk_list"][g, :img["n_chunks"][g]]
    assert (np.diff(lst) < 0).all()                                                           # descending pool order
    img, out, (g,) = find("E1", "largest", "runs72")
    assert (np.diff(img["chunk_list"][g, :img["n_chunks"][g]]) > 0).all()
    img, out, (g,) = find("E1", "largest", "flat_rounds")
    cnt = out["nodes"][g, :out["n_nodes"][g]]["nedges"]
    assert [int(cnt[k:k + 64].sum()) for k in (0, 64, 128, 192)] == [768, 769, 1600, 64]
    assert 1600 > 2 * 12 * 64 and (cnt[192:256] == 1).all()
    img, out, (g,) = find("E1", "largest", "defensive")
    cnt = out["nodes"][g, :out["n_nodes"][g]]["nedges"]
    assert sorted(cnt[cnt <= 0].tolist()) == [-1, 0] and out["info"][g]["kept"] == 39
    # chunk lists that are not in address order and interleave with other games' chunks
    img = K.launches("E1")[0][1]
    unordered = [g for g in range(img["B"]) if img["n_chunks"][g] > 2 and (np.diff(img["chunk_list"][g, :img["n_chunks"][g]]) < 0).any()
                 and (np.diff(img["chunk_list"][g, :img["n_chunks"][g]]) > 0).any()]
    assert len(unordered) > 5


def test_root_and_fresh_cases_hold_what_their_tags_say():
    for slot in (0, 63, 64, 71):
        img, out, (g,) = find("E1", "largest", f"root72_slot{slot}")
        assert out["info"][g]["k_played"] == slot and int(img["nodes"][g, 0]["nedges"]) == 72
    img, out, (g,) = find("E1", "largest", "root1")
    assert int(img["nodes"][g, 0]["nedges"]) == 1 and out["info"][g]["kept"] == 9
    img, out, (g,) = find("E1", "largest", "played_maxN")
    assert int(out["root_visits"][g]) == (1 << 24) - 1 and out["root_w"][g] == 0 and np.signbit(out["root_w"][g])
    img, out, (g,) = find("E1", "largest", "played_Wneg")
    assert out["root_w"][g] == -123.456
    img, out, (g,) = find("E1", "largest", "played_Wpos")
    assert out["root_w"][g] == 7.25
    run = img["edges"][int(img["nodes"][g, 0]["edge_begin"]):][:int(img["nodes"][g, 0]["nedges"])]
    assert (run["act"] == img["played"][g]).sum() == 2                                          # the first match counts
    name, img, out, counts = ref_of("E1", 0)
    kinds = {t[6:] for t in img["tags"] if t.startswith("fresh:")}
    assert kinds == set(K.FRESH_KINDS) and img["tags"][0].startswith("fresh:") and img["tags"][-1].startswith("fresh:")
    for g, t in enumerate(img["tags"]):
        if t.startswith("fresh:"):
            assert out["info"][g]["fresh"] and not out["info"][g]["dropped"], t
            assert int(out["n_chunks"][g]) == 0 and (out["pos_index"][g] == -1).all()
    assert counts == (0, 0)
    g = img["tags"].index("fresh:root_over")
    assert (int(out["root_terminal"][g]), int(out["leaf_kind"][g])) == (1, 0)
    g = img["tags"].index("fresh:inactive")
    assert (int(out["root_terminal"][g]), int(out["leaf_kind"][g])) == (1, 0)
    g = img["tags"].index("fresh:state_w3")
    assert ((img["root_state"][g] != img["nodes"][g, 3]["state"]) == [False, False, False, True]).all()


def test_e3_cases_hold_what_their_tags_say():
    name, img, out, counts = ref_of("E3", 0)
    assert (img["node_cap"] + 63) // 64 == 1026 and img["pos_slots"] == 8192 and img["B"] == 3
    g = img["tags"].index("e3_words_1024_1025")
    old = out["info"][g]["old"]
    assert {1024, 1025} <= set((old >> 6).tolist()) and not out["info"][g]["pruned"]
    g = img["tags"].index("e3_cut_at_1024")
    assert out["info"][g]["cut_word"] == 1024 and out["info"][g]["kept"] >= 65000
    tab = out["pos_index"][g]
    assert (tab != -1).all()                                                                    # every window filled up


# ---- the verifier has teeth -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flaw", R.FLAWS)
def test_a_wrong_restatement_is_rejected_and_differs(flaw):
    rejected = differs = 0
    for shape, i in (("E1", 0), ("E1", 1), ("E1", 2)):
        name, img, out, _ = ref_of(shape, i)
        if flaw == "terminal_bit_ignored":
            g = img["tags"].index("fresh:terminal_bit") if "fresh:terminal_bit" in img["tags"] else None
            if g is None:
                continue
        bad, _ = R.ref_advance(img, flaw=flaw)
        d = R.diff_images(out, bad, img, pos_index_of_kept=True)
        if not d:
            continue
        differs += 1
        with pytest.raises(AssertionError):
            R.verify_advance(img, bad)
        rejected += 1
    assert differs >= 1 and rejected == differs, flaw


def test_three_advances_in_a_row_on_the_restatement():
    """The chain case on the CPU: every image the restatement leaves is a valid arena for the next advance."""
    rng = np.random.default_rng(11)
    img = H.copy_image(K.chain_start())
    pruned = []
    for step, next_sims in enumerate(K.CHAIN_NEXT_SIMS):
        img["next_sims"] = next_sims
        assert H.check_arena(img)
        out, counts = R.ref_advance(img)
        assert R.verify_advance(img, out)
        pruned.append(counts[1])
        assert sum(not i_["fresh"] for i_ in out["info"]) >= 3, step
        img = H.next_move(out, rng)
    assert pruned[1] >= 1 and pruned[0] == 0
