"""The hand-built launches of lz_tree_advance: three engine shapes, every launch a mix of cases so
that the four waves of a workgroup hold trees of different sizes, B never a multiple of 4.  Seeded; every game carries a
tag that says what it holds, and tests/test_advance_ref_cpu.py asserts on the restatement alone that it really holds it.

    E1  node_cap 514, edge_chunk 128      the four-wave form
    E2  node_cap 514, edge_chunk 1024     the same games in chunks of the production size
    E3  node_cap 65 602 (1026 mark words), edge_chunk 1024, B = 3      the one-wave form, 8192 position slots

`next_sims` is one number per launch, so the budget cases of a launch are built relative to its budget
node_cap - (next_sims + 1)."""
import functools

import numpy as np

from tests import hand_arenas as H

SHAPES = {"E1": (514, 128), "E2": (514, 1024), "E3": (65602, 1024)}
# E1 / E2 launches: name -> next_sims (budget 513, 200, 1, 0)
BUDGETS = {"largest": 0, "middle": 313, "one": 512, "zero": 513}
E3_NEXT_SIMS = 100                                                   # budget 65 501
FRESH_KINDS = ("reset", "played_negative", "played_absent", "no_child", "terminal_bit", "state_w3", "root_terminal",
               "inactive", "root_ne-1", "root_ne0", "root_over")


def _ne(rng, nn, lo, hi, root=None):
    ne = rng.integers(lo, hi + 1, nn)
    ne[0] = max(int(ne[0]), 3) if root is None else root
    return ne


def small(rng, tag, nn, c, frac=0.6, lo=1, hi=6, **kw):
    member = np.zeros(nn, bool)
    member[c] = True
    member[c + 1:] = rng.random(nn - c - 1) < frac
    return H.game(tag, nn, c, member, _ne(rng, nn, lo, hi, kw.pop("root", None)), rng, **kw)


def lone_root(tag, ne0):
    return dict(tag=tag, nn=1, c=0, ne=np.array([ne0]), parent=np.array([-1]), member=np.array([True]), fresh="root_ne")


def fresh(rng, kind):
    if kind.startswith("root_ne"):
        return lone_root("fresh:" + kind, int(kind[7:]))
    return small(rng, "fresh:" + kind, 40, 3, fresh=kind, c_detached=kind == "no_child")


def by_counts(rng, tag, nn, c, counts, lo=2, hi=5, window=40, **kw):
    """Members by word (`counts` from c's word on); parents drawn from a wide window so that runs near a cut hold kept
    children, cut children and edges without a child side by side."""
    return H.game(tag, nn, c, H.members_by_word(rng, nn, c, counts), _ne(rng, nn, lo, hi), rng, window=window, **kw)


def marks_and_runs(rng):
    """Cases that do not depend on the budget (placed in the launch with the largest one)."""
    gs = [H.game("chain130", 130, 1, "all", np.full(130, 2), rng, mode="chain"),
          small(rng, "c_lane0", 200, 64), small(rng, "c_lane63", 200, 63), small(rng, "c_last", 150, 149)]
    inter = np.arange(321) % 2 == 1
    gs.append(H.game("interleaved", 321, 1, inter, _ne(rng, 321, 2, 4), rng))
    for nn in (2, 64, 65, 128, 129, 256, 257, 320):
        gs.append(small(rng, f"nn{nn}", nn, 1))
    gs.append(H.game("parent_places", 200, 1, "all", _ne(rng, 200, 3, 6), rng,
                     force_parent={64: 63, 70: 65, 130: 5}))
    ne = np.where(np.arange(41) % 2 == 1, 72, 56)
    ne[0] = 72
    gs.append(H.game("runs72_56", 41, 1, "all", ne, rng))
    gs.append(H.game("runs72", 60, 1, "all", np.full(60, 72), rng, list_order="asc"))
    gs.append(H.game("kept130x64", 131, 1, "all", np.full(131, 64), rng, list_order="desc"))
    ne = np.concatenate([[5], np.full(64, 12), np.full(63, 12), [13], np.full(64, 25), np.full(64, 1), [2, 2, 2]])
    gs.append(H.game("flat_rounds", len(ne), 1, "all", ne, rng, window=200))
    ne = _ne(rng, 40, 2, 5)
    ne[5], ne[9] = 0, -1
    gs.append(H.game("defensive", 40, 1, "all", ne, rng))
    for slot in (0, 63, 64, 71):
        gs.append(small(rng, f"root72_slot{slot}", 30, 2, root=72, played_slot=slot))
    gs.append(H.game("root1", 10, 1, "all", _ne(rng, 10, 1, 3, root=1), rng))
    gs.append(small(rng, "played_maxN", 30, 2, played_n_info=(0xFD << 24) | 0xFFFFFF, played_W=-0.0))
    gs.append(small(rng, "played_Wneg", 30, 2, played_W=-123.456))
    gs.append(small(rng, "played_Wpos", 30, 2, played_W=7.25, duplicate_action=True))
    gs.append(small(rng, "twins", 100, 1, frac=0.9, twins=[(5, 60), (6, 61)]))
    gs.append(H.game("exact_fit", 514, 1, "all", _ne(rng, 514, 1, 3), rng, expect=dict(kept=513, cut=None)))
    return gs


def cuts_middle(rng):
    """Budget 200: exact fit, one over, the cut at every word residue of the four-word look-ahead and in the last word."""
    return [
        by_counts(rng, "exact_fit", 400, 1, [50, 50, 50, 50], expect=dict(kept=200, cut=None)),
        by_counts(rng, "one_over", 400, 1, [50, 50, 50, 50, 1], expect=dict(kept=200, cut=4)),
        by_counts(rng, "cut_w1", 450, 64, [40, 40, 40, 40, 64], expect=dict(kept=160, cut=5)),
        by_counts(rng, "cut_w2", 500, 130, [45, 45, 45, 45, 30], expect=dict(kept=180, cut=6)),
        by_counts(rng, "cut_w3", 514, 200, [48, 48, 48, 48, 20], expect=dict(kept=192, cut=7)),
        by_counts(rng, "cut_last_word", 514, 1, [25] * 8 + [1], expect=dict(kept=200, cut=8)),
        by_counts(rng, "mixed_run", 514, 1, [60] * 8, lo=6, hi=12, window=120, expect=dict(kept=180, cut=3)),
    ]


def with_fresh(rng, gs, kinds):
    """`gs` with fresh-root games in the first, a middle and the last slot (and B no multiple of 4)."""
    fr = [fresh(rng, k) for k in kinds]
    mid = len(gs) // 2
    out = fr[:1] + gs[:mid] + fr[1:-1] + gs[mid:] + fr[-1:]
    if len(out) % 4 == 0:
        out.insert(1, small(rng, "filler", 20, 2))
    return out


@functools.lru_cache(maxsize=None)
def launches(shape):
    """[(name, image)] of an engine shape; the images are shared and must not be written to."""
    cap, chunk = SHAPES[shape]
    if shape == "E3":
        return [("big", e3_image())]
    out = []
    for k, (name, next_sims) in enumerate(BUDGETS.items()):
        rng = np.random.default_rng(2600 + k)
        if name == "largest":
            gs = with_fresh(rng, marks_and_runs(rng), FRESH_KINDS)
        elif name == "middle":
            gs = with_fresh(rng, cuts_middle(rng) + marks_and_runs(rng)[:12], FRESH_KINDS[:4])
        elif name == "one":
            alone = np.arange(300) >= 128
            alone[127] = True
            gs = [H.game("budget1_alone", 300, 127, alone, _ne(rng, 300, 3, 6), rng, window=100, expect=dict(kept=1, cut=2)),
                  by_counts(rng, "cut_own_word", 200, 70, [2, 10], expect=dict(kept=0, cut=1)),
                  small(rng, "c_last", 90, 89, expect=dict(kept=1, cut=None)),
                  small(rng, "cut_own_word", 150, 1, expect=dict(kept=0, cut=0))]
            gs = with_fresh(rng, gs, FRESH_KINDS[4:7])
        else:
            gs = [small(rng, "budget0", nn, c, expect=dict(kept=0)) for nn, c in ((30, 1), (130, 64), (514, 511), (2, 1))]
            gs = with_fresh(rng, gs, FRESH_KINDS[7:10])
        out.append((name, H.build_image(gs, cap, chunk, next_sims, seed=77 + k)))
    return out


def e3_image():
    cap, chunk = SHAPES["E3"]
    rng = np.random.default_rng(2603)
    nn = cap
    # game 0: a sparse subtree with members in words 1024 and 1025
    m = np.zeros(nn, bool)
    m[1] = True
    m[rng.choice(np.arange(2, 65536), 280, replace=False)] = True
    m[[65536, 65540, 65599, 65600, 65601]] = True
    g0 = H.game("e3_words_1024_1025", nn, 1, m, _ne(rng, nn, 1, 2), rng, window=12)
    # game 1: 65 480 members up to word 1023, 40 in word 1024: the cut falls at word 1024
    m = np.arange(nn) >= 1
    m[rng.choice(np.arange(2, 65536), 55, replace=False)] = False
    m[65536 + 40:] = False
    g1 = H.game("e3_cut_at_1024", nn, 1, m, _ne(rng, nn, 1, 2), rng, window=12, twins=[(100, 9000), (101, 9001)],
                expect=dict(kept=65480, cut=1024))
    g2 = fresh(rng, "reset")
    return H.build_image([g0, g1, g2], cap, chunk, E3_NEXT_SIMS, seed=91)


@functools.lru_cache(maxsize=None)
def chain_start():
    """Five deep trees in E1 for three advances in a row (budgets 513, 100, 513)."""
    rng = np.random.default_rng(2610)
    gs = [H.game("deep", 514, 1, "all", _ne(rng, 514, 2, 4), rng, window=3),
          small(rng, "deep", 514, 2, frac=0.95, lo=2, hi=5, window=3),
          H.game("deep", 400, 1, "all", _ne(rng, 400, 1, 3), rng, window=2),
          small(rng, "deep", 300, 5, frac=0.9), fresh(rng, "reset")]
    return H.build_image(gs, SHAPES["E1"][0], SHAPES["E1"][1], 0, seed=93, spare_chunks=9)


CHAIN_NEXT_SIMS = (0, 413, 0)
