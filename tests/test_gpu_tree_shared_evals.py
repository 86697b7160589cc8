"""Shared evaluations of transposed leaves (position index, LzTreeDesc.pos_*): a leaf whose position another node of the same
tree holds takes that node's priors and raw value instead of a network row.  The trees must not change by a bit."""
import numpy as np
import pytest
import torch

from tests.golden_utils import load, states, FIELDS
from tests.tree_parity import to_gpu_batch

DEV = torch.device("cuda:0")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _run(monkeypatch, share: str, games: int, sims: int, moves: int, pos_slots=None, compact=True, seed=5):
    """`moves` searches of a seeded population with kept subtrees (advance between them) on the one-wave tree step."""
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    from liuzhou_amd import v0_core
    monkeypatch.setenv("LZ_TREE_SHARE", share)
    monkeypatch.setenv("LZ_TREE_SPLIT", "0")                    # the one-wave step: the one that looks the index up
    torch.manual_seed(20260314)
    net = FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV))
    st_all = states(load("g1_rules.npz"), "s")
    idx = np.random.default_rng(seed).integers(0, st_all["board"].shape[0], games)
    batch = to_gpu_batch({f: np.ascontiguousarray(np.asarray(st_all[f])[idx]) for f in FIELDS}, DEV)
    m = PortableTreeMCTS(net, games, sims, DEV, add_dirichlet_noise=True, sample_moves=True, reuse_tree=True,
                         reuse_factor=4.0, seed=seed, compact_evals=compact)
    if pos_slots is not None:
        m.engine.desc.pos_slots = int(pos_slots)                 # a smaller table inside the same buffer
    temps = torch.ones(games, device=DEV)
    outs = []
    for _ in range(moves):
        out = m.search_batch(batch, temperatures=temps)
        outs.append((out.chosen_action_indices.clone(), out.policy_dense.clone(), out.root_value.clone()))
        plies = torch.zeros(games, dtype=torch.int64, device=DEV)
        done = torch.zeros(games, dtype=torch.bool, device=DEV)
        v0_core.self_play_step_inplace(*batch.tensors(), plies, done, torch.arange(games, device=DEV),
                                       out.chosen_action_codes.clone(), out.terminal_mask.clone(),
                                       out.chosen_valid_mask.clone(), 512, 2.0)
    torch.cuda.synchronize()
    return m, outs


def _trees(m):
    """Every game's node records and every node's edge run, as bytes (host copies).  Pool indices (edge_begin, cbegin) are
    left out: games take chunks from the shared pool in the order their waves get to it, which varies from run to run."""
    from tests.tree_parity import EDGE_LOGICAL
    e = m.engine
    out = []
    for g in range(e.B):
        nodes = e.game_nodes(g)
        runs = []
        for n in nodes:
            r = e.edge_run(int(n["edge_begin"]), max(0, int(n["nedges"])))
            runs.append(tuple(r[f].tobytes() for f in EDGE_LOGICAL))
        out.append((tuple(nodes[f].tobytes() for f in ("w0", "w1", "w2", "w3", "nedges", "parent")), runs))
    return out


def _same(a, b):
    for (oa, pa, va), (ob, pb, vb) in zip(a[1], b[1]):
        assert torch.equal(oa, ob) and torch.equal(pa, pb) and torch.equal(va, vb)
    ea, eb = a[0].engine, b[0].engine
    assert torch.equal(ea.buf["n_nodes"], eb.buf["n_nodes"]) and torch.equal(ea.buf["root_w"], eb.buf["root_w"])
    assert torch.equal(ea.buf["root_visits"], eb.buf["root_visits"])
    assert _trees(a[0]) == _trees(b[0])


@pytest.mark.gpu
def test_shared_leaves_build_the_same_trees_over_moves_with_kept_subtrees(monkeypatch):
    """Sharing on and off: byte-identical node and edge records, visits, root values and picks over 3 moves with advance
    between them (the index is rebuilt after every compaction); shared leaves are not launched and not consumed."""
    _need_gpu()
    on = _run(monkeypatch, "1", games=96, sims=160, moves=3)
    off = _run(monkeypatch, "0", games=96, sims=160, moves=3)
    _same(on, off)
    shared = int(on[0].engine.share_count.sum())
    assert shared > 0 and int(off[0].engine.share_count.sum()) == 0
    assert on[0].consumed_evals + shared == off[0].consumed_evals
    assert on[0].leaf_evals == on[0].consumed_evals < off[0].leaf_evals
    print(f"shared leaves: {shared} of {off[0].consumed_evals} evaluations")


@pytest.mark.gpu
def test_a_full_position_index_degrades_to_plain_evaluation(monkeypatch):
    """A table of one 64-slot window per game fills up at once: the nodes that find no room are not indexed, their twins
    are evaluated -- fewer shared leaves, the same trees."""
    _need_gpu()
    small = _run(monkeypatch, "1", games=64, sims=160, moves=2, pos_slots=64)
    full = _run(monkeypatch, "1", games=64, sims=160, moves=2)
    off = _run(monkeypatch, "0", games=64, sims=160, moves=2)
    _same(small, off)
    _same(full, off)
    assert 0 < int(small[0].engine.share_count.sum()) < int(full[0].engine.share_count.sum())


@pytest.mark.gpu
def test_shared_leaves_compact_and_dense_launches_agree(monkeypatch):
    """Dense launches (every slot) with sharing on: the shared rows are evaluated and ignored -- same trees as the lists."""
    _need_gpu()
    lists = _run(monkeypatch, "1", games=64, sims=96, moves=2, compact=True)
    dense = _run(monkeypatch, "1", games=64, sims=96, moves=2, compact=False)
    _same(lists, dense)
    assert int(dense[0].engine.share_count.sum()) == int(lists[0].engine.share_count.sum()) > 0


@pytest.mark.gpu
def test_the_root_is_never_a_source(monkeypatch):
    """Node 0 carries the Dirichlet mix in its priors: it is never inserted, so every indexed node is >= 1 and holds the
    state the index finds it under."""
    _need_gpu()
    from liuzhou_amd.tree_engine import pos_slots_for
    m, _ = _run(monkeypatch, "1", games=32, sims=96, moves=2)
    e = m.engine
    slots = pos_slots_for(e.node_cap)
    tab = e.buf["pos_index"].view(e.B, slots).cpu().numpy()
    nn = e.buf["n_nodes"].cpu().numpy()
    for g in range(e.B):
        entries = tab[g][tab[g] >= 0]
        assert (entries >= 1).all() and (entries < nn[g]).all()
        assert len(set(entries.tolist())) == len(entries)
