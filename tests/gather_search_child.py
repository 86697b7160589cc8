"""Child process of tests/test_gpu_net_gather.py: list searches (PortableTreeMCTS, compact_evals) over three consecutive
moves with kept subtrees, in the scenarios named below, on whichever path the environment selects (LZ_TREE_GATHER);
everything the parent compares goes to one .npz.  Run as `python -m tests.gather_search_child OUT.npz`."""
import os
import sys

import numpy as np
import torch

GAMES, SIMS, MOVES = 70, 24, 3
DEV = "cuda:0"
#            name        model      split  graph  playout cap  states      [further PortableTreeMCTS keywords]
SCENARIOS = (("plain",    "b6c64",   "0",   True,  False,       "mixed"),
             ("direct",   "b6c64",   "0",   False, False,       "mixed"),
             ("split",    "b10c128", "1",   True,  False,       "mixed"),
             ("cap",      "b6c64",   "0",   True,  True,        "mixed"),
             ("terminal", "b6c64",   "0",   True,  False,       "terminal"),
             ("forced",   "b6c64",   "0",   True,  False,       "mixed",    dict(forced_playouts_k=2.0)),
             ("gumbel",   "b6c64",   "0",   True,  False,       "mixed",    dict(gumbel_considered=8)),
             # a check behind launches 4, 8, ..., 20 of the 24-simulation searches, a stop allowed from the first of them
             ("kld",      "b6c64",   "0",   True,  True,        "mixed",    dict(kld_stop=(0.02, 4, 4))))


def start_states(kind):
    from oracle import lz_oracle as O
    from tests.golden_utils import FIELDS, load, states as gstates
    if kind == "mixed":
        st = gstates(load("g1_rules.npz"), "s")
        idx = np.random.default_rng(5).integers(0, st["board"].shape[0], GAMES)
    else:                                               # finished games only: no leaf ever needs the network
        st = gstates(load("g2_edges.npz"), "s")
        term = np.flatnonzero(O.terminal_mask_from_next_state({f: np.asarray(st[f]) for f in FIELDS}))
        assert len(term) >= GAMES, "g2_edges.npz holds too few finished games"
        idx = term[:GAMES]
    return {f: np.ascontiguousarray(np.asarray(st[f])[idx]) for f in FIELDS}


def run(rec, name, model, split, graph, cap, kind, extra=None):
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    from oracle import lz_oracle as O
    from tests.tree_parity import EDGE_LOGICAL, game_tree, root_edges, to_gpu_batch
    os.environ["LZ_TREE_SPLIT"] = split
    torch.manual_seed(20260314)
    net = FusedNet(ChessNet(**MODEL_CONFIGS[model]).eval().to(DEV))
    kw = dict(exploration_weight=1.0, add_dirichlet_noise=True, sample_moves=True, reuse_tree=True, reuse_factor=4.0, seed=99,
              compact_evals=True, use_graph=graph)
    if cap:
        kw.update(fast_simulations=6, full_prob=0.5)
    kw.update(extra or {})
    mcts = PortableTreeMCTS(net, GAMES, SIMS, DEV, **kw)
    e = mcts.engine
    cur = start_states(kind)
    temps = torch.ones((GAMES,), device=DEV)
    for mv in range(MOVES):
        out = mcts.search_batch(to_gpu_batch(cur, DEV), temperatures=temps)
        torch.cuda.synchronize()
        p = f"{name}.m{mv}."
        rec[p + "live_count"] = e.live["live_count"][: SIMS + 1].cpu().numpy()
        edges = root_edges(e)
        rec[p + "root_nedges"] = np.asarray([len(x) for x in edges])
        for f in EDGE_LOGICAL:
            rec[p + "root_" + f] = np.concatenate([x[f] for x in edges]) if edges else np.zeros(0)
        rec[p + "root_has_child"] = np.concatenate([x["child"] >= 0 for x in edges])
        rec[p + "chosen"] = out.chosen_action_indices.cpu().numpy()
        rec[p + "policy"] = out.policy_dense.cpu().numpy()
        rec[p + "root_value"] = out.root_value.cpu().numpy()
        rec[p + "n_nodes"] = e.buf["n_nodes"].cpu().numpy()
        rec[p + "root_w"] = e.buf["root_w"].cpu().numpy()
        pick = rec[p + "chosen"]
        nxt = [O.apply_index(O.state_from_batch(cur, i), int(pick[i])) if pick[i] >= 0 else O.state_from_batch(cur, i)
               for i in range(GAMES)]
        cur = O.batch_from_states(nxt)
    # the whole arenas after the last move: every node's state and parent, every edge run's logical fields, in node order
    nodes_all, runs_all = [], []
    for g in range(GAMES):
        nodes, runs = game_tree(e, g)
        nodes_all.append(np.concatenate([nodes["state"].reshape(-1), nodes["nedges"].astype(np.int64),
                                         nodes["parent"].astype(np.int64)]))
        for r in runs:
            runs_all.append(np.concatenate([r[f].astype(np.float64) for f in EDGE_LOGICAL] + [(r["child"] >= 0).astype(np.float64)]))
    rec[name + ".nodes"] = np.concatenate(nodes_all)
    rec[name + ".runs"] = np.concatenate(runs_all) if runs_all else np.zeros(0)
    rec[name + ".live_row_touched"] = np.asarray(bool(e.live["live_row"].any().item() or e.live["live_state"].any().item()))
    rec[name + ".leaf_evals"] = np.asarray(int(mcts.leaf_evals))
    rec[name + ".lists"] = np.asarray(int(mcts.list_searches))
    rec[name + ".graph"] = np.asarray(bool(mcts.use_graph and not mcts.graph_retry_off))
    if cap:
        rec[name + ".cap_counts"] = mcts.cap_counts.cpu().numpy()


def main():
    rec = {}
    for sc in SCENARIOS:
        run(rec, *sc)
    np.savez(sys.argv[1], **rec)
    print("ok", len(rec))


if __name__ == "__main__":
    main()
