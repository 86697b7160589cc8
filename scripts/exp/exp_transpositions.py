"""How many of a search's network evaluations repeat a position the same tree already holds?  (Decides whether an
in-tree position index -- a transposed leaf takes the priors and value of its twin -- would shorten the launches.)

Steady-state population as in bench.py (random-init net, subtree reuse, preroll).  Around every search (after the
advance, before the first launch / after the last expand) the node arena of every game is read back: a node (index >= 1;
the root carries the Dirichlet mix and is never a source) whose 32-byte state an earlier node of the same arena holds
would have been a shared leaf.  Searched trees are unchanged by sharing (bit-identical priors / value), so the count on
the plain search is exactly the count the skip would see.

    python scripts/exp/exp_transpositions.py C3 [steps]     # 16 384 games x 800 sims, 10x128
    python scripts/exp/exp_transpositions.py C2 [steps]     #  4 096 games x 200 sims, 6x64 (two parts, two streams)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
from liuzhou_amd.net_hip import FusedNet
from liuzhou_amd.tree_engine import SteadyStateTreeSelfPlay

WORKLOADS = {"C2": (4096, 200, "b6c64"), "C3": (16384, 800, "b10c128")}


def repeats(e, chunk_games: int = 2048):
    """(nodes >= 1, of them repeating an earlier node >= 1 of the same arena, of them equal to the root) over all games."""
    B, cap = e.B, e.node_cap
    nodes = e.buf["nodes"].view(B, cap, 6)
    nn = e.buf["n_nodes"].to(torch.int64)
    m = int(nn.max().item())
    if m <= 1:
        return 0, 0, 0
    tot = rep = at_root = 0
    for g0 in range(0, B, chunk_games):
        g1 = min(B, g0 + chunk_games)
        st = nodes[g0:g1, 1:m, :4].clone()                                  # (b, m-1, 4) packed states
        idx = torch.arange(1, m, device=st.device)
        valid = idx[None, :] < nn[g0:g1, None]
        sentinel = (-1 - idx)[None, :, None].expand_as(st)                  # unique per slot: never equal to another
        st = torch.where(valid[:, :, None], st, sentinel)
        root = nodes[g0:g1, 0:1, :4]
        at_root += int(((st == root).all(dim=2) & valid).sum().item())
        order = torch.arange(m - 1, device=st.device)[None, :].expand(g1 - g0, m - 1).contiguous()
        for w in (3, 2, 1, 0):                                              # exact lexicographic order: stable sorts
            key = torch.gather(st[:, :, w], 1, order)
            _, o = torch.sort(key, dim=1, stable=True)
            order = torch.gather(order, 1, o)
        srt = torch.gather(st, 1, order[:, :, None].expand(-1, -1, 4))
        same = (srt[:, 1:] == srt[:, :-1]).all(dim=2)
        rep += int(same.sum().item())
        tot += int(valid.sum().item())
    return tot, rep, at_root


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "C3"
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    games, sims, model = WORKLOADS[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(20260314)
    net = FusedNet(ChessNet(**MODEL_CONFIGS[model]).eval().to(dev))
    torch.manual_seed(9973)
    pop = SteadyStateTreeSelfPlay(net, games, sims=sims, device=dev, reuse_tree=True, dual_stream=True, seed=9973,
                                  arena_rows=games * (steps + 12))
    parts = [pop.mcts] if hasattr(pop.mcts, "engine") else list(pop.mcts.parts)
    pop.preroll(120)
    pop.prepare()
    acc = {"searches": 0, "consumed": 0, "launched": 0, "new_nodes": 0, "new_repeats": 0, "new_root_twins": 0,
           "kept_nodes": 0}
    on = [False]

    def hook(part):
        inner = part._search

        def wrapped(add_noise, continue_trees):
            if not on[0]:
                return inner(add_noise, continue_trees)
            e = part.engine
            torch.cuda.synchronize(dev)
            n0, r0, t0 = repeats(e)
            c0 = int(e.eval_count.sum(dtype=torch.int64).item())
            inner(add_noise, continue_trees)
            torch.cuda.synchronize(dev)
            n1, r1, t1 = repeats(e)
            c1 = int(e.eval_count.sum(dtype=torch.int64).item())
            acc["searches"] += 1
            acc["consumed"] += c1 - c0
            acc["launched"] += e.B * (part.sims + 1)
            acc["new_nodes"] += n1 - n0
            acc["new_repeats"] += r1 - r0
            acc["new_root_twins"] += t1 - t0
            acc["kept_nodes"] += n0
        part._search = wrapped

    for p in parts:
        hook(p)
    for _ in range(2):                                                      # settle past the prepare() searches
        pop.step()
    torch.cuda.synchronize(dev)
    on[0] = True
    for _ in range(steps):
        pop.step()
    torch.cuda.synchronize(dev)
    out = dict(workload=name, games=games, sims=sims, model=model, steps=steps, **acc)
    out["share_of_consumed_evals"] = acc["new_repeats"] / max(1, acc["consumed"])
    out["share_of_launched_rows"] = acc["new_repeats"] / max(1, acc["launched"])
    out["kept_nodes_per_search"] = acc["kept_nodes"] / max(1, acc["searches"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
