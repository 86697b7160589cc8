#!/usr/bin/env python3
"""Whole evaluation matches, timed to completion (device synchronised), at the sizes evaluation runs: games/s and
network evaluations/s of
  root      -- the root backend (RootSearchAgent, `--backend v1`),
  tree_seq  -- the tree backend, each agent's games searched by its own engine (play_matches(joint=False)),
  tree_joint-- the tree backend, one search per ply over both agents' games (one network launch per simulation).
The variants alternate within one invocation (`--rounds` rounds of all three); one JSON line per size.  Evaluations
are the leaves the searches evaluated (tree: the engines' evaluation counters; root: not counted, reported as null).

    python scripts/bench_arena.py --games 400 --sims 64 256 --configs b6c64 b10c128 --rounds 2
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=400)
    ap.add_argument("--sims", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--configs", nargs="+", default=["b6c64", "b10c128"])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max_game_plies", type=int, default=512)
    ap.add_argument("--variants", nargs="+", default=["root", "tree_seq", "tree_joint"])
    args = ap.parse_args(argv)
    import torch
    from liuzhou_amd.eval_arena import RootSearchAgent, TreeSearchAgent, play_matches
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    dev = "cuda:0"

    def model(cfg, seed):
        m = ChessNet(**MODEL_CONFIGS[cfg])
        stable_resnet_init(m, seed)
        return m.eval()

    for cfg in args.configs:
        for sims in args.sims:
            ms = (model(cfg, 20260314), model(cfg, 7))
            agents = {"root": [RootSearchAgent(m, dev, sims) for m in ms],
                      "tree_seq": [TreeSearchAgent(m, dev, sims) for m in ms]}
            agents["tree_joint"] = agents["tree_seq"]
            # warm-up (engine construction, graph capture) outside the timed matches
            for v in args.variants:
                play_matches(*agents[v], 32, dev, max_game_plies=8, joint=(v == "tree_joint"), seed=1)
            times = {v: [] for v in args.variants}
            evals = {v: None for v in args.variants}
            results = {}
            for _ in range(args.rounds):
                for v in args.variants:
                    engines = [e for a in agents[v] if isinstance(a, TreeSearchAgent) for k, e in a._engines.items() if isinstance(k, int)]
                    before = sum(int(e.engine.eval_count.sum()) for e in engines)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    st = play_matches(*agents[v], args.games, dev, max_game_plies=args.max_game_plies,
                                      joint=(v == "tree_joint"), seed=3)
                    torch.cuda.synchronize()
                    times[v].append(time.perf_counter() - t0)
                    results[v] = (st.wins, st.losses, st.draws)
                    if v == "tree_seq":
                        evals[v] = sum(int(e.engine.eval_count.sum()) for e in engines) - before
            row = {"config": cfg, "sims": sims, "games": args.games}
            for v in args.variants:
                best = min(times[v])
                row[v] = {"sec": [round(t, 3) for t in times[v]], "games_per_sec": round(args.games / best, 2),
                          "evals_per_sec": None if evals[v] is None else round(evals[v] / best, 1),
                          "wld": results[v]}
            if "tree_joint" in row and "tree_seq" in row:
                row["tree_joint"]["evals_per_sec"] = None if evals["tree_seq"] is None else \
                    round(evals["tree_seq"] / min(times["tree_joint"]), 1)   # the same games: the same evaluations
                row["joint_over_seq_time"] = round(min(times["tree_joint"]) / min(times["tree_seq"]), 3)
            print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
