#!/usr/bin/env python3
"""Round robin of 2..8 checkpoints on the tree backend (all games at once, one engine segment per checkpoint):
W/D/L matrix and points (3 / 1 / 0, as the reference's scripts/tournament_v1_eval.py:28-30) as JSON.

    python scripts/tournament.py ck/a.pt ck/b.pt ck/c.pt --games_per_pair 40 --mcts_simulations 128 --output_json rr.json

With --sample_moves the move sampling is keyed by each game's index in the whole round robin, so a pair's games are not
those of a two-checkpoint match of the same seed; with deterministic picks (the default) they are.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv=None):
    ap = argparse.ArgumentParser(description="Round robin of checkpoints on the tree search.")
    ap.add_argument("checkpoints", nargs="+")
    ap.add_argument("--games_per_pair", type=int, default=40)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--mcts_simulations", type=int, default=128)
    ap.add_argument("--temperature", type=float, default=0.05)
    ap.add_argument("--sample_moves", action="store_true")
    ap.add_argument("--opening_random_moves", type=int, default=0)
    ap.add_argument("--max_game_plies", type=int, default=512)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--output_json", default=None)
    args = ap.parse_args(argv)
    if not 2 <= len(args.checkpoints) <= 8:
        ap.error("a round robin takes 2..8 checkpoints")
    return args


def main(argv=None) -> int:
    args = parse(argv)
    from liuzhou_amd.eval_arena import TreeSearchAgent, load_checkpoint_model, play_round_robin
    agents = [TreeSearchAgent(load_checkpoint_model(p), args.device, args.mcts_simulations, args.temperature,
                              args.sample_moves, seed=args.seed) for p in args.checkpoints]
    rr = play_round_robin(agents, args.games_per_pair, args.device, opening_random_moves=args.opening_random_moves,
                          max_game_plies=args.max_game_plies, seed=args.seed)
    out = {"backend": "portable", "games_per_pair": int(args.games_per_pair),
           "mcts_simulations": int(args.mcts_simulations), "seed": int(args.seed), **rr.to_payload(args.checkpoints)}
    for name, pts in sorted(zip(args.checkpoints, rr.points), key=lambda x: -x[1]):
        print(f"[tournament] {pts:5d} pts  {name}", flush=True)
    if args.output_json:
        os.makedirs(os.path.dirname(args.output_json) or ".", exist_ok=True)
        with open(args.output_json, "w") as f:
            json.dump(out, f, indent=2)
    return 0


if __name__ == "__main__":
    sys.exit(main())
