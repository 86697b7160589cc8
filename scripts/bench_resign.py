"""Resignation with play-through calibration: what stopping lost games early buys, and what the threshold costs in truth.

In one process, alternates resignation off (`resign_threshold` 0) and on (--threshold, default -0.9) at the C2 (2 048 games
x 200 simulations, b6c64) shape of `self_play_tree_gpu` (C3: 16 384 x 800, b10c128, on request), games played to their end
in continuous waves of `--concurrent` slots (an untimed two-ply run before each builds the engine and captures its graphs),
and prints one JSON line per run plus a summary per shape with the spread over the repeated pairs:
  recorded positions/s, games/s, plies per game, share of the games that resigned, and the false-positive rate of the
  play-through games (would-be resigners that went on to draw or win / play-through games that wanted to resign).
The games of an off and an on run with the same seed are the same games up to the ply a game resigns at.

  python scripts/bench_resign.py --shapes C2 --pairs 2 --games 512 --concurrent 256 --checkpoint model.pt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"C3": dict(games=16384, sims=800, model="b10c128"), "C2": dict(games=2048, sims=200, model="b6c64")}


def run_once(net, shape, args, threshold, games, plies, seed):
    import torch
    from liuzhou_amd.tree_engine import self_play_tree_gpu
    s = SHAPES[shape]
    t0 = time.perf_counter()
    _, st = self_play_tree_gpu(net, num_games=games, mcts_simulations=s["sims"], temperature_init=1.0,
                               temperature_final=0.1, temperature_threshold=10, exploration_weight=1.0,
                               device="cuda:0", concurrent_games=min(games, args.concurrent), max_game_plies=plies,
                               seed=seed, resign_threshold=threshold, resign_min_moves=args.min_moves,
                               resign_consecutive=args.consecutive, resign_playthrough_fraction=args.playthrough,
                               resign_streak=args.streak)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    c = st.mcts_counters
    would = int(c.get("playthrough_would_resign", 0))
    return {"shape": shape, "threshold": threshold, "games": games, "positions": st.num_positions,
            "positions_per_s": st.num_positions / st.elapsed_sec, "games_per_s": games / st.elapsed_sec,
            "plies_per_game": st.avg_game_length, "W/L/D": [st.black_wins, st.white_wins, st.draws],
            "resigned_share": int(c.get("resigned_games", 0)) / games,
            "false_positive_rate": (int(c.get("playthrough_false_positive", 0)) / would) if would else None,
            **{k: int(c[k]) for k in ("resigned_games", "resigned_black", "resigned_white", "playthrough_games",
                                      "playthrough_would_resign", "playthrough_false_positive", "resign_avg_ply",
                                      "resign_plies_saved_estimate") if k in c},
            "plies_launched": int(c.get("plies_launched", 0)), "elapsed_s": st.elapsed_sec, "wall_s": wall}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2")
    ap.add_argument("--pairs", type=int, default=2, help="repeated (off, on) pairs per shape")
    ap.add_argument("--games", type=int, default=0, help="games per run (default: the shape's)")
    ap.add_argument("--concurrent", type=int, default=16384, help="slots of the wave")
    ap.add_argument("--plies", type=int, default=144, help="max_game_plies")
    ap.add_argument("--threshold", type=float, default=-0.9, help="resign_threshold of the on runs")
    ap.add_argument("--min_moves", type=int, default=10)
    ap.add_argument("--consecutive", type=int, default=3)
    ap.add_argument("--playthrough", type=float, default=0.1)
    ap.add_argument("--streak", default="side", choices=["side", "ply"])
    ap.add_argument("--checkpoint", default=None, help="a trained checkpoint (default: a seeded random net, whose values say "
                                                       "nothing about who wins: its false-positive rate is a coin's)")
    args = ap.parse_args()
    import torch
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.tree_engine import clear_engine_cache
    for shape in [x.strip() for x in args.shapes.split(",") if x.strip()]:
        s = SHAPES[shape]
        if args.checkpoint:
            from liuzhou_amd.self_play_worker import _infer_model
            ck = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
            state = ck["model_state_dict"] if isinstance(ck, dict) and "model_state_dict" in ck else ck
            model = _infer_model(state)
            model.load_state_dict(state, strict=True)
        else:
            model = ChessNet(**MODEL_CONFIGS[s["model"]])
            stable_resnet_init(model, 20260314)
        net = FusedNet(model.eval().to("cuda:0"))
        games = args.games or s["games"]
        rows = {"off": [], "on": []}
        for i in range(args.pairs):
            for key, thr in (("off", 0.0), ("on", args.threshold)):
                run_once(net, shape, args, thr, min(games, args.concurrent), 2, seed=999)       # engine + graphs, untimed
                r = run_once(net, shape, args, thr, games, args.plies, seed=1000 + i)
                rows[key].append(r)
                print(json.dumps({"run": r}), flush=True)
        med = lambda key, f: statistics.median(r[f] for r in rows[key])
        spread = lambda key, f: {"median": med(key, f), "min": min(r[f] for r in rows[key]), "max": max(r[f] for r in rows[key])}
        fps = [r["false_positive_rate"] for r in rows["on"] if r["false_positive_rate"] is not None]
        out = {"shape": shape, "sims": s["sims"], "games": games, "threshold": args.threshold, "min_moves": args.min_moves,
               "consecutive": args.consecutive, "playthrough_fraction": args.playthrough, "streak": args.streak,
               "games_per_s_ratio": med("on", "games_per_s") / med("off", "games_per_s"),
               "positions_per_s_ratio": med("on", "positions_per_s") / med("off", "positions_per_s"),
               **{f"{k}_{f}": spread(k, f) for k in ("off", "on") for f in ("positions_per_s", "games_per_s", "plies_per_game")},
               "resigned_share": spread("on", "resigned_share"),
               "false_positive_rate": statistics.median(fps) if fps else None}
        print(json.dumps({"summary": out}), flush=True)
        del net
        clear_engine_cache()
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
