"""TD(lambda) value targets: what noting every search's root value and rewriting the value column of finished games costs.

In one process, alternates `value_target_lambda` off (1.0) and on (--lam, default 0.8) at the C2 (2 048 games x 200
simulations, b6c64) and C3 (16 384 x 800, b10c128) shapes of `self_play_tree_gpu`, each run a single wave of `--plies`
plies (max_game_plies; the games are cut there, so every game ends on the last ply and the target kernel rewrites the whole
wave at once -- its worst case; an untimed two-ply run before each builds the engine and captures its graphs), and prints
one JSON line per run plus a summary per shape with the spread over the repeated pairs:
  ms per ply, and the share of value targets that are no longer a game result.
The games of an off and an on run with the same seed are the same games: only the value column differs.

  python scripts/bench_td_targets.py --shapes C2,C3 --pairs 3 --plies 12
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


def run_once(net, shape, lam, plies, seed):
    import torch
    from liuzhou_amd.tree_engine import self_play_tree_gpu
    s = SHAPES[shape]
    t0 = time.perf_counter()
    batch, st = self_play_tree_gpu(net, num_games=s["games"], mcts_simulations=s["sims"], temperature_init=1.0,
                                   temperature_final=0.1, temperature_threshold=10, exploration_weight=1.0,
                                   device="cuda:0", concurrent_games=s["games"], max_game_plies=plies, seed=seed,
                                   value_target_lambda=lam)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    c = st.mcts_counters
    n_plies = max(1, int(c.get("plies_launched", plies)) - int(c.get("masked_extra_plies", 0)))
    v = batch.value_targets
    return {"shape": shape, "lambda": lam, "ms_per_ply": 1e3 * st.elapsed_sec / n_plies, "plies": n_plies,
            "positions": st.num_positions, "positions_per_s": st.num_positions / st.elapsed_sec,
            "blended_share": float(((v != 0) & (v.abs() != 1)).double().mean()) if v.numel() else 0.0,
            "value_abs_mean": float(v.abs().double().mean()) if v.numel() else 0.0,
            "stream_redraws": c.get("stream_redraws", 0), "wall_s": wall}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2,C3")
    ap.add_argument("--pairs", type=int, default=3, help="repeated (off, on) pairs per shape")
    ap.add_argument("--plies", type=int, default=12, help="plies per run (max_game_plies of the single wave)")
    ap.add_argument("--lam", type=float, default=0.8, help="value_target_lambda of the on runs")
    args = ap.parse_args()
    import torch
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.tree_engine import clear_engine_cache
    for shape in [x.strip() for x in args.shapes.split(",") if x.strip()]:
        s = SHAPES[shape]
        model = ChessNet(**MODEL_CONFIGS[s["model"]])
        stable_resnet_init(model, 20260314)
        net = FusedNet(model.eval().to("cuda:0"))
        rows = {"off": [], "on": []}
        for i in range(args.pairs):
            for key, lam in (("off", 1.0), ("on", args.lam)):
                # a short untimed run first builds the engine and captures its graphs (both stay cached for the timed
                # run: the engine does not depend on lambda); a C3 engine takes a large share of the memory
                run_once(net, shape, lam, 2, seed=999)
                r = run_once(net, shape, lam, args.plies, seed=1000 + i)
                rows[key].append(r)
                print(json.dumps({"run": r}), flush=True)
        clear_engine_cache()

        def agg(key, field):
            v = [r[field] for r in rows[key]]
            return {"median": statistics.median(v), "min": min(v), "max": max(v)}
        fields = ("ms_per_ply", "blended_share", "value_abs_mean", "stream_redraws")
        off_ms = statistics.median(r["ms_per_ply"] for r in rows["off"])
        on_ms = statistics.median(r["ms_per_ply"] for r in rows["on"])
        out = {"shape": shape, "lambda": args.lam, "sims": s["sims"], "plies": args.plies,
               "ms_per_ply_ratio": on_ms / off_ms, "ms_per_ply_delta": on_ms - off_ms,
               **{f"{k}_{f}": agg(k, f) for k in ("off", "on") for f in fields}}
        print(json.dumps({"summary": out}), flush=True)
        del net
        clear_engine_cache()
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
