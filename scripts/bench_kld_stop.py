"""KLD-gain early stopping: how many simulations the rule saves and what that does to wall time.

In one process, alternates the rule off and on at the C3 (16 384 games x 800 simulations, b10c128) and C2 (2 048 x 200,
b6c64) shapes of `self_play_tree_gpu`, each run a single wave of `--plies` plies (max_game_plies; the games are cut
there; an untimed two-ply run before each builds the engine and captures its graphs), and prints one JSON line per run
plus a summary per (shape, threshold) with the spread over the repeated pairs:
  mean simulations per search (S - kld_simulations_saved / searches; a run this short ends no game, so searches = games x
  plies), share of searches stopped, network rows per ply (live_total / plies, from the device counters) and their ratio
  to the off run, ms per ply, games/s, stream_redraws (C2's two-stream search).
The nets are randomly initialised (stable_resnet_init): their priors are nearly flat and their values near zero, so the
visit distributions settle more slowly than a trained net's would -- the numbers say what the machinery costs and saves
on such a net, not what a training run gains.

  python scripts/bench_kld_stop.py --shapes C2,C3 --pairs 3 --plies 16 --thresholds 2e-5,1e-4
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


def run_once(net, shape, threshold, interval, min_sims, plies, seed):
    import torch
    from liuzhou_amd.tree_engine import self_play_tree_gpu
    s = SHAPES[shape]
    t0 = time.perf_counter()
    batch, st = self_play_tree_gpu(net, num_games=s["games"], mcts_simulations=s["sims"], temperature_init=1.0,
                                   temperature_final=0.1, temperature_threshold=10, exploration_weight=1.0,
                                   device="cuda:0", concurrent_games=s["games"], max_game_plies=plies, seed=seed,
                                   kld_stop_threshold=threshold, kld_stop_interval=interval,
                                   kld_stop_min_simulations=min_sims)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    c = st.mcts_counters
    n_plies = max(1, int(c.get("plies_launched", plies)) - int(c.get("masked_extra_plies", 0)))
    searches = max(1, s["games"] * n_plies)
    return {"shape": shape, "threshold": threshold, "interval": interval, "games_per_s": st.num_games / st.elapsed_sec,
            "positions_per_s": st.num_positions / st.elapsed_sec, "rows_per_ply": c["leaf_eval_count"] / n_plies,
            "ms_per_ply": 1e3 * st.elapsed_sec / n_plies, "plies": n_plies, "stream_redraws": c.get("stream_redraws", 0),
            "mean_sims_per_search": s["sims"] - c.get("kld_simulations_saved", 0) / searches,
            "stopped_share": c.get("kld_stopped_searches", 0) / searches, "wall_s": wall}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2,C3")
    ap.add_argument("--pairs", type=int, default=3, help="repeated (off, on) pairs per threshold")
    ap.add_argument("--plies", type=int, default=16, help="plies per run (max_game_plies of the single wave)")
    ap.add_argument("--thresholds", default="2e-5,1e-4,5e-4", help="kld_stop_threshold values")
    ap.add_argument("--interval", type=int, default=100, help="kld_stop_interval")
    ap.add_argument("--min_simulations", type=int, default=None, help="kld_stop_min_simulations (default: the interval)")
    args = ap.parse_args()
    import torch
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.tree_engine import clear_engine_cache
    thresholds = [float(x) for x in args.thresholds.split(",") if x.strip()]
    for shape in [x.strip() for x in args.shapes.split(",") if x.strip()]:
        s = SHAPES[shape]
        model = ChessNet(**MODEL_CONFIGS[s["model"]])
        stable_resnet_init(model, 20260314)
        net = FusedNet(model.eval().to("cuda:0"))
        for theta in thresholds:
            rows = {"off": [], "on": []}
            for i in range(args.pairs):
                for key, thr in (("off", 0.0), ("on", theta)):
                    # a short untimed run first builds the engine and captures its graphs (both stay cached for the
                    # timed run); only one engine is alive at a time (a C3 engine takes a large share of the memory)
                    run_once(net, shape, thr, args.interval, args.min_simulations, 2, seed=999)
                    r = run_once(net, shape, thr, args.interval, args.min_simulations, args.plies, seed=1000 + i)
                    rows[key].append(r)
                    print(json.dumps({"run": r}), flush=True)
                    clear_engine_cache()

            def agg(key, field):
                v = [r[field] for r in rows[key]]
                return {"median": statistics.median(v), "min": min(v), "max": max(v)}
            med = lambda key, field: statistics.median(r[field] for r in rows[key])
            fields = ("games_per_s", "rows_per_ply", "ms_per_ply", "mean_sims_per_search", "stopped_share", "stream_redraws")
            out = {"shape": shape, "threshold": theta, "interval": args.interval, "sims": s["sims"],
                   "rows_ratio": med("on", "rows_per_ply") / med("off", "rows_per_ply"),
                   "ms_per_ply_ratio": med("on", "ms_per_ply") / med("off", "ms_per_ply"),
                   "games_per_s_ratio": med("on", "games_per_s") / med("off", "games_per_s"),
                   **{f"{k}_{f}": agg(k, f) for k in ("off", "on") for f in fields}}
            print(json.dumps({"summary": out}), flush=True)
        del net
        clear_engine_cache()
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
