"""Playout cap randomization: what the saving in network rows does to wall time.

In one process, alternates the cap off and on at the C3 (16 384 games x 800 simulations, b10c128) and C2 (2 048 x 200,
b6c64) shapes of `self_play_tree_gpu`, each run a single wave of `--plies` plies (max_game_plies; the games are cut
there; an untimed two-ply run before each builds the engine and captures its graphs), and prints one JSON line per run plus a summary per (shape, setting) with the spread over the repeated pairs:
  games/s, recorded positions/s (falls by design: only full searches record a row), network rows per ply (live_total /
  plies, from the device counters), ms per ply, stream_redraws (C2's two-stream search).
Arithmetic predicts rows per ply at p + (1 - p) F / S of the cap-off run.

  python scripts/bench_playout_cap.py --shapes C2,C3 --pairs 3 --plies 16
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


def run_once(net, shape, fast, prob, plies, seed):
    import torch
    from liuzhou_amd.tree_engine import self_play_tree_gpu
    s = SHAPES[shape]
    t0 = time.perf_counter()
    batch, st = self_play_tree_gpu(net, num_games=s["games"], mcts_simulations=s["sims"], temperature_init=1.0,
                                   temperature_final=0.1, temperature_threshold=10, exploration_weight=1.0,
                                   device="cuda:0", concurrent_games=s["games"], max_game_plies=plies, seed=seed,
                                   playout_cap_fast_simulations=fast, playout_cap_full_prob=prob)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    c = st.mcts_counters
    n_plies = max(1, int(c.get("plies_launched", plies)) - int(c.get("masked_extra_plies", 0)))
    return {"shape": shape, "fast": fast, "full_prob": prob, "games_per_s": st.num_games / st.elapsed_sec,
            "positions_per_s": st.num_positions / st.elapsed_sec, "rows_per_ply": c["leaf_eval_count"] / n_plies,
            "ms_per_ply": 1e3 * st.elapsed_sec / n_plies, "plies": n_plies, "stream_redraws": c.get("stream_redraws", 0),
            "positions": st.num_positions, "full_searches": c.get("full_searches"), "fast_searches": c.get("fast_searches"),
            "wall_s": wall}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2,C3")
    ap.add_argument("--pairs", type=int, default=3, help="repeated (off, on) pairs per setting")
    ap.add_argument("--plies", type=int, default=16, help="plies per run (max_game_plies of the single wave)")
    ap.add_argument("--settings", default="0.25:4,0.5:8",
                    help="p:S/F pairs -- 0.25:4 is p = 0.25, F = S / 4")
    args = ap.parse_args()
    import torch
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.tree_engine import clear_engine_cache
    settings = [(float(a), int(b)) for a, b in (x.split(":") for x in args.settings.split(","))]
    summary = []
    for shape in [x.strip() for x in args.shapes.split(",") if x.strip()]:
        s = SHAPES[shape]
        model = ChessNet(**MODEL_CONFIGS[s["model"]])
        stable_resnet_init(model, 20260314)
        net = FusedNet(model.eval().to("cuda:0"))
        for p, div in settings:
            fast = s["sims"] // div
            rows = {"off": [], "on": []}
            for i in range(args.pairs):
                for key, (F, P) in (("off", (0, 1.0)), ("on", (fast, p))):
                    # a short untimed run first builds the engine and captures its graphs (both stay cached for the
                    # timed run); only one engine is alive at a time (a C3 engine takes a large share of the memory)
                    run_once(net, shape, F, P, 2, seed=999)
                    r = run_once(net, shape, F, P, args.plies, seed=1000 + i)
                    rows[key].append(r)
                    print(json.dumps({"run": r}), flush=True)
                    clear_engine_cache()
            def agg(key, field):
                v = [r[field] for r in rows[key]]
                return {"median": statistics.median(v), "min": min(v), "max": max(v)}
            fields = ("games_per_s", "positions_per_s", "rows_per_ply", "ms_per_ply", "stream_redraws")
            out = {"shape": shape, "full_prob": p, "fast": fast, "sims": s["sims"],
                   "predicted_rows_ratio": p + (1 - p) * fast / s["sims"],
                   "rows_ratio": statistics.median(r["rows_per_ply"] for r in rows["on"]) /
                                 statistics.median(r["rows_per_ply"] for r in rows["off"]),
                   "ms_per_ply_ratio": statistics.median(r["ms_per_ply"] for r in rows["on"]) /
                                       statistics.median(r["ms_per_ply"] for r in rows["off"]),
                   **{f"{k}_{f}": agg(k, f) for k in ("off", "on") for f in fields}}
            summary.append(out)
            print(json.dumps({"summary": out}), flush=True)
        del net
        clear_engine_cache()
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
