"""MCTS-Solver: what the marks, the climb and the decided-edge rule cost, and what they do.

Cost (`--shapes`): in one process, alternates `mcts_solver` off and on at the C2 (2 048 games x 200 simulations, b6c64) and
C3 (16 384 x 800, b10c128) shapes of `self_play_tree_gpu`, each run a single wave of `--plies` plies (an untimed two-ply run
before each builds the engine and captures its graphs), and prints one JSON line per run plus a summary per shape:
  ms per ply, ms per simulation step (ms per ply / (sims + 1): tree kernel + network launch), positions/s, and with the
  solver on: proofs, decided roots and changed picks per search, and the share of decisive games.
With the solver on the search always runs the one-wave tree step (off: the two-wave step up to 8 192 games), so the C2
difference contains that choice; `LZ_TREE_SPLIT=0` for the whole process takes it out.

Effect (`--effect`): on the positions of tests/golden/g20_solver.npz (12 forced wins within three edges) at 50, 200 and
800 simulations of the random-init 6x64 net, `--copies` copies of each with their own random streams, sampled moves at
temperature 1: the share of roots proven won and the share of winning moves played, on against off.

  python scripts/bench_solver.py --shapes C2,C3 --pairs 3 --plies 12
  python scripts/bench_solver.py --shapes "" --effect
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


def run_once(net, shape, solver, plies, seed):
    import torch
    from liuzhou_amd.tree_engine import self_play_tree_gpu
    s = SHAPES[shape]
    t0 = time.perf_counter()
    _batch, st = self_play_tree_gpu(net, num_games=s["games"], mcts_simulations=s["sims"], temperature_init=1.0,
                                    temperature_final=0.1, temperature_threshold=10, exploration_weight=1.0,
                                    device="cuda:0", concurrent_games=s["games"], max_game_plies=plies, seed=seed,
                                    **({"mcts_solver": True} if solver else {}))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    c = st.mcts_counters
    n_plies = max(1, int(c.get("plies_launched", plies)) - int(c.get("masked_extra_plies", 0)))
    searches = max(1, st.num_positions)
    ms_ply = 1e3 * st.elapsed_sec / n_plies
    return {"shape": shape, "solver": int(solver), "ms_per_ply": ms_ply, "ms_per_sim_step": ms_ply / (s["sims"] + 1),
            "plies": n_plies, "positions": st.num_positions, "positions_per_s": st.num_positions / st.elapsed_sec,
            "proofs_per_search": c.get("solver_proofs", 0) / searches,
            "roots_decided_per_search": c.get("solver_roots_decided", 0) / searches,
            "pick_overrides": c.get("solver_pick_overrides", 0),
            "decisive_share": (st.black_wins + st.white_wins) / max(1, st.num_games), "wall_s": wall}


FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g20_solver.npz")
FIELDS = ("board", "marks_black", "marks_white", "phase", "current_player", "pending_marks_required",
          "pending_marks_remaining", "pending_captures_required", "pending_captures_remaining", "forced_removals_done",
          "move_count", "moves_since_capture")


def effect(copies: int, sims_list):
    """The forced-win positions of tests/golden/g20_solver.npz (states s_* and winning_moves bool[12, 220]: the moves a
    brute-force minimax proves winning), `copies` copies each."""
    import numpy as np
    import torch
    from liuzhou_amd.mcts_gpu import GpuStateBatch
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    z = np.load(FIXTURE)
    model = ChessNet(**MODEL_CONFIGS["b6c64"])
    stable_resnet_init(model, 20260314)
    net = FusedNet(model.eval().to("cuda:0"))
    wins = torch.from_numpy(np.repeat(z["winning_moves"], copies, axis=0))
    B = int(wins.shape[0])
    ts = []
    for f in FIELDS:
        a = np.repeat(z["s_" + f], copies, axis=0)
        dt = np.int8 if f == "board" else (bool if f.startswith("marks") else np.int64)
        ts.append(torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to("cuda:0"))
    for sims in sims_list:
        row = {"effect": {"sims": sims, "roots": B}}
        for solver in (False, True):
            m = PortableTreeMCTS(net, B, sims, "cuda:0", exploration_weight=1.0, add_dirichlet_noise=True, sample_moves=True,
                                 seed=7, solver=solver)
            out = m.search_batch(GpuStateBatch(*[t.clone() for t in ts]),
                                 temperatures=torch.ones(B, dtype=torch.float32, device="cuda:0"))
            torch.cuda.synchronize()
            chosen = out.chosen_action_indices.cpu()
            key = "on" if solver else "off"
            row["effect"][key + "_winning_moves_share"] = float(wins[torch.arange(B), chosen].float().mean())
            if solver:
                row["effect"]["on_roots_proven_won_share"] = float((out.root_proven == 3).float().mean())
                row["effect"]["on_pick_overrides"] = int(m.solver_counts[2])
            del m
        print(json.dumps(row), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2,C3")
    ap.add_argument("--pairs", type=int, default=3, help="repeated (off, on) pairs per shape")
    ap.add_argument("--plies", type=int, default=12, help="plies per run (max_game_plies of the single wave)")
    ap.add_argument("--effect", action="store_true", help="the forced-win positions at 50 / 200 / 800 simulations")
    ap.add_argument("--copies", type=int, default=4)
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
            for key, solver in (("off", False), ("on", True)):
                run_once(net, shape, solver, 2, seed=999)           # untimed: engine construction and graph capture
                r = run_once(net, shape, solver, args.plies, seed=1000 + i)
                rows[key].append(r)
                print(json.dumps({"run": r}), flush=True)
                clear_engine_cache()

        def agg(key, field):
            v = [r[field] for r in rows[key]]
            return {"median": statistics.median(v), "min": min(v), "max": max(v)}
        fields = ("ms_per_ply", "ms_per_sim_step", "positions_per_s", "proofs_per_search", "roots_decided_per_search",
                  "pick_overrides", "decisive_share")
        out = {"shape": shape, "sims": s["sims"], "plies": args.plies,
               "ms_per_ply_ratio": statistics.median(r["ms_per_ply"] for r in rows["on"]) /
                                   statistics.median(r["ms_per_ply"] for r in rows["off"]),
               **{f"{k}_{f}": agg(k, f) for k in ("off", "on") for f in fields}}
        print(json.dumps({"summary": out}), flush=True)
        del net
        clear_engine_cache()
        torch.cuda.empty_cache()
    if args.effect:
        effect(args.copies, (50, 200, 800))
    return 0


if __name__ == "__main__":
    sys.exit(main())
