"""Policy surprise weighting: what the extra root-prior launch, the surprise of every recorded row and the resampling of
finished games cost.

In one process, alternates `policy_surprise_weight` off (0) and on (--alpha, default 0.5) at the C2 (2 048 games x 200
simulations, b6c64) and C3 (16 384 x 800, b10c128) shapes of `self_play_tree_gpu`, each run a single wave of `--plies`
plies (max_game_plies; the games are cut there, so every game ends on the last ply and the resampling kernel rewrites the
whole wave at once -- its worst case; an untimed two-ply run before each builds the engine and captures its graphs), and
prints one JSON line per run plus a summary per shape with the spread over the repeated pairs:
  ms per ply, and for the on runs the HIP-event times of the root-prior evaluation, of `lz_wave_note_surprise` (mean per
  ply) and of `lz_wave_surprise_resample` (mean per ply, and the ply on which the games finish).
The games of an off and an on run with the same seed are the same games: only which of a game's rows fill its slots
differs.

  python scripts/bench_policy_surprise.py --shapes C2,C3 --pairs 3 --plies 12
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


class KernelTimes:
    """HIP-event brackets around the feature's three per-ply steps (root_prior, WaveTail.note_surprise / surprise_resample)."""

    def __init__(self):
        self.events = {"root_prior": [], "note_surprise": [], "surprise_resample": []}

    def bracket(self, name, fn):
        import torch

        def timed(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            self.events[name].append((e0, e1))
            return out
        return timed

    def summary(self):
        import torch
        torch.cuda.synchronize()
        out = {}
        for name, ev in self.events.items():
            ms = [a.elapsed_time(b) for a, b in ev]
            if ms:
                out[f"{name}_ms_mean"] = sum(ms) / len(ms)
                out[f"{name}_ms_max"] = max(ms)
        return out


def run_once(net, shape, alpha, plies, seed, timed=False):
    import torch
    from liuzhou_amd import tree_engine
    from liuzhou_amd.wave_tail import WaveTail
    s = SHAPES[shape]
    times = KernelTimes()
    saved = (tree_engine.root_prior, WaveTail.note_surprise, WaveTail.surprise_resample)
    if timed and alpha > 0:
        tree_engine.root_prior = times.bracket("root_prior", saved[0])
        WaveTail.note_surprise = times.bracket("note_surprise", saved[1])
        WaveTail.surprise_resample = times.bracket("surprise_resample", saved[2])
    t0 = time.perf_counter()
    try:
        batch, st = tree_engine.self_play_tree_gpu(
            net, num_games=s["games"], mcts_simulations=s["sims"], temperature_init=1.0, temperature_final=0.1,
            temperature_threshold=10, exploration_weight=1.0, device="cuda:0", concurrent_games=s["games"],
            max_game_plies=plies, seed=seed, policy_surprise_weight=alpha)
    finally:
        tree_engine.root_prior, WaveTail.note_surprise, WaveTail.surprise_resample = saved
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    c = st.mcts_counters
    n_plies = max(1, int(c.get("plies_launched", plies)) - int(c.get("masked_extra_plies", 0)))
    return {"shape": shape, "alpha": alpha, "ms_per_ply": 1e3 * st.elapsed_sec / n_plies, "plies": n_plies,
            "positions": st.num_positions, "positions_per_s": st.num_positions / st.elapsed_sec,
            "rows_replaced_share": c.get("surprise_rows_replaced", 0) / max(1, c.get("surprise_rows", 1)),
            "mean_surprise": c.get("surprise_mean", 0) / 1e6, "stream_redraws": c.get("stream_redraws", 0),
            "wall_s": wall, **times.summary()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2,C3")
    ap.add_argument("--pairs", type=int, default=3, help="repeated (off, on) pairs per shape")
    ap.add_argument("--plies", type=int, default=12, help="plies per run (max_game_plies of the single wave)")
    ap.add_argument("--alpha", type=float, default=0.5, help="policy_surprise_weight of the on runs")
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
            for key, alpha in (("off", 0.0), ("on", args.alpha)):
                # a short untimed run first builds the engine and captures its graphs (both stay cached for the timed
                # run: the engine does not depend on the weight); a C3 engine takes a large share of the memory
                run_once(net, shape, alpha, 2, seed=999)
                r = run_once(net, shape, alpha, args.plies, seed=1000 + i, timed=True)
                rows[key].append(r)
                print(json.dumps({"run": r}), flush=True)
        clear_engine_cache()

        def agg(key, field):
            v = [r[field] for r in rows[key] if field in r]
            return {"median": statistics.median(v), "min": min(v), "max": max(v)} if v else None
        off_ms = statistics.median(r["ms_per_ply"] for r in rows["off"])
        on_ms = statistics.median(r["ms_per_ply"] for r in rows["on"])
        on_fields = ("ms_per_ply", "rows_replaced_share", "mean_surprise", "root_prior_ms_mean", "note_surprise_ms_mean",
                     "surprise_resample_ms_mean", "surprise_resample_ms_max")
        out = {"shape": shape, "alpha": args.alpha, "sims": s["sims"], "plies": args.plies,
               "ms_per_ply_ratio": on_ms / off_ms, "ms_per_ply_delta": on_ms - off_ms,
               "off_ms_per_ply": agg("off", "ms_per_ply"), **{f"on_{f}": agg("on", f) for f in on_fields}}
        print(json.dumps({"summary": out}), flush=True)
        del net
        clear_engine_cache()
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
