"""Position dedup: how many rows of real self-play merge, and what the merge costs next to a trainer epoch.

Plays `--games` games of `self_play_tree_gpu` (b6c64, `--sims` simulations, root noise and sampled moves on, one wave,
fixed seed) once with `opening_random_moves` 0 and once with 6, and for the rows of each run prints one JSON line with
  (a) rows_in -> rows_out, groups and largest_group for the modes exact and symmetric, and the share of rows that sit in
      a merged group per ply bucket (0-3, 4-11, 12-35, 36+).  The ply is not in a row: the wave tail appends one block
      of rows per ply, so the row cursor after every `WaveTail.record` gives each row's ply;
  (b) device-event times of `merge_duplicate_positions` (after a warm-up call; median of --repeats) and of the keys kernel
      alone with its bytes/s (n x (1584 + 220 + 65) bytes) against the HBM peak, next to the wall time of one trainer
      epoch on the same rows in the same process (second of two runs of one epoch, MIOpen immediate mode), and the merge
      as a fraction of the epoch;
  (c) for --weighting-mode (default exact) with dedup_max_copies = --weighting-max-copies (default 4): the rows trained
      per epoch and the wall time of one trainer epoch (second of two runs, the merge included) with
      dedup_weighting="copies" and with "weight" -- the same groups as min(count, M) copies or once with that weight.
Needs a GPU; there is no fallback.

  python scripts/bench_position_dedup.py --games 4096 --sims 64
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BUCKETS = ((0, 4, "0-3"), (4, 12, "4-11"), (12, 36, "12-35"), (36, 1 << 30, "36+"))
HBM_PEAK = 8.0e12                                  # bytes/s, MI355X data sheet
ROW_BYTES = 1584 + 220 + 65


def play(net, games, sims, opening, max_plies, seed):
    """(batch, ply int64[rows] on the host, stats): one wave; the cursor after every ply's record gives the plies."""
    import torch
    from liuzhou_amd import tree_engine
    from liuzhou_amd.wave_tail import WaveTail
    cursors = []
    saved = WaveTail.record

    def record(self, *a, **kw):
        out = saved(self, *a, **kw)
        cursors.append(self.buffer._cursor.clone())          # on the stream, no host read
        return out
    WaveTail.record = record
    try:
        batch, st = tree_engine.self_play_tree_gpu(
            net, num_games=games, mcts_simulations=sims, temperature_init=1.0, temperature_final=0.1,
            temperature_threshold=10, exploration_weight=1.0, device="cuda:0", concurrent_games=games,
            max_game_plies=max_plies, opening_random_moves=opening, seed=seed)
    finally:
        WaveTail.record = saved
    torch.cuda.synchronize()
    ends = torch.cat(cursors).cpu()
    n = int(batch.num_samples)
    if not cursors or int(ends[-1]) != n:
        raise RuntimeError(f"row cursor log ends at {int(ends[-1]) if cursors else None}, the batch has {n} rows")
    ply = torch.searchsorted(ends, torch.arange(n), right=True)
    return batch, ply, st


def timed_ms(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}


def epoch_seconds(batch, batch_size, **kw):
    import torch
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.train_bridge import train_network_from_tensors
    model = ChessNet(**MODEL_CONFIGS["b6c64"])
    stable_resnet_init(model, 20260314)
    secs = []
    for _ in range(2):                                            # the first run warms the allocator and the kernels up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model, metrics = train_network_from_tensors(model, batch, batch_size=batch_size, epochs=1, device="cuda:0", **kw)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    return (secs, metrics) if kw else secs


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--openings", default="0,6", help="opening_random_moves of the runs")
    ap.add_argument("--max-game-plies", type=int, default=512)
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--weighting-mode", default="exact", choices=("exact", "symmetric"))
    ap.add_argument("--weighting-max-copies", type=int, default=4)
    args = ap.parse_args()
    os.environ.setdefault("LZ_TRAIN_MIOPEN", "immediate")
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_position_dedup.py needs a GPU")
    from liuzhou_amd import position_dedup as D
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.tree_engine import clear_engine_cache
    model = ChessNet(**MODEL_CONFIGS["b6c64"])
    stable_resnet_init(model, 20260314)
    net = FusedNet(model.eval().to("cuda:0"))
    for opening in [int(x) for x in args.openings.split(",") if x.strip()]:
        t0 = time.perf_counter()
        batch, ply, st = play(net, args.games, args.sims, opening, args.max_game_plies, args.seed)
        clear_engine_cache()
        five = (batch.state_tensors, batch.legal_masks, batch.policy_targets, batch.value_targets, batch.soft_value_targets)
        n = int(batch.num_samples)
        out = {"opening_random_moves": opening, "games": args.games, "sims": args.sims, "rows": n,
               "self_play_wall_s": time.perf_counter() - t0, "avg_game_length": st.avg_game_length, "modes": {}}
        for mode in ("exact", "symmetric"):
            _, info = D.merge_duplicate_positions(*five, mode=mode)
            in_merged = (info["count"].to(torch.int64)[info["group_of_row"]] > 1).cpu()
            share = {}
            for lo, hi, name in BUCKETS:
                sel = (ply >= lo) & (ply < hi)
                rows = int(sel.sum())
                share[name] = {"rows": rows, "merged_share": float(in_merged[sel].float().mean()) if rows else None}
            merge_ms = timed_ms(lambda: D.merge_duplicate_positions(*five, mode=mode), args.repeats)
            keys_ms = timed_ms(lambda: D.position_keys(five[0], five[1], symmetric=mode == "symmetric"), args.repeats)
            out["modes"][mode] = {**D.stats_of(info), "merged_share_by_ply": share, "merge_ms": merge_ms, "keys_ms": keys_ms,
                                  "keys_bytes_per_s": n * ROW_BYTES / (keys_ms["median"] * 1e-3),
                                  "keys_share_of_hbm_peak": n * ROW_BYTES / (keys_ms["median"] * 1e-3) / HBM_PEAK}
        secs = epoch_seconds(batch, args.batch_size)
        out["epoch_s"] = {"first": secs[0], "second": secs[1]}
        for mode in out["modes"]:
            out["modes"][mode]["merge_share_of_epoch"] = out["modes"][mode]["merge_ms"]["median"] * 1e-3 / secs[1]
        out["weighting"] = {"mode": args.weighting_mode, "max_copies": args.weighting_max_copies}
        for weighting in ("copies", "weight"):
            secs, metrics = epoch_seconds(batch, args.batch_size, dedup_positions=args.weighting_mode,
                                          dedup_max_copies=args.weighting_max_copies, dedup_weighting=weighting)
            out["weighting"][weighting] = {"rows_trained_per_epoch": metrics["position_dedup"]["rows_out"],
                                           "steps_per_epoch": metrics["total_train_steps"],
                                           "epoch_s": {"first": secs[0], "second": secs[1]}}
        print(json.dumps(out), flush=True)
        del batch, five
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
