"""The start bank (game forking, liuzhou_amd/start_bank.py): what its two kernels cost per ply, and what forking does to
the rows of a generation.

Time.  In one process, alternates the rule off and on (`start_capture_prob` --capture, `start_fork_prob` --fork) at the
C2 shape (4 096 games x 200 simulations, b6c64) of `self_play_tree_gpu`, each run a single wave of `--plies` plies (an
untimed two-ply run before each builds the engine and captures its graphs).  The on runs share one bank, so from the
second on the seed kernel forks for real.  Prints one JSON line per run and a summary: ms per ply off and on with the
spread over the repeated pairs, and the HIP-event times of `lz_start_bank_capture` (per ply) and `lz_start_bank_seed`
(once per run: a single wave starts its games before the first ply).  The off runs are the code path without the rule.

Benefit.  Plays --games games to the end on --slots slots (so that slots are re-seated while the bank fills), once with
the rule off and once on, and prints for each: the share of rows `position_dedup` merges away (exact and symmetric), the
share of rows in the movement phases (4, 5 and 7), and for the on run the forked games and their mean move count at the
fork.

  python scripts/bench_start_bank.py --pairs 3 --plies 12
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GAMES, SIMS, MODEL = 4096, 200, "b6c64"


class KernelTimes:
    """HIP-event brackets around WaveTail.start_capture / start_seed."""

    def __init__(self):
        self.events = {"start_capture": [], "start_seed": []}

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
                out[f"{name}_us_median"] = 1e3 * statistics.median(ms)
                out[f"{name}_us_max"] = 1e3 * max(ms)
                out[f"{name}_calls"] = len(ms)
        return out


def play(net, *, games, slots, sims, plies, seed, start=None, timed=False):
    import torch
    from liuzhou_amd import tree_engine
    from liuzhou_amd.wave_tail import WaveTail
    times = KernelTimes()
    saved = (WaveTail.start_capture, WaveTail.start_seed)
    if timed and start:
        WaveTail.start_capture = times.bracket("start_capture", saved[0])
        WaveTail.start_seed = times.bracket("start_seed", saved[1])
    t0 = time.perf_counter()
    try:
        batch, st = tree_engine.self_play_tree_gpu(
            net, num_games=games, mcts_simulations=sims, temperature_init=1.0, temperature_final=0.1,
            temperature_threshold=10, exploration_weight=1.0, device="cuda:0", concurrent_games=slots,
            max_game_plies=plies, seed=seed, **(start or {}))
    finally:
        WaveTail.start_capture, WaveTail.start_seed = saved
    torch.cuda.synchronize()
    c = st.mcts_counters
    n_plies = max(1, int(c.get("plies_launched", plies)) - int(c.get("masked_extra_plies", 0)))
    row = {"on": bool(start), "ms_per_ply": 1e3 * st.elapsed_sec / n_plies, "plies": n_plies, "positions": st.num_positions,
           "wall_s": time.perf_counter() - t0, **{k: v for k, v in c.items() if k.startswith("start_")}, **times.summary()}
    return batch, row


def row_shares(batch):
    """Shares of a generation's rows: merged away by position_dedup (exact, symmetric), and in the movement phases."""
    from liuzhou_amd.position_dedup import merge_duplicate_positions
    n = int(batch.num_samples)
    out = {"rows": n}
    for mode in ("exact", "symmetric"):
        _, info = merge_duplicate_positions(batch.state_tensors, batch.legal_masks, batch.policy_targets, batch.value_targets,
                                            batch.soft_value_targets, mode=mode)
        out[f"merged_away_{mode}"] = 1.0 - info["rows_out"] / max(1, n)
    planes = batch.state_tensors.reshape(n, 11, 36)
    out["movement_phase_share"] = float((planes[:, 7, 0] + planes[:, 8, 0] + planes[:, 10, 0]).sum().item()) / max(1, n)
    out["placement_phase_share"] = float(planes[:, 4, 0].sum().item()) / max(1, n)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3, help="repeated (off, on) pairs of the timing part")
    ap.add_argument("--plies", type=int, default=12, help="plies per timed run (max_game_plies of the single wave)")
    ap.add_argument("--capture", type=float, default=0.02, help="start_capture_prob of the on runs")
    ap.add_argument("--fork", type=float, default=0.5, help="start_fork_prob of the on runs")
    ap.add_argument("--capacity", type=int, default=65536)
    ap.add_argument("--games", type=int, default=GAMES, help="benefit part: games played to the end (0 = skip the part)")
    ap.add_argument("--slots", type=int, default=1024, help="benefit part: concurrent games")
    ap.add_argument("--benefit-sims", type=int, default=SIMS)
    args = ap.parse_args()
    import torch
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.start_bank import StartBank
    from liuzhou_amd.tree_engine import clear_engine_cache
    model = ChessNet(**MODEL_CONFIGS[MODEL])
    stable_resnet_init(model, 20260314)
    net = FusedNet(model.eval().to("cuda:0"))
    rule = dict(start_capture_prob=args.capture, start_fork_prob=args.fork, start_bank_capacity=args.capacity)

    bank = StartBank(args.capacity, "cuda:0")
    rows = {"off": [], "on": []}
    for i in range(args.pairs):
        for key, start in (("off", None), ("on", {**rule, "start_bank": bank})):
            play(net, games=GAMES, slots=GAMES, sims=SIMS, plies=2, seed=999,
                 start={**rule, "start_bank": StartBank(args.capacity, "cuda:0")} if start else None)
            _, r = play(net, games=GAMES, slots=GAMES, sims=SIMS, plies=args.plies, seed=1000 + i, start=start, timed=True)
            rows[key].append(r)
            print(json.dumps({"run": r}), flush=True)
    clear_engine_cache()

    def agg(key, field):
        v = [r[field] for r in rows[key] if field in r]
        return {"median": statistics.median(v), "min": min(v), "max": max(v)} if v else None
    off_ms, on_ms = (statistics.median(r["ms_per_ply"] for r in rows[k]) for k in ("off", "on"))
    print(json.dumps({"summary": {
        "shape": f"{GAMES} games x {SIMS} simulations, {MODEL}, {args.plies} plies", **{k: v for k, v in rule.items()},
        "off_ms_per_ply": agg("off", "ms_per_ply"), "on_ms_per_ply": agg("on", "ms_per_ply"),
        "ms_per_ply_delta": on_ms - off_ms, "ms_per_ply_ratio": on_ms / off_ms,
        "start_capture_us": agg("on", "start_capture_us_median"), "start_seed_us": agg("on", "start_seed_us_median"),
        "forked_games_per_run": [r.get("start_forked_games", 0) for r in rows["on"]],
        "captured_per_run": [r.get("start_captured", 0) for r in rows["on"]]}}), flush=True)

    if args.games > 0:
        for key, start in (("off", None), ("on", {**rule, "start_bank": StartBank(args.capacity, "cuda:0")})):
            batch, r = play(net, games=args.games, slots=args.slots, sims=args.benefit_sims, plies=512, seed=2024, start=start)
            forks = r.get("start_forked_games", 0)
            print(json.dumps({"benefit": {
                "rule": key, "games": args.games, "slots": args.slots, "sims": args.benefit_sims, **row_shares(batch),
                "ms_per_ply": r["ms_per_ply"], "plies": r["plies"], "wall_s": r["wall_s"],
                **({"forked_games": forks, "captured": r.get("start_captured", 0),
                    "fork_avg_move": r.get("start_fork_move_sum", 0) / max(1, forks)} if start else {})}}), flush=True)
            del batch
            clear_engine_cache()
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
