"""Merging duplicate positions across the replay window, record to record: what it costs next to
the composition it replaces (unpack -> tensor merge -> pack), and what it does to a training pass over a window.

Three modes, one JSON line each.  Needs a GPU; there is no fallback.

  kernels   launches lz_replay_position_keys and lz_replay_merge_records --launches times (after --warmup) at every size of
            --rows, on fixed groups.  Meant to run under a kernel trace, in a run of its own:
              rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_replay_merge.py kernels
            (kernel names replay_position_keys_kernel / replay_merge_records_kernel).  Prints the bytes the two kernels
            need per launch (88 header bytes + 65 output bytes per row; 360 bytes per member + 360 per group).
  compare   `ReplayWindow.merge_selection` against `unpack_records` -> `merge_duplicate_positions(weighting="weight")` ->
            `pack_batch` on the same selection, alternated, --repeats times after one warm-up each: wall time around a
            device synchronise (median, min, max) and the peak of `torch.cuda.max_memory_allocated` above what was
            allocated before the call.  Checks that both give the same records.
  train     one pass of `train_network_from_window` (b6c64, batch 4 096, AMP, MIOpen immediate mode) over a window of two
            generations of `self_play_tree_gpu` (--games games each, --sims simulations), merge off and on (symmetric,
            --max-weight), alternated twice; rows per epoch, seconds of the second run, the `merge` stats.

The records of `kernels` and `compare` are synthetic and seeded: n / 4 positions (random boards, about 30 legal actions),
drawn with a skew that gives the most frequent position about (4 / n) ** (1 / 3) of the rows -- the empty board of a
window -- each row under a random board symmetry with a policy of its own.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"


def synthetic_ring(n: int, seed: int):
    """uint8[n,360] records on the device."""
    import torch
    from liuzhou_amd.replay_window import gather_records
    from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
    from liuzhou_amd.trajectory_codec import pack_batch
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    pool = max(1, n // 4)
    rec = torch.zeros((pool, 360), dtype=torch.uint8, device=DEV)
    words = torch.randint(0, 1 << 36, (pool, 4), generator=g, device=DEV, dtype=torch.int64)
    words[:, 0] |= torch.randint(0, 8, (pool,), generator=g, device=DEV, dtype=torch.int64) << 36
    rec[:, :32] = words.view(torch.uint8).view(pool, 32)
    legal = torch.rand((pool, 224), generator=g, device=DEV) < 0.135
    legal[:, 220:] = False
    legal[:, 0] = True
    weights = (1 << torch.arange(8, device=DEV, dtype=torch.int32)).view(1, 1, 8)
    rec[:, 32:60] = (legal.view(pool, 28, 8).to(torch.int32) * weights).sum(dim=2).to(torch.uint8)
    rec[:, 60:348] = torch.rand((pool, 72), generator=g, device=DEV).view(torch.uint8).view(pool, 288)
    out = torch.empty((n, 360), dtype=torch.uint8, device=DEV)
    for a in range(0, n, 65536):
        b = min(n, a + 65536)
        idx = (pool * torch.rand((b - a,), generator=g, device=DEV) ** 3).long().clamp(max=pool - 1)
        sym = torch.randint(0, 8, (b - a,), generator=g, device=DEV, dtype=torch.int32)
        planes, masks, _, _, _ = gather_records(rec, idx, sym)
        policy = torch.rand((b - a, 220), generator=g, device=DEV) * masks
        policy = policy / policy.sum(dim=1, keepdim=True)
        value = torch.randint(-1, 2, (b - a,), generator=g, device=DEV).float()
        soft = torch.rand((b - a,), generator=g, device=DEV) * 2 - 1
        out[a:b] = pack_batch(TensorSelfPlayBatch(planes, masks, policy, value, soft))       # raises if not representable
    return out


def run_kernels(args) -> dict:
    import torch
    from liuzhou_amd import _lib as L
    from liuzhou_amd import position_dedup as D
    from liuzhou_amd import replay_window as RW
    result = {"mode": "kernels", "launches": args.launches, "sizes": []}
    for n in args.rows:
        ring = synthetic_ring(n, args.seed)
        slots = torch.randperm(n, device=DEV)
        keys, sym, bad = RW.record_position_keys(ring, slots, symmetric=True)
        _, order, begin, count = D.group_rows(keys)
        groups = int(count.numel())
        merged = torch.empty((groups, 360), dtype=torch.uint8, device=DEV)
        cnt = torch.empty((groups,), dtype=torch.int32, device=DEV)
        stream = L.stream_ptr(torch.device(DEV))
        for _ in range(args.warmup + args.launches):
            L.check(L.lib().lz_replay_position_keys(L.ptr(ring), L.i64(n), L.ptr(slots), L.i64(n), 1, L.ptr(keys), L.ptr(sym),
                                                    L.ptr(bad), stream), "keys")
            L.check(L.lib().lz_replay_merge_records(L.ptr(ring), L.i64(n), L.ptr(slots), L.i64(n), L.ptr(sym), L.ptr(order),
                                                    L.ptr(begin), L.i64(groups), L.ptr(merged), L.ptr(cnt), L.ptr(bad), stream),
                    "merge")
        torch.cuda.synchronize()
        result["sizes"].append({"rows": n, "groups": groups, "largest_group": int(count.max()),
                                "keys_bytes": n * (88 + 8 + 65), "merge_bytes": n * (360 + 8 + 8 + 1) + groups * (360 + 8 + 4)})
    return result


def _timed(fn, repeats):
    import torch
    fn()                                                            # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times, peaks = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        peaks.append(torch.cuda.max_memory_allocated() - base)
        del out
    return times, peaks


def run_compare(args) -> dict:
    import torch
    from liuzhou_amd import position_dedup as D
    from liuzhou_amd.replay_window import ReplayWindow
    from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
    from liuzhou_amd.trajectory_codec import pack_batch, unpack_records
    result = {"mode": "compare", "repeats": args.repeats, "max_weight": args.max_weight, "sizes": []}
    for n in args.rows:
        window = ReplayWindow(DEV, max_generations=1, capacity_rows=n)
        window.add_generation(synthetic_ring(n, args.seed))
        slots = window.select()

        def merged_records():
            return window.merge_selection(slots, mode="symmetric", max_weight=args.max_weight)

        def composition():
            rows = unpack_records(window.ring.index_select(0, slots))
            outs, info = D.merge_duplicate_positions(rows.state_tensors, rows.legal_masks, rows.policy_targets,
                                                     rows.value_targets, rows.soft_value_targets, mode="symmetric",
                                                     max_copies=args.max_weight, weighting="weight")
            return pack_batch(TensorSelfPlayBatch(*outs)), info["weights"], info

        a, b = merged_records(), composition()
        same = bool(torch.equal(a[0], b[0])) and bool(torch.equal(a[1], b[1]))
        del a, b
        torch.cuda.empty_cache()
        new_t, new_m, old_t, old_m = [], [], [], []
        for _ in range(args.repeats):                               # alternated
            t, m = _timed(merged_records, 1)
            new_t += t; new_m += m
            t, m = _timed(composition, 1)
            old_t += t; old_m += m
        info = merged_records()[2]
        summary = lambda xs: {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}
        result["sizes"].append({
            "rows": n, "groups": info["groups"], "largest_group": info["largest_group"], "same_records_and_weights": same,
            "merge_selection_sec": summary(new_t), "composition_sec": summary(old_t),
            "merge_selection_peak_bytes": max(new_m), "composition_peak_bytes": max(old_m),
            "peak_bytes_per_row": {"merge_selection": max(new_m) / n, "composition": max(old_m) / n},
            "memory_ratio": max(old_m) / max(1, max(new_m)), "time_ratio": statistics.median(old_t) / statistics.median(new_t)})
    return result


def run_train(args) -> dict:
    import torch
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.replay_window import ReplayWindow
    from liuzhou_amd.train_bridge import train_network_from_window
    from liuzhou_amd.tree_engine import self_play_tree_gpu
    os.environ.setdefault("LZ_TRAIN_MIOPEN", "immediate")

    def fresh():
        model = ChessNet(**MODEL_CONFIGS["b6c64"])
        stable_resnet_init(model, 20260314)
        return model.to(DEV)

    net = FusedNet(fresh().eval(), torch.device(DEV))
    window = ReplayWindow(DEV, max_generations=2, capacity_rows=2 * args.games * 144)
    for generation in (1, 2):                                       # two generations of the same network, other seeds
        batch, _ = self_play_tree_gpu(net, num_games=args.games, mcts_simulations=args.sims, temperature_init=1.0,
                                      temperature_final=0.1, temperature_threshold=10, exploration_weight=1.0, device=DEV,
                                      max_game_plies=144, concurrent_games=args.games, seed=args.seed + generation)
        window.add_generation(batch, generation=generation)
    runs = {"off": [], "on": []}
    metrics = {}
    for _ in range(2):                                              # alternated; the second run of each is reported
        for name, kw in (("off", {}), ("on", {"replay_merge_positions": "symmetric", "replay_merge_max_weight": args.max_weight})):
            torch.manual_seed(5)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, m = train_network_from_window(fresh(), window, batch_size=4096, epochs=1, device=DEV,
                                             replay_budget_per_generation=10 ** 9, **kw)
            torch.cuda.synchronize()
            runs[name].append(time.perf_counter() - t0)
            metrics[name] = m
    return {"mode": "train", "games": args.games, "sims": args.sims, "max_weight": args.max_weight,
            "rows_selected": metrics["off"]["replay_window"]["rows_selected"],
            "off": {"rows_per_epoch": metrics["off"]["num_samples"], "steps": metrics["off"]["total_train_steps"],
                    "sec": runs["off"], "avg_loss": metrics["off"]["epoch_stats"][-1]["avg_loss"]},
            "on": {"rows_per_epoch": metrics["on"]["num_samples"], "steps": metrics["on"]["total_train_steps"],
                   "sec": runs["on"], "avg_loss": metrics["on"]["epoch_stats"][-1]["avg_loss"],
                   "merge": metrics["on"]["replay_window"]["merge"], "row_weights": metrics["on"]["row_weights"]}}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("kernels", "compare", "train"))
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 524288])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-weight", type=int, default=4)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=16)
    ap.add_argument("--seed", type=int, default=20261021)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_replay_merge.py needs a GPU; there is no fallback")
    out = {"kernels": run_kernels, "compare": run_compare, "train": run_train}[args.mode](args)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
