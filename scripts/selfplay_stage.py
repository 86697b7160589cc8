#!/usr/bin/env python3
"""`--stage selfplay` of the reference pipeline on MI355X (scripts/big_train_v1.sh:667-704 ->
scripts/train_entry.py --pipeline v1 --stage selfplay): same flags, same outputs (chunk files + the
`v1_sharded_manifest` at --self_play_output, optional --self_play_stats_json), one worker process per device.

    python scripts/selfplay_stage.py --stage selfplay --devices cuda:0,cuda:1 --self_play_games 32768 \
        --mcts_simulations 800 --self_play_concurrent_games 16384 --self_play_output out/selfplay_iter_001.pt

Flags of the other stages (--train_devices, --batch_size, ...) are accepted and ignored so the reference's command
line can be passed through unchanged.  `--search_backend portable` selects the full-tree engine.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pipeline", default="v1")
    ap.add_argument("--stage", default="selfplay", choices=["selfplay"])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--devices", default=None, help="comma-separated self-play devices")
    ap.add_argument("--self_play_games", type=int, default=4)
    ap.add_argument("--mcts_simulations", type=int, default=32)
    ap.add_argument("--temperature_init", type=float, default=1.0)
    ap.add_argument("--temperature_final", type=float, default=0.1)
    ap.add_argument("--temperature_threshold", type=int, default=10)
    ap.add_argument("--exploration_weight", type=float, default=1.0)
    ap.add_argument("--dirichlet_alpha", type=float, default=0.3)
    ap.add_argument("--dirichlet_epsilon", type=float, default=0.25)
    ap.add_argument("--soft_value_k", type=float, default=2.0)
    ap.add_argument("--soft_label_alpha", type=float, default=0.0)
    ap.add_argument("--max_game_plies", type=int, default=512)
    ap.add_argument("--self_play_concurrent_games", type=int, default=8)
    ap.add_argument("--self_play_opening_random_moves", type=int, default=0)
    ap.add_argument("--sparse_ply", type=int, default=1)
    ap.add_argument("--sparse_top_k", type=int, default=8)
    ap.add_argument("--self_play_backend", default="process")
    ap.add_argument("--search_backend", default="cuda_root", choices=["cuda_root", "portable", "tree"])
    ap.add_argument("--policy_target_temperature", type=float, default=None)
    ap.add_argument("--policy_target_prior_pseudocount", type=float, default=0.0)
    ap.add_argument("--playout_cap_fast_simulations", type=int, default=0,
                    help="playout cap randomization (tree backend): simulations of a fast search, 0 = off")
    ap.add_argument("--playout_cap_full_prob", type=float, default=1.0,
                    help="playout cap randomization: probability that a move gets a full search and a training row")
    ap.add_argument("--forced_playouts_k", type=float, default=0.0,
                    help="forced playouts and policy target pruning (tree backend): k of sqrt(k * prior * root visits), 0 = off")
    ap.add_argument("--gumbel_considered", type=int, default=0,
                    help="Gumbel root search with Sequential Halving (tree backend): considered root actions m, 0 = off "
                         "(the paper uses 16)")
    ap.add_argument("--gumbel_c_visit", type=float, default=50.0, help="Gumbel root search: c_visit of sigma")
    ap.add_argument("--gumbel_c_scale", type=float, default=1.0, help="Gumbel root search: c_scale of sigma")
    ap.add_argument("--value_target_lambda", type=float, default=1.0,
                    help="TD(lambda) value targets (tree backend): lambda of y_t = (1 - lambda) Q_t + lambda y_(t+1) over the "
                         "searches' root values, 1 = off (every row gets the final result)")
    ap.add_argument("--mcts_solver", action="store_true",
                    help="MCTS-Solver (tree backend): mark proven wins, draws and losses in the search tree, stop searching "
                         "decided children and never play away a proven win")
    ap.add_argument("--fpu_reduction", type=float, default=None,
                    help="first-play urgency (tree backend): an unvisited child scores the node's own value minus this times "
                         "sqrt(explored prior mass); unset = off (unvisited children score 0), 0 = the node's value")
    ap.add_argument("--fpu_root_reduction", type=float, default=None,
                    help="the reduction at the root (default: --fpu_reduction)")
    ap.add_argument("--cpuct_log", type=float, default=0.0,
                    help="visit-scaled exploration (tree backend): c(n) = exploration_weight + cpuct_log * "
                         "ln((n + cpuct_base + 1) / cpuct_base); 0 = off")
    ap.add_argument("--cpuct_base", type=float, default=19652.0, help="base of the visit-scaled exploration constant")
    ap.add_argument("--self_play_resign_threshold", type=float, default=0.0,
                    help="resignation (tree backend): a game resigns once its searches' root values were <= this value "
                         "--self_play_resign_consecutive times in a row; in [-1, 0), 0 = off")
    ap.add_argument("--self_play_resign_min_moves", type=int, default=10, help="resignation: no resignation before this ply")
    ap.add_argument("--self_play_resign_consecutive", type=int, default=3,
                    help="resignation: eligible low-value searches in a row needed to resign")
    ap.add_argument("--self_play_resign_playthrough_fraction", type=float, default=0.1,
                    help="resignation: seeded share of games that never resign and measure the false positives")
    ap.add_argument("--self_play_resign_streak", default="side", choices=["side", "ply"],
                    help="resignation: 'side' counts the mover's own searches, 'ply' every searched ply (the reference's "
                         "literal counter)")
    ap.add_argument("--kld_stop_threshold", type=float, default=0.0,
                    help="KLD-gain early stopping (tree backend): a search ends once its root visit distribution gains "
                         "less than this per simulation between two checks; 0 = off")
    ap.add_argument("--kld_stop_interval", type=int, default=100, help="KLD-gain early stopping: simulations between checks")
    ap.add_argument("--kld_stop_min_simulations", type=int, default=None,
                    help="KLD-gain early stopping: no stop before this many simulations (default: the interval)")
    ap.add_argument("--move_visit_offset", type=float, default=0.0,
                    help="move selection (tree backend): visits subtracted from every root child before the move is "
                         "sampled; children left with none are not played; 0 = off")
    ap.add_argument("--move_value_cutoff", type=float, default=0.0,
                    help="move selection (tree backend): children whose mean value is more than this below the most "
                         "visited child's are not played; in [0, 2], 0 = off")
    ap.add_argument("--temperature_halflife", type=float, default=0.0,
                    help="move temperature (tree backend): below --temperature_threshold the excess over "
                         "--temperature_final halves every this many plies; 0 = off (the step)")
    ap.add_argument("--policy_surprise_weight", type=float, default=0.0,
                    help="policy surprise weighting (tree backend): share of a game's total row weight handed out in "
                         "proportion to KL(policy target || network prior); in [0, 1], 0 = off (KataGo uses 0.5)")
    ap.add_argument("--start_fork_prob", type=float, default=0.0,
                    help="start bank (tree backend): share of the games that start from a position of an earlier game "
                         "instead of the empty board (liuzhou_amd/start_bank.py); in [0, 1], 0 = off")
    ap.add_argument("--start_capture_prob", type=float, default=0.0,
                    help="start bank: share of the searched positions that is kept in the shard's bank; in [0, 1], 0 = off")
    ap.add_argument("--start_bank_capacity", type=int, default=65536, help="start bank: positions the ring holds")
    ap.add_argument("--start_min_move", type=int, default=1,
                    help="start bank: smallest move count that is kept (1: never the empty board)")
    ap.add_argument("--start_max_move", type=int, default=143, help="start bank: largest move count that is kept")
    ap.add_argument("--self_play_target_samples_per_shard", type=int, default=0)
    ap.add_argument("--self_play_chunk_target_bytes", type=int, default=0)
    ap.add_argument("--self_play_shard_dir", default=None)
    ap.add_argument("--model_init_seed", type=int, default=int(os.environ.get("V1_MODEL_INIT_SEED", "20260314")))
    ap.add_argument("--model", default="b10c128", choices=["b6c64", "b10c128"],
                    help="architecture when no checkpoint is loaded (the reference always builds 10x128)")
    ap.add_argument("--checkpoint_dir", default="./checkpoints_v1")
    ap.add_argument("--load_checkpoint", default=None)
    ap.add_argument("--self_play_output", default=None)
    ap.add_argument("--self_play_iteration_seed", type=int, default=1)
    ap.add_argument("--self_play_stats_json", default=None)
    args, ignored = ap.parse_known_args(argv)
    args.ignored = ignored
    return args


def main(argv=None) -> int:
    args = parse(argv)
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.self_play_stage import run_self_play_stage
    from liuzhou_amd.self_play_worker import _infer_model
    if int(args.self_play_iteration_seed) <= 0:
        raise ValueError(f"self_play_iteration_seed must be positive when provided, got {args.self_play_iteration_seed}")
    devices = [d.strip() for d in str(args.devices or args.device).split(",") if d.strip()]
    if args.load_checkpoint:
        if not os.path.exists(args.load_checkpoint):
            raise FileNotFoundError(f"Checkpoint not found: {args.load_checkpoint}")
        ckpt = torch.load(args.load_checkpoint, map_location="cpu", weights_only=False)
        state = ckpt["model_state_dict"] if isinstance(ckpt, dict) and "model_state_dict" in ckpt else ckpt
        model = _infer_model(state)
        model.load_state_dict(state, strict=True)
    else:
        model = ChessNet(**MODEL_CONFIGS[args.model])
        if int(args.model_init_seed) > 0:
            stable_resnet_init(model, int(args.model_init_seed))
    model.eval()
    output = str(args.self_play_output or os.path.join(args.checkpoint_dir, "selfplay_batch_v1.pt"))
    meta = {"stage": "selfplay", "source_checkpoint": args.load_checkpoint, "self_play_devices": devices,
            "self_play_backend": args.self_play_backend, "search_backend": args.search_backend,
            "self_play_shard_dir": args.self_play_shard_dir, "mcts_simulations": int(args.mcts_simulations),
            "self_play_games": int(args.self_play_games),
            "self_play_concurrent_games": int(args.self_play_concurrent_games),
            "self_play_opening_random_moves": int(args.self_play_opening_random_moves),
            "self_play_iteration_seed": int(args.self_play_iteration_seed),
            "policy_target_temperature": args.policy_target_temperature,
            "policy_target_prior_pseudocount": float(args.policy_target_prior_pseudocount)}
    stats, manifest = run_self_play_stage(
        model_state=model.state_dict(), num_games=int(args.self_play_games), devices=devices, output_path=output,
        iteration_seed=int(args.self_play_iteration_seed), mcts_simulations=int(args.mcts_simulations),
        temperature_init=args.temperature_init, temperature_final=args.temperature_final,
        temperature_threshold=args.temperature_threshold, exploration_weight=args.exploration_weight,
        dirichlet_alpha=args.dirichlet_alpha, dirichlet_epsilon=args.dirichlet_epsilon, soft_value_k=args.soft_value_k,
        soft_label_alpha=args.soft_label_alpha, opening_random_moves=args.self_play_opening_random_moves,
        max_game_plies=args.max_game_plies, concurrent_games_per_device=args.self_play_concurrent_games,
        shard_dir=args.self_play_shard_dir, target_samples_per_shard=args.self_play_target_samples_per_shard,
        chunk_target_bytes=args.self_play_chunk_target_bytes, metadata_base=meta, sparse_ply=args.sparse_ply,
        sparse_top_k=args.sparse_top_k, search_backend=args.search_backend,
        policy_target_temperature=args.policy_target_temperature,
        policy_target_prior_pseudocount=args.policy_target_prior_pseudocount,
        playout_cap_fast_simulations=args.playout_cap_fast_simulations, playout_cap_full_prob=args.playout_cap_full_prob,
        forced_playouts_k=args.forced_playouts_k, gumbel_considered=args.gumbel_considered,
        gumbel_c_visit=args.gumbel_c_visit, gumbel_c_scale=args.gumbel_c_scale,
        value_target_lambda=args.value_target_lambda, **({"mcts_solver": True} if args.mcts_solver else {}),
        **({"fpu_reduction": args.fpu_reduction, "fpu_root_reduction": args.fpu_root_reduction}
           if args.fpu_reduction is not None or args.fpu_root_reduction is not None else {}),
        **({"cpuct_log": args.cpuct_log, "cpuct_base": args.cpuct_base} if args.cpuct_log != 0.0 else {}),
        resign_threshold=args.self_play_resign_threshold, resign_min_moves=args.self_play_resign_min_moves,
        resign_consecutive=args.self_play_resign_consecutive,
        resign_playthrough_fraction=args.self_play_resign_playthrough_fraction,
        resign_streak=args.self_play_resign_streak,
        **({"kld_stop_threshold": args.kld_stop_threshold, "kld_stop_interval": args.kld_stop_interval,
            "kld_stop_min_simulations": args.kld_stop_min_simulations} if args.kld_stop_threshold != 0.0 else {}),
        **({"move_visit_offset": args.move_visit_offset, "move_value_cutoff": args.move_value_cutoff}
           if (args.move_visit_offset != 0.0 or args.move_value_cutoff != 0.0) else {}),
        **({"temperature_halflife": args.temperature_halflife} if args.temperature_halflife != 0.0 else {}),
        **({"policy_surprise_weight": args.policy_surprise_weight} if args.policy_surprise_weight != 0.0 else {}),
        **({"start_fork_prob": args.start_fork_prob, "start_capture_prob": args.start_capture_prob,
            "start_bank_capacity": args.start_bank_capacity, "start_min_move": args.start_min_move,
            "start_max_move": args.start_max_move}
           if (args.start_fork_prob != 0.0 or args.start_capture_prob != 0.0) else {}))
    print(f"[selfplay] games={stats.num_games} positions={stats.num_positions} "
          f"positions/s={stats.positions_per_sec:.1f} W/L/D={stats.black_wins}/{stats.white_wins}/{stats.draws} "
          f"shards={manifest['num_shards']} -> {output}", flush=True)
    if args.self_play_stats_json:
        os.makedirs(os.path.dirname(args.self_play_stats_json) or ".", exist_ok=True)
        with open(args.self_play_stats_json, "w") as f:
            json.dump({"stats": stats.to_dict(), "num_shards": manifest["num_shards"],
                       "num_samples": manifest["num_samples"], "output": output,
                       "value_target_summary": manifest["metadata"].get("value_target_summary", {})}, f, indent=2)
    return 0


if __name__ == "__main__":
    sys.exit(main())
