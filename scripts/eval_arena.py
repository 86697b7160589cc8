#!/usr/bin/env python3
"""Checkpoint evaluation on the device-resident arena: the `--backend v1` (root PUCT) and `--backend portable` (full-tree
search, both checkpoints in one engine) paths of the reference's `scripts/eval_checkpoint.py` (flags of :831-872; other
backends run the v1 path, other backends' flags are accepted and ignored).  The result records the backend that ran.

    python scripts/eval_arena.py --challenger_checkpoint ck/model_iter_003.pt --previous_checkpoint ck/best.pt \
        --eval_games_vs_random 200 --eval_games_vs_previous 400 --mcts_simulations 256 --output_json out/eval.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv=None):
    ap = argparse.ArgumentParser(description="Evaluate checkpoint against random/previous.")
    ap.add_argument("--challenger_checkpoint", required=True)
    ap.add_argument("--previous_checkpoint", default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--backend", default="v1")
    ap.add_argument("--portable_mcts_backend", default=None)      # accepted, no effect: one tree-search implementation
    ap.add_argument("--portable_cpp_threads", type=int, default=None)   # accepted, no effect
    ap.add_argument("--mcts_simulations", type=int, default=256)
    ap.add_argument("--temperature", type=float, default=0.05)
    ap.add_argument("--sample_moves", action="store_true")
    ap.add_argument("--eval_games_vs_random", type=int, default=0)
    ap.add_argument("--eval_games_vs_previous", type=int, default=0)
    ap.add_argument("--v1_opening_random_moves", type=int, default=0)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--match_name", default=None)
    ap.add_argument("--output_json", default=None)
    ap.add_argument("--fpu_reduction", type=float, default=None)         # tree backend: first-play urgency (unset = off)
    ap.add_argument("--fpu_root_reduction", type=float, default=None)    # ... at the root (default: --fpu_reduction)
    ap.add_argument("--cpuct_log", type=float, default=0.0)              # tree backend: visit-scaled cpuct (0 = off)
    ap.add_argument("--cpuct_base", type=float, default=19652.0)
    ap.add_argument("--opening_book", default=None)                      # an OpeningBook file (scripts/build_opening_book.py):
    ap.add_argument("--opening_seed", type=int, default=0)               # colour-swapped pairs from it, assigned by this seed
    args, ignored = ap.parse_known_args(argv)
    args.ignored = ignored
    return args


def backend_of(args) -> str:
    """The search that runs: "portable" (tree search) when asked for, "v1" (root PUCT) for anything else."""
    return "portable" if str(args.backend).strip().lower() == "portable" else "v1"


def opening_book_of(args):
    """The book of --opening_book on the evaluation device, None without the flag.  Refused together with random
    opening moves, before the file or the device is touched."""
    if not args.opening_book:
        return None
    if int(args.v1_opening_random_moves) > 0:
        raise ValueError("--opening_book cannot be combined with --v1_opening_random_moves > 0: the book's positions are "
                         "the openings")
    from liuzhou_amd.opening_book import OpeningBook
    return OpeningBook.load(args.opening_book, args.device)


def main(argv=None) -> int:
    args = parse(argv)
    book = opening_book_of(args)
    from liuzhou_amd.eval_arena import evaluate_checkpoint
    seed = 0 if args.seed is None else int(args.seed)
    backend = backend_of(args)
    common = dict(device=args.device, mcts_simulations=args.mcts_simulations, temperature=args.temperature,
                  sample_moves=bool(args.sample_moves), opening_random_moves=args.v1_opening_random_moves, seed=seed)
    if backend != "v1":
        common["search_backend"] = backend
    if args.fpu_reduction is not None or args.fpu_root_reduction is not None:
        common.update(fpu_reduction=args.fpu_reduction, fpu_root_reduction=args.fpu_root_reduction)
    if args.cpuct_log != 0.0:
        common.update(cpuct_log=args.cpuct_log, cpuct_base=args.cpuct_base)
    if book is not None:
        common.update(opening_book=book, opening_seed=int(args.opening_seed))
    out = {"challenger_checkpoint": args.challenger_checkpoint, "previous_checkpoint": args.previous_checkpoint,
           "backend": backend, "mcts_simulations": int(args.mcts_simulations), "seed": seed}
    if args.eval_games_vs_random > 0:
        out["vs_random"] = evaluate_checkpoint(args.challenger_checkpoint, None, num_games=args.eval_games_vs_random, **common)
    if args.eval_games_vs_previous > 0 and args.previous_checkpoint:
        out["vs_previous"] = evaluate_checkpoint(args.challenger_checkpoint, args.previous_checkpoint,
                                                 num_games=args.eval_games_vs_previous, **common)
    for key in ("vs_random", "vs_previous"):
        if key in out:
            p = out[key]
            print(f"[eval] {args.match_name or key}: W-L-D={p['wins']}-{p['losses']}-{p['draws']} ({p['total_games']} games), "
                  f"win={p['win_rate'] * 100:.2f}% loss={p['loss_rate'] * 100:.2f}% draw={p['draw_rate'] * 100:.2f}%", flush=True)
            if "paired" in p:
                q = p["paired"]
                print(f"[eval] {args.match_name or key}: {q['pairs']} pairs from {q['openings_used']} of {q['book_size']} openings, "
                      f"pentanomial={q['pentanomial']} score={q['score']:.4f} +- {q['score_stderr']:.4f} "
                      f"(as independent games: +- {q['trinomial_stderr']:.4f}) los={q['los']:.3f}", flush=True)
    if args.output_json:
        os.makedirs(os.path.dirname(args.output_json) or ".", exist_ok=True)
        with open(args.output_json, "w") as f:
            json.dump(out, f, indent=2)
    return 0


if __name__ == "__main__":
    sys.exit(main())
