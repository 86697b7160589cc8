#!/usr/bin/env python3
"""Build an opening book for the evaluation arena (liuzhou_amd/opening_book.py) from positions self-play games passed
through: the distinct (up to board symmetry), playable positions of a start bank.

The positions come from a file -- `--records FILE`, a .pt holding `StartBank.state_dict()` or a raw uint8[n, 32] tensor of
packed states -- or from games played here: `--checkpoint CKPT --games N --mcts_simulations S --capture_prob q` plays tree
self-play (`self_play_tree_gpu`) with a bank of its own that only captures (start_fork_prob = 0).  Prints the book's
`meta` as one JSON line.

    python scripts/build_opening_book.py --checkpoint ck/best.pt --games 512 --mcts_simulations 64 --capture_prob 0.05 \
        --min_move 6 --max_move 40 --max_positions 400 --out out/book.pt
    python scripts/eval_arena.py --challenger_checkpoint ck/new.pt --previous_checkpoint ck/best.pt --backend portable \
        --eval_games_vs_previous 400 --opening_book out/book.pt
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv=None):
    ap = argparse.ArgumentParser(description="Build an opening book from start-bank positions.")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--records", default=None, help=".pt: StartBank.state_dict() or a uint8[n,32] tensor")
    src.add_argument("--checkpoint", default=None, help="play self-play games with this checkpoint and keep their positions")
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--mcts_simulations", type=int, default=64)
    ap.add_argument("--capture_prob", type=float, default=0.05)
    ap.add_argument("--bank_capacity", type=int, default=65536)
    ap.add_argument("--concurrent_games", type=int, default=256)
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--min_move", type=int, default=0)
    ap.add_argument("--max_move", type=int, default=143)
    ap.add_argument("--max_positions", type=int, default=None)
    ap.add_argument("--out", required=True)
    return ap.parse_args(argv)


def records_of_file(path: str):
    """uint8[n, 32] (CPU): the filled rows of a saved StartBank, or the raw tensor."""
    import torch
    obj = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(obj, dict) and "entries" in obj and "cursor" in obj:
        entries, cursor = obj["entries"], obj["cursor"]
        if not isinstance(entries, torch.Tensor) or not isinstance(cursor, torch.Tensor) or int(cursor.numel()) != 1:
            raise ValueError(f"{path}: not a StartBank.state_dict()")
        obj = entries[:max(0, min(int(cursor.view(-1)[0].item()), int(entries.shape[0])))]
    if not isinstance(obj, torch.Tensor) or obj.dtype != torch.uint8 or obj.dim() != 2 or int(obj.shape[1]) != 32:
        raise ValueError(f"{path}: expected StartBank.state_dict() or a uint8[n, 32] tensor")
    return obj.contiguous()


def records_of_games(args):
    """The filled rows of a private bank after `--games` games of tree self-play that capture and never fork."""
    from liuzhou_amd.eval_arena import load_checkpoint_model
    from liuzhou_amd.start_bank import StartBank
    from liuzhou_amd.tree_engine import self_play_tree_gpu
    bank = StartBank(int(args.bank_capacity), args.device)
    self_play_tree_gpu(load_checkpoint_model(args.checkpoint).to(args.device), num_games=int(args.games),
                       mcts_simulations=int(args.mcts_simulations), temperature_init=1.0, temperature_final=0.1,
                       temperature_threshold=10, exploration_weight=1.0, device=args.device,
                       concurrent_games=int(args.concurrent_games), seed=int(args.seed), start_bank=bank,
                       start_fork_prob=0.0, start_capture_prob=float(args.capture_prob),
                       start_bank_capacity=int(args.bank_capacity), start_min_move=int(args.min_move),
                       start_max_move=int(args.max_move))
    return bank.entries[:bank.filled()]


def main(argv=None) -> int:
    args = parse(argv)
    from liuzhou_amd.opening_book import OpeningBook
    records = records_of_file(args.records) if args.records else records_of_games(args)
    book = OpeningBook.from_packed(records, min_move=args.min_move, max_move=args.max_move, max_positions=args.max_positions)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    book.save(args.out)
    print(json.dumps(book.meta), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
