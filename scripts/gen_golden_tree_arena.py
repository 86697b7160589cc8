#!/usr/bin/env python3
"""g19 fixture: the reference's own arena worker on its tree-search backend -> tests/golden/g19_tree_arena.npz.

Two tiny checkpoints play `G` games against each other through `scripts/eval_checkpoint.py::_eval_worker_v1` with
`search_backend="portable"`, `portable_mcts_backend="python"` (`_PortableEvalAgent`: a fresh PortableTree every move, no
root noise), deterministic picks and no random openings.  Recorded: the outcome tuple, every game's move sequence, and
every network evaluation of both agents -- value and the three head rows, keyed by the FNV-1a hash of the packed input
planes -- so that a run on another host replays them instead of re-rounding the convolutions
(tests/test_gpu_arena_tree.py::test_tree_arena_reproduces_the_reference_portable_worker).

Runs on a CPU host with the reference checkout, after build() (oracle/_ref), in the manner of oracle/gen_golden.py's
gen_eval_arena, whose set-up it imports:

    python scripts/gen_golden_tree_arena.py
"""
from __future__ import annotations

import importlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G, SIMS = 4, 8


def main() -> int:
    from oracle import gen_golden as gg                       # reference on sys.path, oracle/_ref's v0_core, OUT
    import numpy as np
    import torch
    ec = importlib.import_module("scripts.eval_checkpoint")
    from src.neural_network import bucket_logits_to_scalar
    models = {}
    for tag, seed in (("chall", 17), ("opp", 18)):
        torch.manual_seed(seed)
        models[tag] = gg.ChessNet(board_size=6, num_input_channels=gg.NUM_INPUT_CHANNELS, trunk_channels=8, num_blocks=1,
                                  policy_channels=4, value_channels=4, value_mlp_channels=8).eval()
    rec = {"chall": {}, "opp": {}}

    class Recording(torch.nn.Module):
        def __init__(self, tag):
            super().__init__()
            self.tag, self.inner = tag, models[tag]

        def forward(self, x):
            out = self.inner(x)
            keys = gg._fnv64(np.packbits(x.detach().cpu().numpy().astype(bool).reshape(x.shape[0], -1), axis=1))
            val = bucket_logits_to_scalar(out[3].float(), num_bins=int(out[3].shape[1])).detach().cpu().numpy()
            heads = torch.cat([o.reshape(x.shape[0], -1) for o in out[:3]], dim=1).detach().cpu().numpy().astype(np.float32)
            for i, k in enumerate(keys.tolist()):
                v = (heads[i].copy(), np.float32(val[i]))
                if k in rec[self.tag]:
                    assert np.array_equal(rec[self.tag][k][0], v[0]) and rec[self.tag][k][1] == v[1], "not batch-invariant"
                rec[self.tag][k] = v
            return out

    ec._load_model_from_checkpoint = lambda path, device: Recording("chall" if "chall" in str(path) else "opp").eval()
    moves, ids = {}, {}
    real_apply = ec.apply_move

    def logging_apply(state, move, quiet=True):
        g = ids.pop(id(state), None)
        if g is None:
            g = len(moves)
            moves[g] = []
        moves[g].append(int(gg.action_to_index(move, 6)))
        nxt = real_apply(state, move, quiet=quiet)
        ids[id(nxt)] = g
        logging_apply.keep.append(nxt)                         # keep ids unique while the game is alive
        return nxt
    logging_apply.keep = []
    ec.apply_move = logging_apply
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    try:
        result = ec._eval_worker_v1(0, list(range(G)), G, "cpu", SIMS, 0.1, "chall.pt", "opp.pt", 0, G, 0, False,
                                    "portable", "python", 1)
    finally:
        ec.apply_move = real_apply
    L = max(len(v) for v in moves.values())
    seq = np.full((G, L), -1, np.int32)
    for g, v in moves.items():
        seq[g, :len(v)] = v
    out = {"result": np.asarray(result, np.int64), "moves": seq, "config": np.asarray([G, SIMS], np.int64)}
    for tag in ("chall", "opp"):
        keys = np.asarray(sorted(rec[tag]), np.uint64)
        out[f"{tag}_keys"] = keys
        out[f"{tag}_values"] = np.asarray([rec[tag][int(k)][1] for k in keys], np.float32)
        out[f"{tag}_heads"] = np.stack([rec[tag][int(k)][0] for k in keys]).astype(np.float32)
    path = os.path.join(gg.OUT, "g19_tree_arena.npz")
    np.savez_compressed(path, **out)
    print(f"[g19] result={result} game lengths={[len(v) for v in moves.values()]} "
          f"evaluations chall/opp={len(rec['chall'])}/{len(rec['opp'])} -> {os.path.getsize(path) / 1024:.1f} KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
