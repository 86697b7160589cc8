"""Visit-offset / value-cutoff move selection: what the re-pick changes, and a short run for a kernel trace.

Per shape (C2: 4 096 games x 200 simulations, b6c64, two streams; C3: 16 384 x 800, b10c128) one wave of `--plies` plies
of `self_play_tree_gpu` with the rule off and one with it on, from the opening position, and one JSON line per run:
  off: the share of sampled plies (non-terminal root, temperature > 1e-6) on which the finish played a child with at most
       `--low` visits -- counted on the device behind every search, no host read per ply;
  on:  move_pick_changed / move_pick_applied and the two cut counters, ms per ply next to the off run's.
`--trace`: only a short on run with the solver on, direct launches of finish / move pick / solver pick, for
  rocprofv3 --kernel-trace --stats -- python scripts/bench_move_pick.py --trace --shapes C2 --plies 4
The nets are randomly initialised (stable_resnet_init): nearly flat priors and values near zero, so the numbers say what
the rule does on such a net, not on a trained one.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"C3": dict(games=16384, sims=800, model="b10c128"), "C2": dict(games=4096, sims=200, model="b6c64")}


def watch_low_visit_picks(low: int):
    """Wrap PortableTreeMCTS.complete_search: behind every search, count the sampled plies and those whose played child has
    at most `low` visits (one device tensor per engine -- the halves of a two-stream search run on streams of their own --
    read once at the end).  Returns (counts by engine, undo)."""
    import torch
    from liuzhou_amd import tree_engine as TE
    orig = TE.PortableTreeMCTS.complete_search
    box = {}

    def wrapped(self, state, *, temperatures, **kw):
        out = orig(self, state, temperatures=temperatures, **kw)
        e = self.engine
        if id(e) not in box:
            box[id(e)] = torch.zeros((2,), dtype=torch.int64, device=e.device)
        cols = torch.arange(e.child_action.shape[1], device=e.device)[None, :]
        hit = (e.child_action == e.chosen_index[:, None]) & (cols < e.child_count[:, None])
        n = (e.child_visits * hit).sum(1)
        sampled = (e.terminal_mask == 0) & (temperatures.to(torch.float32) > 1e-6) & hit.any(1)
        box[id(e)] += torch.stack((sampled.sum(), (sampled & (n <= low)).sum()))
        return out
    TE.PortableTreeMCTS.complete_search = wrapped
    return box, lambda: setattr(TE.PortableTreeMCTS, "complete_search", orig)


def run_once(net, shape, plies, seed, sims=None, **kw):
    import torch
    from liuzhou_amd.tree_engine import self_play_tree_gpu
    s = SHAPES[shape]
    _, st = self_play_tree_gpu(net, num_games=s["games"], mcts_simulations=int(sims or s["sims"]), temperature_init=1.0,
                               temperature_final=0.1, temperature_threshold=10, exploration_weight=1.0, device="cuda:0",
                               concurrent_games=s["games"], max_game_plies=plies, seed=seed, **kw)
    torch.cuda.synchronize()
    c = st.mcts_counters
    n_plies = max(1, int(c.get("plies_launched", plies)) - int(c.get("masked_extra_plies", 0)))
    return {"shape": shape, "plies": n_plies, "ms_per_ply": 1e3 * st.elapsed_sec / n_plies,
            **{k: int(v) for k, v in c.items() if k.startswith("move_pick") or k.startswith("solver_")}}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2,C3")
    ap.add_argument("--plies", type=int, default=12)
    ap.add_argument("--sims", type=int, default=None, help="simulations per search (default: the shape's)")
    ap.add_argument("--offset", type=float, default=2.0, help="move_visit_offset of the on run")
    ap.add_argument("--cutoff", type=float, default=0.1, help="move_value_cutoff of the on run")
    ap.add_argument("--low", type=int, default=3, help="off run: a played child with at most this many visits counts as low")
    ap.add_argument("--trace", action="store_true", help="one short on run with the solver on, nothing else")
    args = ap.parse_args()
    import torch
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.tree_engine import clear_engine_cache
    on = dict(move_visit_offset=args.offset, move_value_cutoff=args.cutoff)
    for shape in [x.strip() for x in args.shapes.split(",") if x.strip()]:
        model = ChessNet(**MODEL_CONFIGS[SHAPES[shape]["model"]])
        stable_resnet_init(model, 20260314)
        net = FusedNet(model.eval().to("cuda:0"))
        if args.trace:
            print(json.dumps({"trace": run_once(net, shape, args.plies, 1000, args.sims, mcts_solver=True, **on)}), flush=True)
        else:
            run_once(net, shape, 2, 999, args.sims)                  # builds the engine and captures its graphs
            box, undo = watch_low_visit_picks(args.low)
            off = run_once(net, shape, args.plies, 1000, args.sims)
            undo()
            sampled, low = (int(x) for x in sum(box.values()).tolist())
            off.update(sampled_plies=sampled, low_visit_picks=low, low_visit_share=low / max(1, sampled), low=args.low)
            print(json.dumps({"off": off}), flush=True)
            clear_engine_cache()
            run_once(net, shape, 2, 999, args.sims, **on)
            r = run_once(net, shape, args.plies, 1000, args.sims, **on)
            r.update(offset=args.offset, cutoff=args.cutoff,
                     changed_share=r["move_pick_changed"] / max(1, r["move_pick_applied"]))
            print(json.dumps({"on": r}), flush=True)
        del net
        clear_engine_cache()
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
