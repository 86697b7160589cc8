"""Does the Gumbel target do what the paper says, on this game?  A report, not a gate.

On the states a wave of self-play reaches after `--plies` plies (one network, `--games` games), the KL divergence from
the visit distribution of an 800-simulation PUCT search (no noise, temperature 1) to
  (a) the PUCT visit-count target at n simulations (no noise),
  (b) the Gumbel target at n simulations (`gumbel_considered` = --m), averaged over `--seeds` RNG seeds,
for n in --budgets.  Targets are floored at 1e-6 before the logarithm (a visit-count target from few simulations is zero
on most children, where the KL would be infinite), and renormalised.  One JSON line per budget.

  python scripts/exp_gumbel_kl.py --model b6c64 --games 256 --plies 8 --budgets 16,32,64,200

`--checkpoint FILE` loads a trained state dict; without it the network is the bench's random-init one, whose priors are
nearly flat: the numbers then show little.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="b6c64")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--plies", type=int, default=8)
    ap.add_argument("--budgets", default="16,32,64,200")
    ap.add_argument("--reference-sims", type=int, default=800)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--seeds", type=int, default=8)
    args = ap.parse_args()
    import torch
    from liuzhou_amd import v0_core
    from liuzhou_amd.mcts_gpu import GpuStateBatch
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    dev = torch.device("cuda:0")
    model = ChessNet(**MODEL_CONFIGS[args.model])
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    else:
        stable_resnet_init(model, 20260314)
    net = FusedNet(model.eval().to(dev))
    B = args.games
    ones = torch.ones((B,), dtype=torch.float32, device=dev)

    # the states: `plies` sampled moves of a small PUCT search from the initial position
    state = GpuStateBatch.initial(dev, B)
    walker = PortableTreeMCTS(net, B, 32, dev, add_dirichlet_noise=True, sample_moves=True, seed=4242)
    for t in range(args.plies):
        plies = torch.full((B,), t, dtype=torch.int64, device=dev)
        out = walker.search_batch(state, temperatures=ones, rng_plies=plies,
                                  rng_game_ids=torch.arange(B, dtype=torch.int64, device=dev))
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        v0_core.self_play_step_inplace(*state.tensors(), plies.clone(), done, torch.arange(B, device=dev),
                                       out.chosen_action_codes.clone(), out.terminal_mask.clone(),
                                       out.chosen_valid_mask.clone(), 512, 2.0)
    del walker
    torch.cuda.empty_cache()

    def target(sims, seed, **kw):
        m = PortableTreeMCTS(net, B, sims, dev, add_dirichlet_noise=False, sample_moves=False, seed=seed, **kw)
        out = m.search_batch(state, temperatures=ones)
        torch.cuda.synchronize(dev)
        return out.policy_dense.double().clone(), out.terminal_mask.clone()

    ref, term = target(args.reference_sims, 1)
    live = ~term.bool() & (ref.sum(1) > 0)

    def kl(p, q):
        q = q.clamp_min(1e-6)
        q = q / q.sum(1, keepdim=True)
        t = torch.where(p > 0, p * (torch.log(p.clamp_min(1e-300)) - torch.log(q)), torch.zeros_like(p))
        return float(t.sum(1)[live].mean())

    for n in [int(x) for x in args.budgets.split(",") if x.strip()]:
        puct, _ = target(n, 1)
        g = [kl(ref, target(n, 100 + s, gumbel_considered=args.m)[0]) for s in range(args.seeds)]
        print(json.dumps({"kl": {"model": args.model, "checkpoint": args.checkpoint, "states": int(live.sum()),
                                 "plies": args.plies, "n": n, "m": args.m, "reference_sims": args.reference_sims,
                                 "puct_visit_target": kl(ref, puct), "gumbel_target_mean": sum(g) / len(g),
                                 "gumbel_target_min": min(g), "gumbel_target_max": max(g)}}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
