"""First-play urgency and the visit-scaled exploration constant: what the shaped select step costs.

In one process, for the C2 half (2 048 games x 200 simulations, b6c64) and C3 (16 384 x 800, b10c128) launch shapes of
`PortableTreeMCTS`, alternates five variants `--runs` times each, after one untimed search per variant (engine construction,
graph capture, warm caches):
  off_split      the plain search with the two-waves-per-game step (today's default up to 8 192 games; above that launch size
                 the library takes the one-wave step anyway, and the variant says so)
  off_one_wave   the plain search with the one-wave step (LZ_TREE_SPLIT=0): what a shaped search gives up before it computes
                 anything
  fpu            first-play urgency 0.2 / 0.1
  table          c(n) with log 1.25, base 19652
  both
Per run: one search of a mixed-phase batch from tests/golden/g1_rules.npz, replayed from its hipGraph -- wall time between
two device synchronisations, positions/s = games / that time -- and the same search once more with direct launches and the
step kernel bracketed by device events (lz_prof_enable / lz_prof_aux_summary kind 0): microseconds per step-kernel launch.
Every variant launches every slot at every simulation (compact_evals=False): the list and gathering forms are chosen by
the launch size and by LZ_TREE_SPLIT, and would differ between the variants.
One JSON line per run, one summary per shape and variant (median, min, max: the spread is the number to read first).

  python scripts/bench_puct_shape.py --shapes C2,C3 --runs 3
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"C2": dict(games=2048, sims=200, model="b6c64"), "C3": dict(games=16384, sims=800, model="b10c128")}
VARIANTS = {"off_split": (None, {}), "off_one_wave": ("0", {}),
            "fpu": (None, dict(fpu_reduction=0.2, fpu_root_reduction=0.1)),
            "table": (None, dict(cpuct_log=1.25, cpuct_base=19652.0)),
            "both": (None, dict(fpu_reduction=0.2, fpu_root_reduction=0.1, cpuct_log=1.25, cpuct_base=19652.0))}
FIELDS = ("board", "marks_black", "marks_white", "phase", "current_player", "pending_marks_required",
          "pending_marks_remaining", "pending_captures_required", "pending_captures_remaining", "forced_removals_done",
          "move_count", "moves_since_capture")


def positions(games: int, seed: int = 0):
    import numpy as np
    import torch
    from liuzhou_amd.mcts_gpu import GpuStateBatch
    z = np.load(os.path.join(ROOT, "tests", "golden", "g1_rules.npz"))
    idx = np.random.default_rng(seed).integers(0, z["s_board"].shape[0], games)
    ts = []
    for f in FIELDS:
        dt = np.int8 if f == "board" else (bool if f.startswith("marks") else np.int64)
        ts.append(torch.from_numpy(np.ascontiguousarray(z["s_" + f][idx].astype(dt))).to("cuda:0"))
    return GpuStateBatch(*ts)


def build(net, shape, variant):
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    split, kw = VARIANTS[variant]
    if split is None:
        os.environ.pop("LZ_TREE_SPLIT", None)
    else:
        os.environ["LZ_TREE_SPLIT"] = split                       # read at every launch, frozen into a captured graph
    s = SHAPES[shape]
    return PortableTreeMCTS(net, s["games"], s["sims"], "cuda:0", exploration_weight=1.0, add_dirichlet_noise=True,
                            sample_moves=True, use_graph=True, compact_evals=False, seed=7, **kw)


def search(m, batch):
    import torch
    temps = torch.ones(batch.batch_size, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.search_batch(batch, temperatures=temps)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def step_kernel_us(m, batch):
    """One search with direct launches (a captured graph cannot be bracketed inside), the step kernel between device
    events: (us per launch, launches)."""
    from liuzhou_amd import _lib as L
    lib = L.lib()
    m.use_graph = False
    search(m, batch)                                                # settle: the first direct launch
    L.check(lib.lz_prof_enable(1), "prof_enable")
    try:
        search(m, batch)
        ms, n, u = ctypes.c_double(0.0), ctypes.c_int64(0), ctypes.c_int64(0)
        L.check(lib.lz_prof_aux_summary(0, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(u)), "prof_aux_summary")
    finally:
        lib.lz_prof_enable(0)
        m.use_graph = True
    return (1e3 * ms.value / n.value if n.value else float("nan")), int(n.value)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2,C3")
    ap.add_argument("--runs", type=int, default=3, help="timed runs per variant, the variants alternating")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    args = ap.parse_args()
    import torch
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    names = [v.strip() for v in args.variants.split(",") if v.strip()]
    for shape in [x.strip() for x in args.shapes.split(",") if x.strip()]:
        s = SHAPES[shape]
        model = ChessNet(**MODEL_CONFIGS[s["model"]])
        stable_resnet_init(model, 20260314)
        net = FusedNet(model.eval().to("cuda:0"))
        batch = positions(s["games"])
        engines = {}
        for v in names:                                             # warm up every variant: construction, capture, one replay
            engines[v] = build(net, shape, v)
            search(engines[v], batch)
            search(engines[v], batch)
        rows = {v: [] for v in names}
        for i in range(args.runs):
            for v in names:                                         # alternate: a drift of the machine hits every variant
                split, _kw = VARIANTS[v]
                if split is None:
                    os.environ.pop("LZ_TREE_SPLIT", None)
                else:
                    os.environ["LZ_TREE_SPLIT"] = split
                sec = search(engines[v], batch)
                us, launches = step_kernel_us(engines[v], batch)
                r = {"shape": shape, "variant": v, "run": i, "search_ms": 1e3 * sec, "positions_per_s": s["games"] / sec,
                     "step_kernel_us": us, "step_launches": launches,
                     "two_wave_step": bool(v == "off_split" and s["games"] <= 8192)}
                rows[v].append(r)
                print(json.dumps({"run": r}), flush=True)
        for v in names:
            def agg(field):
                x = [r[field] for r in rows[v]]
                return {"median": statistics.median(x), "min": min(x), "max": max(x)}
            print(json.dumps({"summary": {"shape": shape, "variant": v, "games": s["games"], "sims": s["sims"],
                                          "runs": args.runs, **{f: agg(f) for f in ("search_ms", "positions_per_s",
                                                                                    "step_kernel_us")}}}), flush=True)
        del engines, net
        os.environ.pop("LZ_TREE_SPLIT", None)
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
