"""Kernel times of the distributional value target (profiles/r23_value_dist.md).

  loss:       rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/micro/value_dist_ab.py loss [--lib SO]
  merge:      rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/micro/value_dist_ab.py merge
  summarise:  python scripts/micro/value_dist_ab.py summarise OUT [OUT ...]

`loss` launches, alternately and in this order, lz_policy_value_loss_weighted_fwd_bwd (`<true,false>`) and, where the
library has it, lz_policy_value_loss_dist_fwd_bwd with row weights (`<true,true>`) twice: with no row pointing into the
table (dist_row all -1) and with every row pointing into it (a table of rows / 4 rows); --launches times each after
--warmup, at 512 and 4 096 rows of seeded inputs.  `--lib` names another build of the HIP library, e.g. one of the
parent commit, loaded on its own: it need not have the new entry.  `merge` launches lz_replay_merge_records and
lz_merge_value_distributions on the selection of scripts/bench_replay_merge.py (524 288 rows, symmetric groups), ring
addressing, every merged group a table row; then lz_merge_value_distributions alone on one group of 16 384 identical
members (tensor addressing).  `summarise` reads the kernel traces and prints the median, the quartiles and the extremes of
the kernel durations in microseconds, one JSON line per trace directory; the two uses of `<true,true>` are told apart by
their order in the trace (0 % first).  Needs a GPU; there is no fallback."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

ROWS = (512, 4096)
DEV = "cuda:0"


def run_loss(args) -> int:
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("value_dist_ab.py needs a GPU")
    from liuzhou_amd import _lib as L
    lib = C.CDLL(args.lib or L.LIB)
    weighted = lib.lz_policy_value_loss_weighted_fwd_bwd
    weighted.restype, weighted.argtypes = L.DECLS["lz_policy_value_loss_weighted_fwd_bwd"]
    dist = getattr(lib, "lz_policy_value_loss_dist_fwd_bwd", None)
    if dist is not None:
        dist.restype, dist.argtypes = L.DECLS["lz_policy_value_loss_dist_fwd_bwd"]
    dev = torch.device(DEV)
    g = torch.Generator(device=dev).manual_seed(23)
    for B in ROWS:
        heads = [torch.log_softmax(torch.randn((B, 36), generator=g, device=dev), dim=1) for _ in range(3)]
        vl = torch.randn((B, 101), generator=g, device=dev) * 2
        mask = (torch.rand((B, 220), generator=g, device=dev) < 0.2).to(torch.uint8)
        mask[:, 216] = 1
        target = torch.rand((B, 220), generator=g, device=dev) * mask
        target = target / target.sum(dim=1, keepdim=True)
        value = torch.randint(-1, 2, (B,), generator=g, device=dev).float()
        soft = torch.rand((B,), generator=g, device=dev) * 2 - 1
        rw = torch.rand((B,), generator=g, device=dev) * 2
        D = B // 4
        table = torch.softmax(torch.randn((D, 101), generator=g, device=dev), dim=1)
        none = torch.full((B,), -1, dtype=torch.int32, device=dev)
        every = torch.randint(0, D, (B,), generator=g, device=dev).to(torch.int32)
        wsum = torch.full((1,), float(B), device=dev)
        terms = torch.empty((B, 4), device=dev)
        grads = [torch.empty((B, 36), device=dev) for _ in range(3)] + [torch.empty((B, 101), device=dev)]
        base = [L.ptr(t) for t in (*heads, vl, mask, target, value, soft, rw)] + \
               [L.i64(B), C.c_float(0.3), C.c_float(0.0), C.c_float(1.0), L.ptr(wsum), C.c_float(1.0), L.ptr(terms),
                *(L.ptr(t) for t in grads), L.stream_ptr(dev)]
        calls = [(weighted, base)]
        if dist is not None:
            calls += [(dist, base + [L.ptr(none), L.ptr(table), L.i64(D)]), (dist, base + [L.ptr(every), L.ptr(table), L.i64(D)])]
        for i in range(args.warmup + args.launches):
            for fn, a in calls:
                if fn(*a) != 0:
                    raise RuntimeError("launch refused")
            if i % 50 == 49:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
    print(json.dumps({"mode": "loss", "lib": args.lib or L.LIB, "dist_entry": dist is not None, "rows": ROWS,
                      "launches": args.launches, "warmup": args.warmup}), flush=True)
    return 0


def run_merge(args) -> int:
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("value_dist_ab.py needs a GPU")
    from bench_replay_merge import synthetic_ring
    from liuzhou_amd import _lib as L
    from liuzhou_amd import position_dedup as D
    from liuzhou_amd import replay_window as RW
    n = args.rows
    ring = synthetic_ring(n, args.seed)
    slots = torch.randperm(n, device=DEV)
    keys, sym, bad = RW.record_position_keys(ring, slots, symmetric=True)
    _, order, begin, count = D.group_rows(keys)
    groups = int(count.numel())
    rows = D.table_rows(count)
    tables = int((count > 1).sum())
    merged = torch.empty((groups, 360), dtype=torch.uint8, device=DEV)
    cnt = torch.empty((groups,), dtype=torch.int32, device=DEV)
    dist = torch.empty((tables, 101), dtype=torch.float32, device=DEV)
    flat = ring.view(-1)
    stream = L.stream_ptr(torch.device(DEV))
    for _ in range(args.warmup + args.launches):
        L.check(L.lib().lz_replay_merge_records(L.ptr(ring), L.i64(n), L.ptr(slots), L.i64(n), L.ptr(sym), L.ptr(order),
                                                L.ptr(begin), L.i64(groups), L.ptr(merged), L.ptr(cnt), L.ptr(bad), stream), "merge")
        L.check(L.lib().lz_merge_value_distributions(L.ptr(flat[348:]), L.ptr(flat[352:]), L.i64(360), L.i64(n), L.ptr(slots),
                                                     L.i64(n), L.ptr(order), L.ptr(begin), L.i64(groups), L.ptr(rows),
                                                     C.c_float(0.3), L.ptr(dist), L.i64(tables), stream), "value distributions")
    torch.cuda.synchronize()
    # one group of `--opening` identical members: the sequential limit of one wave
    c = args.opening
    value, soft = torch.full((c,), 1.0, device=DEV), torch.full((c,), 0.25, device=DEV)
    one_order = torch.arange(c, dtype=torch.int64, device=DEV)
    one_begin = torch.tensor([0, c], dtype=torch.int64, device=DEV)
    one_row = torch.zeros((1,), dtype=torch.int32, device=DEV)
    one = torch.empty((1, 101), dtype=torch.float32, device=DEV)
    for _ in range(args.warmup + args.launches):
        L.check(L.lib().lz_merge_value_distributions(L.ptr(value), L.ptr(soft), L.i64(4), L.i64(c), None, L.i64(c),
                                                     L.ptr(one_order), L.ptr(one_begin), L.i64(1), L.ptr(one_row), C.c_float(0.3),
                                                     L.ptr(one), L.i64(1), stream), "value distributions")
    torch.cuda.synchronize()
    print(json.dumps({"mode": "merge", "rows": n, "groups": groups, "table_rows": tables, "largest_group": int(count.max()),
                      "opening": c, "launches": args.launches, "warmup": args.warmup}), flush=True)
    return 0


def _stats(us):
    q = statistics.quantiles(us, n=4) if len(us) >= 2 else [us[0]] * 3
    return {"launches": len(us), "median_us": round(statistics.median(us), 3), "q1_us": round(q[0], 3), "q3_us": round(q[2], 3),
            "min_us": round(min(us), 3), "max_us": round(max(us), 3)}


def summarise(args) -> int:
    for d in args.dirs:
        seen = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row["Kernel_Name"]
                    grid = int(row["Grid_Size_X"] if "Grid_Size_X" in row else row["Grid_Size"]) // 256
                    start, end = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                    if "policy_value_loss_kernel" in name:
                        kind = "dist" if ("true, true" in name or "ILb1ELb1E" in name) else "weighted"
                        seen.setdefault((kind, grid * 4), []).append((start, (end - start) / 1e3))
                    elif "merge_value_distributions_kernel" in name:
                        seen.setdefault(("value_distributions", grid), []).append((start, (end - start) / 1e3))
                    elif "replay_merge_records_kernel" in name:
                        seen.setdefault(("replay_merge_records", grid), []).append((start, (end - start) / 1e3))
        out = {"trace": d}
        for (kind, size), rows in sorted(seen.items()):
            us = [u for _, u in sorted(rows)]
            if kind == "dist":                                       # 0 % and 100 % of the rows in the table, alternately
                for tag, part in (("dist_0pct", us[0::2]), ("dist_100pct", us[1::2])):
                    out[f"{tag}_{size}"] = _stats(part[args.skip:])
            else:
                out[f"{kind}_{size}" + ("_blocks" if kind != "weighted" else "")] = _stats(us[args.skip:])
        print(json.dumps(out), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("loss")
    r.add_argument("--lib", default=None)
    r.add_argument("--launches", type=int, default=300)
    r.add_argument("--warmup", type=int, default=20)
    m = sub.add_parser("merge")
    m.add_argument("--rows", type=int, default=524288)
    m.add_argument("--opening", type=int, default=16384)
    m.add_argument("--launches", type=int, default=20)
    m.add_argument("--warmup", type=int, default=3)
    m.add_argument("--seed", type=int, default=20261021)
    s = sub.add_parser("summarise")
    s.add_argument("dirs", nargs="+")
    s.add_argument("--skip", type=int, default=20, help="leading launches per kernel and size to leave out (the warm-up)")
    args = ap.parse_args()
    return {"loss": run_loss, "merge": run_merge, "summarise": summarise}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
