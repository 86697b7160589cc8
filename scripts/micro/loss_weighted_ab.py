"""Kernel time of the fused loss with and without row weights (profiles/r21_row_weights.md).

  run:        rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/micro/loss_weighted_ab.py run [--lib SO]
  summarise:  python scripts/micro/loss_weighted_ab.py summarise OUT [OUT ...]

`run` launches lz_policy_value_loss_fwd_bwd and, where the library has it, lz_policy_value_loss_weighted_fwd_bwd
alternately, --launches times each, at 512 and 4 096 rows of seeded inputs (after --warmup launches of each).  `--lib`
names another build of the HIP library, e.g. one of the parent commit, loaded on its own: it need not have the weighted
entry.  `summarise` reads the kernel traces and prints, per kernel name and row count, the median, the quartiles and the
extremes of the kernel durations in microseconds as one JSON line per trace directory.  The row count is read off the
grid: one 256-thread workgroup per four rows.  Needs a GPU; there is no fallback."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

ROWS = (512, 4096)


def run(args) -> int:
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("loss_weighted_ab.py needs a GPU")
    from liuzhou_amd import _lib as L
    lib = C.CDLL(args.lib or L.LIB)
    entries = []
    for name in ("lz_policy_value_loss_fwd_bwd", "lz_policy_value_loss_weighted_fwd_bwd"):
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = L.DECLS[name]
            entries.append((name, fn))
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(21)
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
        wsum = torch.full((1,), float(B), device=dev)
        terms = torch.empty((B, 4), device=dev)
        grads = [torch.empty((B, 36), device=dev) for _ in range(3)] + [torch.empty((B, 101), device=dev)]
        front = [L.ptr(t) for t in (*heads, vl, mask, target, value, soft)]
        tail = [L.i64(B), C.c_float(0.3), C.c_float(0.0), C.c_float(1.0), L.ptr(wsum), C.c_float(1.0), L.ptr(terms),
                *(L.ptr(t) for t in grads), L.stream_ptr(dev)]
        calls = [(fn, front + ([L.ptr(rw)] if "weighted" in name else []) + tail) for name, fn in entries]
        for i in range(args.warmup + args.launches):
            for fn, a in calls:
                if fn(*a) != 0:
                    raise RuntimeError("launch refused")
            if i % 50 == 49:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
    print(json.dumps({"lib": args.lib or L.LIB, "entries": [n for n, _ in entries], "rows": ROWS, "launches": args.launches,
                      "warmup": args.warmup}), flush=True)
    return 0


def summarise(args) -> int:
    for d in args.dirs:
        durations = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row["Kernel_Name"]
                    if "policy_value_loss_kernel" not in name:
                        continue
                    kind = "weighted" if "<true>" in name or "ILb1E" in name else "unweighted"
                    rows = int(row["Grid_Size_X"] if "Grid_Size_X" in row else row["Grid_Size"]) // 256 * 4
                    durations.setdefault((kind, rows), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        out = {"trace": d}
        for (kind, rows), us in sorted(durations.items()):
            us = us[args.skip:]                                    # the warm-up launches come first in the trace
            q = statistics.quantiles(us, n=4)
            out[f"{kind}_{rows}"] = {"launches": len(us), "median_us": round(statistics.median(us), 3), "q1_us": round(q[0], 3),
                                     "q3_us": round(q[2], 3), "min_us": round(min(us), 3), "max_us": round(max(us), 3)}
        print(json.dumps(out), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--lib", default=None)
    r.add_argument("--launches", type=int, default=300)
    r.add_argument("--warmup", type=int, default=20)
    s = sub.add_parser("summarise")
    s.add_argument("dirs", nargs="+")
    s.add_argument("--skip", type=int, default=20, help="leading launches per kernel and row count to leave out (the warm-up)")
    args = ap.parse_args()
    return run(args) if args.cmd == "run" else summarise(args)


if __name__ == "__main__":
    sys.exit(main())
