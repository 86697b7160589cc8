"""Validation of a checkpoint on rows it was not trained on (csrc/lz_valid.hip, csrc/lz_valid.h).

In a generational loop generation i is unseen data for the weights trained on the generations before it, so evaluating
it before the training pass (test-then-train) is a validation number without holding out a row: no leakage through
duplicate positions, rows of the same game or board symmetries.

`row_metrics(...)`      one kernel: the loss kernel's combined logits / masked log-softmax / two-hot target per row, plus
                        arg-maxima, entropies, the expected value and its calibration bin -> rows f32[B,12], cls i32[B,4]
`MetricSums(device)`    sums of the rows by phase and calibration bin in float64 on the device, one association (bit-equal
                        to the host build and the numpy restatement); `.result()` is its only host read
`validate_network(...)` a model (PyTorch module or the fp16 kernels self-play runs) over a generation, batch by batch

HIP only: there is no CPU path for the row metrics.
"""
from __future__ import annotations

import copy
import ctypes as C
import os
from contextlib import nullcontext
from typing import Any, Callable, Dict, Optional, Tuple

import torch

from . import _lib as L

ROW_COLUMNS = ("kl", "ce", "h_target", "h_net", "top1", "p_top", "bucket_ce", "v_hat", "sq_err", "sign_ok", "decisive",
               "policy_valid")
CLS_COLUMNS = ("phase", "calibration_bin", "net_top_action", "target_top_action")
POLICY_COLUMNS = ROW_COLUMNS[:6]              # averaged over the rows with a policy target
PHASES = 7
CAL_BINS = 10
GROUPS = 1 + PHASES + CAL_BINS
ACC_COLS = len(ROW_COLUMNS) + 2               # + rows counted, rows skipped
EVALUATORS = ("module", "fused")


def row_metrics(lp1: torch.Tensor, lp2: torch.Tensor, lpm: torch.Tensor, vlogits: torch.Tensor, planes: torch.Tensor,
                masks: torch.Tensor, policy: torch.Tensor, value: torch.Tensor, soft: torch.Tensor, *,
                soft_label_alpha: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (rows float32[B,12] in the order of ROW_COLUMNS, cls int32[B,4] in the order of CLS_COLUMNS)."""
    L.require_hip(lp1, "valid_row_metrics")
    dev = lp1.device
    B = int(lp1.shape[0])
    f32 = lambda t, w: t.detach().reshape(B, w).to(device=dev, dtype=torch.float32).contiguous()
    a1, a2, a3, av = f32(lp1, 36), f32(lp2, 36), f32(lpm, 36), f32(vlogits, 101)
    pl, tgt = f32(planes, 396), f32(policy, 220)
    mask = masks.reshape(B, 220).to(dev).contiguous()
    mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)
    val = value.reshape(B).to(device=dev, dtype=torch.float32).contiguous()
    sft = soft.reshape(B).to(device=dev, dtype=torch.float32).contiguous()
    alpha = float(max(0.0, min(1.0, soft_label_alpha)))
    rows = torch.empty((B, len(ROW_COLUMNS)), dtype=torch.float32, device=dev)
    cls = torch.empty((B, len(CLS_COLUMNS)), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().lz_valid_row_metrics(L.ptr(a1), L.ptr(a2), L.ptr(a3), L.ptr(av), L.ptr(mask), L.ptr(tgt), L.ptr(val),
                                             L.ptr(sft), L.ptr(pl), L.i64(B), C.c_float(alpha), L.ptr(rows), L.ptr(cls),
                                             L.stream_ptr(dev)), "valid_row_metrics")
    return rows, cls


def _ratio(num: float, den: float) -> Optional[float]:
    return (num / den) if den > 0 else None


def _group(acc_row, zsum: float) -> Dict[str, Any]:
    """One row of acc -> its averages: policy columns over the rows with a policy target, sign_ok over the decisive rows,
    the rest over the rows counted."""
    s = dict(zip(ROW_COLUMNS, (float(x) for x in acc_row[:len(ROW_COLUMNS)])))
    n, skipped = float(acc_row[-2]), float(acc_row[-1])
    out: Dict[str, Any] = {"rows": int(round(n)), "skipped_non_finite_rows": int(round(skipped)),
                           "policy_rows": int(round(s["policy_valid"])), "decisive_rows": int(round(s["decisive"]))}
    for k in POLICY_COLUMNS:
        out[k] = _ratio(s[k], s["policy_valid"])
    out["sign_ok"] = _ratio(s["sign_ok"], s["decisive"])
    for k in ("bucket_ce", "v_hat", "sq_err"):
        out[k] = _ratio(s[k], n)
    out["mean_z"] = _ratio(zsum, n)
    return out


def summarize(acc, zsum) -> Dict[str, Any]:
    """acc float64[18,14], zsum float64[18] (anything indexable, on the host) -> the result dict of the sums."""
    acc = [[float(x) for x in row] for row in acc]
    zsum = [float(x) for x in zsum]
    out = _group(acc[0], zsum[0])
    out["by_phase"] = {str(k): _group(acc[1 + k], zsum[1 + k]) for k in range(PHASES)}
    cal, ece, n_bins = [], 0.0, 0.0
    for b in range(CAL_BINS):
        g = _group(acc[1 + PHASES + b], zsum[1 + PHASES + b])
        cal.append({"bin": b, "lo": -1.0 + 0.2 * b, "hi": -1.0 + 0.2 * (b + 1), "count": g["rows"], "mean_v_hat": g["v_hat"],
                    "mean_z": g["mean_z"]})
        n_bins += g["rows"]
    for c in cal:
        if c["count"] > 0:
            ece += c["count"] / n_bins * abs(c["mean_v_hat"] - c["mean_z"])
    out["calibration"] = cal
    out["ece"] = ece if n_bins > 0 else None
    return out


class MetricSums:
    """acc float64[18,14] (+ the sum of z per group) on the device: group 0 every row, 1..7 the phases, 8..17 the
    calibration bins.  `add` launches one kernel on the current stream; nothing is read back before `result`."""

    def __init__(self, device) -> None:
        self.device = torch.device(device)
        self._buf = torch.zeros((GROUPS, ACC_COLS + 1), dtype=torch.float64, device=self.device)
        L.require_hip(self._buf, "MetricSums")
        # one allocation, read back in one copy: acc is the first 18 x 14 doubles, zsum the 18 after them
        self._flat = self._buf.view(-1)
        self.acc = self._flat[:GROUPS * ACC_COLS].view(GROUPS, ACC_COLS)
        self.zsum = self._flat[GROUPS * ACC_COLS:]

    def reset(self) -> None:
        self._flat.zero_()

    def add(self, rows: torch.Tensor, cls: torch.Tensor, value: Optional[torch.Tensor] = None) -> None:
        L.require_hip(rows, "valid_reduce")
        B = int(rows.shape[0])
        if rows.dtype != torch.float32 or tuple(rows.shape) != (B, len(ROW_COLUMNS)) or cls.dtype != torch.int32 or \
                tuple(cls.shape) != (B, len(CLS_COLUMNS)) or rows.device != self.device or cls.device != self.device:
            raise ValueError(f"expected rows float32[B,12] and cls int32[B,4] on {self.device}")
        rows, cls = rows.contiguous(), cls.contiguous()
        val = None
        if value is not None:
            val = value.reshape(-1).to(device=self.device, dtype=torch.float32).contiguous()
            if int(val.numel()) != B:
                raise ValueError(f"value must hold {B} entries")
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_valid_reduce(L.ptr(rows), L.ptr(cls), L.ptr(val), L.i64(B), L.ptr(self.acc),
                                            L.ptr(self.zsum) if val is not None else None, L.stream_ptr(self.device)),
                    "valid_reduce")

    def result(self) -> Dict[str, Any]:
        flat = self._flat.tolist()                          # the one host read
        n = GROUPS * ACC_COLS
        return summarize([flat[g * ACC_COLS:(g + 1) * ACC_COLS] for g in range(GROUPS)], flat[n:])


# ---- the rows of a generation, batch by batch ---------------------------------------------------------------------------------
def _finite_rows(planes, policy, value, soft) -> torch.Tensor:
    """The trainer's filter (train_network_from_tensors): rows with a non-finite target or plane are dropped."""
    return torch.isfinite(value) & torch.isfinite(soft) & torch.isfinite(policy).all(dim=1) & \
        torch.isfinite(planes.reshape(planes.size(0), -1)).all(dim=1)


def _source(data, dev: torch.device) -> Tuple[int, Callable[[torch.Tensor], Tuple[torch.Tensor, ...]]]:
    """-> (rows, fetch(index int64 on dev) -> planes, masks, policy, value, soft on dev)."""
    from .trajectory_buffer import TensorSelfPlayBatch
    if isinstance(data, TensorSelfPlayBatch):
        t = [getattr(data, k) for k in ("state_tensors", "legal_masks", "policy_targets", "value_targets", "soft_value_targets")]
        five = (t[0].to(dev).to(torch.float32), t[1].to(dev), t[2].to(dev).to(torch.float32),
                t[3].to(dev).to(torch.float32).view(-1), t[4].to(dev).to(torch.float32).view(-1))
        return int(data.num_samples), lambda idx: tuple(x.index_select(0, idx) for x in five)
    if isinstance(data, torch.Tensor):
        from .trajectory_codec import RECORD_BYTES, unpack_records
        if data.dtype != torch.uint8 or data.dim() != 2 or int(data.shape[1]) != RECORD_BYTES:
            raise ValueError(f"expected uint8[n, {RECORD_BYTES}] records, got {data.dtype} {tuple(data.shape)}")
        rec = data.to(dev)

        def fetch(idx):
            b = unpack_records(rec.index_select(0, idx))
            return b.state_tensors, b.legal_masks, b.policy_targets, b.value_targets, b.soft_value_targets
        return int(rec.shape[0]), fetch
    if isinstance(data, (tuple, list)) and len(data) == 2 and hasattr(data[0], "gather") and hasattr(data[0], "slots_of"):
        window, gens = data
        gens = [int(gens)] if isinstance(gens, int) else [int(g) for g in gens]
        if not gens:
            raise ValueError("no generation to validate")
        if torch.device(window.device) != dev:
            raise ValueError(f"the window lives on {window.device}, validation runs on {dev}")
        slots = torch.cat([window.slots_of(g) for g in gens])           # ids only: the rows are decoded batch by batch
        return int(slots.numel()), lambda idx: window.gather(slots.index_select(0, idx))
    raise TypeError("data must be a TensorSelfPlayBatch, a uint8[n, 360] record tensor or (ReplayWindow, generation ids)")


def _forward_fn(model, evaluator: str, use_amp: bool, dev: torch.device):
    if evaluator == "fused":
        from .net_hip import FusedNet, fused_unsupported_reason
        if isinstance(model, FusedNet):
            return model, None
        why = fused_unsupported_reason(model)
        if why is not None:
            raise RuntimeError(f"fused network kernel does not cover this model: {why}")
        return FusedNet(model, dev), None                   # packs a copy of the weights; the module is only read
    module = model
    p = next(module.parameters(), None)
    if p is not None and p.device != dev:
        module = copy.deepcopy(model).to(dev)               # the caller's module stays where and as it is
    flags = [(m, bool(m.training)) for m in module.modules()]      # per module: a caller may keep some of them in eval()
    module.eval()
    amp = (lambda: torch.amp.autocast("cuda", enabled=True)) if use_amp else nullcontext

    def run(planes):
        with torch.no_grad(), amp():
            return module(planes)
    return run, flags


def validate_network(model, data, *, batch_size: int = 4096, evaluator: str = "module", use_amp: bool = True,
                     soft_label_alpha: float = 0.0, device: str = "cuda:0", max_rows: int = 0, seed: int = 0) -> Dict[str, Any]:
    """Metrics of `model` on the rows of `data` (a TensorSelfPlayBatch, uint8[n,360] records, or (ReplayWindow, generation
    ids), decoded batch by batch).  evaluator "module": the PyTorch module in eval() under no_grad, autocast as `use_amp`;
    "fused": the fp16 kernels of FusedNet, the arithmetic self-play sees.  `max_rows` > 0: a seeded subset without
    replacement, drawn on a generator of its own.  The model's parameters and buffers, the `training` flag of every
    submodule and the default generators are left as they were.  Host reads: one per batch for the non-finite filter
    (the count of rows kept) and the one of `MetricSums.result()` at the end; the sums themselves stay on the device."""
    if evaluator not in EVALUATORS:
        raise ValueError(f"evaluator must be one of {EVALUATORS}, got {evaluator!r}")
    if type(batch_size) is not int or batch_size < 1:
        raise ValueError(f"batch_size must be a positive integer, got {batch_size!r}")
    if type(max_rows) is not int or max_rows < 0:
        raise ValueError(f"max_rows must be a non-negative integer, got {max_rows!r}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"liuzhou_amd.validate_network: needs a HIP device (got {dev}); this build has no CPU path.")
    forward, restore = _forward_fn(model, evaluator, bool(use_amp), dev)
    try:
        n, fetch = _source(data, dev)
        if max_rows and max_rows < n:
            gen = torch.Generator(device="cpu")
            gen.manual_seed(int(seed))
            order = torch.randperm(n, generator=gen)[:max_rows].sort().values.to(dev)
        else:
            order = torch.arange(n, dtype=torch.int64, device=dev)
        sums = MetricSums(dev)
        filtered = 0
        # like the trainer (LZ_TRAIN_MIOPEN): only the nominal batch size is worth a MIOpen kernel search
        mode = os.environ.get("LZ_TRAIN_MIOPEN", "auto").strip().lower()
        can_imm = hasattr(torch.backends, "miopen") and evaluator == "module" and mode != "find"
        for start in range(0, int(order.numel()), batch_size):
            planes, masks, policy, value, soft = fetch(order[start:start + batch_size])
            finite = _finite_rows(planes, policy, value, soft)
            keep = torch.nonzero(finite).view(-1)           # the filter's host read, one per batch (as the trainer's has one)
            filtered += int(finite.numel()) - int(keep.numel())
            if int(keep.numel()) == 0:
                continue
            if int(keep.numel()) != int(finite.numel()):
                planes, masks, policy, value, soft = (t.index_select(0, keep) for t in (planes, masks, policy, value, soft))
            planes = planes.contiguous()
            imm = can_imm and (mode == "immediate" or int(planes.shape[0]) != batch_size)
            with (torch.backends.miopen.flags(immediate=True) if imm else nullcontext()):
                lp1, lp2, lpm, vlogits = forward(planes)[:4]
            rows, cls = row_metrics(lp1, lp2, lpm, vlogits, planes, masks, policy, value, soft,
                                    soft_label_alpha=soft_label_alpha)
            sums.add(rows, cls, value)
        out = sums.result()
        out["filtered_non_finite_rows"] = filtered
        out["evaluator"] = evaluator
        return out
    finally:
        for m, was_training in (restore or ()):
            m.training = was_training
