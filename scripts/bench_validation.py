"""Validation measurements: the two kernels of csrc/lz_valid.hip per batch of 512 and 4 096 rows
against a plain PyTorch composition of the same twelve quantities and their grouped sums (alternated rounds in one
process, median and minimum), and `validate_network` in rows/s for both evaluators on b6c64 and b10c128 beside one
training pass over the same rows.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
from liuzhou_amd.train_bridge import train_network_from_tensors
from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
from liuzhou_amd.validation import MetricSums, row_metrics, validate_network

dev = torch.device("cuda:0")
N, ROUNDS, REPS = 16384, 7, 50
ALPHA = 0.3
g = torch.Generator(device=dev).manual_seed(1)


def make_rows(n):
    mask = torch.rand((n, 220), device=dev, generator=g) < 0.12
    mask[:, 0] = True
    target = torch.rand((n, 220), device=dev, generator=g) * mask
    target = target / target.sum(1, keepdim=True)
    planes = torch.zeros((n, 11, 6, 6), device=dev)
    planes[:, :4] = (torch.rand((n, 4, 6, 6), device=dev, generator=g) < 0.2).float()
    phase = torch.randint(0, 8, (n,), device=dev, generator=g)
    planes[:, 4:] = (phase.view(n, 1) == torch.arange(1, 8, device=dev).view(1, 7)).float().view(n, 7, 1, 1)
    value = torch.randint(-1, 2, (n,), device=dev, generator=g).float()
    soft = torch.rand(n, device=dev, generator=g) * 2 - 1
    return TensorSelfPlayBatch(planes, mask, target, value, soft)


_from = torch.arange(36, device=dev).repeat_interleave(4)
_r, _c = _from // 6, _from % 6
_d = torch.arange(4, device=dev).repeat(36)
_nr = _r + torch.tensor([-1, 1, 0, 0], device=dev)[_d]
_nc = _c + torch.tensor([0, 0, -1, 1], device=dev)[_d]
_on = (_nr >= 0) & (_nr < 6) & (_nc >= 0) & (_nc < 6)
_dest = torch.where(_on, _nr * 6 + _nc, torch.zeros_like(_nr))
_centres = torch.linspace(-1.0, 1.0, 101, device=dev)


def torch_rows(lp1, lp2, lpm, vl, planes, mask, target, value, soft):
    """The twelve columns and the two group ids as a PyTorch composition (the conventions of the kernel)."""
    B = lp1.shape[0]
    moves = torch.where(_on, lp2[:, _from] + lp1[:, _dest], torch.full((), float("-inf"), device=dev))
    comb = torch.cat([lp1, moves, lpm, torch.zeros((B, 4), device=dev)], dim=1)
    c = torch.where(mask, comb, torch.full_like(comb, float("-inf")))
    lse = torch.logsumexp(c, dim=1, keepdim=True)
    ok = mask.any(dim=1, keepdim=True) & torch.isfinite(lse)
    lse = torch.where(ok, lse, torch.zeros_like(lse))
    lp = torch.where(mask, c - lse, torch.zeros_like(c))
    lp = torch.where(torch.isfinite(lp), lp, torch.full_like(lp, -50.0)).clamp(min=-50.0)
    ce = -(target * lp).sum(1)
    ent = -(target * target.clamp(min=1e-8).log()).sum(1)
    p = torch.where(ok & mask & (c > float("-inf")), (c - lse).exp(), torch.zeros_like(c))
    h_net = -(torch.where(p > 0, p * (c - lse), torch.zeros_like(p))).sum(1)
    net_top = c.argmax(1)
    tgt_top = torch.where(mask, target, torch.full_like(target, float("-inf"))).argmax(1)
    valid = (target.sum(1) > 1e-8) & mask.any(1)
    p_top = p.gather(1, tgt_top.view(-1, 1)).view(-1)
    mixed = ((1 - ALPHA) * value + ALPHA * soft).clamp(-1, 1)
    u = (mixed + 1) / 0.02
    lo = u.floor().long().clamp(0, 100)
    hi = (lo + 1).clamp(0, 100)
    frac = torch.where(hi == lo, torch.zeros_like(u), (u - lo.float()).clamp(0, 1))
    vlog = torch.log_softmax(vl, dim=1)
    bce = -((1 - frac) * vlog.gather(1, lo.view(-1, 1)).view(-1) + frac * vlog.gather(1, hi.view(-1, 1)).view(-1))
    v_hat = (vlog.exp() * _centres).sum(1)
    draw = value.abs() < 1e-8
    z = torch.zeros_like(ce)
    rows = torch.stack([torch.where(valid, ce - ent, z), torch.where(valid, ce, z), torch.where(valid, ent, z),
                        torch.where(valid, h_net, z), (valid & (net_top == tgt_top)).float(), torch.where(valid, p_top, z), bce,
                        v_hat, (v_hat - value) ** 2, (~draw & (v_hat * value > 0)).float(), (~draw).float(), valid.float()], dim=1)
    cell0 = planes[:, 4:, 0, 0] != 0
    phase = torch.where(cell0.any(1), cell0.float().argmax(1), torch.full((B,), -1, device=dev))
    bins = ((v_hat + 1) * 5).floor().clamp(0, 9).long()
    return rows, phase, bins


def torch_sums(rows, phase, bins, value):
    fin = torch.isfinite(rows).all(1)
    r = torch.cat([rows.double(), torch.ones_like(value).double().view(-1, 1), value.double().view(-1, 1)], dim=1) * fin.view(-1, 1)
    acc = torch.zeros((18, 14), dtype=torch.float64, device=dev)
    acc[0] = r.sum(0)
    acc.index_add_(0, (phase + 1).clamp(min=0), r * (phase >= 0).view(-1, 1))
    acc.index_add_(0, bins + 8, r)
    return acc


def timed_us(fn):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / REPS * 1e3


def stats(v):
    v = sorted(v)
    return {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2)}


def bench_kernels(B):
    b = make_rows(B)
    lp = [torch.log_softmax(torch.randn((B, 36), device=dev, generator=g), dim=1) for _ in range(3)]
    vl = 2 * torch.randn((B, 101), device=dev, generator=g)
    args = (*lp, vl, b.state_tensors, b.legal_masks, b.policy_targets, b.value_targets, b.soft_value_targets)
    sums = MetricSums(dev)
    rows, cls = row_metrics(*args, soft_label_alpha=ALPHA)
    arms = {"hip_row_metrics": lambda: row_metrics(*args, soft_label_alpha=ALPHA),
            "hip_reduce": lambda: sums.add(rows, cls, b.value_targets),
            "hip_both": lambda: sums.add(*row_metrics(*args, soft_label_alpha=ALPHA), b.value_targets),
            "torch_rows": lambda: torch_rows(*args),
            "torch_both": lambda: torch_sums(*torch_rows(*args), b.value_targets)}
    for fn in arms.values():                                         # warm-up
        for _ in range(3):
            fn()
    times = {k: [] for k in arms}
    names = list(arms)
    for r in range(ROUNDS):                                          # alternated rounds, one process
        for k in (names if r % 2 == 0 else names[::-1]):
            times[k].append(timed_us(arms[k]))
    out = {k: stats(v) for k, v in times.items()}
    t_rows, _, _ = torch_rows(*args)
    out["max_abs_diff_hip_vs_torch_rows"] = float((rows - t_rows).abs().max())
    return out


def bench_networks(name):
    data = make_rows(N)
    model = ChessNet(**MODEL_CONFIGS[name])
    stable_resnet_init(model, 20260314)
    model.to(dev).eval()
    out = {}
    kw = dict(batch_size=4096, soft_label_alpha=ALPHA, device="cuda:0")
    for ev in ("module", "fused"):
        validate_network(model, data, evaluator=ev, **kw)            # warm-up: MIOpen kernel search, weight packing
    tkw = dict(batch_size=4096, epochs=1, soft_label_alpha=ALPHA, device="cuda:0")
    train_network_from_tensors(model, data, **tkw)
    model.eval()
    times = {"module": [], "fused": [], "train": []}
    for r in range(5):
        for k in (("module", "fused", "train") if r % 2 == 0 else ("train", "fused", "module")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if k == "train":
                train_network_from_tensors(model, data, **tkw)
                model.eval()
            else:
                validate_network(model, data, evaluator=k, **kw)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    for k, v in times.items():
        v = sorted(v)
        out[k] = {"rows_per_sec_median": round(N / v[len(v) // 2], 1), "rows_per_sec_best": round(N / v[0], 1)}
    return out


print(json.dumps({"rows": N, "alpha": ALPHA, "reps_per_round": REPS, "rounds": ROUNDS,
                  "kernels_batch_512": bench_kernels(512), "kernels_batch_4096": bench_kernels(4096),
                  "b6c64": bench_networks("b6c64"), "b10c128": bench_networks("b10c128"),
                  "device": torch.cuda.get_device_name(0)}), flush=True)
