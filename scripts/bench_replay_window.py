"""Replay-window measurements: whole training steps through `train_network_from_window` against
`train_network_from_tensors` on the same rows (b10c128, batch 512, AMP, symmetry augmentation on both sides, alternated
epochs as in scripts/bench_train.py), the batch kernel on its own, and what the allocator holds for a window against the
five tensors.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
from liuzhou_amd.replay_window import ReplayWindow
from liuzhou_amd.symmetry import transform_samples
from liuzhou_amd.train_bridge import train_network_from_tensors, train_network_from_window
from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch

dev = torch.device("cuda:0")
N, BATCH, REPS = 16384, 512, 6
g = torch.Generator(device=dev).manual_seed(1)


def rows():
    mask = torch.rand((N, 220), device=dev, generator=g) < 0.12
    mask[:, 0] = True
    target = torch.rand((N, 220), device=dev, generator=g) * mask
    target = target / target.sum(1, keepdim=True)
    planes = torch.zeros((N, 11, 6, 6), device=dev)
    planes[:, :4] = (torch.rand((N, 4, 6, 6), device=dev, generator=g) < 0.2).float()
    phase = torch.randint(0, 8, (N,), device=dev, generator=g)
    planes[:, 4:] = (phase.view(N, 1) == torch.arange(1, 8, device=dev).view(1, 7)).float().view(N, 7, 1, 1)
    value = torch.randint(-1, 2, (N,), device=dev, generator=g).float()
    soft = torch.rand(N, device=dev, generator=g) * 2 - 1
    return TensorSelfPlayBatch(planes, mask, target, value, soft)


def timed_us(fn, reps=200):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


torch.cuda.synchronize()
base = torch.cuda.memory_allocated(dev)
batch = rows()
torch.cuda.synchronize()
tensors_bytes = torch.cuda.memory_allocated(dev) - base
window = ReplayWindow(dev, max_generations=1, capacity_rows=N)
torch.cuda.synchronize()
window_bytes = torch.cuda.memory_allocated(dev) - base - tensors_bytes
window.add_generation(batch)

torch.manual_seed(0)
model = ChessNet(**MODEL_CONFIGS["b10c128"])
stable_resnet_init(model, 20260314)
model.to(dev)
kw = dict(batch_size=BATCH, epochs=1, device="cuda:0", symmetry_augment=True)
train_network_from_tensors(model, batch, **kw)                      # MIOpen warm-up
train_network_from_window(model, window, **kw)
times = {"tensors": [], "window": []}
for rep in range(REPS):
    for side in (("tensors", "window") if rep % 2 == 0 else ("window", "tensors")):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if side == "tensors":
            _, m = train_network_from_tensors(model, batch, **kw)
        else:
            _, m = train_network_from_window(model, window, **kw)
        torch.cuda.synchronize()
        times[side].append((time.perf_counter() - t0) / m["total_train_steps"] * 1e3)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}

idx = torch.randperm(N, device=dev)[:BATCH]
sym = torch.randint(0, 8, (BATCH,), device=dev).to(torch.int8)
masks_u8 = batch.legal_masks.view(torch.uint8)


def from_tensors():
    transform_samples(batch.state_tensors, masks_u8, batch.policy_targets, sym, idx)
    batch.value_targets.index_select(0, idx), batch.soft_value_targets.index_select(0, idx)


print(json.dumps({
    "rows": N, "batch": BATCH, "model": "b10c128", "amp": True, "symmetry_augment": True,
    "step_ms_tensors": round(med["tensors"], 4), "step_ms_window": round(med["window"], 4),
    "window_vs_tensors_pct": round((med["window"] / med["tensors"] - 1) * 100, 2),
    "step_ms_tensors_all": [round(t, 4) for t in times["tensors"]], "step_ms_window_all": [round(t, 4) for t in times["window"]],
    "steps_per_epoch": N // BATCH, "alternated_epochs": REPS,
    "batch_us_window_gather": round(timed_us(lambda: window.gather(idx, sym)), 2),
    "batch_us_tensors_gather": round(timed_us(from_tensors), 2),
    "allocated_bytes_five_tensors": int(tensors_bytes), "allocated_bytes_window": int(window_bytes),
    "bytes_per_row_five_tensors": round(tensors_bytes / N, 1), "bytes_per_row_window": round(window_bytes / N, 1),
    "device": torch.cuda.get_device_name(0)}), flush=True)
