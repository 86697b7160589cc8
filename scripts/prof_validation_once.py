"""300 batches of the two validation kernels at one batch size, for a kernel trace of its own
(`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/prof_validation_once.py 4096`):
kernel durations without the Python call around them (profiles/r20_validation.md)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from liuzhou_amd.validation import MetricSums, row_metrics

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
mask = torch.rand((B, 220), device=dev, generator=g) < 0.12
mask[:, 0] = True
target = torch.rand((B, 220), device=dev, generator=g) * mask
target = target / target.sum(1, keepdim=True)
planes = torch.zeros((B, 11, 6, 6), device=dev)
planes[:, :4] = (torch.rand((B, 4, 6, 6), device=dev, generator=g) < 0.2).float()
phase = torch.randint(0, 8, (B,), device=dev, generator=g)
planes[:, 4:] = (phase.view(B, 1) == torch.arange(1, 8, device=dev).view(1, 7)).float().view(B, 7, 1, 1)
value = torch.randint(-1, 2, (B,), device=dev, generator=g).float()
soft = torch.rand(B, device=dev, generator=g) * 2 - 1
heads = [torch.log_softmax(torch.randn((B, 36), device=dev, generator=g), dim=1) for _ in range(3)]
vlogits = 2 * torch.randn((B, 101), device=dev, generator=g)
sums = MetricSums(dev)
for _ in range(300):
    rows, cls = row_metrics(*heads, vlogits, planes, mask, target, value, soft, soft_label_alpha=0.3)
    sums.add(rows, cls, value)
torch.cuda.synchronize()
print(B, sums.result()["rows"])
