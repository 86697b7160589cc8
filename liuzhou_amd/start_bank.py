"""The start bank: a device-resident ring of packed positions that self-play games fork from (search_rules:
`start_fork_prob` / `start_capture_prob`).

`entries` uint8[capacity, 32] holds `lz::Packed` records (csrc/lz_rules.h: four little-endian 64-bit words, lossless for
every reachable state), `cursor` int64[1] the number of positions ever appended: row (total + r) % capacity takes the
r-th new position, `filled = min(total, capacity)`, and the filled entries are the physical rows [0, filled).  The per-ply
device tail fills it (`lz_start_bank_capture`) and reads it (`lz_start_bank_seed`); a bank belongs to its caller and
survives calls of `self_play_tree_gpu`, so positions of one chunk or iteration start games of the next."""
from __future__ import annotations

from typing import Dict

import torch

from .search_rules import START_MAX_CAPACITY

RECORD_BYTES = 32


class StartBank:
    def __init__(self, capacity: int, device) -> None:
        if isinstance(capacity, bool) or int(capacity) != capacity or not 1 <= int(capacity) <= START_MAX_CAPACITY:
            raise ValueError(f"StartBank: capacity must be an integer in [1, 2**24], got {capacity!r}")
        self.capacity, self.device = int(capacity), torch.device(device)
        self.entries = torch.zeros((self.capacity, RECORD_BYTES), dtype=torch.uint8, device=self.device)
        self.cursor = torch.zeros((1,), dtype=torch.int64, device=self.device)

    def total(self) -> int:
        """Positions ever appended (one device read)."""
        return int(self.cursor.item())

    def filled(self) -> int:
        return min(self.total(), self.capacity)

    def append_packed(self, packed: torch.Tensor) -> None:
        """Host-side append of uint8[n, 32] records with the ring rule of the capture kernel: record r goes to row
        (total + r) % capacity, and of more records than rows only the last `capacity` are written."""
        if packed.dtype != torch.uint8 or packed.dim() != 2 or int(packed.shape[1]) != RECORD_BYTES:
            raise ValueError("StartBank.append_packed: records must be uint8[n, 32]")
        n = int(packed.shape[0])
        if n == 0:
            return
        total = self.total()
        first = max(0, n - self.capacity)
        rows = (torch.arange(first, n, dtype=torch.int64) + total) % self.capacity
        self.entries.index_copy_(0, rows.to(self.device), packed[first:].to(self.device).contiguous())
        self.cursor.fill_(total + n)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"entries": self.entries.detach().cpu().clone(), "cursor": self.cursor.detach().cpu().clone()}

    def load_state_dict(self, state: Dict[str, torch.Tensor]) -> None:
        entries, cursor = state["entries"], state["cursor"]
        if entries.dtype != torch.uint8 or tuple(entries.shape) != (self.capacity, RECORD_BYTES):
            raise ValueError(f"StartBank.load_state_dict: entries must be uint8[{self.capacity}, 32], got "
                             f"{entries.dtype}{list(entries.shape)}")
        if cursor.dtype != torch.int64 or int(cursor.numel()) != 1 or int(cursor.view(-1)[0].item()) < 0:
            raise ValueError("StartBank.load_state_dict: cursor must be one non-negative int64")
        self.entries.copy_(entries.to(self.device))
        self.cursor.copy_(cursor.view(1).to(self.device))
