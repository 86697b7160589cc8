"""The 8 symmetries of the 6x6 board (the dihedral group D4) on training rows, state batches and packed records.

No rule of Liuzhou chess names a particular cell, so every element sigma maps a game onto an equivalent one.  Element
ids (cells are r*6+c):

    0 identity (r, c)          1 rotate 90 (c, 5-r)       2 rotate 180 (5-r, 5-c)    3 rotate 270 (5-c, r)
    4 flip left-right (r, 5-c) 5 flip up-down (5-r, c)    6 transpose (c, r)         7 anti-transpose (5-c, 5-r)

A transformed row holds at cell sigma(x) what the source held at x, and at action P_sigma(a) what it held at a:
placement a -> sigma(a), movement 36+4*from+d -> 36+4*sigma(from)+sigma_d(d), selection 180+cell -> 180+sigma(cell), the
auxiliary indices 216..219 unchanged.  `compose(a, b)` is "b first, then a".

The transforms launch the gfx950 kernels of csrc/lz_symmetry.hip for HIP tensors and the host build of the same C ABI
for CPU tensors (device dispatch like `v0_core`).  The tables come from the compiled header (csrc/lz_symmetry.h);
`np_*` below is an independent numpy restatement from the (r, c) formulas, the checker of the CPU tests.
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L

NUM_SYMMETRIES = 8
NUM_ACTIONS = 220
NAMES = ("identity", "rot90", "rot180", "rot270", "flip_lr", "flip_ud", "transpose", "anti_transpose")
STATE_FIELDS = ("board", "marks_black", "marks_white", "phase", "current_player", "pending_marks_required",
                "pending_marks_remaining", "pending_captures_required", "pending_captures_remaining",
                "forced_removals_done", "move_count", "moves_since_capture")
_STATE_DTYPES = (torch.int8, torch.bool, torch.bool) + (torch.int64,) * 9


# ---- the compiled tables -------------------------------------------------------------------------------------------
@lru_cache(maxsize=1)
def tables() -> Dict[str, np.ndarray]:
    """The tables of csrc/lz_symmetry.h as compiled into the host library: cells int32[8,36], actions int32[8,220],
    inverse int32[8], compose int32[8,8], directions int32[8,4]."""
    out = {"cells": np.zeros((8, 36), np.int32), "actions": np.zeros((8, 220), np.int32),
           "inverse": np.zeros(8, np.int32), "compose": np.zeros((8, 8), np.int32),
           "directions": np.zeros((8, 4), np.int32)}
    H = L.host_lib()
    args = [C.c_void_p(out[k].ctypes.data) for k in ("cells", "actions", "inverse", "compose", "directions")]
    L.check(H.lz_symmetry_tables(*args), "symmetry.tables")
    for v in out.values():
        v.setflags(write=False)
    return out


def _check_id(k) -> int:
    k = int(k)
    if not 0 <= k < NUM_SYMMETRIES:
        raise ValueError(f"symmetry id {k} is outside 0..7")
    return k


def inverse(k: int) -> int:
    return int(tables()["inverse"][_check_id(k)])


def compose(a: int, b: int) -> int:
    """The element sigma_a o sigma_b (apply b first, then a)."""
    return int(tables()["compose"][_check_id(a), _check_id(b)])


def cell_permutation(k: int) -> torch.Tensor:
    """int64[36]: sigma_k(cell)."""
    return torch.from_numpy(tables()["cells"][_check_id(k)].astype(np.int64))


def action_permutation(k: int) -> torch.Tensor:
    """int64[220]: P_sigma_k(action)."""
    return torch.from_numpy(tables()["actions"][_check_id(k)].astype(np.int64))


# ---- transforms ----------------------------------------------------------------------------------------------------
def _sym_arg(sym, n: int, device) -> Tuple[torch.Tensor, int]:
    if isinstance(sym, int):
        sym = torch.full((n,), _check_id(sym), dtype=torch.int8, device=device)
    if not isinstance(sym, torch.Tensor) or sym.dtype not in (torch.int8, torch.int32):
        raise TypeError("sym must be an int or an int8 / int32 tensor")
    if sym.numel() != n:
        raise ValueError(f"sym has {sym.numel()} ids for {n} rows")
    if sym.device != torch.device(device):
        raise ValueError(f"sym lives on {sym.device}, the rows on {device}")
    return sym.contiguous(), 1 if sym.dtype == torch.int8 else 4


def transform_samples(planes: torch.Tensor, masks: Optional[torch.Tensor], policy: Optional[torch.Tensor],
                      sym, idx: Optional[torch.Tensor] = None):
    """Row j of each output = sigma_{sym[j]} of source row idx[j] (idx None: row j), in one pass.

    planes float32[n,11,6,6]; masks bool / uint8 [n,220] and policy float32[n,220], both or neither; sym an int or an
    int8 / int32 tensor of the output rows; idx int64[m].  Returns (planes, masks, policy) of m rows (None for the
    masks / policy that were not given).  Ids outside 0..7 and indices outside [0, n) give an all-zero output row."""
    if (masks is None) != (policy is None):
        raise ValueError("masks and policy are transformed together")
    dev = planes.device
    n = int(planes.shape[0])
    pl = planes.reshape(n, 396)
    if pl.dtype != torch.float32:
        raise TypeError("planes must be float32")
    pl = pl.contiguous()
    if idx is not None:
        idx = idx.to(torch.int64).contiguous()
        m = int(idx.numel())
    else:
        m = n
    sym_t, width = _sym_arg(sym, m, dev)
    out_planes = torch.empty((m, 11, 6, 6), dtype=torch.float32, device=dev)
    out_masks = out_policy = mk = pol = None
    if masks is not None:
        mk = masks.reshape(n, NUM_ACTIONS).contiguous()
        if mk.dtype not in (torch.bool, torch.uint8):
            raise TypeError("masks must be bool or uint8")
        pol = policy.reshape(n, NUM_ACTIONS)
        if pol.dtype != torch.float32:
            raise TypeError("policy must be float32")
        pol = pol.contiguous()
        out_masks = torch.empty((m, NUM_ACTIONS), dtype=mk.dtype, device=dev)
        out_policy = torch.empty((m, NUM_ACTIONS), dtype=torch.float32, device=dev)
    for t in (mk, pol, idx):
        if t is not None and t.device != dev:
            raise ValueError(f"all tensors must live on {dev}")
    with L.device_ctx(dev):
        st = L.lib_for(planes).lz_symmetry_gather_samples(
            L.ptr(pl), L.ptr(mk), L.ptr(pol), L.i64(n), L.ptr(idx), L.ptr(sym_t), width, L.ptr(out_planes),
            L.ptr(out_masks), L.ptr(out_policy), L.i64(m), L.stream_ptr(dev))
    L.check(st, "symmetry.transform_samples")
    return out_planes, out_masks, out_policy


StatesLike = Union[Dict[str, torch.Tensor], Sequence[torch.Tensor]]


def transform_states(states: StatesLike, sym):
    """sigma_{sym[i]} of every state of a 12-tensor batch (a dict keyed like `STATE_FIELDS` or the tensors in that
    order): board and marks permuted, the scalar fields copied.  Returns the same kind of container."""
    as_dict = isinstance(states, dict)
    ts = [states[f] for f in STATE_FIELDS] if as_dict else list(states)
    if len(ts) != 12:
        raise ValueError("a state batch has 12 tensors")
    B = int(ts[0].shape[0])
    dev = ts[0].device
    ins = [t.to(dt).contiguous() for t, dt in zip(ts, _STATE_DTYPES)]
    outs = [torch.empty_like(t) for t in ins]
    sym_t, width = _sym_arg(sym, B, dev)
    with L.device_ctx(dev):
        a, b = L.soa(ins), L.soa(outs)
        st = L.lib_for(ins[0]).lz_symmetry_transform_states(C.byref(a), L.ptr(sym_t), width, C.byref(b), L.i64(B),
                                                            L.stream_ptr(dev))
    L.check(st, "symmetry.transform_states")
    outs = [o.view(t.shape) for o, t in zip(outs, ts)]
    return dict(zip(STATE_FIELDS, outs)) if as_dict else outs


def transform_packed(packed: torch.Tensor, sym) -> torch.Tensor:
    """sigma_{sym[i]} of packed 32-byte records int64[B,4] (csrc/lz_rules.h:pack); the device build runs the wave
    function of the tree search's symmetric leaf evaluation."""
    if packed.dtype != torch.int64 or packed.dim() != 2 or packed.shape[1] != 4:
        raise ValueError("packed records are int64[B,4]")
    p = packed.contiguous()
    B = int(p.shape[0])
    out = torch.empty_like(p)
    sym_t, width = _sym_arg(sym, B, p.device)
    with L.device_ctx(p.device):
        st = L.lib_for(p).lz_symmetry_transform_packed(L.ptr(p), L.ptr(sym_t), width, L.ptr(out), L.i64(B),
                                                       L.stream_ptr(p.device))
    L.check(st, "symmetry.transform_packed")
    return out


# ---- numpy restatement from the (r, c) formulas (the checker) ------------------------------------------------------
_RC = (lambda r, c: (r, c), lambda r, c: (c, 5 - r), lambda r, c: (5 - r, 5 - c), lambda r, c: (5 - c, r),
       lambda r, c: (r, 5 - c), lambda r, c: (5 - r, c), lambda r, c: (c, r), lambda r, c: (5 - c, 5 - r))
_DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1))             # lz_rules.h:move_dest: -6, +6, -1, +1


def np_cell_perm(k: int) -> np.ndarray:
    out = np.zeros(36, np.int64)
    for r in range(6):
        for c in range(6):
            rr, cc = _RC[k](r, c)
            out[r * 6 + c] = rr * 6 + cc
    return out


def np_dir_perm(k: int) -> np.ndarray:
    """The image of each direction: the linear part of the map applied to the step vector."""
    r0, c0 = _RC[k](0, 0)
    out = np.zeros(4, np.int64)
    for d, (dr, dc) in enumerate(_DIRS):
        r1, c1 = _RC[k](dr, dc)
        out[d] = _DIRS.index((r1 - r0, c1 - c0))
    return out


def np_action_perm(k: int) -> np.ndarray:
    cell, dirs = np_cell_perm(k), np_dir_perm(k)
    out = np.arange(NUM_ACTIONS, dtype=np.int64)
    out[:36] = cell
    frm, d = np.divmod(np.arange(144), 4)
    out[36:180] = 36 + 4 * cell[frm] + dirs[d]
    out[180:216] = 180 + cell
    return out


def np_compose(a: int, b: int) -> int:
    want = np_cell_perm(a)[np_cell_perm(b)]
    return next(k for k in range(8) if np.array_equal(np_cell_perm(k), want))


def np_transform_samples(planes, masks, policy, sym, idx=None):
    planes = np.asarray(planes).reshape(-1, 11, 36)
    idx = np.arange(planes.shape[0]) if idx is None else np.asarray(idx)
    sym = np.broadcast_to(np.asarray(sym), idx.shape)
    op = np.zeros((len(idx), 11, 36), planes.dtype)
    om = None if masks is None else np.zeros((len(idx), NUM_ACTIONS), np.asarray(masks).dtype)
    opol = None if policy is None else np.zeros((len(idx), NUM_ACTIONS), np.uint32)
    for k in np.unique(sym):
        rows = np.flatnonzero(sym == k)
        src = idx[rows]
        op[rows[:, None, None], np.arange(11)[None, :, None], np_cell_perm(int(k))[None, None, :]] = planes[src]
        if masks is not None:
            P = np_action_perm(int(k))
            om[rows[:, None], P[None, :]] = np.asarray(masks)[src]
            opol[rows[:, None], P[None, :]] = np.ascontiguousarray(policy, np.float32).view(np.uint32)[src]
    return op.reshape(-1, 11, 6, 6), om, (None if opol is None else opol.view(np.float32))


def np_transform_states(states: Dict[str, np.ndarray], sym) -> Dict[str, np.ndarray]:
    B = np.asarray(states["board"]).shape[0]
    sym = np.broadcast_to(np.asarray(sym), (B,))
    out = {f: np.array(states[f], copy=True) for f in STATE_FIELDS}
    for f in ("board", "marks_black", "marks_white"):
        src = np.asarray(states[f]).reshape(B, 36)
        dst = out[f].reshape(B, 36)
        for k in np.unique(sym):
            rows = np.flatnonzero(sym == k)
            dst[rows[:, None], np_cell_perm(int(k))[None, :]] = src[rows]
    return out


def np_transform_packed(packed: np.ndarray, sym) -> np.ndarray:
    p = np.asarray(packed, np.int64).view(np.uint64).reshape(-1, 4)
    sym = np.broadcast_to(np.asarray(sym), (p.shape[0],))
    bits = (p[:, :, None] >> np.arange(36, dtype=np.uint64)) & np.uint64(1)          # [B,4,36]
    out = np.zeros_like(p)
    for i in range(p.shape[0]):
        cell = np_cell_perm(int(sym[i])).astype(np.uint64)
        out[i] = (bits[i] << cell[None, :]).sum(axis=1, dtype=np.uint64)
    out[:, 0] |= p[:, 0] & ~np.uint64(0xFFFFFFFFF)
    return out.view(np.int64)
