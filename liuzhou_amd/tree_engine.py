"""Device-resident full-tree PUCT search (variant P) -- host side.

`TreeEngine` owns the HBM arenas of B concurrent search trees (csrc/lz_engine.hip) and exposes the same
split-phase protocol as the reference's C++ tree batch (`v1/python/portable_cpp_mcts.py:270-282`:
prepare roots -> evaluate -> complete, then sims x (select -> evaluate -> complete)), plus
`search()` which enqueues a whole move's search from C++ with the fused network kernel in the loop.

`PortableTreeMCTS.search_batch(state, ...)` gives it the `V1RootMCTS`-style interface (same
`RootSearchBatchOutput`), `self_play_tree_gpu` is the tree-search twin of `self_play_v1_gpu`, and
`SteadyStateTreeSelfPlay` is the fixed-population driver used by bench.py.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import time
from typing import Dict, List, Optional, Tuple

import torch

from contextlib import contextmanager

from . import _lib as L
from . import v0_core
from .game_rng import GameRng, PURPOSE_PICK, PURPOSE_PLAYOUT_CAP
from .gumbel import considered_table, gumbel_on
from .mcts_gpu import GpuStateBatch, RootSearchBatchOutput, TOTAL_ACTION_DIM, states_to_model_input, \
    encode_actions_fast
from .net_hip import DescArray, FusedNet, LzNetDesc, MAX_MULTI_NETS, multi_compatible
from .puct_shape import CPUCT_BASE_DEFAULT, CPUCT_TABLE_LEN, cpuct_table, parse_puct_shape
from .self_play_types import SelfPlayV1Stats
from .streams import CAPTURE_MODE
from .trajectory_buffer import TensorSelfPlayBatch, TensorTrajectoryBuffer
from .kld_stop import KldStop, parse_kld_stop
from .move_pick import temperature_table
from .policy_surprise import counters_from_block as surprise_counters_from_block, root_prior
from .resign import counters_from_block
from .search_rules import (START_COUNTER_KEYS, SearchRules, engine_counters, forced_playouts_on, parse_eval_symmetry,
                           persistent_default as _persistent_default, playout_cap_on, search_simulations)

MAX_CHILDREN = 72
OUT_CAP = 80


class LzTreeDesc(C.Structure):
    _fields_ = [("num_games", C.c_int64), ("node_cap", C.c_int32), ("edge_chunk", C.c_int32), ("path_cap", C.c_int32),
                ("chunk_cap", C.c_int32), ("exploration_weight", C.c_double)] + \
               [(n, C.c_void_p) for n in (
                   "root_state", "nodes", "edges", "n_nodes", "n_edges", "root_visits", "root_w",
                   "root_init_value", "path", "path_len", "leaf_kind", "leaf_state", "leaf_value", "root_terminal",
                   "active", "leaf_edge", "leaf_parent",
                   "trace_kind", "trace_leaf", "trace_heads", "trace_priors", "trace_value")] + \
               [("trace_cap", C.c_int64), ("eval_count", C.c_void_p)] + \
               [(n, C.c_void_p) for n in ("chunk_list", "n_chunks", "free_chunks", "pool_top", "pool_stats")] + \
               [("pool_chunks", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("live_state", "live_row", "live_count")] + [("live_count_cap", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("pos_index", "node_value", "leaf_src", "share_count")] + [("pos_slots", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("leaf_sym", "trace_sym", "sym_salt", "sym_game", "sym_ply")] + \
               [("sym_seed", C.c_uint64), ("sym_mode", C.c_int32), ("sym_fixed", C.c_int32)] + \
               [("seg_games", C.c_int64), ("seg_off", C.c_void_p)] + \
               [(n, C.c_void_p) for n in ("sim_budget", "root_noise")] + \
               [("forced_k", C.c_double), ("forced_count", C.c_void_p)] + \
               [("gumbel_m", C.c_int32), ("gumbel_sims", C.c_int32), ("gumbel_c_visit", C.c_double),
                ("gumbel_c_scale", C.c_double)] + \
               [(n, C.c_void_p) for n in ("gumbel_g", "gumbel_table", "gumbel_gl", "gumbel_base", "gumbel_root_base",
                                          "gumbel_root_value", "gumbel_count")] + [("gumbel_stride", C.c_int64)] + \
               [("solver", C.c_int32), ("root_proven", C.c_void_p), ("solver_count", C.c_void_p)] + \
               [("kld_interval", C.c_int32), ("kld_min_sims", C.c_int32), ("kld_threshold", C.c_double)] + \
               [(n, C.c_void_p) for n in ("kld_snapshot", "kld_budget", "kld_stops", "kld_saved", "kld_trace")] + \
               [("puct_shape", C.c_int32), ("cpuct_table_len", C.c_int32), ("fpu_reduction", C.c_double),
                ("fpu_root_reduction", C.c_double), ("cpuct_table", C.c_void_p)]


class LzTreeWaveDesc(C.Structure):
    _fields_ = [("batch_k", C.c_int32), ("path_cap", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("path", "path_len", "leaf_kind", "leaf_state", "leaf_value", "leaf_edge",
                                          "leaf_parent", "sims_done", "unfinished", "eval_row", "eval_state",
                                          "eval_count", "eval_total")] + \
               [("max_backtrack_steps", C.c_int32), ("reserved_", C.c_int32)]


WAVE_PATH_CAP = 176            # entries per leaf path of a wave (the kernel's level stack holds 160: a game lasts <= 144 plies)
EDGE_CHUNK = 1024              # edges per chunk of the engine's edge pool (32 KB); a run of <= 72 edges never straddles chunks
# pool sizing: 3 x sims nodes of 32 edges per game.  Measured peak use (bench.py `reuse.edge_pool.peak_use_frac`, round 4):
# 15 edges per simulation of the budget at C3 (16 384 x 800) and 17 at C2 -- a steady-state population is mostly in the
# movement phase with 10-20 legal moves, and a kept subtree rarely exceeds the new search -- so 96 is 6 x head-room
POOL_EDGES_PER_NODE = 32
POOL_NODES_PER_SIM = 3
MAX_NODE_CAP = 524288          # lz_tree_advance marks a game's nodes in LDS: 8 192 words of 64 with one wave per workgroup
                               # (round 6; four waves per workgroup up to 65 536 nodes, the limit until round 5)
AUTO_NODE_CAP = 65536          # arenas sized automatically (auto_reuse_factor) stay within the four-wave form
PATH_CAP = 192                 # a game lasts <= 144 plies (game_state.py:87-89), so no descent is deeper than that
REUSE_FACTOR_CAP = 40.0
POS_SLOTS_MAX = 8192           # position index: slots per game (a window that finds no room just leaves a node unindexed)
SPLIT_MAX_GAMES = 8192         # lz_engine.hip kSplitMaxGames: larger launches take the one-wave tree step


def pos_slots_for(node_cap: int) -> int:
    """Slots of a game's position index: a power of two >= 2 x node_cap (load <= 1/2), 64 .. POS_SLOTS_MAX."""
    n = 64
    while n < 2 * int(node_cap) and n < POS_SLOTS_MAX:
        n *= 2
    return n


def shares_leaves(num_games: int) -> bool:
    """Does the fused search of an engine of `num_games` games look transposed leaves up in its position index?  Only
    the one-wave tree step does (LZ_TREE_SHARE=0: never); mirrors lz_engine.hip split_step."""
    if os.environ.get("LZ_TREE_SHARE", "1").strip().startswith("0"):
        return False
    if os.environ.get("LZ_TREE_SPLIT", "").strip().startswith("0"):
        return True
    limit = int(os.environ.get("LZ_TREE_SPLIT_MAX", "0") or 0) or SPLIT_MAX_GAMES
    return int(num_games) > limit


def auto_reuse_factor(num_games: int, sims: int, device, memory_fraction: float = 0.10, cap: float = REUSE_FACTOR_CAP) -> float:
    """Room for kept subtrees in the per-game NODE arena, as a multiple of `sims` nodes: a kept subtree that would leave
    no room for the next search is pruned, so more room = fewer deviations from the reference's unbounded tree (runs of
    near-forced moves keep almost the whole tree several times in a row).  Since round 4 only the 48-byte node records
    are per game (edges come from the engine's pool), so the factor is `cap` unless `memory_fraction` of the free memory
    or the 65 536-node limit say less (C3: 40 -> 32 802 nodes = 1.5 MB per game, 25.8 GB; rounds 1-3 had worst-case edge
    regions per game and reached 11-12 with 210 GB)."""
    free, _total = torch.cuda.mem_get_info(torch.device(device))
    per_game = free * float(memory_fraction) / max(1, int(num_games))
    f = (per_game / 48.0 - (sims + 2)) / max(1, sims)
    f = min(float(cap), f, (AUTO_NODE_CAP - sims - 2) / max(1, sims))
    return max(1.0, float(int(f * 4) / 4.0))


def chunk_cap_for(node_cap: int, chunk: int) -> int:
    """Entries of a game's chunk list: the worst case of its node arena (72 children everywhere), so that only the node
    arena bounds a single game (include/liuzhou_hip.h)."""
    return -(-int(node_cap) * MAX_CHILDREN // (int(chunk) - (MAX_CHILDREN - 1))) + 1


def auto_pool_chunks(num_games: int, max_sims: int, node_cap: int, chunk: int, device, memory_fraction: float = 0.5) -> int:
    """Chunks of the engine's edge pool.  Never more than the worst case (every node of every game with 72 children:
    then an allocation cannot fail, which is what small engines get); large engines get the MEAN case with head-room --
    POOL_NODES_PER_SIM x sims nodes x POOL_EDGES_PER_NODE edges per game, at least 64 worst-case games -- because the sum
    over thousands of games is stable although single games vary by 20x; bounded by `memory_fraction` of the free memory
    and by the 2^31 pool indices (64 GB)."""
    worst = int(num_games) * chunk_cap_for(node_cap, chunk)
    # per game: the mean case rounded up to whole chunks, + 1 for the open, partly filled chunk every game holds
    mean = int(num_games) * (-(-min(int(node_cap), POOL_NODES_PER_SIM * (int(max_sims) + 1)) * POOL_EDGES_PER_NODE // int(chunk)) + 1)
    floor = min(int(num_games), 64) * chunk_cap_for(node_cap, chunk)
    n = min(worst, max(mean, floor))
    free, _total = torch.cuda.mem_get_info(torch.device(device))
    n = min(n, int(free * float(memory_fraction)) // (int(chunk) * 32), (1 << 31) // int(chunk) - 2)
    return max(n, 2)


def samples_per_launch_pass(net) -> int:
    """Positions one pass of the fused network kernel evaluates over the whole chip: workgroups per launch x samples per
    workgroup (csrc/lz_net.hip: 256 x 16 for 64 channels, 512 x 8 in the half-workgroup shape, 256 x 8 for 128 channels)."""
    ch, flags = int(net.desc.channels), int(net.desc.flags)
    groups = int(net.desc.max_blocks) if int(net.desc.max_blocks) > 0 else (512 if (ch == 64 and flags & 1) else 256)
    return groups * (16 if (ch == 64 and not flags & 1) else 8)


class TreeEngine:
    def __init__(self, num_games: int, max_sims: int, device, exploration_weight: float = 1.0,
                 reuse_factor: float = 0.0, batch_k: int = 1, edge_chunk: int = EDGE_CHUNK,
                 pool_chunks: Optional[int] = None, compact_evals: bool = False, max_backtrack_steps: int = 0,
                 segment_games: Optional[int] = None) -> None:
        """`segment_games`: the slots form num_games / segment_games segments of that many slots (a multiple of 16), slot
        g searched with network g // segment_games (search_multi: one network launch per simulation for all segments,
        compact lists always on).
        `max_backtrack_steps` (batch_k > 1): the reference's MAX_BACKTRACK_STEPS (src/mcts.py:337; 0 = its 128).
        `compact_evals`: the fused search evaluates, per simulation, only the leaves that need the network (compact
        device-side list, `LzTreeDesc.live_*`) -- a launch then costs ceil(live / samples per pass) network passes instead
        of one per slot, so a draining wave gets cheaper as its games end; bit-identical results.
        `reuse_factor` > 0 reserves room for kept subtrees of up to reuse_factor * max_sims nodes in every game's node
        arena (advance(); < 0: auto_reuse_factor).  Edges live in ONE pool per engine, handed out in chunks of `edge_chunk`
        records (`pool_chunks`: None = auto_pool_chunks).
        `batch_k` > 1: the legacy search's waves (src/mcts.py `batch_K`): up to batch_k distinct leaves per game are
        collected, evaluated together and backed up per wave (select_wave / expand_wave / search)."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("TreeEngine needs a HIP device (no CPU path)")
        self.device, self.B, self.max_sims = dev, int(num_games), int(max_sims)
        B = self.B
        if float(reuse_factor) < 0:
            reuse_factor = auto_reuse_factor(B, self.max_sims, dev)
        self.reuse_factor = float(reuse_factor)
        extra = int(max(0.0, float(reuse_factor)) * self.max_sims)
        self.node_cap = self.max_sims + 2 + extra
        self.path_cap = min(self.node_cap + 1, PATH_CAP)
        if self.node_cap > MAX_NODE_CAP:
            raise ValueError(f"at most {MAX_NODE_CAP} nodes per game, got {self.node_cap}")
        self.edge_chunk = int(edge_chunk)
        if self.edge_chunk < 128 or self.edge_chunk & (self.edge_chunk - 1):
            raise ValueError(f"edge_chunk must be a power of two >= 128, got {edge_chunk}")
        self.chunk_cap = chunk_cap_for(self.node_cap, self.edge_chunk)
        self.pool_chunks = int(pool_chunks) if pool_chunks is not None else \
            auto_pool_chunks(B, self.max_sims, self.node_cap, self.edge_chunk, dev)
        if (self.pool_chunks + 1) * self.edge_chunk > (1 << 31):
            raise ValueError(f"edge pool of {self.pool_chunks} x {self.edge_chunk} records exceeds 2^31 pool indices")
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.buf: Dict[str, torch.Tensor] = {
            "root_state": z((B, 4), torch.int64),
            "nodes": z((B * self.node_cap, 6), torch.int64),            # 48-byte node records
            "edges": torch.empty((self.pool_chunks * self.edge_chunk, 4), dtype=torch.int64, device=dev),   # 32-byte records
            "n_nodes": z((B,), torch.int32), "n_edges": z((B,), torch.int32), "root_visits": z((B,), torch.int32),
            "root_w": z((B,), torch.float64), "root_init_value": z((B,), torch.float32),
            "path": z((B * self.path_cap,), torch.int32), "path_len": z((B,), torch.int32),
            "leaf_kind": z((B,), torch.int32), "leaf_state": z((B, 4), torch.int64), "leaf_value": z((B,), torch.float32),
            "root_terminal": z((B,), torch.uint8), "active": torch.ones((B,), dtype=torch.uint8, device=dev),
            "leaf_edge": z((B,), torch.int32), "leaf_parent": z((B,), torch.int32),
            "chunk_list": z((B * self.chunk_cap,), torch.int32), "n_chunks": z((B,), torch.int32),
            "free_chunks": torch.arange(self.pool_chunks, dtype=torch.int32, device=dev),
            "pool_top": torch.full((1,), self.pool_chunks, dtype=torch.int32, device=dev),
            # [0] expansions refused because the pool was empty (0 in a correctly sized engine), [1] fewest free chunks seen
            # + [2] fresh roots that still have to take the chunk of their first expansion (reserved for them)
            "pool_stats": torch.tensor([0, self.pool_chunks, 0], dtype=torch.int32, device=dev),
            # position index (LzTreeDesc.pos_*): table of node indices per game, raw value per node, source of a shared leaf
            "pos_index": torch.full((B * pos_slots_for(self.node_cap),), -1, dtype=torch.int32, device=dev),
            "node_value": z((B * self.node_cap,), torch.float32), "leaf_src": z((B,), torch.int32),
        }
        d = LzTreeDesc()
        d.num_games, d.node_cap, d.edge_chunk, d.path_cap = B, self.node_cap, self.edge_chunk, self.path_cap
        d.chunk_cap, d.pool_chunks = self.chunk_cap, self.pool_chunks
        d.pos_slots = pos_slots_for(self.node_cap)
        if int(L.lib().lz_tree_desc_bytes()) != C.sizeof(LzTreeDesc):
            raise RuntimeError(f"LzTreeDesc layout mismatch: library {int(L.lib().lz_tree_desc_bytes())} B, "
                               f"Python {C.sizeof(LzTreeDesc)} B")
        d.exploration_weight = float(exploration_weight)
        for name, t in self.buf.items():
            setattr(d, name, t.data_ptr())
        self.desc = d
        self.batch_k = max(1, int(batch_k))
        if self.batch_k > 32:
            raise ValueError(f"batch_k must be <= 32, got {self.batch_k}")
        K = self.batch_k
        self.wbuf: Dict[str, torch.Tensor] = {}
        self.wdesc = None
        if K > 1:                                                       # slot-major [K][B] per-leaf arrays of a wave
            self.wbuf = {
                "path": z((K * B * WAVE_PATH_CAP,), torch.int32), "path_len": z((K * B,), torch.int32),
                "leaf_kind": z((K * B,), torch.int32), "leaf_state": z((K * B, 4), torch.int64),
                "leaf_value": z((K * B,), torch.float32), "leaf_edge": z((K * B,), torch.int32),
                "leaf_parent": z((K * B,), torch.int32), "sims_done": z((B,), torch.int32),
                "unfinished": z((1,), torch.int32), "eval_row": z((K * B,), torch.int32),
                "eval_state": z((K * B, 4), torch.int64), "eval_count": z((1,), torch.int64),
                "eval_total": z((1,), torch.int64),
            }
            wd = LzTreeWaveDesc()
            wd.batch_k, wd.path_cap = K, WAVE_PATH_CAP
            wd.max_backtrack_steps = max(0, int(max_backtrack_steps))
            for name, t in self.wbuf.items():
                setattr(wd, name, t.data_ptr())
            self.wdesc = wd
        # evaluator scratch (fused network inputs / outputs): one row per leaf slot of a wave
        self.planes = z((B, 11, 6, 6), torch.float32)
        self.lp1, self.lp2, self.lpm = (z((K * B, 36), torch.float32) for _ in range(3))
        self.values = z((K * B,), torch.float32)
        # finish outputs
        self.policy_dense = z((B, TOTAL_ACTION_DIM), torch.float32)
        self.chosen_index = z((B,), torch.int32)
        self.chosen_code = z((B, 4), torch.int32)
        self.chosen_valid = z((B,), torch.bool)
        self.terminal_mask = z((B,), torch.bool)
        self.root_value = z((B,), torch.float32)
        self.child_count = z((B,), torch.int32)
        self.child_action = z((B, OUT_CAP), torch.int32)
        self.child_visits = z((B, OUT_CAP), torch.int32)
        self.child_prior = z((B, OUT_CAP), torch.float32)
        self.reuse_dropped = z((2,), torch.int32)      # [0] kept subtrees dropped whole (defensive), [1] pruned to fit
        self.eval_count = z((B,), torch.int32)          # evaluations the games' expand steps consumed (LzTreeDesc.eval_count)
        self.desc.eval_count = self.eval_count.data_ptr()
        self.share_count = z((B,), torch.int32)         # leaves that took a transposed twin's evaluation (LzTreeDesc.share_count)
        self.desc.share_count = self.share_count.data_ptr()
        # forced playouts and policy target pruning (set_forced_playouts; LzTreeDesc.forced_k / forced_count)
        self.forced_k = 0.0
        self.forced_count = z((B,), torch.int32)        # descents that took a due root child, summed over the searches
        self.child_target_visits = z((B, OUT_CAP), torch.int32)   # finish() with forced_k > 0: the pruned visits N' of the target
        self.pruned_visits = z((B,), torch.int32)       # finish() with forced_k > 0: sum(N - N') of the last search
        # Gumbel root search (set_gumbel; LzTreeDesc.gumbel_*): the buffers exist only once it is switched on
        self.gumbel_m, self.gumbel_c_visit, self.gumbel_c_scale = 0, 50.0, 1.0
        self.gumbel: Dict[str, torch.Tensor] = {}
        # MCTS-Solver (set_solver; LzTreeDesc.solver / root_proven / solver_count): the buffers exist only once it is on
        self.solver = False
        self.root_proven: Optional[torch.Tensor] = None
        self.solver_count: Optional[torch.Tensor] = None
        self.solver_overrides: Optional[torch.Tensor] = None
        # PUCT shape (set_puct_shape; LzTreeDesc.puct_shape ..): the c(n) table exists only once that half is switched on
        self.puct_shape = parse_puct_shape()
        self.cpuct_table: Optional[torch.Tensor] = None
        # KLD-gain early stopping (set_kld_stop; LzTreeDesc.kld_*): the buffers exist only once it is switched on
        self.kld_stop = parse_kld_stop()
        self.kld: Dict[str, torch.Tensor] = {}
        self.segment_games = None if segment_games is None else int(segment_games)
        self.num_segments = 1
        if self.segment_games is not None:
            G = self.segment_games
            if G <= 0 or G % 16 or B % G:
                raise ValueError(f"segment_games must be a positive multiple of 16 dividing num_games, got {G} of {B}")
            self.num_segments = B // G
            if self.num_segments > MAX_MULTI_NETS:
                raise ValueError(f"at most {MAX_MULTI_NETS} segments, got {self.num_segments}")
            if self.batch_k > 1:
                raise ValueError("segments (several networks) need batch_k = 1")
            compact_evals = True
            self.seg_off = z(((self.max_sims + 2) * (self.num_segments + 1),), torch.int64)
            self.desc.seg_games, self.desc.seg_off = G, self.seg_off.data_ptr()
        self.compact_evals = bool(compact_evals) and self.batch_k == 1
        self.live_total = z((1,), torch.int64)          # compact_evals: evaluations launched so far (sum of the per-simulation counts)
        if self.compact_evals:
            self.live = {"live_state": z((B, 4), torch.int64), "live_row": z((B,), torch.int32),
                         "live_count": z((self.max_sims + 2,), torch.int64)}
            for name, t in self.live.items():
                setattr(self.desc, name, t.data_ptr())
            self.desc.live_count_cap = self.max_sims + 2
        # persistent search kernel (lz_tree_search_persistent, one launch per move): built, parity-tested and MEASURED
        # SLOWER than the two-stream launch pairs at C2 (profiles/r03_experiments.md: 164-170 k against 192-194 k
        # positions/s), so it is opt-in (LZ_TREE_PERSISTENT=1 / the `persistent` attribute).  The CU's second workgroup
        # starts `stagger_us` late (LZ_TREE_STAGGER_US) so that the pair sharing a CU alternates network pass / tree step
        self.persistent = _persistent_default()
        self.stagger_us = int(os.environ.get("LZ_TREE_STAGGER_US", "40"))
        self._cu_slots: Optional[torch.Tensor] = None
        self.phase_ticks: Optional[torch.Tensor] = None

    def enable_trace(self, steps: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Parity tests: record, per step of a search (slot 0 = root step, slot s = s-th simulation), what the expand
        kernel consumed -- leaf kind / state, head rows, the softmax over the legal set, the value (LzTreeDesc.trace_*).
        Must be called before the search is captured into a graph (kernel arguments are frozen at capture)."""
        n = (self.max_sims + 1) if steps is None else int(steps)
        B, dev = self.B, self.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.trace = {"trace_kind": z((n, B), torch.int32), "trace_leaf": z((n, B, 4), torch.int64),
                      "trace_heads": z((n, B, 108), torch.float32), "trace_priors": z((n, B, 220), torch.float32),
                      "trace_value": z((n, B), torch.float32), "trace_sym": z((n, B), torch.int32)}
        for name, t in self.trace.items():
            setattr(self.desc, name, t.data_ptr())
        self.desc.trace_cap = n
        return self.trace

    def set_eval_symmetry(self, mode, seed: int = 0, game: Optional[torch.Tensor] = None,
                          ply: Optional[torch.Tensor] = None) -> None:
        """Symmetric leaf evaluation (LzTreeDesc.sym_*): every evaluation is of sigma_k(leaf), the heads mapped back in the
        expand step.  `mode`: "none", "random" (k per evaluation from Philox keyed by `seed`, the game key `game[g]`, its
        ply `ply[g]` -- device tensors read at every launch -- a per-run salt and the leaf state) or a fixed id 0..7.  Must be
        set before a search is captured into a graph."""
        d = self.desc
        if mode == "none":
            d.sym_mode = 0
            return
        if self.batch_k > 1:
            raise ValueError("eval_symmetry is not supported by the legacy waves (batch_k > 1): their wave kernels "
                             "evaluate leaves without the symmetry hook")
        dev = self.device
        if "leaf_sym" not in self.buf:
            self.buf["leaf_sym"] = torch.zeros((self.B,), dtype=torch.int32, device=dev)
            self.buf["sym_salt"] = torch.zeros((self.B,), dtype=torch.int32, device=dev)
            d.leaf_sym, d.sym_salt = self.buf["leaf_sym"].data_ptr(), self.buf["sym_salt"].data_ptr()
        # per-run salt: the run's seed lives in device memory too, so an engine whose searches were captured under another
        # seed (a cached engine, reset_run) still draws that run's own ids
        self.buf["sym_salt"].fill_(int(seed) * 0x9E3779B1 & 0x7FFFFFFF)
        if mode == "random":
            if game is None or ply is None:
                raise ValueError("eval_symmetry='random' needs the per-game RNG keys (game, ply)")
            self._sym_keys = (game, ply)
            d.sym_game, d.sym_ply = game.data_ptr(), ply.data_ptr()
            d.sym_mode, d.sym_fixed, d.sym_seed = 2, 0, int(seed) & 0xFFFFFFFFFFFFFFFF
        else:
            d.sym_mode, d.sym_fixed = 1, int(mode)
        self.persistent = False           # the persistent kernel's own network pass is not part of this: the fused search

    def set_playout_cap(self, sim_budget: Optional[torch.Tensor], root_noise: Optional[torch.Tensor]) -> None:
        """Playout cap (LzTreeDesc.sim_budget / root_noise): int32[B] simulations of every search per game and uint8[B]
        root noise switch, device tensors read at every launch (None: off).  Only search() honours them; must be set
        before a search is captured into a graph."""
        for name, t, dt in (("sim_budget", sim_budget, torch.int32), ("root_noise", root_noise, torch.uint8)):
            if t is not None and (t.dtype != dt or t.numel() != self.B or not t.is_contiguous() or t.device != self.device):
                raise ValueError(f"{name} must be a contiguous {dt} tensor of {self.B} elements on {self.device}")
            setattr(self.desc, name, None if t is None else t.data_ptr())
        self._cap_arrays = (sim_budget, root_noise)              # keep them alive while the descriptor points at them
        if self.kld_stop.on:                                      # the rule writes the very array the searches read
            if sim_budget is None:
                raise ValueError("KLD-gain early stopping needs the per-game budget array")
            self.desc.kld_budget = sim_budget.data_ptr()

    def set_forced_playouts(self, k: float) -> None:
        """Forced playouts and policy target pruning (LzTreeDesc.forced_k; 0 = off): select() and search() force due root
        children in the games whose root-noise switch is on, finish() forms the training target from the pruned visits
        (`child_target_visits`, `pruned_visits`; `forced_count` sums the forced descents).  Must be set before a search is
        captured into a graph."""
        on = forced_playouts_on(k)
        if on and self.gumbel_m > 0:
            raise ValueError("forced playouts and the Gumbel root search are two rules for the same root level")
        if on and self.batch_k > 1:
            raise ValueError("forced playouts are not supported by the legacy waves (batch_k > 1)")
        if on and self.segment_games is not None:
            raise ValueError("forced playouts are not supported with several networks in one search")
        self.forced_k = float(k)
        self.desc.forced_k = self.forced_k
        self.desc.forced_count = self.forced_count.data_ptr() if on else None
        if on:
            self.persistent = False       # the persistent kernel refuses the descriptor: the launch-pair search

    def set_gumbel(self, considered: int, c_visit: float = 50.0, c_scale: float = 1.0,
                   sims: Optional[int] = None) -> None:
        """Gumbel root search with Sequential Halving (LzTreeDesc.gumbel_*; considered = 0: off).  In the games whose
        root-noise switch is on, select() / search() pick the root child by the Sequential Halving schedule of
        `gumbel.considered_table(considered, sims)` (`sims`: the simulations of a search, default max_sims) and
        g + log P + sigma(completed Q); the root step records `gumbel["gl"]`, `["base"]`, `["root_base"]`, `["root_value"]`,
        and finish() picks the move and forms the training target by the same rule (`gumbel["score"]`, `["vmix"]`).  Such a
        search never mixes Dirichlet noise into its root priors.  The variates are read from `gumbel["g"]` (float32[B,
        OUT_CAP]) at every launch: refresh them in place (GameRng.gumbel_into).  `gumbel["count"]` sums the searches whose
        root step ran the rule.  Must be set before a search is captured into a graph."""
        on = gumbel_on(considered, c_visit, c_scale)
        if on and self.batch_k > 1:
            raise ValueError("the Gumbel root search is not supported by the legacy waves (batch_k > 1)")
        if on and self.segment_games is not None:
            raise ValueError("the Gumbel root search is not supported with several networks in one search")
        if on and self.forced_k > 0.0:
            raise ValueError("the Gumbel root search and forced playouts are two rules for the same root level")
        if on and self.puct_shape.on:
            raise ValueError("the Gumbel root search is not supported with first-play urgency / the visit-scaled cpuct")
        if on and self.kld_stop.on:
            raise ValueError("the Gumbel root search is not supported with KLD-gain early stopping")
        d = self.desc
        self.gumbel_m = int(considered)
        self.gumbel_c_visit, self.gumbel_c_scale = float(c_visit), float(c_scale)
        d.gumbel_m = self.gumbel_m
        if not on:
            return
        n = max(1, self.max_sims if sims is None else int(sims))
        B, dev = self.B, self.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        if not self.gumbel:
            self.gumbel = {"g": z((B, OUT_CAP), torch.float32), "gl": z((B, OUT_CAP), torch.float32),
                           "base": z((B, OUT_CAP), torch.int32), "root_base": z((B,), torch.int32),
                           "root_value": z((B,), torch.float32), "count": z((B,), torch.int32),
                           "score": z((B, OUT_CAP), torch.float64), "vmix": z((B,), torch.float64)}
        self.gumbel["table"] = torch.from_numpy(considered_table(self.gumbel_m, n)).to(dev).contiguous()
        d.gumbel_sims, d.gumbel_stride = n, OUT_CAP
        d.gumbel_c_visit, d.gumbel_c_scale = self.gumbel_c_visit, self.gumbel_c_scale
        for name in ("g", "table", "gl", "base", "root_base", "root_value", "count"):
            setattr(d, "gumbel_" + name, self.gumbel[name].data_ptr())
        self.persistent = False           # the persistent kernel refuses the descriptor: the launch-pair search

    def set_puct_shape(self, fpu_reduction: Optional[float] = None, fpu_root_reduction: Optional[float] = None,
                       cpuct_log: float = 0.0, cpuct_base: float = CPUCT_BASE_DEFAULT,
                       table_len: int = CPUCT_TABLE_LEN) -> None:
        """First-play urgency and the visit-scaled exploration constant (LzTreeDesc.puct_shape; off
        by default).  `fpu_reduction` (None: off; 0.0 is on): an unvisited child scores the node's own mean value minus
        fpu_reduction * sqrt(explored prior mass), clamped at -1; `fpu_root_reduction` (None: fpu_reduction) is the root's
        reduction.  `cpuct_log` > 0: c(n) = exploration_weight + cpuct_log * ln((n + cpuct_base + 1) / cpuct_base) from a
        table of `table_len` float64 entries built by puct_shape.cpuct_table and uploaded here once (visit counts beyond it
        take the last entry).  select() / search() / search_multi honour both, finish() with forced playouts prunes under
        c(root visits).  Everything off: nothing is allocated and the descriptor is as before.  Must be set before a search
        is captured into a graph."""
        shape = parse_puct_shape(fpu_reduction, fpu_root_reduction, cpuct_log, cpuct_base)
        if shape.on and self.batch_k > 1:
            raise ValueError("first-play urgency / the visit-scaled cpuct are not supported by the legacy waves (batch_k > 1)")
        if shape.on and self.gumbel_m > 0:
            raise ValueError("first-play urgency / the visit-scaled cpuct are not supported with the Gumbel root search")
        d = self.desc
        self.puct_shape = shape
        d.puct_shape = shape.flags
        d.fpu_reduction, d.fpu_root_reduction = shape.fpu_reduction, shape.fpu_root_reduction
        if shape.table:
            tab = cpuct_table(float(d.exploration_weight), shape.cpuct_log, shape.cpuct_base, int(table_len))
            self.cpuct_table = torch.tensor(tab, dtype=torch.float64, device=self.device)
            d.cpuct_table, d.cpuct_table_len = self.cpuct_table.data_ptr(), len(tab)
        else:
            self.cpuct_table = None
            d.cpuct_table, d.cpuct_table_len = None, 0
        if shape.on:
            self.persistent = False       # the persistent kernel refuses the descriptor: the launch-pair search

    def set_kld_stop(self, kld_stop: Optional[KldStop], trace: bool = False) -> None:
        """KLD-gain early stopping (LzTreeDesc.kld_*; None / threshold 0 = off).  search() then runs
        one check of the rule behind launch 0 (the snapshot) and behind every launch s = k * interval with s + 1 < sims; a
        stopped game's entry of the budget array set by set_playout_cap() -- required, and refilled by the caller before
        every search -- becomes s + 1.  `kld["stops"]` / `kld["saved"]` (int64[B]) sum the stopped searches and the
        simulations they did not run, `kld["snapshot"]` (int32[B, 72]) holds the root visits of the last check, `trace`
        adds `kld["trace"]` (float64[B]: the last per-simulation gain; tests).  Call after set_playout_cap() and before a
        search is captured into a graph."""
        ks = parse_kld_stop() if kld_stop is None else kld_stop
        d = self.desc
        if ks.on:
            if self.batch_k > 1:
                raise ValueError("KLD-gain early stopping is not supported by the legacy waves (batch_k > 1)")
            if self.segment_games is not None:
                raise ValueError("KLD-gain early stopping is not supported with several networks in one search")
            if self.gumbel_m > 0:
                raise ValueError("KLD-gain early stopping is not supported with the Gumbel root search (its Sequential "
                                 "Halving schedule is a function of a fixed budget)")
            budget = getattr(self, "_cap_arrays", (None, None))[0]
            if budget is None:
                raise ValueError("KLD-gain early stopping needs the per-game budget array (set_playout_cap) first")
        self.kld_stop = ks
        d.kld_threshold, d.kld_interval, d.kld_min_sims = (ks.threshold, ks.interval, ks.min_simulations) if ks.on else (0.0, 0, 0)
        if not ks.on:
            d.kld_snapshot = d.kld_budget = d.kld_stops = d.kld_saved = d.kld_trace = None
            return
        B, dev = self.B, self.device
        if not self.kld:
            self.kld = {"snapshot": torch.zeros((B, MAX_CHILDREN), dtype=torch.int32, device=dev),
                        "stops": torch.zeros((B,), dtype=torch.int64, device=dev),
                        "saved": torch.zeros((B,), dtype=torch.int64, device=dev)}
        if trace and "trace" not in self.kld:
            self.kld["trace"] = torch.zeros((B,), dtype=torch.float64, device=dev)
        d.kld_snapshot, d.kld_budget = self.kld["snapshot"].data_ptr(), budget.data_ptr()
        d.kld_stops, d.kld_saved = self.kld["stops"].data_ptr(), self.kld["saved"].data_ptr()
        d.kld_trace = self.kld["trace"].data_ptr() if "trace" in self.kld else None
        self.persistent = False           # the persistent kernel refuses the descriptor: the launch-pair search

    def kld_check(self, step: int) -> None:
        """One check of the rule behind launch `step` (lz_tree_kld_check; tests drive single checks with it)."""
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_tree_kld_check(C.byref(self.desc), L.i64(step), self._stream()), "tree_kld_check")

    def set_solver(self, on: bool = True) -> None:
        """MCTS-Solver (LzTreeDesc.solver; off by default): the expand step marks proven edges and carries them up the
        tree, select() / search() take a proven win, avoid proven losses and end a descent at a decided edge, and
        solver_pick() (after finish()) keeps the played move from throwing a proven win away.  `root_proven` int32[B]
        (0 unknown, 1 lost, 2 drawn, 3 won for the root's mover), `solver_count` int32[B] (marks made, summed over the
        searches) and `solver_overrides` int32[B] (picks changed).  Must be set before a search is captured into a graph."""
        on = bool(on)
        if on and self.batch_k > 1:
            raise ValueError("the MCTS-Solver is not supported by the legacy waves (batch_k > 1)")
        if on and self.segment_games is not None:
            raise ValueError("the MCTS-Solver is not supported with several networks in one search")
        self.solver = on
        d = self.desc
        d.solver = 1 if on else 0
        if not on:
            d.root_proven = d.solver_count = None
            return
        if self.root_proven is None:
            z = lambda: torch.zeros((self.B,), dtype=torch.int32, device=self.device)
            self.root_proven, self.solver_count, self.solver_overrides = z(), z(), z()
        d.root_proven, d.solver_count = self.root_proven.data_ptr(), self.solver_count.data_ptr()
        self.persistent = False           # the persistent kernel refuses the descriptor: the launch-pair search

    def solver_pick(self, force_uniform: Optional[torch.Tensor] = None) -> None:
        """lz_tree_solver_pick over the last finish()'s picks (nothing is launched while the solver is off)."""
        if not self.solver:
            return
        if force_uniform is not None and force_uniform.dtype != torch.uint8:
            force_uniform = force_uniform.to(torch.uint8)
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_tree_solver_pick(C.byref(self.desc), L.ptr(force_uniform), L.ptr(self.chosen_index),
                                                L.ptr(self.chosen_code), L.ptr(self.chosen_valid),
                                                L.ptr(self.solver_overrides), self._stream()), "tree_solver_pick")

    def move_pick(self, temperatures: torch.Tensor, uniforms: Optional[torch.Tensor], visit_offset: float = 0.0,
                  value_cutoff: float = 0.0, force_uniform: Optional[torch.Tensor] = None, sample_moves: bool = True,
                  counters: Optional[torch.Tensor] = None) -> None:
        """lz_tree_move_pick over the last finish()'s picks, with the temperatures / uniforms / force mask that finish was
        given: the visit-offset / value-cutoff re-pick of the games whose move was sampled from the visits (move_pick.py,
        DESIGN.md section 19).  `counters` int64[4] (optional): games applied to, children cut by the offset, children cut
        by the value cutoff, picks changed.  Nothing is launched with both parameters 0 or without `sample_moves`; call it
        before solver_pick()."""
        if float(visit_offset) == 0.0 and float(value_cutoff) == 0.0:
            return
        if force_uniform is not None and force_uniform.dtype != torch.uint8:
            force_uniform = force_uniform.to(torch.uint8)
        if counters is not None and (counters.dtype != torch.int64 or counters.numel() < 4 or not counters.is_contiguous()):
            raise ValueError("move_pick counters must be a contiguous int64 tensor of 4 entries")
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_tree_move_pick(C.byref(self.desc), L.ptr(temperatures), L.ptr(force_uniform), L.ptr(uniforms),
                                              C.c_int(int(bool(sample_moves))), C.c_double(float(visit_offset)),
                                              C.c_double(float(value_cutoff)), L.ptr(self.chosen_index),
                                              L.ptr(self.chosen_code), L.ptr(counters), self._stream()), "tree_move_pick")

    _NODE_DT = [("w0", "<u8"), ("w1", "<u8"), ("w2", "<u8"), ("w3", "<u8"), ("edge_begin", "<i4"), ("nedges", "<i4"),
                ("parent", "<i4"), ("old_begin", "<i4")]
    _EDGE_DT = [("W", "<f8"), ("P", "<f4"), ("n_info", "<u4"), ("child", "<i4"), ("cbegin", "<i4"),
                ("act", "u1"), ("cn", "u1"), ("pad", "V6")]

    def game_nodes(self, g: int, count: Optional[int] = None):
        """Host copy of game g's node records (numpy structured array; inspection / tests, not the hot loop)."""
        import numpy as np
        nn = int(self.buf["n_nodes"][g]) if count is None else int(count)
        return self.buf["nodes"].view(self.B, self.node_cap, 6)[g, :nn].contiguous().cpu().numpy().view(np.dtype(self._NODE_DT)).reshape(nn)

    def edge_run(self, begin: int, count: int):
        """Host copy of `count` edge records from pool index `begin` (a node's run: Node.edge_begin / nedges)."""
        import numpy as np
        return self.buf["edges"][int(begin):int(begin) + int(count)].contiguous().cpu().numpy().view(np.dtype(self._EDGE_DT)).reshape(int(count))

    def root_edge_records(self, g: int):
        """The root's edge records of game g, read from the pool (host copy: inspection / adapters, not the hot loop):
        list of {action_index, prior, visit_count, value_sum (child mover's side), child_white, terminal}."""
        node = self.game_nodes(g, 1)[0]
        e0, ne = int(node["edge_begin"]), int(node["nedges"])
        if ne <= 0:
            return []
        recs = self.edge_run(e0, ne)
        return [{"action_index": int(r["act"]), "prior": float(r["P"]), "visit_count": int(r["n_info"] & 0xFFFFFF),
                 "value_sum": float(r["W"]), "child_white": bool((r["n_info"] >> 24) & 1),
                 "terminal": bool((r["n_info"] >> 24) & 2), "info": int(r["n_info"] >> 24)} for r in recs]

    def pool_status(self) -> Dict[str, int]:
        """Edge pool: chunks, free now, fewest free seen since construction, refused expansions (must stay 0)."""
        refused, low = (int(v) for v in self.buf["pool_stats"][:2].tolist())
        return {"chunks": self.pool_chunks, "chunk_edges": self.edge_chunk, "free": int(self.buf["pool_top"].item()),
                "fewest_free": low, "refused_expansions": refused,
                "bytes": self.pool_chunks * self.edge_chunk * 32}

    def hbm_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.buf.values())

    def _stream(self):
        return L.stream_ptr(self.device)

    # ---- state plumbing ----
    def set_roots(self, state: GpuStateBatch, active: Optional[torch.Tensor] = None) -> None:
        ts = [t if t.is_contiguous() else t.contiguous() for t in state.tensors()]
        s = L.soa(ts)
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_pack_states(C.byref(s), L.i64(self.B), L.ptr(self.buf["root_state"]), self._stream()),
                    "pack_states")
        if active is not None:
            self.buf["active"].copy_(active.to(torch.uint8))
        else:
            self.buf["active"].fill_(1)

    def begin(self) -> None:
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_tree_begin(C.byref(self.desc), self._stream()), "tree_begin")

    def select(self) -> None:
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_tree_select(C.byref(self.desc), self._stream()), "tree_select")

    def leaf_planes(self) -> torch.Tensor:
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_packed_to_model_input(L.ptr(self.buf["leaf_state"]), L.i64(self.B), L.ptr(self.planes),
                                                     self._stream()), "packed_to_model_input")
        return self.planes

    def expand(self, *, is_root: bool, values: torch.Tensor, heads=None, priors220: Optional[torch.Tensor] = None,
               noise: Optional[torch.Tensor] = None, epsilon: float = 0.25) -> None:
        lp1 = lp2 = lpm = None
        if priors220 is None:
            lp1, lp2, lpm = heads
        nz_stride = int(noise.shape[1]) if noise is not None else 0
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_tree_expand(C.byref(self.desc), C.c_int(1 if is_root else 0), L.ptr(lp1), L.ptr(lp2),
                                           L.ptr(lpm), L.ptr(priors220), L.ptr(values), L.ptr(noise), L.i64(nz_stride),
                                           C.c_float(float(epsilon)), self._stream()), "tree_expand")

    # ---- waves of batch_k leaves (legacy search, src/mcts.py:318-497) ----
    def select_wave(self, sims: int, reset_budget: bool = False) -> None:
        """Up to min(batch_k, sims - used) distinct leaves per game into the [batch_k][B] slot arrays (wbuf)."""
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_tree_wave_select(C.byref(self.desc), C.byref(self.wdesc), L.i64(sims),
                                                C.c_int(1 if reset_budget else 0), self._stream()), "tree_wave_select")

    def expand_wave(self, *, values: torch.Tensor, heads=None, priors220: Optional[torch.Tensor] = None,
                    slot_major: bool = False) -> None:
        """Back up / expand the wave's leaves in the reference's order.  Evaluator rows: the compact list
        (wbuf eval_state / eval_row), or slot-major [batch_k][B] with `slot_major` / `priors220`."""
        lp1 = lp2 = lpm = None
        if priors220 is None:
            lp1, lp2, lpm = heads
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_tree_wave_expand(C.byref(self.desc), C.byref(self.wdesc), L.ptr(lp1), L.ptr(lp2),
                                                L.ptr(lpm), L.ptr(priors220), L.ptr(values),
                                                C.c_int(1 if slot_major else 0), self._stream()),
                    "tree_wave_expand")

    def search_waves(self, net: FusedNet, sims: int, waves: int, noise: Optional[torch.Tensor] = None,
                     epsilon: float = 0.25, continue_trees: bool = False, skip_roots: bool = False) -> None:
        """[roots ->] `waves` x (select batch_k leaves, evaluate batch_k * B slots, expand + backup); C++ loop."""
        nz_stride = int(noise.shape[1]) if noise is not None else 0
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_tree_search_waves(
                C.byref(self.desc), C.byref(self.wdesc), C.byref(net.desc), L.i64(sims), L.i64(waves), L.ptr(self.lp1),
                L.ptr(self.lp2), L.ptr(self.lpm), L.ptr(self.values), L.ptr(noise), L.i64(nz_stride),
                C.c_float(float(epsilon)), C.c_int(1 if continue_trees else 0), C.c_int(1 if skip_roots else 0),
                self._stream()), "tree_search_waves")

    def finish_waves(self, net: FusedNet, sims: int, max_rounds: int = 4096) -> int:
        """Games that found fewer open leaves than batch_k in some wave still have budget: further rounds until every
        game has used `sims` simulations (one host read per round; rare outside tiny endgame trees)."""
        rounds, chunk = 0, 8             # a round in which every game is done costs a few empty launches: 8 per host read
        while int(self.wbuf["unfinished"].item()) > 0 and rounds < max_rounds:
            self.search_waves(net, sims, chunk, skip_roots=True)
            rounds += chunk
        return rounds

    def finish(self, temperatures: torch.Tensor, uniforms: Optional[torch.Tensor],
               target_temperatures: Optional[torch.Tensor] = None, prior_pseudocount: float = 0.0,
               force_uniform: Optional[torch.Tensor] = None, sample_moves: Optional[bool] = None,
               pruned: Optional[bool] = None) -> None:
        """`sample_moves` defaults to "sample iff uniforms are given".  `pruned`: go through lz_tree_finish_pruned (default:
        when forced playouts are on; with forced_k = 0 it writes what lz_tree_finish writes, `child_target_visits` =
        `child_visits` and `pruned_visits` = 0)."""
        sample = uniforms is not None if sample_moves is None else bool(sample_moves)
        if force_uniform is not None and force_uniform.dtype != torch.uint8:
            force_uniform = force_uniform.to(torch.uint8)
        # the arguments the three entry points share; each appends its own outputs and the stream
        head = (C.byref(self.desc), L.ptr(temperatures), L.ptr(target_temperatures), C.c_float(float(prior_pseudocount)),
                L.ptr(force_uniform), C.c_int(int(sample)), L.ptr(uniforms), L.ptr(self.policy_dense),
                L.ptr(self.chosen_index), L.ptr(self.chosen_code), L.ptr(self.chosen_valid), L.ptr(self.terminal_mask),
                L.ptr(self.root_value), L.ptr(self.child_count), L.ptr(self.child_action), L.ptr(self.child_visits),
                L.ptr(self.child_prior), L.i64(OUT_CAP))
        if self.gumbel_m > 0:               # Gumbel root search: the plain finish, then pick and target of the Gumbel games
            name, tail = "tree_finish_gumbel", (L.ptr(self.gumbel["score"]), L.ptr(self.gumbel["vmix"]))
        elif (self.forced_k > 0.0) if pruned is None else bool(pruned):   # policy target pruning: the same outputs + N' / the cut
            name, tail = "tree_finish_pruned", (L.ptr(self.child_target_visits), L.ptr(self.pruned_visits))
        else:
            name, tail = "tree_finish", ()
        with torch.cuda.device(self.device):
            L.check(getattr(L.lib(), "lz_" + name)(*head, *tail, self._stream()), name)

    def advance(self, played_action: Optional[torch.Tensor] = None, reset: Optional[torch.Tensor] = None,
                next_sims: Optional[int] = None) -> None:
        """Tree reuse (a21): promote the played child of every game to root, keeping its subtree.  Call after
        set_roots() with the post-move states; `played_action` int32[B] defaults to the last finish()'s picks."""
        pa = self.chosen_index if played_action is None else played_action.to(torch.int32).contiguous()
        if reset is not None and reset.dtype != torch.uint8:
            reset = reset.to(torch.uint8)
        sims = self.max_sims if next_sims is None else int(next_sims)
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_tree_advance(C.byref(self.desc), L.ptr(pa), L.ptr(reset), L.i64(sims),
                                            L.ptr(self.reuse_dropped[0:1]), L.ptr(self.reuse_dropped[1:2]),
                                            self._stream()), "tree_advance")

    def search(self, net: FusedNet, sims: int, noise: Optional[torch.Tensor] = None, epsilon: float = 0.25,
               continue_trees: bool = False, compact: Optional[bool] = None) -> None:
        """Whole search of one move (C++ loop: begin, root, sims x select/eval/expand); `continue_trees`: the
        trees were prepared by advance() (kept subtrees / fresh roots), no begin.  `compact` (engines built with
        `compact_evals`): False launches every slot of every simulation (cheaper while nearly all games are live: no scan
        kernel per simulation), True / None the compact lists; results are bit-identical either way."""
        if int(sims) > self.max_sims:
            raise ValueError(f"sims={sims} exceeds the arena capacity max_sims={self.max_sims}")
        if self.batch_k > 1:
            self.search_waves(net, sims, -(-int(sims) // self.batch_k), noise, epsilon, continue_trees)
            return
        nz_stride = int(noise.shape[1]) if noise is not None else 0
        if self.persistent_ok(net):
            # one launch per move: a workgroup owns 8 games, no kernel boundary between simulations (csrc/lz_search.hip)
            if self._cu_slots is None:
                self._cu_slots = torch.zeros((4096,), dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                rc = L.lib().lz_tree_search_persistent(
                    C.byref(self.desc), C.byref(net.desc), L.i64(sims), L.ptr(self.lp1), L.ptr(self.lp2), L.ptr(self.lpm),
                    L.ptr(self.values), L.ptr(noise), L.i64(nz_stride), C.c_float(float(epsilon)),
                    C.c_int(1 if continue_trees else 0), L.ptr(self._cu_slots), L.i64(self.stagger_us),
                    L.ptr(self.phase_ticks), self._stream())
            if rc in (-2, -3) and not torch.cuda.is_current_stream_capturing():
                # LZ_ERR_UNSUPPORTED / LZ_ERR_LAUNCH (e.g. the kernel's ~80 KB of dynamic LDS refused on this part): the
                # header promises the launch-pair search as the fallback -- nothing has run yet, so take it, for good
                print(f"[liuzhou_amd] persistent search kernel unavailable (status {rc}); using lz_tree_search", flush=True)
                self.persistent = False
            else:
                L.check(rc, "tree_search_persistent")
                return
        fn = L.lib().lz_tree_search_continue if continue_trees else L.lib().lz_tree_search
        use_lists = self.compact_evals and (compact is None or bool(compact) or self.kld_stop.on)
        desc = self.desc
        if self.compact_evals and not use_lists:                    # the same engine, dense launches for this move
            desc = LzTreeDesc()
            C.memmove(C.byref(desc), C.byref(self.desc), C.sizeof(LzTreeDesc))
            desc.live_state = desc.live_row = desc.live_count = None
            desc.live_count_cap = 0
        with torch.cuda.device(self.device):
            L.check(fn(C.byref(desc), C.byref(net.desc), L.i64(sims), L.ptr(self.planes),
                       L.ptr(self.lp1), L.ptr(self.lp2), L.ptr(self.lpm), L.ptr(self.values),
                       L.ptr(noise), L.i64(nz_stride), C.c_float(float(epsilon)), self._stream()),
                    "tree_search")
        if self.compact_evals:                                      # evaluations launched: the leaves the lists held / every slot
            if use_lists:
                self.live_total.add_(self.live["live_count"][: int(sims) + 1].sum())
            else:
                self.live_total.add_(self.B * (int(sims) + 1))

    def search_multi(self, nets, sims: int, noise: Optional[torch.Tensor] = None, epsilon: float = 0.25,
                     continue_trees: bool = False) -> None:
        """search() with one FusedNet per segment (lz_tree_search_multi): one network launch per simulation evaluates
        every segment's leaves with its own network; each tree is the one search() builds with that network."""
        if self.segment_games is None:
            raise ValueError("search_multi needs an engine built with segment_games")
        if len(nets) != self.num_segments:
            raise ValueError(f"{self.num_segments} segments need as many networks, got {len(nets)}")
        if int(sims) > self.max_sims:
            raise ValueError(f"sims={sims} exceeds the arena capacity max_sims={self.max_sims}")
        arr = nets if isinstance(nets, DescArray) else DescArray(nets)
        fn = L.lib().lz_tree_search_multi_continue if continue_trees else L.lib().lz_tree_search_multi
        nz_stride = int(noise.shape[1]) if noise is not None else 0
        with torch.cuda.device(self.device):
            L.check(fn(C.byref(self.desc), arr.arr, C.c_int32(len(arr)), L.i64(sims), L.ptr(self.lp1), L.ptr(self.lp2),
                       L.ptr(self.lpm), L.ptr(self.values), L.ptr(noise), L.i64(nz_stride), C.c_float(float(epsilon)),
                       self._stream()), "tree_search_multi")
        # evaluations launched: the rows of every segment, not the padding between them (live_count is the padded total)
        seg = self.seg_off[: (int(sims) + 1) * (len(arr) + 1)].view(int(sims) + 1, len(arr) + 1)
        start = torch.div(seg[:, :-1] + 15, 16, rounding_mode="floor") * 16
        self.live_total.add_((seg[:, 1:] - start).clamp_min(0).sum())

    def persistent_ok(self, net: FusedNet) -> bool:
        """Whether search() runs the one-launch-per-move kernel: 64-channel net in fp16 mode, not switched off
        (`persistent` attribute; env LZ_TREE_PERSISTENT=0)."""
        return (bool(self.persistent) and self.batch_k <= 1 and int(net.desc.channels) == 64 and not (int(net.desc.flags) & (4 | 8))
                and not self.compact_evals)

    def enable_phase_ticks(self) -> torch.Tensor:
        """Measurement aid: int64[workgroups, 4] = 100 MHz ticks each workgroup of the persistent search kernel spent in
        network passes / tree steps during the LAST search, its arrival slot on its CU and the CU key (must be enabled
        before the search is captured)."""
        n = int(L.lib().lz_tree_search_persistent_grid(L.i64(self.B)))
        self.phase_ticks = torch.zeros((n, 4), dtype=torch.int64, device=self.device)
        return self.phase_ticks


def persistent_search_available(net, batch_k: int = 1) -> bool:
    """Does the search of `net` run as the one-launch-per-move kernel (csrc/lz_search.hip; opt-in)?  Then one engine over
    all games already puts two workgroups on every CU, and the two-stream split (DualStreamTreeMCTS) has nothing to add."""
    if not _persistent_default():
        return False
    return isinstance(net, FusedNet) and int(batch_k) <= 1 and int(net.desc.channels) == 64 and not (int(net.desc.flags) & 4)


def dirichlet_noise(shape, alpha: float, device, generator=None) -> torch.Tensor:
    """Gamma(alpha) draws; the expand kernel mixes them with weight epsilon and renormalises the priors
    (the same distribution as Dirichlet noise after normalisation over the legal children)."""
    a = torch.full(shape, float(alpha), dtype=torch.float32, device=device)
    g = torch._standard_gamma(a) if generator is None else torch._standard_gamma(a, generator=generator)
    return g


class PriorEvaluator:
    """External evaluator of the split-phase protocol in the reference's own form (`PortableCppTreeBatch`:
    prepare roots -> evaluate -> complete(priors, values), v1/python/portable_cpp_mcts.py:270-282):
    `fn(planes float32[B,11,6,6], packed_states int64[B,4]) -> (priors float32[B,220], values float32[B])`, both on the
    engine's device; the priors are used as given (renormalised over the legal set by the expand kernel)."""

    def __init__(self, fn) -> None:
        self.fn = fn

    def __call__(self, planes: torch.Tensor, packed: torch.Tensor):
        return self.fn(planes, packed)


class PortableTreeMCTS:
    """Full-tree search with the V1RootMCTS calling convention (search_batch -> RootSearchBatchOutput)."""

    def __init__(self, net: FusedNet, num_games: int, num_simulations: int, device, exploration_weight: float = 1.0,
                 add_dirichlet_noise: bool = True, dirichlet_alpha: float = 0.3, dirichlet_epsilon: float = 0.25,
                 sample_moves: bool = True, use_graph: Optional[bool] = None, reuse_tree: bool = False,
                 reuse_factor: float = -1.0, policy_target_temperature: Optional[float] = None,
                 policy_target_prior_pseudocount: float = 0.0, batch_k: int = 1, seed: int = 12345,
                 game_offset: int = 0, game_stride: Optional[int] = None, trace: bool = False,
                 collect_timing: bool = False, compact_evals: Optional[bool] = None,
                 segment_games: Optional[int] = None, multi_launch: bool = True,
                 cpuct_table_len: int = CPUCT_TABLE_LEN, rules: Optional[SearchRules] = None, **rule_options) -> None:
        """`net` a list of K networks with `segment_games` (a multiple of 16, num_games = K * segment_games): slot g is
        searched with network g // segment_games, every segment in the same simulation steps (compact lists always on).
        FusedNets of one layout share one network launch per simulation (lz_tree_search_multi); any other mix runs the
        split-phase protocol, each segment's rows through its own evaluator.  Not with batch_k > 1, eval_symmetry or the
        persistent kernel.  `multi_launch=False` takes the split-phase path for FusedNets too (parity tests).  A single
        network behaves as below.
        `compact_evals` (fused network only): per simulation only the leaves that need the network are evaluated
        (`TreeEngine(compact_evals=True)`); True = in every search; None = the engine is built for both forms when a launch
        of all slots is at least two network passes per CU (C3: eight) and uses the lists for the searches that say so
        (`search_batch(compact=True)`, the runner's hint that the wave is draining) -- env LZ_TREE_COMPACT=0 / 1 overrides.
        `net`: a FusedNet (the production path: the whole search of a move is enqueued from C++ with the fused network
        kernel in the loop, one hipGraph per move), or any module returning `ChessNet.forward`'s 4-tuple -- then the search
        runs the split-phase protocol (select -> planes -> module -> expand) with that module as an external fp32
        evaluator, on its own device (the reference's `PortableMCTS` with an arbitrary model, portable_mcts.py:381-386).
        `seed` / `game_offset` / `game_stride`: keys of the per-game counter RNG (game_rng.GameRng) behind the root noise
        and the move sampling.  `trace`: record what every expand step consumed (TreeEngine.enable_trace; parity tests).
        `batch_k` > 1: the legacy search's waves (src/mcts.py `batch_K`, default 16 there): up to batch_k distinct
        leaves per game are collected, evaluated in one network launch of batch_k * B positions and backed up per wave.
        `reuse_tree`: keep the played child's subtree between consecutive search_batch calls on the same games
        (the reference's portable self-play does, v1/python/portable_self_play.py:191); the arenas then hold
        (1 + reuse_factor) * sims nodes per game (reuse_factor < 0: as much as a third of the free memory allows).  `policy_target_*`: portable_mcts.py:690-700.
        `rules` (a search_rules.SearchRules), or the same options under the constructor's own names in `rule_options`
        (`eval_symmetry`, `fast_simulations` / `full_prob`, `forced_playouts_k`, `gumbel_considered` / `gumbel_c_visit` /
        `gumbel_c_scale`, `solver`, `fpu_reduction` / `fpu_root_reduction` / `cpuct_log` / `cpuct_base`, `kld_stop` (a
        KldStop), `move_visit_offset` / `move_value_cutoff`): the optional rules of the search, described in
        search_rules; a configuration one of them cannot run in is a ValueError before anything is allocated.  What they
        leave on the engine: `full_search` (uint8[B], the playout cap's mask of the last search) and `cap_counts`,
        `sim_budget` / `last_sim_budget` (int32[B], refilled before every search by the cap's draw or with
        `num_simulations`, lowered by the KLD-gain rule), `forced_counts`, `gumbel_searches`, `solver_counts`,
        `kld_counts`, `move_pick_counts`; parity runs inject their own draws through `injected_full_search`,
        `injected_sim_budget` (honoured after the cap's draw) and `injected_gumbel` ([B, <= OUT_CAP])."""
        search_simulations(num_simulations)
        self.nets = list(net) if isinstance(net, (list, tuple)) else [net]
        self.multi = segment_games is not None
        if rules is not None and rule_options:
            raise TypeError(f"pass `rules` or the options by name, not both: {sorted(rule_options)}")
        self.rules = r = SearchRules.parse_engine(num_simulations, **rule_options) if rules is None else rules
        self.fused_multi = self.multi and bool(multi_launch) and multi_compatible(self.nets)
        self.fused = isinstance(self.nets[0], FusedNet) and (not self.multi or self.fused_multi)
        r.refuse(batch_k=batch_k, several_networks=self.multi or len(self.nets) != 1, fused=self.fused,
                 persistent=_persistent_default(), sample_moves=sample_moves,
                 policy_target_temperature=policy_target_temperature,
                 policy_target_prior_pseudocount=policy_target_prior_pseudocount)
        self.cap, self.forced, self.gumbel, self.solver = r.cap, r.forced, r.gumbel, r.solver
        self.kld_stop, self.kld, self.move_pick, self.puct_shape = r.kld, r.kld_on, r.repick, r.shape
        if not self.multi and len(self.nets) != 1:
            raise ValueError("several networks need segment_games")
        if self.multi:
            if len(self.nets) * int(segment_games) != int(num_games):
                raise ValueError(f"{len(self.nets)} networks x segment_games={segment_games} != num_games={num_games}")
            if int(batch_k) > 1 or r.symmetric:
                raise ValueError("several networks in one search: batch_k = 1 and eval_symmetry='none' only")
            if sum(isinstance(n, PriorEvaluator) for n in self.nets) not in (0, len(self.nets)):
                raise ValueError("PriorEvaluators and networks cannot share one search")
            compact_evals = True
        net = self.nets[0]
        self.net, self.sims = net, int(num_simulations)
        self._desc_array = DescArray(self.nets) if self.fused_multi else None
        self.reuse_tree = bool(reuse_tree)
        self.batch_k = max(1, int(batch_k))
        env_c = os.environ.get("LZ_TREE_COMPACT", "").strip()
        if env_c in ("0", "1") and not self.multi:
            compact_evals = env_c == "1"
        # asked for explicitly: every search uses the lists.  Chosen automatically: the engine can do both and launches
        # every slot unless a search is told otherwise (`compact=` of search_batch: the runner's hint that the wave is
        # draining) -- while nearly all games are live the lists shorten nothing and cost a scan kernel per simulation
        # (a search that shares transposed leaves takes them out of the lists, so it uses the lists throughout)
        self.compact_default = compact_evals is True
        if compact_evals is None:
            compact_evals = self.fused and int(num_games) >= 2 * samples_per_launch_pass(net)
            self.compact_default = compact_evals and self.batch_k == 1 and shares_leaves(num_games)
        if self.cap or self.kld:     # a dense launch would evaluate every slot at every simulation, stopped games included
            compact_evals = self.compact_default = True
        self.engine = TreeEngine(num_games, num_simulations, device, exploration_weight,
                                 reuse_factor=float(reuse_factor) if self.reuse_tree else 0.0, batch_k=self.batch_k,
                                 compact_evals=bool(compact_evals) and self.fused and self.batch_k == 1,
                                 segment_games=segment_games if self.fused_multi else None)
        if trace:
            self.engine.enable_trace()
        if self.forced:
            self.engine.set_forced_playouts(r.forced_k)
        self._pruned_total = torch.zeros((1,), dtype=torch.int64, device=self.engine.device)   # sum of pruned_visits
        self.injected_gumbel: Optional[torch.Tensor] = None      # parity runs: [B, <= OUT_CAP] instead of the RNG's draws
        if self.gumbel:
            self.engine.set_gumbel(r.gumbel_considered, r.gumbel_c_visit, r.gumbel_c_scale, int(num_simulations))
        self._roots_decided = torch.zeros((1,), dtype=torch.int64, device=self.engine.device)
        if self.solver:
            self.engine.set_solver(True)
        # visit-offset / value-cutoff move selection: the counter block exists only when the rule is on
        self._move_pick_counts = (torch.zeros((4,), dtype=torch.int64, device=self.engine.device)
                                  if self.move_pick else None)
        if self.puct_shape.on:
            self.engine.set_puct_shape(**self.puct_shape.kwargs(), table_len=int(cpuct_table_len))
        if not self.fused:
            if self.batch_k > 1:
                raise ValueError("an external evaluator supports batch_k = 1 only")
            self._eval_devices = [None if isinstance(n, PriorEvaluator) else
                                  (n.device if isinstance(n, FusedNet) else next(n.parameters()).device) for n in self.nets]
            self._eval_device = self._eval_devices[0]
        self.rng = GameRng(num_games, device, seed=seed, game_offset=game_offset, game_stride=game_stride)
        self.eval_symmetry = r.eval_symmetry
        self.engine.set_eval_symmetry(self.eval_symmetry, seed, self.rng.game, self.rng.ply)
        self._game0 = self.rng.game.clone()
        self._uniforms = torch.zeros((self.engine.B,), dtype=torch.float32, device=self.engine.device)
        self.injected_noise: Optional[torch.Tensor] = None       # parity runs: [B, <= OUT_CAP] instead of the RNG's draws
        self.injected_uniforms: Optional[torch.Tensor] = None
        self._evals_dev = torch.zeros((1,), dtype=torch.int64, device=self.engine.device)
        self.extra_rounds = 0
        self.graph_retry_off = False                             # a failed graph capture made this engine launch directly
        self._collect_timing = bool(collect_timing)
        self._timing_events = []
        self._timing_ms: Dict[str, float] = {}
        self._timing_calls: Dict[str, int] = {}
        self.target_temperature = None if policy_target_temperature is None else float(policy_target_temperature)
        self.prior_pseudocount = float(policy_target_prior_pseudocount)
        self._have_trees = False
        self.add_noise, self.alpha, self.eps = bool(add_dirichlet_noise), float(dirichlet_alpha), float(dirichlet_epsilon)
        self.sample_moves = bool(sample_moves)
        self._root_evals = 0
        # hipGraph: the whole search of a move (1 + sims) x (select, fused net, expand) is captured once and
        # replayed every move; all buffers are static, noise / roots are refreshed in place before the replay.
        if use_graph is None:
            use_graph = os.environ.get("LZ_TREE_GRAPH", "on").strip().lower() not in ("off", "0", "false")
        self.use_graph = bool(use_graph)
        self._graphs = {}
        self._tail_graph = None
        self._tail_rounds = 0
        self._noise_buf = torch.zeros((self.engine.B, OUT_CAP), dtype=torch.float32, device=self.engine.device)
        # playout cap: per-game budget / root noise switch of the next search, filled on the device before every launch
        self.injected_full_search: Optional[torch.Tensor] = None   # parity runs: bool[B] instead of the RNG's draws
        self.cap_counts = torch.zeros((2,), dtype=torch.int64, device=self.engine.device)   # full / fast searches of live games
        # KLD-gain early stopping: the same budget array (the rule lowers what the cap's draw, or `sims`, put there)
        self.injected_sim_budget: Optional[torch.Tensor] = None    # parity runs: int32[B] instead of the draw / `sims`
        self.full_search: Optional[torch.Tensor] = None
        if self.cap or self.kld:
            z = lambda dt: torch.zeros((self.engine.B,), dtype=dt, device=self.engine.device)
            self.sim_budget = z(torch.int32)
            if self.cap:
                self._cap_u = z(torch.float32)
                self.bind_full_search(z(torch.uint8))
            else:
                self.engine.set_playout_cap(self.sim_budget, None)
            if self.kld:
                self.engine.set_kld_stop(self.kld_stop, trace=bool(trace))

    def bind_full_search(self, buf: torch.Tensor) -> None:
        """Use `buf` (uint8[B], contiguous; DualStreamTreeMCTS hands each part a slice of one mask) as the full / fast mask
        of the playout cap, which the searches also read as their root noise switch.  Before the first search."""
        self.full_search = buf
        self.engine.set_playout_cap(self.sim_budget, buf)

    def bind_sim_budget(self, buf: torch.Tensor) -> None:
        """Use `buf` (int32[B], contiguous; DualStreamTreeMCTS hands each part a slice of one array) as the per-game budget
        of the playout cap and of KLD-gain early stopping.  Before the first search."""
        self.sim_budget = buf
        self.engine.set_playout_cap(buf, self.full_search if self.cap else None)

    @property
    def last_sim_budget(self) -> Optional[torch.Tensor]:
        """int32[B]: every game's budget as the last search left it (None: neither the cap nor the KLD-gain rule is on)."""
        return self.sim_budget if (self.cap or self.kld) else None

    @property
    def kld_counts(self) -> torch.Tensor:
        """int64[2] on the device: searches the KLD-gain rule stopped and the simulations they did not run, so far (zeros
        when off)."""
        if not self.kld:
            return torch.zeros((2,), dtype=torch.int64, device=self.engine.device)
        k = self.engine.kld
        return torch.stack((k["stops"].sum(), k["saved"].sum()))

    def _reset_kld_counts(self) -> None:
        if self.kld:
            self.engine.kld["stops"].zero_(); self.engine.kld["saved"].zero_()

    def _fill_sim_budget(self) -> None:
        """Budgets of a search without the cap's draw (KLD-gain early stopping alone): `sims` for every game, or the
        injected ones.  On the device, outside the captured search."""
        if self.injected_sim_budget is not None:
            self.sim_budget.copy_(self.injected_sim_budget.to(device=self.engine.device, dtype=torch.int32))
        else:
            self.sim_budget.fill_(self.sims)

    @property
    def last_full_search(self) -> Optional[torch.Tensor]:
        """bool[B]: which games' last search was full (None: the playout cap is off)."""
        return self.full_search.bool() if self.cap else None

    @property
    def forced_counts(self) -> torch.Tensor:
        """int64[2] on the device: forced descents and pruned visits of the searches so far (zeros when off)."""
        return torch.cat((self.engine.forced_count.sum(dtype=torch.int64).view(1), self._pruned_total))

    @property
    def solver_counts(self) -> torch.Tensor:
        """int64[3] on the device: proofs (edges and roots the expand step decided), searches that ended with a decided
        root, and picks the solver changed, so far (zeros when off)."""
        if not self.solver:
            return torch.zeros((3,), dtype=torch.int64, device=self.engine.device)
        e = self.engine
        return torch.cat((e.solver_count.sum(dtype=torch.int64).view(1), self._roots_decided,
                          e.solver_overrides.sum(dtype=torch.int64).view(1)))

    @property
    def move_pick_counts(self) -> torch.Tensor:
        """int64[4] on the device: games the move re-pick applied to, children cut by the visit offset, children cut by the
        value cutoff and picks that differ from the finish's, so far (zeros when off)."""
        if not self.move_pick:
            return torch.zeros((4,), dtype=torch.int64, device=self.engine.device)
        return self._move_pick_counts

    def _reset_move_pick_counts(self) -> None:
        if self.move_pick:
            self._move_pick_counts.zero_()

    def _reset_solver_counts(self) -> None:
        self._roots_decided.zero_()
        if self.solver:
            self.engine.solver_count.zero_(); self.engine.solver_overrides.zero_()

    @property
    def gumbel_searches(self) -> torch.Tensor:
        """int64[1] on the device: searches of live games that ran the Gumbel rule so far (zero when off)."""
        if not self.gumbel:
            return torch.zeros((1,), dtype=torch.int64, device=self.engine.device)
        return self.engine.gumbel["count"].sum(dtype=torch.int64).view(1)

    def _draw_playout_cap(self, active: Optional[torch.Tensor]) -> None:
        """Full / fast mask of this move on the device (no host synchronisation): u = uniform(seed, game, ply, purpose 3),
        full iff u < full_prob (compared in double precision); budgets and root noise switch from it."""
        if self.injected_full_search is not None:
            full = self.injected_full_search.to(device=self.engine.device, dtype=torch.bool)
        else:
            self.rng.uniform_into(self._cap_u, PURPOSE_PLAYOUT_CAP)
            full = self._cap_u.double() < self.rules.cap_full_prob
        self.full_search.copy_(full)
        self.sim_budget.copy_(torch.where(full, self.sims, self.rules.cap_fast_simulations))
        if self.injected_sim_budget is not None:
            self.sim_budget.copy_(self.injected_sim_budget.to(device=self.engine.device, dtype=torch.int32))
        live = torch.ones_like(full) if active is None else active.to(device=full.device, dtype=torch.bool)
        self.cap_counts.add_(torch.stack(((full & live).sum(), (~full & live).sum())))

    # ---- tracing: roctx ranges (torch.cuda.nvtx is roctx on ROCm) + HIP-event timing buckets, as the reference's
    # V1RootMCTS._nvtx_range / _timed (v1/python/mcts_gpu.py:565-602); bucket names follow its runner
    # (self_play_gpu_runner.py:276-281): root_puct_ms = the search, pack_writeback_ms = policy / pick extraction ----
    @contextmanager
    def _timed(self, name: str):
        torch.cuda.nvtx.range_push(f"lz.tree.{name}")
        if not self._collect_timing:
            try:
                yield
            finally:
                torch.cuda.nvtx.range_pop()
            return
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream(self.engine.device))
        try:
            yield
        finally:
            b.record(torch.cuda.current_stream(self.engine.device))
            self._timing_events.append((name, a, b))
            torch.cuda.nvtx.range_pop()

    def get_timing(self, reset: bool = False) -> Dict[str, Dict[str, float]]:
        """{"timing_ms": {...}, "timing_calls": {...}} like V1RootMCTS.get_timing (one device synchronisation)."""
        if self._timing_events:
            torch.cuda.synchronize(self.engine.device)
            for name, a, b in self._timing_events:
                self._timing_ms[name] = self._timing_ms.get(name, 0.0) + float(a.elapsed_time(b))
                self._timing_calls[name] = self._timing_calls.get(name, 0) + 1
            self._timing_events = []
        out = {"timing_ms": dict(self._timing_ms), "timing_calls": dict(self._timing_calls)}
        if reset:
            self._timing_ms, self._timing_calls = {}, {}
        return out

    def _evaluate_external(self, planes: torch.Tensor, net=None, eval_device=None):
        """External fp32 evaluator: module(planes) -> (log_p1, log_p2, log_pmc, value_logits); scalar value = bucket
        expectation (src/neural_network.py:201-210), everything back on the engine's device."""
        dev = self.engine.device
        net = self.net if net is None else net
        eval_device = self._eval_device if eval_device is None else eval_device
        with torch.inference_mode():
            lp1, lp2, lpm, raw = net(planes.to(eval_device))
            if raw.dim() == 2 and int(raw.shape[1]) == 1:          # a scalar value head (portable_mcts.py:374-375)
                val = raw[:, 0].float()
            else:
                probs = torch.softmax(raw.float(), dim=-1)
                centers = torch.linspace(-1.0, 1.0, steps=raw.shape[-1], dtype=probs.dtype, device=probs.device)
                val = (probs * centers).sum(-1)
        f = lambda t: t.float().to(dev).contiguous()
        return f(lp1), f(lp2), f(lpm), f(val)

    def _search_split(self, noise: Optional[torch.Tensor], continue_trees: bool) -> None:
        e = self.engine
        if not continue_trees:
            e.begin()
        for s in range(self.sims + 1):
            if s > 0:
                e.select()
            if self.multi:
                self._expand_segments(s, noise)
                continue
            if isinstance(self.net, PriorEvaluator):
                pri, val = self.net(e.leaf_planes(), e.buf["leaf_state"])
                e.expand(is_root=(s == 0), values=val.to(torch.float32).contiguous(),
                         priors220=pri.to(torch.float32).contiguous(), noise=noise if s == 0 else None, epsilon=self.eps)
                continue
            lp1, lp2, lpm, val = self._evaluate_external(e.leaf_planes())
            e.expand(is_root=(s == 0), values=val, heads=(lp1, lp2, lpm), noise=noise if s == 0 else None,
                     epsilon=self.eps)

    def _expand_segments(self, s: int, noise: Optional[torch.Tensor]) -> None:
        """Split-phase step with one evaluator per segment: segment k's leaves that need the network (leaf_kind 1: not
        inactive slots, terminal leaves) go to network k, as the compact lists of the fused path; the other rows are
        never read by the expand step and stay zero."""
        e = self.engine
        planes = e.leaf_planes()
        G = e.B // len(self.nets)
        need = e.buf["leaf_kind"] == 1
        prior_mode = isinstance(self.nets[0], PriorEvaluator)
        if prior_mode:
            pri = torch.zeros((e.B, TOTAL_ACTION_DIM), dtype=torch.float32, device=e.device)
        heads = [torch.zeros((e.B, 36), dtype=torch.float32, device=e.device) for _ in range(3)]
        val = torch.zeros((e.B,), dtype=torch.float32, device=e.device)
        for k, n in enumerate(self.nets):
            rows = torch.nonzero(need[k * G:(k + 1) * G]).view(-1) + k * G
            if int(rows.numel()) == 0:
                continue
            if prior_mode:
                p, v = n(planes.index_select(0, rows), e.buf["leaf_state"].index_select(0, rows))
                pri.index_copy_(0, rows, p.to(torch.float32))
                val.index_copy_(0, rows, v.to(torch.float32).view(-1))
                continue
            if isinstance(n, FusedNet):                            # the fused search's own input: packed leaves
                lp1, lp2, lpm, _, v = n.forward_packed(e.buf["leaf_state"].index_select(0, rows))
            else:
                lp1, lp2, lpm, v = self._evaluate_external(planes.index_select(0, rows), n, self._eval_devices[k])
            for h, x in zip(heads, (lp1, lp2, lpm)):
                h.index_copy_(0, rows, x.reshape(-1, 36))
            val.index_copy_(0, rows, v.view(-1))
        if prior_mode:
            e.expand(is_root=(s == 0), values=val, priors220=pri, noise=noise if s == 0 else None, epsilon=self.eps)
        else:
            e.expand(is_root=(s == 0), values=val, heads=tuple(heads), noise=noise if s == 0 else None, epsilon=self.eps)

    def _run_search(self, sims: int, noise, continue_trees: bool, lists: bool) -> None:
        if self.fused_multi:
            self.engine.search_multi(self._desc_array, sims, noise, self.eps, continue_trees)
        else:
            self.engine.search(self.net, sims, noise, self.eps, continue_trees, compact=lists)

    def _search(self, add_noise: bool, continue_trees: bool) -> None:
        e = self.engine
        noise = self._noise_buf if add_noise else None
        if not self.fused:
            self._search_split(noise, continue_trees)
            return
        lists = bool(getattr(self, "compact_now", self.compact_default)) and e.compact_evals
        self.list_searches = getattr(self, "list_searches", 0) + int(lists)      # searches that used the compact lists
        self.last_search_lists = lists
        if not self.use_graph:
            self._run_search(self.sims, noise, continue_trees, lists)
            return
        key = (add_noise, continue_trees, lists)
        g = self._graphs.get(key)
        if g is None:
            self.captures = getattr(self, "captures", 0) + 1        # this search synchronises the host (warm-up, capture)
            if not continue_trees:
                # warm-up launch outside capture: every kernel of the search must be loaded before a stream capture
                # starts.  Two simulations reach all of them (root expand + select, expand + select, last expand), and a
                # fresh search starts by resetting the trees, so what the warm-up leaves behind does not matter -- a full
                # search here cost 1.6 s per engine at C3.  A continued search must run exactly once and is only reached
                # after a fresh one
                # (an engine with compact lists warms up both launch forms: the other one may be captured later inside a
                #  continued search, which cannot be preceded by a warm-up of its own)
                counted = (e.live_total.clone(), e.eval_count.clone(), e.share_count.clone())   # warm-ups are not searches
                forced_counted = e.forced_count.clone() if self.forced else None
                gumbel_counted = e.gumbel["count"].clone() if self.gumbel else None
                solver_counted = e.solver_count.clone() if self.solver else None
                for form in ((lists, not lists) if (e.compact_evals and not self.fused_multi) else (lists,)):
                    self._run_search(min(self.sims, 2), noise, False, form)
                e.live_total.copy_(counted[0]); e.eval_count.copy_(counted[1]); e.share_count.copy_(counted[2])
                if forced_counted is not None:
                    e.forced_count.copy_(forced_counted)
                if gumbel_counted is not None:
                    e.gumbel["count"].copy_(gumbel_counted)
                if solver_counted is not None:
                    e.solver_count.copy_(solver_counted)
            torch.cuda.synchronize(e.device)
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
                    self._run_search(self.sims, noise, continue_trees, lists)
                if os.environ.get("LZ_TREE_GRAPH_FAULT", "") == "capture":      # test hook: pretend the capture failed
                    raise RuntimeError("injected stream capture failure (LZ_TREE_GRAPH_FAULT=capture)")
            except RuntimeError as exc:
                # Capture failed (the reference's worker retries a failed finalize-graph capture once with the graph off,
                # v1/python/self_play_worker.py:24-30,434-442): nothing of the captured search has run, so the same search
                # is launched directly, and this engine stays on direct launches.  Recorded in the manifest.
                torch.cuda.synchronize(e.device)
                self.use_graph = False
                self.graph_retry_off = True
                self._graphs.clear()
                print(f"[liuzhou_amd] hipGraph capture of the tree search failed ({exc!r}); falling back to direct launches",
                      flush=True)
                self._run_search(self.sims, noise, continue_trees, lists)
                return
            self._graphs[key] = g
        g.replay()

    @property
    def leaf_evals(self) -> int:
        """Network evaluations so far (batch_k > 1: one host read of the device-side counters)."""
        if self.engine.compact_evals:
            return int(self.engine.live_total.item())
        n = self._root_evals
        if self.batch_k > 1:
            n += int(self.engine.wbuf["eval_total"].item()) + int(self.engine.wbuf["eval_count"].item())
        return n

    @property
    def consumed_evals(self) -> int:
        """Evaluations the searches actually consumed (expanded leaves and fresh roots): `leaf_evals` minus terminal
        leaves, inactive slots and the unused evaluation of kept roots.  One host read."""
        return int(self.engine.eval_count.sum(dtype=torch.int64).item())

    def _finish_waves(self) -> None:
        """batch_k > 1: games whose waves found fewer open leaves than batch_k still have budget (narrow trees)."""
        if self.batch_k <= 1:
            return
        e = self.engine
        while self.tail_step():
            pass

    def tail_step(self) -> bool:
        """One host read of `unfinished` (waits for this engine's stream only) and, if some game still has budget, 8
        more rounds replayed as one graph (the leftover rounds are a handful of games with tiny network batches).
        Returns whether rounds were launched -- several engines on several streams take turns calling this."""
        e = self.engine
        if self.batch_k <= 1 or int(e.wbuf["unfinished"].item()) == 0 or self._tail_rounds >= 4096:
            self._tail_rounds = 0
            return False
        if not self.use_graph:
            e.search_waves(self.net, self.sims, 8, skip_roots=True)
        else:
            if self._tail_graph is None:
                torch.cuda.synchronize(e.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
                    e.search_waves(self.net, self.sims, 8, skip_roots=True)
                self._tail_graph = g
            self._tail_graph.replay()
        self._tail_rounds += 8
        self.extra_rounds += 8
        return True

    def reset_trees(self) -> None:
        """Forget the kept subtrees: the next search_batch starts every game from a fresh root."""
        self._have_trees = False

    def reset_run(self, seed: int) -> None:
        """A cached engine starts another run (self_play_tree_gpu called again with the same network and shape): fresh
        trees, RNG keys and counters as after construction; arenas, descriptors and captured graphs are kept."""
        self._have_trees = False
        self.rng.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.rng.game.copy_(self._game0)
        self.rng.ply.zero_()
        if self.eval_symmetry != "none":
            self.engine.buf["sym_salt"].fill_(int(seed) * 0x9E3779B1 & 0x7FFFFFFF)
        self._root_evals = 0
        self.extra_rounds = 0
        self.engine.eval_count.zero_()
        self.engine.share_count.zero_()
        self.engine.live_total.zero_()
        self.engine.reuse_dropped.zero_()
        self.cap_counts.zero_()
        self.engine.forced_count.zero_(); self._pruned_total.zero_()
        if self.gumbel:
            self.engine.gumbel["count"].zero_()
        self._reset_solver_counts()
        self._reset_kld_counts()
        self._reset_move_pick_counts()
        # refused expansions / fewest free chunks are per run too (a cached engine must not report an earlier run's)
        # (pool_stats[2], the chunks reserved for fresh roots, follows the trees' state and is NOT a per-run statistic)
        self.engine.buf["pool_stats"][:2].copy_(torch.tensor([0, self.engine.pool_chunks], dtype=torch.int32))
        self.get_timing(reset=True)
        if self.batch_k > 1:
            self.engine.wbuf["eval_total"].zero_(); self.engine.wbuf["eval_count"].zero_()

    def prepare(self, state: GpuStateBatch) -> None:
        """Set-up outside any timed region: load every kernel and capture the graphs (a fresh search, and a continued
        one with subtree reuse) by searching `state` once or twice; the trees built here are thrown away."""
        temps = torch.ones((self.engine.B,), dtype=torch.float32, device=self.engine.device)
        game0 = self.rng.game.clone()
        for _ in range(2 if self.reuse_tree else 1):
            self.search_batch(state, temperatures=temps)
        self.rng.game.copy_(game0)
        self.rng.ply.zero_()
        self._have_trees = False
        self._root_evals = 0
        self.extra_rounds = 0
        self.engine.eval_count.zero_()
        self.engine.share_count.zero_()
        self.engine.live_total.zero_()
        self.cap_counts.zero_()
        self.engine.forced_count.zero_(); self._pruned_total.zero_()
        if self.gumbel:
            self.engine.gumbel["count"].zero_()
        self._reset_solver_counts()
        self._reset_kld_counts()
        self._reset_move_pick_counts()
        self.get_timing(reset=True)
        if self.batch_k > 1:
            self.engine.wbuf["eval_total"].zero_(); self.engine.wbuf["eval_count"].zero_()

    def search_batch(self, state: GpuStateBatch, *, temperatures: torch.Tensor, active: Optional[torch.Tensor] = None,
                     add_dirichlet_noise: Optional[bool] = None, reset: Optional[torch.Tensor] = None,
                     played_action: Optional[torch.Tensor] = None,
                     force_uniform_random_mask: Optional[torch.Tensor] = None,
                     rng_game_ids: Optional[torch.Tensor] = None,
                     rng_plies: Optional[torch.Tensor] = None, compact: Optional[bool] = None) -> RootSearchBatchOutput:
        """`compact`: see `launch_search`.
        `state`: the games' current positions.  With `reuse_tree`, games whose position is the child reached by
        `played_action` (default: the move this engine picked last time) keep that child's subtree; `reset` marks
        games that were re-seated.  Anything that does not match simply starts a fresh tree.  `rng_game_ids` /
        `rng_plies` int64[B]: the runner's own game numbering and ply counters as RNG keys (default: slot-derived ids
        that advance on `reset`, plies counted per search)."""
        self.launch_search(state, active=active, add_dirichlet_noise=add_dirichlet_noise, reset=reset,
                           played_action=played_action, rng_game_ids=rng_game_ids, rng_plies=rng_plies, compact=compact)
        return self.complete_search(state, temperatures=temperatures,
                                    force_uniform_random_mask=force_uniform_random_mask)

    def launch_search(self, state: GpuStateBatch, *, active: Optional[torch.Tensor] = None,
                      add_dirichlet_noise: Optional[bool] = None, reset: Optional[torch.Tensor] = None,
                      played_action: Optional[torch.Tensor] = None, rng_game_ids: Optional[torch.Tensor] = None,
                      rng_plies: Optional[torch.Tensor] = None, compact: Optional[bool] = None) -> None:
        """First half of search_batch: everything up to the end of the captured search, nothing that waits for the
        device (so that several engines on several streams can be launched back to back)."""
        e = self.engine
        # compact lists or dense launches for this move (engines built with compact_evals; the runner passes a hint from
        # the number of live games: the lists pay once a launch gets at least one network pass per CU shorter)
        self.compact_now = self.compact_default if (compact is None or self.cap or self.kld) else bool(compact)
        add_noise = self.add_noise if add_dirichlet_noise is None else bool(add_dirichlet_noise)
        if self.gumbel:
            add_noise = False             # the Gumbel variates are the exploration: no Dirichlet mix, no noise draws
        e.set_roots(state, active)
        continue_trees = self.reuse_tree and self._have_trees
        self.rng.begin_move(reset if self._have_trees else None, rng_game_ids, rng_plies)
        self._explicit_plies = rng_plies is not None
        if self.cap:
            self._draw_playout_cap(active)
        elif self.kld:
            self._fill_sim_budget()
        with self._timed("root_puct_ms"):
            if continue_trees:
                e.advance(played_action, reset, self.sims)
            if add_noise:
                if self.injected_noise is not None:
                    self._noise_buf.zero_()
                    self._noise_buf[:, : int(self.injected_noise.shape[1])].copy_(self.injected_noise.to(torch.float32))
                else:
                    self.rng.gamma_into(self._noise_buf, self.alpha, MAX_CHILDREN)
            if self.gumbel:               # refreshed in place: the captured graph reads this buffer at every replay
                gbuf = e.gumbel["g"]
                if self.injected_gumbel is not None:
                    gbuf.zero_()
                    gbuf[:, : int(self.injected_gumbel.shape[1])].copy_(self.injected_gumbel.to(torch.float32))
                else:
                    self.rng.gumbel_into(gbuf, MAX_CHILDREN)
            self._search(add_noise, continue_trees)
        self._have_trees = True

    def complete_search(self, state: GpuStateBatch, *, temperatures: torch.Tensor,
                        force_uniform_random_mask: Optional[torch.Tensor] = None,
                        tails_done: bool = False) -> RootSearchBatchOutput:
        """Second half: leftover waves (batch_k > 1, host reads), policy / pick extraction, output record."""
        e = self.engine
        dev = e.device
        if self.batch_k > 1:
            if not tails_done:
                self._finish_waves()
            self._root_evals += e.B                                   # wave evaluations are counted on the device
        else:
            self._root_evals += e.B * (self.sims + 1)
        need_u = self.sample_moves or force_uniform_random_mask is not None
        uniforms = None
        with self._timed("pack_writeback_ms"):
            if need_u:
                uniforms = self._uniforms
                if self.injected_uniforms is not None:
                    uniforms.copy_(self.injected_uniforms.to(torch.float32))
                else:
                    self.rng.uniform_into(uniforms, PURPOSE_PICK)
            self.rng.end_move(getattr(self, "_explicit_plies", False))
            temps = temperatures.to(torch.float32).contiguous()
            tt = None if self.target_temperature is None else torch.full_like(temps, self.target_temperature)
            e.finish(temps, uniforms, tt, self.prior_pseudocount, force_uniform_random_mask, self.sample_moves)
            if self.forced:
                self._pruned_total.add_(e.pruned_visits.sum(dtype=torch.int64))
            if self.move_pick:            # re-pick of the sampled moves; in front of the solver, which keeps the last word
                e.move_pick(temps, uniforms, self.rules.move_visit_offset, self.rules.move_value_cutoff, force_uniform_random_mask,
                            self.sample_moves, self._move_pick_counts)
            if self.solver:               # a proven win is played, a proven loss is not while another move exists
                e.solver_pick(force_uniform_random_mask)
                self._roots_decided.add_((e.root_proven != 0).sum(dtype=torch.int64))
            model_input = states_to_model_input(state)
            legal_mask, _ = encode_actions_fast(state)
        return RootSearchBatchOutput(
            model_input=model_input, legal_mask=legal_mask, policy_dense=e.policy_dense, root_value=e.root_value,
            terminal_mask=e.terminal_mask, chosen_action_indices=e.chosen_index.to(torch.int64),
            chosen_action_codes=e.chosen_code, chosen_valid_mask=e.chosen_valid,
            **({"root_proven": e.root_proven} if self.solver else {}))


class DualStreamTreeMCTS:
    """Two half-size searches on two HIP streams, same interface as PortableTreeMCTS.

    Within one game the simulation chain (select -> evaluate -> expand) is strictly sequential, and the tree kernel
    is latency-bound: while it runs, the matrix pipes idle.  With the games split in two halves, each with its own
    engine, hipGraph and stream, one half's tree kernel overlaps the other half's network kernel.  The network runs
    4-wave workgroups of 8 samples (two per CU, `FusedNet(half_workgroups=True)`), so that a half batch alone still
    covers every CU.  Results are identical to one engine over all games (games are independent)."""

    SUMMED = ("leaf_evals", "consumed_evals", "cap_counts", "gumbel_searches", "forced_counts", "solver_counts",
              "kld_counts", "move_pick_counts")

    def __init__(self, model, num_games: int, num_simulations: int, device, num_parts: Optional[int] = None, **kw) -> None:
        search_simulations(num_simulations)
        dev = torch.device(device)
        self.B = int(num_games)
        k = 2 if num_parts is None else int(num_parts)      # 3 and 4 parts measured 34 % slower than 2 on C2
        k = max(1, min(k, self.B))
        base_n, extra = divmod(self.B, k)
        sizes = [base_n + (1 if i < extra else 0) for i in range(k)]
        self.bounds = []
        start = 0
        for n in sizes:
            self.bounds.append((start, start + n))
            start += n
        self.device = dev
        from .streams import overlapping_streams
        self.streams = overlapping_streams(dev, k)              # probed: two new streams CAN share a hardware queue
        self._pair_mode = overlapping_streams.last_mode
        self.parts = []
        base = model if isinstance(model, FusedNet) else FusedNet(model, dev)
        kw.pop("game_offset", None); kw.pop("game_stride", None)
        # one arena factor for the whole batch: sized per part, the first part would take its share of the free memory
        # and the next one a share of what is left -- unequal arenas, unequal subtree-drop rates
        if kw.get("reuse_tree", False) and float(kw.get("reuse_factor", -1.0)) < 0:
            kw["reuse_factor"] = auto_reuse_factor(self.B, int(num_simulations), dev)
        for (a, _b), n in zip(self.bounds, sizes):
            # waves of batch_k leaves are large launches: full 8-wave workgroups (they fill the chip on their own)
            half = int(kw.get("batch_k", 1)) <= 1
            # global game ids: slot a + g of the whole batch, so that a game's RNG stream does not depend on the split
            self.parts.append(PortableTreeMCTS(base.variant(half_workgroups=half), n, num_simulations, dev,
                                               game_offset=a, game_stride=self.B, **kw))
        self.sims = int(num_simulations)
        first = self.parts[0]
        self.rules, self.cap, self.forced, self.gumbel, self.solver = first.rules, first.cap, first.forced, first.gumbel, first.solver
        self.kld, self.kld_stop, self.move_pick, self.puct_shape = first.kld, first.kld_stop, first.move_pick, first.puct_shape
        # playout cap: one full / fast mask over all games, each part writing its slice (the wave tail reads the whole)
        self.full_search = None
        if self.cap:
            self.full_search = torch.zeros((self.B,), dtype=torch.uint8, device=dev)
            for (a, b), part in zip(self.bounds, self.parts):
                part.bind_full_search(self.full_search[a:b])
        # KLD-gain early stopping: likewise one budget array over all games, each part refilling and lowering its slice
        self.sim_budget = None
        self.injected_sim_budget: Optional[torch.Tensor] = None    # parity runs: int32[B], cut for the parts at every search
        if self.kld:
            self.sim_budget = torch.zeros((self.B,), dtype=torch.int32, device=dev)
            for (a, b), part in zip(self.bounds, self.parts):
                part.bind_sim_budget(self.sim_budget[a:b])
        self.serialize = False        # measurement aid: run the halves one after the other on the caller's stream
        # Overlap watch.  A probed pair of streams can still end up on one hardware queue later (the runtime maps streams
        # to its 4 queues when they become active; other streams of the process come and go): the halves then run one
        # after the other, +50 % per ply, for the rest of the run (seen in ~1 of 6 worker runs inside a long-lived
        # process).  So the first searches, and every 64th after them, are bracketed by events; a search whose two halves
        # did not overlap (union of the two intervals ~ their sum) twice in a row makes the engine draw new streams.
        self._watch: List[List[torch.cuda.Event]] = []
        self._watch_left = 6
        self._searches = 0
        self._serial_seen = 0
        self.stream_redraws = 0
        # Round 6: a THIRD way of not sharing the chip showed up (a (-1, 0) priority pair in bench.py's C2 runner leg, every
        # time): both halves start together, take the same time -- and that time is what ONE half after the other takes
        # (31 ms instead of 20.5: their kernels alternate instead of running side by side).  Neither "union ~ sum" nor
        # "one nested in the other" sees that; only a reference does: one search of every run is launched with both halves
        # on ONE stream on purpose (`_t_serial` = what no overlap costs), and a search whose union exceeds 0.85 of it has
        # not overlapped, whatever its intervals look like (healthy: 0.66).
        self._t_serial: Optional[float] = None
        self.overlap_ratio: Optional[float] = None          # union / _t_serial of the last watched search (statistics)

    @property
    def last_sim_budget(self) -> Optional[torch.Tensor]:
        if self.kld:
            return self.sim_budget
        return torch.cat([p.sim_budget for p in self.parts]) if self.cap else None

    @property
    def last_full_search(self) -> Optional[torch.Tensor]:
        return self.full_search.bool() if self.cap else None

    def prepare(self, state: GpuStateBatch) -> None:
        for (a, b), part in zip(self.bounds, self.parts):
            part.prepare(state._map(lambda t, a=a, b=b: t[a:b]))
        torch.cuda.synchronize(self.device)

    @property
    def use_graph(self) -> bool:
        return self.parts[0].use_graph

    @use_graph.setter
    def use_graph(self, v: bool) -> None:
        for p in self.parts:
            p.use_graph = bool(v)

    def reset_trees(self) -> None:
        for p in self.parts:
            p.reset_trees()

    def reset_run(self, seed: int) -> None:
        for p in self.parts:
            p.reset_run(seed)
        self._watch, self._watch_left, self._searches, self._serial_seen = [], 6, 0, 0
        self._t_serial = None                                # re-calibrated per run (the launch form may differ)

    def _check_overlap(self) -> None:
        """Look at finished overlap brackets (never waits) and re-draw the streams if the halves ran one after the other."""
        self._searches += 1
        if self._watch_left <= 0 and self._searches % 64 == 0:
            self._watch_left = 2
        while self._watch and all(e.query() for e in self._watch[0][:4]):
            s0, e0, s1, e1, calib = self._watch.pop(0)
            d0, d1 = s0.elapsed_time(e0), s1.elapsed_time(e1)
            if calib:                                            # the deliberately serialised search: the reference
                self._t_serial = d0 + d1
                continue
            self._watch_left -= 1
            lead = s0.elapsed_time(s1)                           # start of part 1 relative to part 0 (ms, may be < 0)
            union = max(d0, lead + d1) - min(0.0, lead)
            # Two signatures of halves that do not share the chip: (a) one after the other on one hardware queue -- disjoint
            # intervals, union ~ sum; (b) one half STARVED by the other -- nested intervals: both start together, one
            # finishes in about half the time of the other (seen once in round 6 with a (-1, 0) priority pair: the whole
            # runner leg at 31.9 ms per ply, which test (a) alone did not flag).  Halves that overlap properly take about the
            # same time: they are equal work on equal shares of the chip.
            serial = union > 0.9 * (d0 + d1) or min(d0, d1) < 0.62 * max(d0, d1)
            if self._t_serial is not None and self._t_serial > 2.0:
                # (c) whatever the intervals look like: the search took what the two halves take one after the other
                self.overlap_ratio = union / self._t_serial
                serial = serial or union > 0.85 * self._t_serial
            if os.environ.get("LZ_WATCH_DEBUG", "0") == "1":
                print(f"[lz watch] search {self._searches}: d0 {d0:.2f} ms, d1 {d1:.2f} ms, lead {lead:.2f} ms, union {union:.2f}, "
                      f"serial reference {self._t_serial} -> {'serial' if serial else 'ok'}", file=sys.stderr, flush=True)
            if d0 > 1.0 and d1 > 1.0 and serial:
                self._serial_seen += 1
                self._watch_left = max(self._watch_left, 2)
                if self._serial_seen >= 2 and self.stream_redraws < 6:
                    from .streams import overlapping_streams
                    self._old_streams = getattr(self, "_old_streams", []) + list(self.streams)   # keep them: work may be queued
                    # a priority pair that failed is replaced by an equal-priority, probed pair (the kind that has never been
                    # seen to starve a half); an equal-priority pair by another one
                    self._pair_mode = "probe"
                    self.streams = overlapping_streams(self.device, len(self.parts), mode=self._pair_mode)
                    self.stream_redraws += 1
                    self._serial_seen = 0
                    self._watch_left = 4
                    self._watch.clear()
                    return
            else:
                self._serial_seen = 0

    @property
    def graph_retry_off(self) -> bool:
        return any(p.graph_retry_off for p in self.parts)

    def get_timing(self, reset: bool = False) -> Dict[str, Dict[str, float]]:
        """Sum over the parts (their searches overlap on the device, so these are stream-busy times, not wall time)."""
        out: Dict[str, Dict[str, float]] = {"timing_ms": {}, "timing_calls": {}}
        for p in self.parts:
            t = p.get_timing(reset)
            for k in out:
                for name, v in t[k].items():
                    out[k][name] = out[k].get(name, 0) + v
        return out

    def search_batch(self, state: GpuStateBatch, *, temperatures: torch.Tensor, active: Optional[torch.Tensor] = None,
                     add_dirichlet_noise: Optional[bool] = None, reset: Optional[torch.Tensor] = None,
                     played_action: Optional[torch.Tensor] = None,
                     force_uniform_random_mask: Optional[torch.Tensor] = None,
                     rng_game_ids: Optional[torch.Tensor] = None,
                     rng_plies: Optional[torch.Tensor] = None, compact: Optional[bool] = None) -> RootSearchBatchOutput:
        main = torch.cuda.current_stream(self.device)
        cut = lambda t, a, b: None if t is None else t[a:b]
        outs = []
        self._check_overlap()
        # the reference search of a run: the 4th (the graphs of both launch keys exist by then), both halves on the caller's
        # stream; retried at the next search if a part still captured something in it
        calib = (not self.serialize and len(self.parts) == 2 and self._t_serial is None and self._searches >= 4 and
                 not any(len(w) > 4 and w[4] for w in self._watch))
        streams = (main,) * len(self.parts) if (self.serialize or calib) else self.streams
        subs = [state._map(lambda t, a=a, b=b: t[a:b]) for a, b in self.bounds]
        watch = None
        if not self.serialize and len(self.parts) == 2 and (self._watch_left > 0 or calib):
            watch = [torch.cuda.Event(enable_timing=True) for _ in range(4)]           # start / end of the two searches
        captures = sum(getattr(p, "captures", 0) for p in self.parts)
        t_host = time.perf_counter()
        for i, ((a, b), part, st, sub) in enumerate(zip(self.bounds, self.parts, streams, subs)):     # launch every part first ...
            st.wait_stream(main)
            with torch.cuda.stream(st):
                if watch is not None:
                    watch[2 * i].record(st)
                if self.injected_sim_budget is not None:
                    part.injected_sim_budget = self.injected_sim_budget[a:b]
                part.launch_search(sub, active=cut(active, a, b), add_dirichlet_noise=add_dirichlet_noise,
                                   reset=cut(reset, a, b), played_action=cut(played_action, a, b),
                                   rng_game_ids=cut(rng_game_ids, a, b), rng_plies=cut(rng_plies, a, b), compact=compact)
                if watch is not None:
                    watch[2 * i + 1].record(st)
        # A search in which a part captured its graph (warm-up, host synchronisation, capture) finishes part 0 on the host
        # before part 1 starts: its bracket says "serial" whatever the streams do -- with subtree reuse the first two
        # searches of every run capture (fresh key, continued key) and drew a spurious new pair at the third
        # ... and so does a search whose two launches the HOST spread out (another thread of the process held the runtime: the
        # streaming worker's copier pins staging memory, ~80 ms per GB): part 1 then starts late for a reason no other pair of
        # streams would cure.  Two graph replays take a few hundred microseconds to launch.
        host_ms = (time.perf_counter() - t_host) * 1e3
        if watch is not None and sum(getattr(p, "captures", 0) for p in self.parts) == captures and (host_ms < 6.0 or calib):
            self._watch.append(watch + [calib])
        todo = list(zip(self.parts, streams))                  # leftover rounds (batch_k > 1): the parts take turns,
        while todo:                                            # so that their small rounds overlap on the device
            nxt = []
            for part, st in todo:
                with torch.cuda.stream(st):
                    if part.tail_step():
                        nxt.append((part, st))
            todo = nxt
        for (a, b), part, st, sub in zip(self.bounds, self.parts, streams, subs):     # ... then the parts that may wait
            with torch.cuda.stream(st):
                outs.append(part.complete_search(sub, temperatures=temperatures[a:b],
                                                 force_uniform_random_mask=cut(force_uniform_random_mask, a, b),
                                                 tails_done=True))
        if not self.serialize:
            for st in self.streams:
                main.wait_stream(st)
        return RootSearchBatchOutput(*(torch.cat([getattr(o, f) for o in outs], dim=0)
                                       for f in ("model_input", "legal_mask", "policy_dense", "root_value", "terminal_mask",
                                                 "chosen_action_indices", "chosen_action_codes", "chosen_valid_mask")),
                                     **({"root_proven": torch.cat([o.root_proven for o in outs], dim=0)} if self.solver else {}))


for _name in DualStreamTreeMCTS.SUMMED:                  # counters of the whole batch: the parts' sums
    setattr(DualStreamTreeMCTS, _name, property(lambda self, n=_name: sum(getattr(p, n) for p in self.parts)))


class SteadyStateTreeSelfPlay:
    """B games, always full (finished games are re-seated); one step = one searched move for every game."""

    def __init__(self, model, num_games: int, sims: int, device, dtype: str = "float16", seed: int = 12345,
                 temperature_init: float = 1.0, temperature_final: float = 0.1, temperature_threshold: int = 10,
                 max_game_plies: int = 512, exploration_weight: float = 1.0, reuse_tree: bool = False,
                 reuse_factor: float = -1.0, dual_stream: bool = False, batch_k: int = 1,
                 arena_rows: Optional[int] = None) -> None:
        """`arena_rows`: trajectory rows to preallocate (one per game and step; the arena doubles -- one host sync and a
        copy -- when it runs out, so timed runs size it for all their steps)."""
        from .steady_state import SteadyStateRootSelfPlay
        from .mcts_gpu import V1RootMCTSConfig
        dev = torch.device(device)
        self.net = model if isinstance(model, FusedNet) else FusedNet(model, dev)
        self.dev, self.B, self.sims = dev, int(num_games), int(sims)
        # reuse the population bookkeeping (states, plies, trajectory arena, preroll, reset)
        self.pop = SteadyStateRootSelfPlay(self.net, num_games, V1RootMCTSConfig(num_simulations=1), dev, seed=seed,
                                           temperature_init=temperature_init, temperature_final=temperature_final,
                                           temperature_threshold=temperature_threshold, max_game_plies=max_game_plies,
                                           fused_search=False, arena_rows=arena_rows)
        # two streams pay for 64 channels (two 4-wave workgroups share a CU); the 128-channel kernel fills a CU's registers
        # with one workgroup, so its launches cannot overlap -- LZ_DUAL_128=1 tries it anyway (experiment)
        allow = self.net.pack.channels == 64 or os.environ.get("LZ_DUAL_128", "0") == "1"
        self.dual_stream = bool(dual_stream and allow and int(num_games) >= 2
                                and not persistent_search_available(self.net, batch_k))
        if self.dual_stream:
            parts = int(os.environ.get("LZ_TREE_PARTS", "0")) or None           # experiment: more than two parts
            self.mcts = DualStreamTreeMCTS(self.net, num_games, sims, dev, num_parts=parts,
                                           exploration_weight=exploration_weight,
                                           reuse_tree=reuse_tree, reuse_factor=reuse_factor, batch_k=batch_k, seed=seed)
        else:
            one = self.net
            if os.environ.get("LZ_SINGLE_STREAM_HALF_WG", "0") == "1":      # experiment: 4-wave workgroups, two per CU, one stream
                one = self.net.variant(half_workgroups=True)
            self.mcts = PortableTreeMCTS(one, num_games, sims, dev, exploration_weight, reuse_tree=reuse_tree,
                                         reuse_factor=reuse_factor, batch_k=batch_k, seed=seed)
        self._reseated = torch.zeros((self.B,), dtype=torch.uint8, device=dev)
        self.positions = 0
        self._nn_events = []

    @property
    def leaf_evals(self) -> int:
        return self.mcts.leaf_evals

    @property
    def consumed_evals(self) -> int:
        return self.mcts.consumed_evals

    def preroll(self, n: int = 120) -> None:
        self.pop.preroll(n)

    def prepare(self) -> None:
        """Kernel loading and graph capture before anything is timed (the searches run here are discarded)."""
        self.mcts.prepare(self.pop.states)
        for e in ([self.mcts.engine] if hasattr(self.mcts, "engine") else [p.engine for p in self.mcts.parts]):
            e.reuse_dropped.zero_()
        torch.cuda.synchronize(self.dev)

    def step(self) -> None:
        p = self.pop
        temps = torch.where(p.plies < p.t_thr, p.t_init, p.t_final).to(torch.float32)
        search = self.mcts.search_batch(p.states, temperatures=temps, reset=self._reseated, rng_plies=p.plies)
        self._reseated.zero_()
        p.finish_step(search, reseated=self._reseated)
        self.positions += self.B


from collections import OrderedDict

_ENGINE_CACHE: "OrderedDict[tuple, object]" = OrderedDict()


def _engine_cache_limit() -> int:
    """Search engines kept alive between self_play_tree_gpu calls (LZ_ENGINE_CACHE, default 1; 0 = off).  An engine owns
    its arenas (C3: ~90 GB), so the default keeps only the last one."""
    try:
        return max(0, int(os.environ.get("LZ_ENGINE_CACHE", "1")))
    except ValueError:
        return 1


def clear_engine_cache() -> None:
    """Drop the cached engines (and give their arenas back to the allocator)."""
    _ENGINE_CACHE.clear()
    torch.cuda.empty_cache()


def self_play_tree_gpu(model, num_games: int, mcts_simulations: int, temperature_init: float, temperature_final: float,
                       temperature_threshold: int, exploration_weight: float, device: str,
                       add_dirichlet_noise: bool = True, dirichlet_alpha: float = 0.3, dirichlet_epsilon: float = 0.25,
                       soft_value_k: float = 2.0, opening_random_moves: int = 0, max_game_plies: int = 512,
                       sample_moves: bool = True, concurrent_games: int = 8, verbose: bool = False,
                       policy_target_temperature: Optional[float] = None,
                       policy_target_prior_pseudocount: float = 0.0, reuse_tree: bool = True,
                       reuse_factor: float = -1.0, dual_stream: Optional[bool] = None, continuous_waves: bool = True,
                       device_tail: bool = True, batch_k: int = 1, evaluator: str = "auto", seed: int = 12345,
                       collect_timing: bool = False, row_log=None, start_bank=None,
                       **search_options) -> Tuple[TensorSelfPlayBatch, SelfPlayV1Stats]:
    """Tree-search twin of self_play_v1_gpu (same outputs); mirrors v1/python/portable_self_play.py:82-284,
    including the subtree reuse it performs on every move (:191, `reuse_tree`).
    `model` may also be a `PriorEvaluator` (states -> priors over the 220 actions + values, the reference's own
    split-phase hand-off).  `evaluator`: "fused" = the hand-written fp16 network kernel inside the captured search (6x64 / 10x128 nets);
    "module" = `model` itself as an external fp32 evaluator behind the split-phase protocol, whatever its size or
    device (what the reference's portable runner does with its `model`); "auto" = fused when the net has a fused
    kernel.  `seed`: key of the per-game counter RNG (noise, sampled moves); game ids are the runner's game numbers.
    `row_log` (finished_log.FinishedRowLog, the streaming worker): the rows of every game leave through the log when the
    game ends and the returned batch is empty; needs `device_tail` and `continuous_waves`.
    `search_options`: the optional rules of the search and of the per-ply tail -- symmetric evaluation, playout cap,
    forced playouts, Gumbel root search, TD(lambda) value targets, MCTS-Solver, first-play urgency / visit-scaled cpuct,
    resignation, KLD-gain early stopping, move re-pick, temperature half-life, policy surprise weighting, the start bank
    -- under the names
    and defaults of `search_rules.SearchRules.parse`; what each does, the mcts_counters it adds and what it cannot run
    with are described in search_rules.  A refusal is a ValueError before anything is allocated.
    `start_bank` (start_bank.StartBank, with the start bank rule on): the bank the games fork from and the searched
    positions go to; it is the caller's and survives the call.  Without one the call makes a private, empty bank."""
    dev = torch.device(device)
    rules = SearchRules.parse(mcts_simulations, **search_options)
    cap, resign, surprise, start = rules.cap, rules.resign_kwargs(), rules.surprise, rules.start_kwargs()
    if row_log is not None and not (device_tail and continuous_waves):
        raise RuntimeError("self_play_tree_gpu: a finished-row log needs device_tail and continuous_waves")
    if evaluator not in ("auto", "fused", "module"):
        raise ValueError(f"evaluator must be auto / fused / module, got {evaluator!r}")
    if isinstance(model, (FusedNet, PriorEvaluator)):
        use_fused = isinstance(model, FusedNet)
    else:
        from .net_hip import fused_supported
        use_fused = evaluator == "fused" or (evaluator == "auto" and fused_supported(model))
    rules.refuse(batch_k=batch_k, fused=use_fused, persistent=_persistent_default(), sample_moves=sample_moves,
                 device_tail=bool(device_tail), prior_evaluator=isinstance(model, PriorEvaluator),
                 policy_target_temperature=policy_target_temperature,
                 policy_target_prior_pseudocount=policy_target_prior_pseudocount)
    if start_bank is not None:
        if not start:
            raise ValueError("self_play_tree_gpu: a start bank was passed but the rule is off (start_fork_prob and "
                             "start_capture_prob are both 0)")
        if int(start_bank.capacity) != start["start_bank_capacity"]:
            raise ValueError(f"self_play_tree_gpu: the start bank holds {int(start_bank.capacity)} positions, "
                             f"start_bank_capacity is {start['start_bank_capacity']}")
    elif start:
        from .start_bank import StartBank
        start_bank = StartBank(start["start_bank_capacity"], dev)
    net = model if isinstance(model, (FusedNet, PriorEvaluator)) else FusedNet(model, dev) if use_fused else model.eval()
    wave = max(1, min(int(concurrent_games), int(num_games)))
    # two half-batches on two streams (see DualStreamTreeMCTS) once a wave is large enough to fill the chip twice over
    if dual_stream is None:
        dual_stream = use_fused and net.pack.channels == 64 and wave >= 1024 and int(batch_k) <= 1   # waves: large launches already
    if use_fused and persistent_search_available(net, batch_k) and not rules.symmetric:
        dual_stream = False                                  # the persistent kernel overlaps the phases inside every CU
    cls = DualStreamTreeMCTS if (dual_stream and use_fused and net.pack.channels == 64 and wave >= 2) else PortableTreeMCTS
    t_setup = time.perf_counter()
    kw = dict(exploration_weight=float(exploration_weight), add_dirichlet_noise=bool(add_dirichlet_noise),
              dirichlet_alpha=float(dirichlet_alpha), dirichlet_epsilon=float(dirichlet_epsilon),
              sample_moves=bool(sample_moves), reuse_tree=bool(reuse_tree), reuse_factor=float(reuse_factor),
              policy_target_temperature=policy_target_temperature,
              policy_target_prior_pseudocount=float(policy_target_prior_pseudocount), batch_k=int(batch_k),
              collect_timing=bool(collect_timing), rules=rules.engine())
    # Engines (arenas, descriptors) and their captured graphs are kept between calls with the same network buffers and
    # shape -- the worker calls this once per chunk and the staged loop once per iteration, and construction + capture
    # were 12.5 % of a C2 run.  `FusedNet.refresh()` writes new weights into the same buffers, so a
    # cached graph stays valid across checkpoints.  A PriorEvaluator / external module is never cached.
    # Only a caller-owned FusedNet is a stable key: for a module a fresh FusedNet is packed per call, its engine could
    # never be found again and would only pin its arenas.  Engines stay alive after the return -- call
    # `clear_engine_cache()` before handing the GPU's memory to something else (training on the same device).
    key = None
    if use_fused and isinstance(model, FusedNet) and _engine_cache_limit() > 0:
        key = (cls.__name__, int(net.pack.wfrag.data_ptr()), int(net.pack.fparams.data_ptr()), int(net.desc.flags),
               str(dev), wave, int(mcts_simulations), kw["rules"],
               tuple(sorted((k, repr(v)) for k, v in kw.items() if k != "rules")),
               os.environ.get("LZ_TREE_GRAPH", "on"), os.environ.get("LZ_TREE_PERSISTENT", "0"))
    mcts = _ENGINE_CACHE.pop(key, None) if key is not None else None
    cache_hit = mcts is not None
    if mcts is None:
        if key is not None:
            while len(_ENGINE_CACHE) >= _engine_cache_limit():      # make room BEFORE allocating the new arenas
                _ENGINE_CACHE.popitem(last=False)
            torch.cuda.empty_cache()
        mcts = cls(net, wave, mcts_simulations, dev, seed=seed, **kw)
    else:
        mcts.reset_run(seed)
    if key is not None:
        _ENGINE_CACHE[key] = mcts
    setup_sec = time.perf_counter() - t_setup
    buffer = TensorTrajectoryBuffer(dev, TOTAL_ACTION_DIM, max_steps_hint=max_game_plies, concurrent_games_hint=wave)
    outcome = torch.zeros((3,), dtype=torch.int64, device=dev)
    lengths = torch.zeros((int(num_games),), dtype=torch.int64, device=dev)
    # playout cap: plies (searches) of every game, which `lengths` (recorded rows) no longer equals
    game_plies = torch.zeros((int(num_games),), dtype=torch.int64, device=dev) if cap else None
    # device_tail: rows / move / finalisation on the device (wave_tail.WaveTail); continuous_waves: one wave whose
    # finished slots start the remaining games at once instead of sequential waves that idle until their longest game
    tail = None
    delta_hist = None
    if device_tail:
        from .wave_tail import WaveTail
        tail = WaveTail(buffer, wave, int(max_game_plies), dev, soft_value_k=float(soft_value_k), row_log=row_log,
                        **({"value_target_lambda": rules.td_lambda} if rules.td else {}),
                        **resign, **({"seed": int(seed)} if (resign or surprise or start) else {}),
                        **({"start_bank": start_bank, **{k: v for k, v in start.items() if k != "start_bank_capacity"}}
                           if start else {}),
                        **({"policy_surprise_weight": rules.surprise_weight,
                            "prior_fn": lambda search: root_prior(net, search, use_fused)} if surprise else {}))
        tail.collect_timing = bool(collect_timing)
        outcome, delta_hist = tail.outcome, tail.delta_hist
        if cap:
            tail.record_mask = mcts.full_search
    continuous = tail is not None and bool(continuous_waves)
    # temperature half-life: the schedule as a table, indexed by the ply on the device (tail and host loop alike)
    temp_table = None
    if rules.halflife:
        temp_table = torch.from_numpy(temperature_table(temperature_init, temperature_final, temperature_threshold,
                                                        rules.temperature_halflife, int(max_game_plies))).to(dev)
    wasted_plies = 0
    started = time.perf_counter()
    for base in range(0, wave if continuous else int(num_games), wave):
        g = min(wave, int(num_games) - base)
        states = GpuStateBatch.initial(dev, wave)
        step_index = None if row_log is not None else torch.full((wave, max_game_plies), -1, dtype=torch.int64, device=dev)
        step_counts = torch.zeros((wave,), dtype=torch.int64, device=dev)
        plies = torch.zeros((wave,), dtype=torch.int64, device=dev)
        done = torch.zeros((wave,), dtype=torch.bool, device=dev)
        if g < wave:
            done[g:] = True
        mcts.reset_trees()
        slot_ids = torch.arange(wave, dtype=torch.int64, device=dev)
        searched = torch.zeros((wave,), dtype=torch.int64, device=dev) if cap else None   # host loop: searches per slot
        if tail is not None:
            force_n = int(opening_random_moves)
            # compact evaluation lists once the wave has drained by at least one network pass per CU (the engine was built
            # for both launch forms if that can happen at all; two plies of lag in the estimate only delay the switch)
            lists_below = wave - (samples_per_launch_pass(net) if use_fused else 0)
            if cap:
                tail.game_plies = game_plies if continuous else game_plies[base:base + g]
            if resign or surprise or start:
                tail.game_base = 0 if continuous else base
            tail.run(lambda st, temps, dn, reseated: mcts.search_batch(
                         st, temperatures=temps, active=~dn, reset=reseated,
                         force_uniform_random_mask=(plies < force_n) if force_n > 0 else None,
                         rng_game_ids=tail.slot_game + (0 if continuous else base), rng_plies=plies,
                         **({"compact": True} if (use_fused and tail.live_estimate <= lists_below) else {})),
                     states, plies, done, step_index, step_counts, lengths if continuous else lengths[base:base + g],
                     temperature_init, temperature_final, temperature_threshold,
                     games_to_start=int(num_games) - wave if continuous else 0,
                     **({"temperature_table": temp_table} if temp_table is not None else {}))

            wasted_plies += 1
            continue
        while True:
            active = torch.nonzero(~done).view(-1)
            if int(active.numel()) == 0:
                break
            if temp_table is not None:
                temps = temp_table.index_select(0, plies.clamp(0, int(temp_table.numel()) - 1))
            else:
                temps = torch.where(plies < int(temperature_threshold), float(temperature_init),
                                    float(temperature_final)).to(torch.float32)
            force = (plies < int(opening_random_moves)) if int(opening_random_moves) > 0 else None
            out = mcts.search_batch(states, temperatures=temps, active=~done, force_uniform_random_mask=force,
                                    rng_game_ids=slot_ids + base, rng_plies=plies)
            rec = active
            if cap:                                          # only the full searches record a row
                rec = active[mcts.full_search.index_select(0, active).bool()]
                searched.index_add_(0, active, torch.ones_like(active))
            if not cap or int(rec.numel()) > 0:
                rows = buffer.append_steps(out.model_input.index_select(0, rec), out.legal_mask.index_select(0, rec),
                                           out.policy_dense.index_select(0, rec),
                                           states.current_player.index_select(0, rec))
                step_index[rec, step_counts.index_select(0, rec)] = rows
                step_counts.index_add_(0, rec, torch.ones_like(rec))
            fin, result, _ = v0_core.self_play_step_inplace(
                *states.tensors(), plies, done, active, out.chosen_action_codes.index_select(0, active),
                out.terminal_mask.index_select(0, active), out.chosen_valid_mask.index_select(0, active),
                int(max_game_plies), float(soft_value_k))
            if int(fin.numel()) > 0:
                boards = states.board.index_select(0, fin)
                delta = (boards.eq(1).sum(dim=(1, 2)) - boards.eq(-1).sum(dim=(1, 2))).to(torch.float32)
                soft = torch.tanh(delta / 18.0 * float(soft_value_k))
                f_slots, f_len, f_out = buffer.finalize_games_inplace(
                    step_index_matrix=step_index, step_counts=step_counts, slots=fin, result_from_black=result,
                    soft_value_from_black=soft)
                if int(f_slots.numel()) > 0:
                    lengths.index_copy_(0, f_slots + base, f_len)
                outcome.add_(f_out)
                if cap:                                      # games booked by plies: those without a recorded row too
                    game_plies.index_copy_(0, fin + base, searched.index_select(0, fin))
                    r = result.to(dev).view(-1)[step_counts.index_select(0, fin) == 0]
                    outcome.add_(torch.stack(((r > 0).sum(), (r < 0).sum(), (r == 0).sum())))
    t_sync = time.perf_counter()
    torch.cuda.synchronize(dev)
    sync_ms = (time.perf_counter() - t_sync) * 1e3
    elapsed = max(1e-9, time.perf_counter() - started)
    if tail is not None:
        tail.check_overflow()
    if row_log is not None:
        row_log.close()                                      # the last segment leaves; the rows are the consumer's now
    t_build = time.perf_counter()
    batch = buffer.build()
    torch.cuda.synchronize(dev)
    build_sec = time.perf_counter() - t_build
    positions = int(lengths.sum().item()) if row_log is not None else batch.num_samples
    o = outcome.tolist()
    hist = delta_hist.tolist() if delta_hist is not None else []
    keys = ("root_puct_ms", "pack_writeback_ms", "self_play_step_ms", "finalize_ms")
    timing = mcts.get_timing() if collect_timing else {"timing_ms": {}, "timing_calls": {}}
    if tail is not None and collect_timing:
        for k, v in tail.get_timing().items():
            timing["timing_ms"][k] = timing["timing_ms"].get(k, 0.0) + v["ms"]
            timing["timing_calls"][k] = timing["timing_calls"].get(k, 0) + v["calls"]
    t_ms = {k: float(timing["timing_ms"].get(k, 0.0)) for k in keys}
    t_total = sum(t_ms.values())
    # what the bounded arenas did to this run (the reference's tree is unbounded): must all be 0 for results that equal an
    # unbounded tree's; a refused expansion means the edge pool was sized too small for this workload -- say so loudly
    engines = [p.engine for p in getattr(mcts, "parts", [])] or [mcts.engine]
    compact_lists = all(e.compact_evals for e in engines)
    refused = sum(e.pool_status()["refused_expansions"] for e in engines)
    dropped = sum(int(e.reuse_dropped[0].item()) for e in engines)
    pruned = sum(int(e.reuse_dropped[1].item()) for e in engines)
    if refused:
        print(f"[liuzhou_amd] WARNING: {refused} tree expansions found no free edge chunk (pool of "
              f"{sum(e.pool_chunks for e in engines)} chunks); those leaves stayed unexpanded for a visit.  Pass a larger "
              "`pool_chunks` to TreeEngine or lower `concurrent_games`.", flush=True)
    stats = SelfPlayV1Stats(
        num_games=num_games, num_positions=positions, black_wins=int(o[0]), white_wins=int(o[1]), draws=int(o[2]),
        avg_game_length=float((game_plies if cap else lengths).to(torch.float32).mean().item()), elapsed_sec=elapsed,
        positions_per_sec=float(positions / elapsed), games_per_sec=float(num_games / elapsed),
        step_timing_ms=t_ms, step_timing_ratio={k: (t_ms[k] / t_total if t_total > 0 else 0.0) for k in keys},
        step_timing_calls={k: int(timing["timing_calls"].get(k, 0)) for k in keys},
        # the device-tail loop runs one fully masked ply per wave after the last game has ended (wave_tail.WaveTail.run)
        # (with compact evaluation lists a fully masked ply launches no evaluation at all)
        # (... unless that ply was launched densely: the two-plies-old live estimate had not seen the wave end yet)
        mcts_counters={"leaf_eval_count": int(mcts.leaf_evals) - (
                           wasted_plies * wave * (int(mcts_simulations) + 1)
                           if int(batch_k) <= 1 and not (compact_lists and (cap or rules.kld_on or getattr(mcts, "last_search_lists", False)))
                           else 0),
                       "compact_eval_lists": int(compact_lists), "search_parts": len(engines),
                       "list_searches": int(sum(getattr(p, "list_searches", 0) for p in (getattr(mcts, "parts", None) or [mcts]))),
                       "masked_extra_plies": wasted_plies, "graph_retry_off": int(bool(mcts.graph_retry_off)),
                       # where the wall time outside `elapsed_sec` (the plies) goes: engine construction or cache hit,
                       # build() of the five tensors; graph capture happens inside the first plies
                       "engine_cache_hit": int(cache_hit), "setup_ms": int(setup_sec * 1e3), "build_ms": int(build_sec * 1e3),
                       "reuse_pruned": pruned, "reuse_dropped": dropped, "edge_pool_refused": refused,
                       "final_sync_ms": int(sync_ms), "stream_redraws": int(getattr(mcts, "stream_redraws", 0)),
                       # two-stream search: last watched search / the run's one-stream reference search, in percent
                       # (~66: the halves share the chip; ~100: they do not)
                       **({"stream_overlap_pct": int(round(100.0 * mcts.overlap_ratio))}
                          if getattr(mcts, "overlap_ratio", None) is not None else {}),
                       **({"loop_ms": int(tail.loop_ms), "host_wait_ms": int(tail.host_wait_ms),
                           "plies_launched": int(tail.plies_launched)} if tail is not None else {}),
                       # the rules that are on: the engine's counter blocks (search_rules.RULE_SPECS), the rows the playout
                       # cap's full searches recorded, and the tail's blocks of resignation and policy surprise weighting
                       **engine_counters(rules, mcts), **({"recorded_positions": int(positions)} if cap else {}),
                       **(counters_from_block(tail.resign_counters.tolist()) if resign else {}),
                       **(surprise_counters_from_block(tail.surprise_counters.tolist(), float(tail.surprise_sum.item()))
                          if surprise else {}),
                       **(dict(zip(START_COUNTER_KEYS, (int(x) for x in tail.start_counters.tolist()))) if start else {})},
        piece_delta_buckets={str(d - 18): int(v) for d, v in enumerate(hist)}, device=str(dev))
    return batch, stats
