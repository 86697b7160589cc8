"""Hand-built roots for the tree read-out kernels: B games in one TreeEngine whose root records -- node 0, its edge run, the
chunk bookkeeping, the root scalars and the option arrays a variant reads -- are written straight into the arena, the way
`_engine_with_root_edges` of tests/test_gpu_reference_cases.py used to do for one game.

The host half (`layout`, `check_bounds`) needs no GPU: it builds the numpy records and asserts that every index a read-out
kernel derives from them lies inside the buffer the device half allocates.  The device half (`HandEngine`) uploads exactly
those records, so a GPU run never reads outside what the harness allocated.

Record layouts: EDGE_DT / NODE_DT of tests/tree_parity.py (include/liuzhou_hip.h)."""
import numpy as np

from tests.golden_utils import FIELDS
from tests.readout_ref import game_status, index_to_code as _code   # noqa: F401  (`_code`: tests/test_gpu_move_pick.py)
from tests.tree_parity import EDGE_DT, NODE_DT

MAX_CHILDREN = 72            # the header's promise; the kernels' two slots of 64 lanes would hold 128
EDGE_CHUNK = 1024
GUMBEL_STRIDE = 80
ACTIONS = 220


def root_from_state(st, i, **kw):
    """The state part of a root dict (tests/readout_ref.ref_finish) from row `i` of a state dict of numpy arrays."""
    board = np.asarray(st["board"][i])
    phase, player = int(st["phase"][i]), int(st["current_player"][i])
    r = dict(state={f: np.asarray(st[f][i]).copy() for f in FIELDS}, phase=phase, player=1 if player == 1 else -1,
             status=game_status(phase, int((board == 1).sum()), int((board == -1).sum()), int(st["move_count"][i]),
                                int(st["moves_since_capture"][i])))
    r.update(kw)
    return r


def edge_records(root):
    """The root's edge run as EDGE_DT records (child = -1: no node hangs from any of them)."""
    n = max(int(root["ne"]), 0)
    e = np.zeros(n, EDGE_DT)
    if n:
        e["act"] = np.asarray(root["act"], np.uint8)
        e["P"] = np.asarray(root["P"], np.float32)
        e["n_info"] = np.asarray(root["N"], np.uint32) | (np.asarray(root["info"], np.uint32) << 24)
        e["W"] = np.asarray(root["W"], np.float64)
        e["child"] = -1
    return e


def layout(roots, edge_chunk=EDGE_CHUNK, pool_chunks=None, options=None):
    """Numpy image of what the device half writes: game g's run at the start of chunk g of the edge pool, booked as the
    game's first chunk.  `options`: the arrays a variant reads (gumbel_gl / gumbel_base [B, GUMBEL_STRIDE], gumbel_root_base,
    gumbel_root_value, root_proven, root_noise, kld_snapshot [B, 72], kld_budget, active, cpuct_table)."""
    B = len(roots)
    pool_chunks = B if pool_chunks is None else int(pool_chunks)
    L = dict(B=B, edge_chunk=int(edge_chunk), pool_chunks=pool_chunks, roots=roots, options=dict(options or {}),
             edge_begin=np.arange(B, dtype=np.int64) * int(edge_chunk),
             nedges=np.array([int(r["ne"]) for r in roots], np.int32),
             runs=[edge_records(r) for r in roots],
             root_visits=np.array([int(r["root_visits"]) for r in roots], np.int32),
             root_w=np.array([float(r["root_w"]) for r in roots], np.float64),
             root_init_value=np.array([r["root_init_value"] for r in roots], np.float32),
             root_terminal=np.array([int(bool(r["root_terminal"])) for r in roots], np.uint8))
    check_bounds(L)
    return L


def check_bounds(L, out_caps=(36, 72, 80)):
    """Every index the six read-out kernels derive from the records, against the buffers of `HandEngine`."""
    B, chunk, pool = L["B"], L["edge_chunk"], L["pool_chunks"] * L["edge_chunk"]
    assert chunk >= 128 and chunk & (chunk - 1) == 0 and L["pool_chunks"] >= B >= 1
    for g in range(B):
        ne, e0 = int(L["nedges"][g]), int(L["edge_begin"][g])
        assert -1 <= ne <= MAX_CHILDREN, (g, ne)
        assert 0 <= e0 and e0 + max(ne, 1) <= pool, (g, "run outside the pool")        # a lane without a child reads e0 + 0
        assert e0 // chunk == (e0 + max(ne, 1) - 1) // chunk, (g, "run straddles a chunk")
        run = L["runs"][g]
        assert len(run) == max(ne, 0)
        if ne > 0:
            act = run["act"].astype(np.int64)
            assert act.min() >= 0 and act.max() < ACTIONS, (g, "policy_dense column")       # prow[act], index_to_code
            assert len(np.unique(act)) == ne, (g, "actions must be distinct")
            assert (run["child"] == -1).all()
            assert int((run["n_info"] & 0xFFFFFF).max()) < (1 << 24)
            for cap in out_caps:                                                             # child_* [B, cap]: k < min(ne, cap)
                assert g * cap + min(ne, cap) <= B * cap
            assert ne <= GUMBEL_STRIDE and ne <= 2 * 64                                      # gl / base rows, two lane slots
    for name, width in (("gumbel_gl", GUMBEL_STRIDE), ("gumbel_base", GUMBEL_STRIDE), ("kld_snapshot", MAX_CHILDREN)):
        if name in L["options"]:
            assert np.asarray(L["options"][name]).shape == (B, width), name
    for name in ("gumbel_root_base", "gumbel_root_value", "root_proven", "root_noise", "kld_budget", "active"):
        if name in L["options"]:
            assert np.asarray(L["options"][name]).shape == (B,), name
    if "cpuct_table" in L["options"]:
        n = len(L["options"]["cpuct_table"])
        assert n >= 2
        for g in range(B):                                       # the kernel's own clamp, restated: [0, n - 1]
            T = int(L["root_visits"][g])
            assert 0 <= ((T if T > 0 else 0) if T < n - 1 else n - 1) <= n - 1


class HandEngine:
    """The device half: a TreeEngine of B games holding exactly the records of `layout`."""

    def __init__(self, L, device, c_puct=1.0):
        import torch
        from liuzhou_amd.tree_engine import TreeEngine
        from tests.tree_parity import to_gpu_batch
        B, dev = L["B"], device
        self.L, self.B, self.dev = L, B, dev
        eng = TreeEngine(B, 2, dev, c_puct, edge_chunk=L["edge_chunk"], pool_chunks=L["pool_chunks"])
        self.engine = eng
        st = {f: np.stack([np.asarray(r["state"][f]) for r in L["roots"]]) for f in FIELDS}
        eng.set_roots(to_gpu_batch(st, dev))
        eng.begin()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        nodes = eng.buf["nodes"].view(B, eng.node_cap, 6)
        rec = nodes[:, 0].contiguous().cpu().numpy().view(NODE_DT).reshape(B).copy()
        rec["edge_begin"], rec["nedges"], rec["parent"] = L["edge_begin"], L["nedges"], -1
        nodes[:, 0] = up(rec.view(np.int64).reshape(B, 6))
        pool = np.zeros(L["pool_chunks"] * L["edge_chunk"], EDGE_DT)
        for g in range(B):
            e0 = int(L["edge_begin"][g])
            pool[e0:e0 + len(L["runs"][g])] = L["runs"][g]
        assert eng.buf["edges"].shape[0] == len(pool)
        eng.buf["edges"].copy_(up(pool.view(np.int64).reshape(len(pool), 4)))
        eng.buf["n_edges"].copy_(up((L["edge_begin"] + np.maximum(L["nedges"], 0)).astype(np.int32)))
        eng.buf["chunk_list"].view(B, eng.chunk_cap)[:, 0] = torch.arange(B, dtype=torch.int32, device=dev)
        eng.buf["n_chunks"].fill_(1)
        eng.buf["free_chunks"].copy_(torch.roll(torch.arange(eng.pool_chunks, dtype=torch.int32, device=dev), -B))
        eng.buf["pool_top"].fill_(eng.pool_chunks - B)
        eng.buf["root_visits"].copy_(up(L["root_visits"]))
        eng.buf["root_w"].copy_(up(L["root_w"]))
        eng.buf["root_init_value"].copy_(up(L["root_init_value"]))
        eng.buf["root_terminal"].copy_(up(L["root_terminal"]))
        self.keep = {}
        o, d = L["options"], eng.desc
        if "active" in o:
            eng.buf["active"].copy_(up(np.asarray(o["active"], np.uint8)))
        if "root_noise" in o:
            self.keep["root_noise"] = up(np.asarray(o["root_noise"], np.uint8))
            d.root_noise = self.keep["root_noise"].data_ptr()
        if "cpuct_table" in o:
            self.keep["cpuct_table"] = up(np.asarray(o["cpuct_table"], np.float64))
            d.cpuct_table, d.cpuct_table_len, d.puct_shape = self.keep["cpuct_table"].data_ptr(), len(o["cpuct_table"]), 2
        if "forced_k" in o:
            d.forced_k = float(o["forced_k"])
        if "gumbel_m" in o:
            eng.set_gumbel(int(o["gumbel_m"]), float(o.get("gumbel_c_visit", 50.0)), float(o.get("gumbel_c_scale", 1.0)))
            assert eng.gumbel["gl"].shape[1] == GUMBEL_STRIDE
            eng.gumbel["gl"].copy_(up(np.asarray(o["gumbel_gl"], np.float32)))
            eng.gumbel["base"].copy_(up(np.asarray(o["gumbel_base"], np.int32)))
            eng.gumbel["root_base"].copy_(up(np.asarray(o["gumbel_root_base"], np.int32)))
            eng.gumbel["root_value"].copy_(up(np.asarray(o["gumbel_root_value"], np.float32)))
        if "root_proven" in o:
            eng.set_solver(True)
            eng.root_proven.copy_(up(np.asarray(o["root_proven"], np.int32)))
        if "kld_budget" in o:
            self.keep["kld_budget"] = up(np.asarray(o["kld_budget"], np.int32))
            self.keep["kld_snapshot"] = up(np.asarray(o["kld_snapshot"], np.int32))
            d.sim_budget = d.kld_budget = self.keep["kld_budget"].data_ptr()
            d.kld_snapshot = self.keep["kld_snapshot"].data_ptr()
            d.kld_threshold, d.kld_interval, d.kld_min_sims = float(o["kld_threshold"]), int(o["kld_interval"]), \
                int(o["kld_min_sims"])
        torch.cuda.synchronize()


def one_root(actions, visits, q_root_side, priors):
    """The one-game root of tests/test_gpu_reference_cases.py: the initial position (black to move) with the given children;
    q is given from the root mover's side and the children are white-to-move positions, so W = -q * N in the child
    mover's frame."""
    from oracle import lz_oracle as O
    n = len(actions)
    v, q = np.asarray(visits, np.float64), np.asarray(q_root_side, np.float64)
    return root_from_state(O.initial_states(1), 0, ne=n, act=list(actions), P=list(priors), N=list(visits), W=-q * v,
                           info=[1] * n, root_visits=int(np.sum(visits)), root_w=float(np.sum(q * v)), root_init_value=0.0,
                           root_terminal=0)
