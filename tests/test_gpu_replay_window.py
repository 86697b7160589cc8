"""GPU: lz_replay_gather_rows against the kernel pair it fuses and against tests/replay_ref.py, byte for byte; the
device ring of liuzhou_amd/replay_window.py; train_network_from_window against train_network_from_tensors; the record
output of gather_trajectories; the staged loop with a window."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import replay_ref as R
from tests.test_replay_window_cpu import HAND

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 3
SENTINEL = 0xA5
ERR_ARG = -1
ODD = (0x7FC12345, 0x80000000, 0x00000001, 0x7F800000)             # NaN payload, -0.0, subnormal, +inf


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from liuzhou_amd import _lib
    return _lib


def _rows(n=64, seed=5):
    """n rows the record format holds: all eight phases, 0 / 1 / 71 / 72 legal actions, and on the legal entries of every
    row that has them a NaN payload, -0.0, a subnormal and +inf."""
    rng = np.random.default_rng(seed)
    planes = np.zeros((n, 11, 36), np.float32)
    masks = np.zeros((n, 220), np.uint8)
    policy = np.zeros((n, 220), np.uint32)
    for i in range(n):
        planes[i, :4] = rng.integers(0, 2, (4, 36))
        if i % 8:
            planes[i, 3 + i % 8] = 1.0
        legal = np.sort(rng.choice(220, (0, 1, 71, 72)[(i // 8) % 4], replace=False))
        masks[i, legal] = 1
        policy[i, legal] = rng.random(len(legal)).astype(np.float32).view(np.uint32)
        for k, a in enumerate(legal[:4]):
            policy[i, a] = ODD[(i + k) % 4]
    value = rng.integers(-1, 2, n).astype(np.float32)
    soft = (rng.random(n) * 2 - 1).astype(np.float32)
    return planes.reshape(n, 11, 6, 6), masks, policy.view(np.float32), value, soft


@pytest.fixture(scope="module")
def ring(L):
    """64 records from pack_batch + the four hand-written ones (tests/test_replay_window_cpu.py), what the kernel pair
    makes of every record, and what the restatement makes of it."""
    from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
    from liuzhou_amd.trajectory_codec import pack_batch, unpack_records
    rows = _rows()
    batch = TensorSelfPlayBatch(*(torch.from_numpy(a).to(DEV) for a in rows))
    packed = pack_batch(batch)
    hand = torch.from_numpy(np.stack([HAND[k] for k in sorted(HAND)])).to(DEV)
    rec = torch.cat([packed, hand]).contiguous()
    names = {k: 64 + i for i, k in enumerate(sorted(HAND))}
    full = unpack_records(rec)
    host = rec.cpu().numpy()
    # pack -> restatement reproduces the source rows (no -0.0 off the legal set in them)
    dp, dm, dq, dv, ds = R.decode_records(host[:64])
    assert np.array_equal(dp, rows[0]) and np.array_equal(dm, rows[1]) and np.array_equal(dq, rows[2].view(np.uint32))
    assert np.array_equal(dv, rows[3].view(np.uint32)) and np.array_equal(ds, rows[4].view(np.uint32))
    return {"rec": rec, "host": host, "full": full, "names": names, "capacity": int(rec.shape[0])}


def _sentinel(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def _outputs(m):
    return [_sentinel((m + GUARD, 396), torch.float32), _sentinel((m + GUARD, 220), torch.uint8),
            _sentinel((m + GUARD, 220), torch.float32), _sentinel((m + GUARD,), torch.float32),
            _sentinel((m + GUARD,), torch.float32)]


def _call(L, rec, capacity, slots, sym, width, m, outs):
    st = L.lib().lz_replay_gather_rows(L.ptr(rec), L.i64(capacity), L.ptr(slots), L.ptr(sym), width, L.i64(m),
                                       *(L.ptr(t) for t in outs), L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return st


def _bytes(t):
    t = t.contiguous()
    return t.view(torch.uint8).cpu().numpy().reshape(t.shape[0], -1)


def _case(ring, m, seed):
    """Slots and ids of one launch: the 73-bit record first, duplicates, slots -1 and `capacity`, ids -1 and 8, and among
    the valid rows every id 0..7 (m permitting)."""
    rng = np.random.default_rng(seed)
    cap = ring["capacity"]
    slots = rng.integers(0, cap, m)
    slots[0] = ring["names"]["phase3_73"]
    sym = (np.arange(m) + seed) % 8
    if m >= 3:
        slots[1], slots[2] = -1, cap
    if m >= 5:
        slots[4] = slots[3]                                          # a duplicate
        sym[3] = -1
    if m >= 16:
        sym[9], slots[10], slots[11] = 8, slots[0], ring["names"]["phase7_one"]
        slots[12], slots[13] = ring["names"]["phase0_none"], ring["names"]["phase3_72"]
    return slots.astype(np.int64), sym


@pytest.mark.parametrize("m", [1, 3, 4, 5, 257])
def test_kernel_equals_the_pair_and_the_restatement(L, ring, m):
    from liuzhou_amd import symmetry as S
    full, cap = ring["full"], ring["capacity"]
    for mode in ("int8", "int32", "null"):
        slots_h, sym_h = _case(ring, m, seed=m + len(mode))
        slots = torch.from_numpy(slots_h).to(DEV)
        if mode == "null":
            sym_h, sym, width = None, None, 7                        # sym_width is not looked at without sym
            pair_sym = torch.zeros(m, dtype=torch.int8, device=DEV)
        else:
            sym = torch.from_numpy(sym_h.astype(np.int8 if mode == "int8" else np.int32)).to(DEV)
            width, pair_sym = (1 if mode == "int8" else 4), sym
        outs = _outputs(m)
        assert _call(L, ring["rec"], cap, slots, sym, width, m, outs) == 0
        # the existing pair on the same records: unpack everything, then gather + transform
        pp, pm, pq = S.transform_samples(full.state_tensors, full.legal_masks.view(torch.uint8), full.policy_targets,
                                         pair_sym, slots)
        ok = torch.from_numpy((slots_h >= 0) & (slots_h < cap) & (True if sym_h is None else (sym_h >= 0) & (sym_h < 8))).to(DEV)
        safe = slots.clamp(0, cap - 1)
        zero = torch.zeros((), dtype=torch.int32, device=DEV)
        pv = torch.where(ok, full.value_targets.view(torch.int32)[safe], zero)
        ps = torch.where(ok, full.soft_value_targets.view(torch.int32)[safe], zero)
        pair = [pp.reshape(m, 396), pm, pq, pv, ps]
        ref = R.gather_ref(ring["host"], slots_h, sym_h)
        ref = [ref[0].reshape(m, 396), ref[1], ref[2], ref[3], ref[4]]
        for name, got, a, b in zip(("planes", "masks", "policy", "value", "soft"), outs, pair, ref):
            g = _bytes(got)
            assert np.array_equal(g[:m], _bytes(a)), f"{mode} m={m} {name}: differs from the kernel pair"
            assert np.array_equal(g[:m], np.ascontiguousarray(b).view(np.uint8).reshape(m, -1)), \
                f"{mode} m={m} {name}: differs from the restatement"
            assert (g[m:] == SENTINEL).all(), f"{mode} m={m} {name}: guard rows written"
        planes = outs[0].cpu().numpy()
        for j in np.flatnonzero(~ok.cpu().numpy()):
            assert not planes[j].any() and not _bytes(outs[2])[j].any() and not _bytes(outs[3])[j].any()


def test_kernel_refuses_bad_arguments_without_a_launch(L, ring):
    m, cap = 4, ring["capacity"]
    slots = torch.arange(m, dtype=torch.int64, device=DEV)
    sym = torch.zeros(m, dtype=torch.int8, device=DEV)
    outs = _outputs(m)
    rec = ring["rec"]
    assert _call(L, rec, cap, slots, sym, 1, -1, outs) == ERR_ARG
    assert _call(L, rec, -1, slots, sym, 1, m, outs) == ERR_ARG
    for width in (0, 2, 8):
        assert _call(L, rec, cap, slots, sym, width, m, outs) == ERR_ARG
    assert _call(L, None, cap, slots, sym, 1, m, outs) == ERR_ARG
    assert _call(L, rec, cap, None, sym, 1, m, outs) == ERR_ARG
    for i in range(5):
        assert _call(L, rec, cap, slots, sym, 1, m, outs[:i] + [None] + outs[i + 1:]) == ERR_ARG, i
    assert _call(L, rec, cap, slots, sym, 1, 0, outs) == 0 and _call(L, None, 0, None, None, 0, 0, [None] * 5) == 0
    for t in outs:
        assert (_bytes(t) == SENTINEL).all()
    # capacity 0: every slot is outside the ring, every row zero
    assert _call(L, rec, 0, slots, None, 0, m, outs) == 0
    for t in outs:
        g = _bytes(t)
        assert not g[:m].any() and (g[m:] == SENTINEL).all()


def test_kernel_launch_is_capturable(L, ring):
    """Captured once, replayed on other slots and ids written into the same buffers: no allocation, no synchronisation."""
    m, cap = 5, ring["capacity"]
    slots = torch.zeros(m, dtype=torch.int64, device=DEV)
    sym = torch.zeros(m, dtype=torch.int32, device=DEV)
    outs = _outputs(m)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = L.lib().lz_replay_gather_rows(L.ptr(ring["rec"]), L.i64(cap), L.ptr(slots), L.ptr(sym), 4, L.i64(m),
                                           *(L.ptr(t) for t in outs), L.stream_ptr(torch.device(DEV)))
    assert st == 0
    for seed in (1, 2):
        slots_h, sym_h = _case(ring, m, seed)
        slots.copy_(torch.from_numpy(slots_h))
        sym.copy_(torch.from_numpy(sym_h.astype(np.int32)))
        graph.replay()
        torch.cuda.synchronize()
        ref = R.gather_ref(ring["host"], slots_h, sym_h)
        for got, want in zip(outs, (ref[0].reshape(m, 396),) + ref[1:]):
            g = _bytes(got)
            assert np.array_equal(g[:m], np.ascontiguousarray(want).view(np.uint8).reshape(m, -1)), seed
            assert (g[m:] == SENTINEL).all()


# ---- the ring on the device ------------------------------------------------------------------------------------------
def _slice(batch, a, b):
    from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
    return TensorSelfPlayBatch(*(t[a:b] for t in (batch.state_tensors, batch.legal_masks, batch.policy_targets,
                                                  batch.value_targets, batch.soft_value_targets)))


def _cat(*batches):
    from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
    return TensorSelfPlayBatch(*(torch.cat([getattr(b, f) for b in batches]) for f in
                                 ("state_tensors", "legal_masks", "policy_targets", "value_targets", "soft_value_targets")))


def _same_rows(got, batch):
    planes, masks, policy, value, soft = got
    return (torch.equal(planes.view(torch.int32), batch.state_tensors.view(torch.int32))
            and masks.dtype == torch.bool and torch.equal(masks, batch.legal_masks.to(torch.bool))
            and torch.equal(policy.view(torch.int32), batch.policy_targets.view(torch.int32))
            and torch.equal(value.view(torch.int32), batch.value_targets.view(torch.int32))
            and torch.equal(soft.view(torch.int32), batch.soft_value_targets.view(torch.int32)))


def test_ring_wraps_evicts_and_survives_a_restart(L):
    from liuzhou_amd.replay_window import ReplayWindow
    from liuzhou_amd.trajectory_codec import pack_batch
    from tests.test_gpu_symmetry import _dataset
    data = _dataset(n=25)
    a, b, c = _slice(data, 0, 10), _slice(data, 10, 18), _slice(data, 18, 25)
    w = ReplayWindow(DEV, max_generations=3, capacity_rows=16)
    assert w.nbytes == 16 * 360 and w.num_rows == 0
    assert w.add_generation(a) == {"generation": 0, "first_slot": 0, "rows": 10, "evicted": [], "filtered_non_finite_rows": 0}
    # one non-finite row is dropped and counted; 10 + 7 > 16 evicts generation 0; slots 10..15, 0: the ring wraps
    b.value_targets = b.value_targets.clone()
    b.value_targets[3] = float("nan")
    keep = [i for i in range(8) if i != 3]
    b_kept = _slice(data, 10, 18)
    b_kept = type(b_kept)(*(t[keep] for t in (b_kept.state_tensors, b_kept.legal_masks, b_kept.policy_targets,
                                              b_kept.value_targets, b_kept.soft_value_targets)))
    assert w.add_generation(b, generation=4) == {"generation": 4, "first_slot": 10, "rows": 7, "evicted": [0],
                                                 "filtered_non_finite_rows": 1}
    assert w.add_generation(pack_batch(c)) == {"generation": 5, "first_slot": 1, "rows": 7, "evicted": [],
                                               "filtered_non_finite_rows": 0}      # records are taken as they are
    assert w.generations == [(4, 10, 7), (5, 1, 7)] and w.num_rows == 14
    assert w.slots_of(4).tolist() == [10, 11, 12, 13, 14, 15, 0]
    assert _same_rows(w.gather(w.slots_of(4)), b_kept) and _same_rows(w.gather(w.slots_of(5)), c)
    # refusals leave the window as it is
    before = (w.generations, w.ring.clone())
    bad = _slice(data, 0, 4)
    bad.state_tensors = bad.state_tensors.clone()
    bad.state_tensors[1, 0, 0, 0] = 0.5
    for rows, gid in ((bad, None), (c, 5), (_slice(data, 0, 0), None), (_slice(data, 0, 17), None),
                      (torch.zeros((3, 359), dtype=torch.uint8, device=DEV), None)):
        with pytest.raises(ValueError):
            w.add_generation(rows, generation=gid)
    with pytest.raises(RuntimeError, match="HIP device"):
        w.add_generation(pack_batch(c).cpu())
    assert (w.generations, True) == (before[0], torch.equal(w.ring, before[1]))
    # restart: the same capacity puts every generation back on its slots, another one lays them out again
    state = w.state_dict()
    assert not state["records"].is_cuda and tuple(state["records"].shape) == (14, 360)
    for cap in (16, 40):
        fresh = ReplayWindow(DEV, max_generations=3, capacity_rows=cap)
        fresh.load_state_dict(state)
        assert [(g, n) for g, _, n in fresh.generations] == [(4, 7), (5, 7)]
        assert cap != 16 or fresh.generations == w.generations
        assert _same_rows(fresh.gather(fresh.slots_of(4)), b_kept) and _same_rows(fresh.gather(fresh.slots_of(5)), c)
        with pytest.raises(ValueError):
            fresh.add_generation(a, generation=5)                   # the id counter came along
        assert fresh.add_generation(a)["generation"] == 6
    with pytest.raises(ValueError):
        ReplayWindow(DEV, max_generations=1, capacity_rows=16).load_state_dict(state)
    sel = w.select(3, seed=1)
    assert sel[:7].tolist() == w.slots_of(5).tolist() and sel.numel() == 10 and set(sel[7:].tolist()) <= set(w.slots_of(4).tolist())


# ---- the trainer -----------------------------------------------------------------------------------------------------
@pytest.fixture
def deterministic_training(monkeypatch):
    """The recipe of tests/test_gpu_symmetry.py: fixed convolution kernels and MIOpen's deterministic algorithms."""
    monkeypatch.setenv("LZ_TRAIN_MIOPEN", "immediate")
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _weights(model):
    torch.cuda.synchronize()
    return torch.cat([p.detach().float().flatten() for p in model.parameters()]).cpu()


def _train_tensors(batch, **kw):
    from liuzhou_amd.train_bridge import train_network_from_tensors
    from tests.test_gpu_symmetry import _model
    torch.manual_seed(123)
    model, m = train_network_from_tensors(_model(), batch, batch_size=256, epochs=2, lr=2e-3, device=DEV, **kw)
    return _weights(model), m


def _train_window(generations, **kw):
    from liuzhou_amd.replay_window import ReplayWindow
    from liuzhou_amd.train_bridge import train_network_from_window
    from tests.test_gpu_symmetry import _model
    w = ReplayWindow(DEV, max_generations=len(generations), capacity_rows=sum(g.num_samples for g in generations) + 5)
    w.add_generation(generations[0], generation=3)                  # off slot 0 from the second generation on
    for g in generations[1:]:
        w.add_generation(g)
    torch.manual_seed(123)
    model, m = train_network_from_window(_model(), w, batch_size=256, epochs=2, lr=2e-3, device=DEV, **kw)
    return _weights(model), m


def test_window_trainer_equals_the_tensor_trainer(deterministic_training, L):
    from tests.test_gpu_symmetry import _dataset
    data = _dataset()
    assert data.num_samples == 1536
    _train_tensors(data)                                            # warm-up: kernel selection, allocator
    # (a) one generation: the same weights and epoch statistics, with and without augmentation
    for kw in ({}, {"symmetry_augment": True, "symmetry_seed": 9}):
        w_t, m_t = _train_tensors(data, **kw)
        w_w, m_w = _train_window([data], **kw)
        assert torch.equal(w_t, w_w), (kw, float((w_t - w_w).abs().max()))
        assert m_t["epoch_stats"] == m_w["epoch_stats"]
        assert m_t.get("symmetry_augment") == m_w.get("symmetry_augment")
        assert set(m_w) - set(m_t) == {"replay_window"} and set(m_t) <= set(m_w)
        assert m_w["num_samples"] == 1536 and m_w["replay_window"]["rows_selected"] == [1536]
    assert m_w["replay_window"]["generations"] == [3] and m_w["replay_window"]["window_rows"] == 1536
    assert m_w["replay_window"]["window_bytes"] == (1536 + 5) * 360
    # (b) two generations, the whole older one: the concatenation, newest first
    old, new = _slice(data, 0, 512), _slice(data, 512, 1536)
    w_t, m_t = _train_tensors(_cat(new, old))
    w_w, m_w = _train_window([old, new], replay_budget_per_generation=512)
    assert torch.equal(w_t, w_w) and m_t["epoch_stats"] == m_w["epoch_stats"]
    assert m_w["replay_window"]["generations"] == [4, 3] and m_w["replay_window"]["rows_selected"] == [1024, 512]


def test_window_trainer_budget_rule(deterministic_training, L):
    from tests.test_gpu_symmetry import _dataset
    data = _dataset()
    gens = [_slice(data, 0, 600), _slice(data, 600, 1000), _slice(data, 1000, 1536)]
    _, m = _train_window(gens, replay_budget_per_generation=100)
    assert m["replay_window"]["rows_held"] == [536, 400, 600] and m["replay_window"]["rows_selected"] == [536, 100, 100]
    assert m["num_samples"] == 736 and m["total_train_steps"] == 2 * 3
    _, m = _train_window(gens)                                      # budget 0: 536 // 2 from each older generation
    assert m["replay_window"]["rows_selected"] == [536, 268, 268] and m["num_samples"] == 1072
    assert m["replay_window"]["generations"] == [5, 4, 3] and m["replay_window"]["evicted"] == []
    assert m["total_train_steps"] == 2 * 5


# ---- plumbing --------------------------------------------------------------------------------------------------------
def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_gather_trajectories_returns_the_records_in_a_group_of_one(L):
    """tests/replay_world1.py in a child process with a time limit, like the world-size-1 RCCL test."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    try:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "replay_world1.py"), str(_free_port())],
                             capture_output=True, text=True, timeout=240, env=env)
    except subprocess.TimeoutExpired as exc:
        pytest.fail(f"the world-size-1 job did not finish in 240 s: {exc.stdout} {exc.stderr}")
    assert res.returncode == 0, res.stdout + res.stderr
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    assert out == {"world": 1, "rows": out["rows"], "forced_equals_pack_batch": True, "unforced_equals_pack_batch": True,
                   "default_returns_the_batch": True, "records_shape_ok": True} and out["rows"] > 0


PARENT_KEYS = {"workload", "world_size", "backend", "overlap", "player_ranks", "trainer_rank", "iterations", "tail",
               "steady_state_positions_per_sec"}
PARENT_ITERATION_KEYS = {"iteration", "positions", "self_play_sec", "gather_sec", "train_sec", "handoff_sec", "iteration_sec",
                         "positions_per_sec", "train_samples", "avg_loss", "samples_stepped", "weights_equal_on_all_ranks",
                         "weights_digest", "net_check"}


def _staged_loop(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "staged_loop.py"), "--iterations", "3",
                          "--games-per-gpu", "64", "--sims", "8", "--max-game-plies", "40", "--batch-size", "512", *extra],
                         capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])


def test_staged_loop_trains_on_a_window_of_two_generations(L):
    out = _staged_loop("--replay-generations", "2")
    its = out["iterations"]
    assert set(out) == PARENT_KEYS and len(its) == 3
    for it in its:
        assert set(it) == PARENT_ITERATION_KEYS | {"replay"}
    held = [it["positions"] - it["replay"]["filtered_non_finite_rows"] for it in its]       # rows that entered the window
    assert its[0]["replay"]["generations"] == [1] and its[0]["train_samples"] == held[0] > 0
    r = its[1]["replay"]
    assert r["generations"] == [2, 1] and r["rows_held"] == [held[1], held[0]]
    assert r["rows_selected"] == [held[1], min(held[0], held[1])]                           # budget 0: newest // 1
    assert its[1]["train_samples"] == held[1] + r["rows_selected"][1]
    assert its[2]["replay"]["generations"] == [3, 2] and its[2]["replay"]["evicted"] == [1]
    assert r["window_bytes"] == 2 * 64 * 40 * 360 and r["window_rows"] == held[0] + held[1]
    assert all(it["avg_loss"] is not None for it in its)


def test_staged_loop_default_keeps_the_parent_keys(L):
    out = _staged_loop()
    assert set(out) == PARENT_KEYS
    for it in out["iterations"]:
        assert set(it) == PARENT_ITERATION_KEYS and it["train_samples"] == it["positions"]


def test_staged_loop_lag1_three_ranks_feed_the_window_with_gathered_records(L):
    """Two players and a trainer on one GPU (gloo, as tests/test_gpu_distributed.py runs them), lag-1 schedule: the records
    of the gather go into the window under the generation they were played in, the tail included.  A game cannot end
    within 6 plies, so every generation has 2 x 48 x 6 rows."""
    from tests.test_gpu_distributed import _staged_loop as multi_rank_loop
    rows = 2 * 48 * 6
    out = multi_rank_loop(3, 1, iterations=3, games=48, plies=6, extra=("--replay-generations", "2"))
    its = out["iterations"]
    assert [it["positions"] for it in its] == [rows] * 3 and out["overlap"] == 1
    assert its[0]["train_samples"] == 0 and its[0]["replay"] is None              # nothing gathered yet
    assert its[1]["train_samples"] == rows and its[1]["replay"]["generations"] == [1]
    assert its[2]["train_samples"] == 2 * rows and its[2]["replay"]["generations"] == [2, 1]
    assert its[2]["replay"]["rows_selected"] == [rows, rows] and its[2]["replay"]["window_bytes"] == 2 * 2 * 48 * 6 * 360
    tail = out["tail"]
    assert tail["train_samples"] == 2 * rows and tail["replay"]["generations"] == [3, 2] and tail["replay"]["evicted"] == [1]
    assert all(it["weights_equal_on_all_ranks"] is True for it in its) and tail["avg_loss"] is not None
