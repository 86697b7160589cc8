"""GPU: merging duplicate positions across the replay window, record to record -- the two kernels
of csrc/lz_replay_merge.hip through the C ABI against the restatement (tests/replay_merge_ref.py, anchored on the host
build by tests/test_replay_merge_cpu.py) and against the live composition they replace (unpack, the tensor kernels of
csrc/lz_dedup.hip, pack), byte for byte; `train_network_from_window(replay_merge_positions=...)` against itself with the
merge off and against the tensor trainer's `dedup_weighting="weight"`, weight for weight; one staged-loop iteration
against the same call made by hand."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from tests import position_dedup as PD
from tests import replay_merge_ref as R
from tests.test_gpu_row_weights import (DEV, FIVE, _batch, _model, _stack, _take, _train, _train_window, _weights,  # noqa: F401
                                        deterministic_training, unique_rows)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261021
ERR_ARG, ERR_ALIGN = -1, -4
GUARD = 0xA5


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from liuzhou_amd import _lib
    return _lib


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def gpu_keys(L, rec, slots, symmetric, capacity=None):
    """lz_replay_position_keys on device copies, the outputs followed by guard bytes that must stay."""
    m = len(slots)
    d_rec, d_slots = dv(rec), dv(np.asarray(slots, np.int64))
    keys = torch.full((m + 1, 8), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    sym = torch.full((m + 8,), 0x5A, dtype=torch.int8, device=DEV)
    bad = torch.zeros(2, dtype=torch.int32, device=DEV)
    bad[1] = 77
    st = L.lib().lz_replay_position_keys(L.ptr(d_rec), L.i64(len(rec) if capacity is None else capacity), L.ptr(d_slots),
                                         L.i64(m), int(symmetric), L.ptr(keys), L.ptr(sym), L.ptr(bad), L.stream_ptr(DEV))
    torch.cuda.synchronize()
    keys, sym, bad = keys.cpu().numpy(), sym.cpu().numpy(), bad.cpu().numpy()
    assert (keys[m] == 0x5A5A5A5A5A5A5A5A).all() and (sym[m:] == 0x5A).all() and bad[1] == 77
    return st, keys[:m].copy(), sym[:m].copy(), int(bad[0])


def gpu_merge(L, rec, slots, sym, order, begin, capacity=None):
    G = len(begin) - 1
    d = [dv(rec), dv(np.asarray(slots, np.int64)), dv(np.asarray(sym, np.int8)), dv(np.asarray(order, np.int64)),
         dv(np.asarray(begin, np.int64))]
    out = torch.full((G + 1, 360), GUARD, dtype=torch.uint8, device=DEV)
    count = torch.full((G + 1,), -7, dtype=torch.int32, device=DEV)
    over = torch.zeros(2, dtype=torch.int32, device=DEV)
    over[1] = 77
    st = L.lib().lz_replay_merge_records(L.ptr(d[0]), L.i64(len(rec) if capacity is None else capacity), L.ptr(d[1]),
                                         L.i64(len(slots)), L.ptr(d[2]), L.ptr(d[3]), L.ptr(d[4]), L.i64(G), L.ptr(out),
                                         L.ptr(count), L.ptr(over), L.stream_ptr(DEV))
    torch.cuda.synchronize()
    out, count, over = out.cpu().numpy(), count.cpu().numpy(), over.cpu().numpy()
    assert (out[G] == GUARD).all() and count[G] == -7 and over[1] == 77
    return st, out[:G].copy(), count[:G].copy(), int(over[0])


# ---- the kernels against the restatement -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rings():
    rng = np.random.default_rng(SEED)
    out = {}
    for name, rec in (("grid", R.grid_records(SEED, False)), ("grid spread", R.grid_records(SEED, True)),
                      ("edges", R.edge_records(SEED)[0])):
        slots = np.concatenate([rng.permutation(len(rec)), rng.integers(0, len(rec), 7)]).astype(np.int64)
        out[name] = (np.ascontiguousarray(rec), slots)
    return out


@pytest.mark.parametrize("mode", PD.MODES)
@pytest.mark.parametrize("name", ["grid", "grid spread", "edges"])
def test_kernels_are_bit_identical_to_the_restatement(L, rings, name, mode):
    rec, slots = rings[name]
    symmetric = int(mode == "symmetric")
    want_keys, want_sym, _ = R.keys_ref(rec, slots, symmetric)
    st, keys, sym, bad = gpu_keys(L, rec, slots, symmetric)
    assert st == 0 and bad == 0 and _same(keys, want_keys) and _same(sym, want_sym)
    _, order, begin = PD.group(want_keys)
    want, want_count, want_over = R.merge_ref(rec, slots, want_sym, order, begin)
    st, out, count, over = gpu_merge(L, rec, slots, want_sym, order, begin)
    assert st == 0 and over == want_over and _same(count, want_count)
    for g in range(len(count)):
        assert _same(out[g], want[g]), (name, mode, g, int(count[g]))


def test_kernels_on_a_wrapping_selection_with_repeated_and_invalid_slots(L):
    rec = R.grid_records(SEED, True)
    ring = np.ascontiguousarray(np.concatenate([rec[:6], rec[:6], rec[100:104]]))     # 16 slots
    slots = np.array([13, 14, 15, 0, 1, 2, 3, 3, 5, 3, -1, 16, 7, 1 << 40, -(1 << 62)], np.int64)
    for symmetric in (0, 1):
        want_keys, want_sym, want_bad = R.keys_ref(ring, slots, symmetric)
        st, keys, sym, bad = gpu_keys(L, ring, slots, symmetric)
        assert st == 0 and bad == want_bad == 4 and _same(keys, want_keys) and _same(sym, want_sym)
        gor, order, begin = PD.group(keys)
        want, want_count, want_over = R.merge_ref(ring, slots, sym, order, begin)
        st, out, count, over = gpu_merge(L, ring, slots, sym, order, begin)
        assert st == 0 and over == want_over and _same(count, want_count) and _same(out, want)
        for j in (10, 11, 13, 14):
            assert count[gor[j]] == 0 and not out[gor[j]].any()


def test_kernel_gives_zero_records_for_bad_order_range_slot_and_sym(L):
    rec = R.grid_records(SEED, True)
    slots = np.arange(len(rec), dtype=np.int64)
    keys, sym, _ = R.keys_ref(rec, slots, 1)
    _, order, begin = PD.group(keys)
    m = len(slots)
    big = int(np.argmax(np.diff(begin)))
    _, good, good_count, _ = gpu_merge(L, rec, slots, sym, order, begin)
    broken = order.copy()
    broken[begin[big] + 555] = m                                     # an entry of the last chunk
    st, out, count, over = gpu_merge(L, rec, slots, sym, broken, begin)
    want, want_count, want_over = R.merge_ref(rec, slots, sym, broken, begin)
    assert st == 0 and count[big] == 0 and not out[big].any() and _same(out, want) and _same(count, want_count)
    far, odd = slots.copy(), sym.copy()
    far[order[begin[big] + 599]] = len(rec)
    st, out, count, _ = gpu_merge(L, rec, far, sym, order, begin)
    assert st == 0 and count[big] == 0 and not out[big].any() and _same(np.delete(out, big, 0), np.delete(good, big, 0))
    odd[order[begin[big] + 300]] = 8
    st, out, count, _ = gpu_merge(L, rec, slots, odd, order, begin)
    assert st == 0 and count[big] == 0 and not out[big].any() and _same(np.delete(out, big, 0), np.delete(good, big, 0))
    ranges = np.array([5, 5, 3, m + 1, m + 2], np.int64)             # empty, reversed, past the end, impossible
    st, out, count, _ = gpu_merge(L, rec, slots, sym, order, ranges)
    assert st == 0 and not count.any() and not out.any()


def test_kernels_refuse_bad_arguments_without_a_launch(L):
    rec = dv(R.edge_records(SEED)[0])
    n = int(rec.shape[0])
    slots, order = torch.arange(n, device=DEV), torch.arange(n, device=DEV)
    keys, sym = torch.zeros((n, 8), dtype=torch.int64, device=DEV), torch.zeros(n, dtype=torch.int8, device=DEV)
    bad, begin = torch.zeros(1, dtype=torch.int32, device=DEV), torch.tensor([0, n], device=DEV)
    out, count = torch.full((1, 360), 9, dtype=torch.uint8, device=DEV), torch.full((1,), 9, dtype=torch.int32, device=DEV)
    K, M, p, s = L.lib().lz_replay_position_keys, L.lib().lz_replay_merge_records, L.ptr, L.stream_ptr(DEV)
    assert K(None, 0, None, 0, 1, None, None, None, s) == 0
    assert K(p(rec), n, p(slots), -1, 1, p(keys), p(sym), p(bad), s) == ERR_ARG
    assert K(p(rec), -1, p(slots), n, 1, p(keys), p(sym), p(bad), s) == ERR_ARG
    assert K(p(rec), n, p(slots), n, 2, p(keys), p(sym), p(bad), s) == ERR_ARG
    for i in (0, 2, 5, 6, 7):
        args = [p(rec), n, p(slots), n, 1, p(keys), p(sym), p(bad)]
        args[i] = None
        assert K(*args, s) == ERR_ARG, i
    assert K(rec.data_ptr() + 4, n - 1, p(slots), n, 1, p(keys), p(sym), p(bad), s) == ERR_ALIGN
    assert K(p(rec), n, p(slots), n, 1, keys.data_ptr() + 4, p(sym), p(bad), s) == ERR_ALIGN
    good = [p(rec), n, p(slots), n, p(sym), p(order), p(begin), 1, p(out), p(count), p(bad)]
    assert M(*good[:7], 0, None, None, None, s) == 0 and M(*good[:3], 0, *good[4:], s) == 0
    for i, value in ((1, -1), (3, -1), (7, -1)):
        args = list(good)
        args[i] = value
        assert M(*args, s) == ERR_ARG
    for i in (0, 2, 4, 5, 6, 8, 9, 10):
        args = list(good)
        args[i] = None
        assert M(*args, s) == ERR_ARG, i
    for i, t in ((0, rec), (5, order), (6, begin), (8, out)):
        args = list(good)
        args[3], args[i] = n - 1, t.data_ptr() + 4
        assert M(*args, s) == ERR_ALIGN, i
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and int(count[0]) == 9 and int(bad[0]) == 0 and not bool(keys.any())


# ---- the kernels against the live composition -------------------------------------------------------------------------------------
def test_kernels_equal_unpack_tensor_merge_pack_on_the_grid(L):
    from liuzhou_amd import position_dedup as D
    from liuzhou_amd import replay_window as RW
    from liuzhou_amd.trajectory_codec import pack_batch, unpack_records
    a, b = PD.grid(SEED, True), PD.grid(SEED + 1, False)
    rows = {f: np.concatenate([a[f], b[f][:700]]) for f in FIVE}     # all eight frames, and about 300 identical rows
    n = len(rows["value"])
    assert 2000 <= n <= 2200
    ring, _ = pack_batch(_batch(rows), return_bad=True)              # the rows that are not representable: any 360 bytes
    slots = torch.from_numpy(np.random.default_rng(SEED).permutation(n)).to(DEV)
    live = unpack_records(ring.index_select(0, slots))
    for mode in PD.MODES:
        want_keys, want_sym, want_bad = D.position_keys(live.state_tensors, live.legal_masks, symmetric=mode == "symmetric")
        keys, sym, bad = RW.record_position_keys(ring, slots, symmetric=mode == "symmetric")
        assert int(bad) == int(want_bad) == 0 and torch.equal(keys, want_keys) and torch.equal(sym, want_sym)
        outs, info = D.merge_duplicate_positions(live.state_tensors, live.legal_masks, live.policy_targets, live.value_targets,
                                                 live.soft_value_targets, mode=mode, max_copies=4, weighting="weight")
        from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
        want, want_over = pack_batch(TensorSelfPlayBatch(*outs), return_bad=True)
        _, order, begin, _ = D.group_rows(keys)
        merged, count, over = RW.merge_record_groups(ring, slots, sym, order, begin)
        assert int(over) == int(want_over) and torch.equal(count, info["count"])
        assert tuple(merged.shape) == (info["groups"], 360) and torch.equal(merged, want)
        assert info["merged_groups"] >= 10 and (mode == "exact" or info["largest_group"] >= 600)


# ---- the trainer --------------------------------------------------------------------------------------------------------------------
def _images(rows, k, seed):
    """The rows under the board symmetry k, each with a policy of its own on its legal actions."""
    from liuzhou_amd import symmetry as SY
    rng = np.random.default_rng(seed)
    n = len(rows["value"])
    pl, mk, _ = SY.np_transform_samples(rows["planes"], rows["masks"], rows["policy"], k)
    pol = (rng.random((n, 220)) * (mk != 0)).astype(np.float32)
    pol /= pol.sum(axis=1, keepdims=True, dtype=np.float32)
    return {"planes": np.ascontiguousarray(pl, np.float32).reshape(rows["planes"].shape), "masks": np.ascontiguousarray(mk, np.uint8),
            "policy": pol, "value": rng.integers(-1, 2, n).astype(np.float32), "soft": rng.uniform(-1, 1, n).astype(np.float32)}


MERGE_KEYS = {"rows_in", "rows_out", "groups", "merged_groups", "merged_rows", "largest_group", "not_representable", "mode",
              "max_weight", "merge_sec"}


def test_merge_on_a_window_without_duplicates_trains_to_the_same_bits(deterministic_training, unique_rows, L):
    old, new = _take(unique_rows, 0, 96), _take(unique_rows, 96, 256)
    _train_window([old, new], replay_budget_per_generation=96)      # warm-up: kernel selection, allocator
    for decay in ({}, {"replay_age_decay": 0.5}):
        w_off, m_off = _train_window([old, new], replay_budget_per_generation=96, **decay)
        for mode in ("exact", "symmetric"):
            w_on, m_on = _train_window([old, new], replay_budget_per_generation=96, replay_merge_positions=mode, **decay)
            assert torch.equal(w_off, w_on), (decay, mode, float((w_off - w_on).abs().max()))
            merge = m_on["replay_window"]["merge"]
            assert set(merge) == MERGE_KEYS and merge["rows_in"] == merge["rows_out"] == merge["groups"] == 256
            assert merge["merged_groups"] == 0 and merge["largest_group"] == 1 and merge["mode"] == mode
            assert m_on["num_samples"] == m_off["num_samples"] == 256 and "merge" not in m_off["replay_window"]
            assert m_on["row_weights"] == {"source": "replay_merge", "min": 0.5 if decay else 1.0, "max": 1.0,
                                           "zero_weight_rows": 0}
            assert [st["samples"] for st in m_on["epoch_stats"]] == [st["samples"] for st in m_off["epoch_stats"]]


def test_one_generation_with_duplicates_equals_the_tensor_trainer_with_weights(deterministic_training, unique_rows, L):
    x = unique_rows
    rows = _stack(x, _images(_take(x, 0, 64), 1, 1), _images(_take(x, 32, 96), 6, 2), _take(x, 200, 232))
    kw = {"dedup_positions": "symmetric", "dedup_max_copies": 4, "dedup_weighting": "weight"}
    _train(rows, **kw)                                              # warm-up
    w_tensor, m_tensor = _train(rows, **kw)
    w_window, m_window = _train_window([rows], replay_merge_positions="symmetric", replay_merge_max_weight=4)
    assert torch.equal(w_tensor, w_window), float((w_tensor - w_window).abs().max())
    d, merge = m_tensor["position_dedup"], m_window["replay_window"]["merge"]
    assert {k: merge[k] for k in d if k in merge and k != "mode"} == {k: d[k] for k in d if k in merge and k != "mode"}
    assert merge["groups"] == 256 and merge["rows_in"] == 416 and merge["largest_group"] == 3 and merge["merged_groups"] == 128
    assert m_window["num_samples"] == 256 and m_window["row_weights"] == dict(m_tensor["row_weights"], source="replay_merge")
    assert m_window["row_weights"]["max"] == 3.0 and m_window["row_weights"]["min"] == 1.0
    # the cap: weight min(count, 2)
    _, m_two = _train_window([rows], replay_merge_positions="symmetric", replay_merge_max_weight=2)
    assert m_two["row_weights"]["max"] == 2.0
    # exact mode merges the identical copies alone
    _, m_exact = _train_window([rows], replay_merge_positions="exact", replay_merge_max_weight=4)
    exact = len(np.unique(PD.keys(rows["planes"], rows["masks"], False)[0], axis=0))
    assert m_exact["replay_window"]["merge"]["groups"] == exact <= 416 - 32


@pytest.mark.parametrize("augment", [False, True])
def test_two_generations_equal_the_tensor_trainer_on_the_concatenation(deterministic_training, unique_rows, L, augment):
    x = unique_rows
    old = _stack(_take(x, 0, 128), _images(_take(x, 100, 160), 3, 3))
    new = _stack(_take(x, 64, 256), _images(_take(x, 0, 32), 5, 4))
    kw = {"symmetry_augment": True, "symmetry_seed": 11} if augment else {}
    _train(_stack(new, old), dedup_positions="symmetric", **kw)     # warm-up
    w_tensor, m_tensor = _train(_stack(new, old), dedup_positions="symmetric", dedup_max_copies=4, dedup_weighting="weight", **kw)
    w_window, m_window = _train_window([old, new], replay_budget_per_generation=10 ** 6, replay_merge_positions="symmetric",
                                       replay_merge_max_weight=4, **kw)
    assert torch.equal(w_tensor, w_window), float((w_tensor - w_window).abs().max())
    merge = m_window["replay_window"]["merge"]
    assert merge["rows_in"] == 188 + 224 and merge["groups"] == 256 == m_tensor["position_dedup"]["groups"]
    assert m_window["replay_window"]["rows_selected"] == [224, 188]
    if augment:
        assert m_window["symmetry_augment"] == m_tensor["symmetry_augment"]


def test_merge_is_refused_with_the_draw_options_on_a_filled_window(unique_rows, L):
    from liuzhou_amd.replay_window import ReplayWindow
    from liuzhou_amd.train_bridge import train_network_from_window
    w = ReplayWindow(DEV, max_generations=1, capacity_rows=64)
    w.add_generation(_batch(_take(unique_rows, 0, 64)))
    for kw in ({"policy_draw_weight": 0.5}, {"anti_draw_penalty": 0.1}):
        with pytest.raises(ValueError, match="drawn game"):
            train_network_from_window(None, w, replay_merge_positions="exact", device=DEV, **kw)


# ---- the staged loop ----------------------------------------------------------------------------------------------------------------
def test_a_staged_loop_iteration_with_the_flag_equals_the_call_by_hand(deterministic_training, monkeypatch, capsys, L):
    import json
    from liuzhou_amd import train_bridge as TB
    from liuzhou_amd.replay_window import ReplayWindow
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    cli = __import__("staged_loop")
    real = TB.train_network_from_window
    calls = []

    def spy(model, window, **kw):
        before = (copy.deepcopy(model), window.state_dict(), window.table.max_generations, window.table.capacity_rows,
                  torch.get_rng_state(), torch.cuda.get_rng_state(DEV))
        model, metrics = real(model, window, **kw)
        calls.append((before, kw, _weights(model), metrics))
        return model, metrics
    monkeypatch.setattr(TB, "train_network_from_window", spy)
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    assert cli.main(["--iterations", "2", "--games-per-gpu", "64", "--sims", "8", "--max-game-plies", "40", "--batch-size", "512",
                     "--replay-generations", "2", "--replay-merge-positions", "symmetric", "--replay-merge-max-weight", "4"]) == 0
    out = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    its = out["iterations"]
    assert len(its) == len(calls) == 2
    for it, (_, kw, _, metrics) in zip(its, calls):
        assert kw["replay_merge_positions"] == "symmetric" and kw["replay_merge_max_weight"] == 4.0 and "replay_age_decay" not in kw
        merge = it["replay"]["merge"]
        assert merge == metrics["replay_window"]["merge"] and set(merge) == MERGE_KEYS
        assert merge["rows_in"] == sum(it["replay"]["rows_selected"]) and it["train_samples"] == merge["groups"] < merge["rows_in"]
        assert merge["merged_groups"] > 0 and merge["largest_group"] >= 64        # every game starts from the empty board
        assert it["row_weights"]["source"] == "replay_merge" and it["row_weights"]["max"] == 4.0
    assert its[1]["replay"]["generations"] == [2, 1]
    (model, state, gens, rows, cpu_rng, gpu_rng), kw, want, metrics = calls[1]     # the second iteration, by hand
    window = ReplayWindow(DEV, max_generations=gens, capacity_rows=rows)
    window.load_state_dict(state)
    torch.set_rng_state(cpu_rng)
    torch.cuda.set_rng_state(gpu_rng, DEV)
    model, mine = real(model, window, **kw)
    assert torch.equal(_weights(model), want)
    drop = lambda m: {k: v for k, v in m.items() if not k.endswith("_sec")}
    assert drop(mine["replay_window"]["merge"]) == drop(metrics["replay_window"]["merge"])
    assert mine["row_weights"] == metrics["row_weights"] and mine["num_samples"] == metrics["num_samples"]
