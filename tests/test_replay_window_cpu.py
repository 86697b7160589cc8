"""CPU: the replay window's bookkeeping and selection rule (liuzhou_amd/replay_window.py), the numpy restatement of the
record decoder (tests/replay_ref.py) against hand-written records, and what the new entry points refuse."""
import inspect

import numpy as np
import pytest
import torch

from liuzhou_amd import replay_window as RW
from tests import replay_ref as R


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ---- hand-written records --------------------------------------------------------------------------------------------
# actions 0..35 and 180..215: mask words 0 (all), 1 (bits 0..3), 5 (bits 20..31 = actions 180..191), 6 (bits 0..23)
_M72 = [0xFFFFFFFF, 0x0000000F, 0, 0, 0, 0xFFF00000, 0x00FFFFFF]
_P72 = [(i + 1) / 128.0 for i in range(72)]
_A72 = list(range(36)) + list(range(180, 216))

HAND = {
    # phase 0, no legal action: own on cells 0 and 5, opponent on cell 1
    "phase0_none": R.make_record([0x21, 0x2, 0, 0], [0] * 7, [], 1.0, 0.5),
    # phase 7, one legal action (219); every bit and byte the layout does not own is set: w0 above bit 38, w1..w3 above
    # bit 35, mask bits 220..223, policy slots past the legal count, the pad
    "phase7_one": R.make_record([(7 << 36) | (1 << 35) | (1 << 40) | (1 << 63), 1 << 63, (1 << 35) | (1 << 36), 1 << 50],
                                [0, 0, 0, 0, 0, 0, 0xF8000000], [1.0, 5.0, 7.0], -1.0, -0.25, pad=0xDEADBEEF),
    # phase 3, 72 legal actions: the policy slots go to the legal actions in ascending order
    "phase3_72": R.make_record([(3 << 36) | (1 << 7), 1 << 8, 1 << 7, 0], _M72, _P72, 0.0, 0.125),
    # 73 legal bits: the 73rd (action 219) gets policy 0
    "phase3_73": R.make_record([(3 << 36) | (1 << 7), 1 << 8, 1 << 7, 0], _M72[:6] + [0x08FFFFFF], _P72, 0.0, 0.125),
}


def _expect(own=(), opp=(), own_marked=(), opp_marked=(), phase=0, legal=(), policy=()):
    planes = np.zeros((11, 36), np.float32)
    for p, cells in enumerate((own, opp, own_marked, opp_marked)):
        planes[p, list(cells)] = 1.0
    if phase:
        planes[3 + phase] = 1.0
    masks = np.zeros(220, np.uint8)
    masks[list(legal)] = 1
    pol = np.zeros(220, np.float32)
    for a, p in zip(legal, policy):
        pol[a] = p
    return planes.reshape(11, 6, 6), masks, pol


EXPECTED = {
    "phase0_none": (_expect(own=(0, 5), opp=(1,)), 1.0, 0.5),
    "phase7_one": (_expect(own=(35,), own_marked=(35,), phase=7, legal=(219,), policy=(1.0,)), -1.0, -0.25),
    "phase3_72": (_expect(own=(7,), opp=(8,), own_marked=(7,), phase=3, legal=_A72, policy=_P72), 0.0, 0.125),
    "phase3_73": (_expect(own=(7,), opp=(8,), own_marked=(7,), phase=3, legal=_A72 + [219], policy=_P72 + [0.0]), 0.0, 0.125),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_decoder_on_hand_written_records(name):
    planes, masks, policy, value, soft = R.decode_records(HAND[name][None, :])
    (ep, em, eq), ev, es = EXPECTED[name]
    assert np.array_equal(planes[0], ep)
    assert np.array_equal(masks[0], em)
    assert np.array_equal(policy[0], _bits(eq))
    assert value[0] == _bits(ev) and soft[0] == _bits(es)
    assert int(masks[0].sum()) == {"phase0_none": 0, "phase7_one": 1, "phase3_72": 72, "phase3_73": 73}[name]


def test_decoder_carries_policy_bit_patterns_and_gather_ref_zeroes_invalid_rows():
    odd = [0x7FC12345, 0x80000000, 0x00000001, 0x7F800000]          # NaN payload, -0.0, subnormal, +inf
    rec = R.make_record([0, 0, 0, 0], [0b1111, 0, 0, 0, 0, 0, 0], odd, 1.0, -1.0)
    _, masks, policy, _, _ = R.decode_records(rec[None, :])
    assert policy[0, :4].tolist() == odd and int(masks[0].sum()) == 4
    ring = np.stack([HAND["phase3_72"], rec])
    planes, masks, policy, value, soft = R.gather_ref(ring, [1, -1, 2, 0, 0], [0, 0, 0, 8, 1])
    assert policy[0, :4].tolist() == odd
    for j in (1, 2, 3):                                              # slot -1, slot == capacity, id 8
        assert not planes[j].any() and not masks[j].any() and not policy[j].any() and value[j] == 0 and soft[j] == 0
    # rotate 90: (r, c) -> (c, 5 - r); cell 7 = (1, 1) -> (1, 4) = cell 10, action 0 -> action 5
    assert planes[4, 0].reshape(36)[10] == 1.0 and planes[4, 0].sum() == 1.0
    assert policy[4, 5] == _bits(1 / 128.0) and value[4] == _bits(0.0) and soft[4] == _bits(0.125)


# ---- table against the list model ------------------------------------------------------------------------------------
def test_table_and_ring_model_agree_over_a_scripted_sequence():
    table, model = RW.GenerationTable(3, 10), R.RingModel(3, 10)
    script = [(4, None), (3, None), (0, None), (11, None), (2, 1), (2, 5), (5, 9), (3, 9), (10, 20), (-1, None), (1, None),
              (1, None), (1, None), (7, 30)]
    saw_wrap = saw_count_evict = saw_capacity_evict = False
    errors = 0
    for count, gid in script:
        before = (list(table.entries), table.head, table.last_id)
        try:
            want = model.add(count, gid)
        except ValueError:
            with pytest.raises(ValueError):
                table.add(count, gid)
            assert (list(table.entries), table.head, table.last_id) == before        # a refusal changes nothing
            errors += 1
            continue
        live_before, rows_before = len(before[0]), sum(c for _, _, c in before[0])
        got = table.add(count, gid)
        assert got == want
        if want["evicted"]:
            if rows_before + count > 10:
                saw_capacity_evict = True
            elif live_before + 1 > 3:
                saw_count_evict = True
        assert [g for g, _, _ in table.entries] == model.order
        assert table.num_rows == model.live_rows() <= 10 and len(table.entries) <= 3
        for g, first, cnt in table.entries:
            slots = [(first + r) % 10 for r in range(cnt)]
            assert slots == model.slots(g)
            saw_wrap = saw_wrap or first + cnt > 10
    # (0), (11), (2 as id 1), (3 as id 9 again), (-1): an empty generation, one larger than the ring, two stale ids
    assert errors == 5 and saw_wrap and saw_count_evict and saw_capacity_evict
    with pytest.raises(ValueError):
        RW.GenerationTable(0, 10)
    with pytest.raises(ValueError):
        RW.GenerationTable(2, 0)


# ---- selection -------------------------------------------------------------------------------------------------------
def _table():
    t = RW.GenerationTable(4, 100)
    t.add(30, 1)
    t.add(40, 2)          # evicted below
    t.add(25, 3)
    t.add(20, 5)          # 30 + 40 + 25 + 20 > 100: generation 1 goes, the ring wraps
    t.add(12, 8)
    return t


def _ranges(t):
    return {g: {(f + r) % t.capacity_rows for r in range(c)} for g, f, c in t.entries}


@pytest.mark.parametrize("budget", [7, 22, 1000, 0, -3])
def test_select_follows_the_rule_on_the_cpu_generator(budget):
    t = _table()
    assert [g for g, _, _ in t.entries] == [2, 3, 5, 8]
    ranges = _ranges(t)
    live = set().union(*ranges.values())
    evicted = set(range(100)) - live
    state = torch.random.get_rng_state().clone()
    slots = RW.select_slots(t, budget, 11, "cpu")
    assert torch.equal(torch.random.get_rng_state(), state)                          # the default stream is untouched
    assert slots.dtype == torch.int64
    s = slots.tolist()
    assert len(set(s)) == len(s) and not set(s) & evicted
    eff = budget if budget > 0 else 12 // 3
    want = [(8, 12), (5, min(20, eff)), (3, min(25, eff)), (2, min(40, eff))]
    assert [(g, k) for g, _, _, k in t.shares(budget)] == want
    pos = 0
    for (g, k), (_, first, count) in zip(want, reversed(t.entries)):
        part = s[pos:pos + k]
        pos += k
        assert set(part) <= ranges[g]
        rows = [(x - first) % 100 for x in part]
        assert rows == sorted(rows)                                                  # ascending row order
        if g == 8 or k == count:
            assert rows == list(range(count))                                        # everything, in row order
    assert pos == len(s)
    again = RW.select_slots(t, budget, 11, "cpu")
    assert torch.equal(slots, again)                                                 # same (seed, ids): same draw


def test_select_depends_on_seed_and_newest_id_and_draws_uniformly():
    def table(newest):
        t = RW.GenerationTable(2, 3000)
        t.add(1000, 1)
        t.add(10, newest)
        return t
    a = RW.select_slots(table(2), 200, 5, "cpu")
    assert torch.equal(a, RW.select_slots(table(2), 200, 5, "cpu"))
    assert not torch.equal(a, RW.select_slots(table(3), 200, 5, "cpu"))              # another newest id
    assert not torch.equal(a, RW.select_slots(table(2), 200, 6, "cpu"))              # another seed
    assert a.numel() == 210 and a[:10].tolist() == list(range(1000, 1010))
    # without replacement from the whole generation: over 50 seeds every quarter of it gets its share (250 +- 6 sigma)
    hits = torch.zeros(1000)
    for seed in range(50):
        hits[RW.select_slots(table(2), 200, seed, "cpu")[10:]] += 1
    assert hits.sum() == 50 * 200 and hits.max() <= 50
    quarters = hits.view(4, 250).sum(1)
    assert ((quarters - 2500).abs() < 6 * (10000 * 0.25 * 0.75) ** 0.5).all(), quarters
    assert RW.select_slots(RW.GenerationTable(2, 8), 3, 0, "cpu").numel() == 0       # an empty window


# ---- refusals --------------------------------------------------------------------------------------------------------
def _cpu_batch(n=2):
    from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
    return TensorSelfPlayBatch(torch.zeros(n, 11, 6, 6), torch.zeros(n, 220, dtype=torch.bool), torch.zeros(n, 220),
                               torch.zeros(n), torch.zeros(n))


def test_window_trainer_refuses_ddp_and_has_no_dedup_options():
    from liuzhou_amd.train_bridge import train_network_from_tensors, train_network_from_window
    for strategy in ("ddp", "DDP", "bogus"):
        with pytest.raises(ValueError):
            train_network_from_window(None, None, parallel_strategy=strategy)
    theirs = inspect.signature(train_network_from_tensors).parameters
    ours = inspect.signature(train_network_from_window).parameters
    assert not [k for k in ours if k.startswith("dedup")]
    assert set(ours) - set(theirs) == {"window", "replay_budget_per_generation", "replay_seed"}
    assert set(theirs) - set(ours) == {"samples", "dedup_positions", "dedup_max_copies"}
    for k in set(ours) & set(theirs):
        assert ours[k].default == theirs[k].default and ours[k].kind == theirs[k].kind, k
    assert ours["replay_budget_per_generation"].default == 0 and ours["replay_seed"].default == 0


def test_gather_refuses_records_without_the_compact_path():
    from liuzhou_amd.distributed import gather_trajectories
    with pytest.raises(ValueError, match="compact"):
        gather_trajectories(_cpu_batch(), compact=False, as_records=True)
    assert inspect.signature(gather_trajectories).parameters["as_records"].default is False
    same = _cpu_batch()
    assert gather_trajectories(same) is same                                         # the default path is untouched


def test_cpu_tensors_are_refused():
    from liuzhou_amd.distributed import gather_trajectories
    with pytest.raises(RuntimeError, match="HIP device"):
        RW.ReplayWindow("cpu", max_generations=2, capacity_rows=8)
    with pytest.raises(RuntimeError, match="HIP device"):
        gather_trajectories(_cpu_batch(), as_records=True)                           # records are packed on the device
    w = object.__new__(RW.ReplayWindow)                                              # no device to build one on here
    w.device, w.table = torch.device("cpu"), RW.GenerationTable(2, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        w.add_generation(_cpu_batch())
    with pytest.raises(RuntimeError, match="HIP device"):
        w.add_generation(torch.zeros(2, 360, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP device"):
        w.gather(torch.zeros(2, dtype=torch.int64))
    assert w.table.entries == []


def test_abi_bookkeeping_of_the_new_export():
    from liuzhou_amd import _lib as L
    assert "lz_replay_gather_rows" in L.SYMBOLS and "lz_replay_gather_rows" not in L.HOST_SYMBOLS      # HIP only
    restype, argtypes = L.DECLS["lz_replay_gather_rows"]
    assert len(argtypes) == 12
    import ctypes
    assert restype is ctypes.c_int
    assert [i for i, t in enumerate(argtypes) if issubclass(t, ctypes.c_int64)] == [1, 5]           # capacity, m
    assert [i for i, t in enumerate(argtypes) if issubclass(t, ctypes.c_int32)] == [4]              # sym_width
    assert all(t is ctypes.c_void_p for i, t in enumerate(argtypes) if i not in (1, 4, 5))
