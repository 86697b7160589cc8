"""CPU: merging duplicate positions across the replay window, record to record -- the host build's two entry points
(lz_replay_position_keys, lz_replay_merge_records) and the Python functions on CPU tensors against the restatement
(tests/replay_merge_ref.py) byte for byte, the weights of the merged groups, the trainer's keywords, the command-line
flags, and the host code under the address and undefined-behaviour sanitizers (tests/replay_merge_host_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from liuzhou_amd import _lib as L
from liuzhou_amd import position_dedup as D
from liuzhou_amd import replay_window as RW
from liuzhou_amd import row_weights as W
from tests import position_dedup as PD
from tests import replay_merge_ref as R
from tests.replay_ref import decode_records, make_record

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED = 20261021
ERR_ARG, ERR_ALIGN = -1, -4


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def H():
    return L.host_lib()


@pytest.fixture(scope="module")
def rings():
    """name -> (records, slots): the grid under one frame and under all eight, and the hand-built edge records; every
    ring is selected in an order of its own with some slots twice."""
    rng = np.random.default_rng(SEED)
    out = {}
    for name, rec in (("grid", R.grid_records(SEED, False)), ("grid spread", R.grid_records(SEED, True)),
                      ("edges", R.edge_records(SEED)[0])):
        slots = np.concatenate([rng.permutation(len(rec)), rng.integers(0, len(rec), 7)]).astype(np.int64)
        out[name] = (np.ascontiguousarray(rec), slots)
    return out


def _abi_keys(H, rec, slots, symmetric, capacity=None):
    m = len(slots)
    keys, sym, bad = np.full((m, 8), 7, np.int64), np.full(m + 8, 7, np.int8), np.zeros(1, np.int32)
    st = H.lz_replay_position_keys(_p(rec), len(rec) if capacity is None else capacity, _p(slots), m, symmetric, _p(keys),
                                   _p(sym), _p(bad), None)
    assert (sym[m:] == 7).all()                                      # nothing behind the output is written
    return st, keys, sym[:m].copy(), int(bad[0])


def _abi_merge(H, rec, slots, sym, order, begin, capacity=None, m=None):
    G = len(begin) - 1
    out, count, over = np.full((G + 1, 360), 0xA5, np.uint8), np.full(G + 1, -7, np.int32), np.zeros(1, np.int32)
    st = H.lz_replay_merge_records(_p(rec), len(rec) if capacity is None else capacity, _p(slots),
                                   len(slots) if m is None else m, _p(sym), _p(order), _p(begin), G, _p(out), _p(count),
                                   _p(over), None)
    assert (out[G] == 0xA5).all() and count[G] == -7                 # the sentinel record behind the output is untouched
    return st, out[:G], count[:G], int(over[0])


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- both entry points against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", PD.MODES)
@pytest.mark.parametrize("name", ["grid", "grid spread", "edges"])
def test_keys_and_merged_records_are_bit_identical_to_the_restatement(H, rings, name, mode):
    rec, slots = rings[name]
    symmetric = int(mode == "symmetric")
    want_keys, want_sym, want_bad = R.keys_ref(rec, slots, symmetric)
    st, keys, sym, bad = _abi_keys(H, rec, slots, symmetric)
    assert st == 0 and bad == want_bad == 0 and _same(keys, want_keys) and _same(sym, want_sym)
    gor, order, begin = PD.group(want_keys)
    want, want_count, want_over = R.merge_ref(rec, slots, want_sym, order, begin)
    st, out, count, over = _abi_merge(H, rec, slots, want_sym, order, begin)
    assert st == 0 and over == want_over and _same(count, want_count)
    for g in range(len(count)):
        assert _same(out[g], want[g]), (name, mode, g, int(count[g]))
    if (name, mode) in (("grid", "exact"), ("grid spread", "symmetric")):
        assert sorted(np.diff(begin).tolist())[-4] >= 255 and max(np.diff(begin)) >= 600      # every chunk boundary
    # the Python functions on CPU tensors take the same path through the ABI
    t_rec, t_slots = torch.from_numpy(rec), torch.from_numpy(slots)
    k, s, b = RW.record_position_keys(t_rec, t_slots, symmetric=bool(symmetric))
    assert k.dtype == torch.int64 and s.dtype == torch.int8 and b.dtype == torch.int32 and int(b) == 0
    assert _same(k.numpy(), want_keys) and _same(s.numpy(), want_sym)
    g_of, t_order, t_begin, t_count = D.group_rows(k)
    assert np.array_equal(g_of.numpy(), gor) and np.array_equal(t_order.numpy(), order) and np.array_equal(t_begin.numpy(), begin)
    merged, cnt, ov = RW.merge_record_groups(t_rec, t_slots, s, t_order, t_begin)
    assert merged.dtype == torch.uint8 and cnt.dtype == torch.int32 and int(ov) == want_over
    assert _same(merged.numpy(), want) and _same(cnt.numpy(), want_count)


def test_the_edge_records_cover_the_issue(rings):
    """What the edge ring must hold, said once: every legal count, junk everywhere the layout does not own, odd bit
    patterns on a lone record's legal slots, members without a policy, every first-member frame."""
    rec, notes = R.edge_records(SEED)
    assert {n for kind, n in notes if kind == "lone"} == {n for kind, n in notes if kind == "triple"} == {0, 1, 71, 72, 73, 220}
    assert {k for kind, k in notes if kind == "frames"} == set(range(8))
    _, masks, policy, value, _ = decode_records(rec)
    for i, (kind, n) in enumerate(notes):
        if kind in ("lone", "triple"):
            assert int(masks[i].sum()) == n
            w = rec[i][:32].view(np.uint64)
            assert all(int(w[p]) >> 36 for p in (1, 2, 3)) and int(rec[i][32:60].view(np.uint32)[6]) >> 28 == 0xF
            assert rec[i][356:360].all()
            if n < 72:
                assert rec[i][60:348].view(np.uint32)[n:].all()          # junk past the legal count
        if kind == "lone" and n >= 8:
            assert set(R.ODD_BITS) <= set(int(x) for x in policy[i][masks[i] != 0])
    keys, sym, _ = R.keys_ref(rec, np.arange(len(rec)), 1)
    _, order, begin = PD.group(keys)
    firsts = {(notes[order[begin[g]]], int(sym[order[begin[g]]])) for g in range(len(begin) - 1)}
    assert len({int(sym[i]) for i, (kind, _) in enumerate(notes) if kind == "frames"}) == 8
    sizes = sorted(np.diff(begin).tolist())
    assert sizes.count(9) == 8 and sizes.count(3) == 7 and firsts      # 8 frame groups, 6 triples + the one without a policy


def test_junk_in_unowned_bits_changes_nothing(H):
    rng = np.random.default_rng(3)
    rec, notes = R.edge_records(SEED)
    clean = rec.copy()
    for r in clean:                                                  # the canonical twin of every record
        w = r[:32].view(np.uint64)
        w[0] &= np.uint64((1 << 39) - 1)
        w[1:] &= np.uint64(R.FULL)
        r[32:60].view(np.uint32)[6] &= np.uint32(0x0FFFFFFF)
        r[356:360] = 0
        n = int(decode_records(r[None])[1].sum())
        r[60:348].view(np.uint32)[min(n, 72):] = 0
    slots = rng.permutation(len(rec)).astype(np.int64)
    for symmetric in (0, 1):
        a, b = _abi_keys(H, rec, slots, symmetric), _abi_keys(H, clean, slots, symmetric)
        assert _same(a[1], b[1]) and _same(a[2], b[2])
        _, order, begin = PD.group(a[1])
        x, y = _abi_merge(H, rec, slots, a[2], order, begin), _abi_merge(H, clean, slots, a[2], order, begin)
        assert _same(x[1], y[1]) and _same(x[2], y[2]) and x[3] == y[3] == 4      # 73 and 220 legal bits, lone and triple
        lone = [g for g in range(len(begin) - 1) if begin[g + 1] - begin[g] == 1]
        for g in lone:                                               # a group of one is the canonical record itself
            assert _same(x[1][g], clean[slots[order[begin[g]]]])


def test_a_lone_record_keeps_odd_bit_patterns(H):
    words, actions = [0x123456789, 0x0F0F0F0F0, 5, 9 << 20], [0, 31, 32, 63, 64, 127, 128, 219]
    rec = make_record([words[0] | (3 << 36)] + words[1:], R._mask_words(actions), list(R.ODD_BITS), 0.0, 0.0)
    rec[348:352] = np.frombuffer(np.uint32(0xFFC00001).tobytes(), np.uint8)
    rec[352:356] = np.frombuffer(np.uint32(0x00000001).tobytes(), np.uint8)
    ring = np.stack([rec, rec])
    slots, sym = np.array([1], np.int64), np.zeros(1, np.int8)
    st, out, count, over = _abi_merge(H, ring, slots, sym, np.array([0], np.int64), np.array([0, 1], np.int64))
    assert st == 0 and count.tolist() == [1] and over == 0 and _same(out[0], rec)
    # two copies are summed: the -0.0 and the subnormals add up, the NaN stays a NaN, the infinities stay
    st, out, count, _ = _abi_merge(H, ring, np.array([0, 1], np.int64), np.zeros(2, np.int8), np.array([0, 1], np.int64),
                                   np.array([0, 2], np.int64))
    want, _, _ = R.merge_ref(ring, [0, 1], [0, 0], [0, 1], [0, 2])
    got_p, want_p = out[0][60:348].view(np.float32), want[0][60:348].view(np.float32)
    assert count.tolist() == [2] and _same(out[0][:60], want[0][:60])
    assert np.array_equal(np.isnan(got_p), np.isnan(want_p)) and _same(got_p[~np.isnan(got_p)], want_p[~np.isnan(want_p)])
    assert out[0][60:64].view(np.uint32)[0] == 0                     # (-0.0 + -0.0 from a sum that starts at +0.0) / 2 = +0.0


def test_the_policy_count_skips_members_without_a_policy(H):
    words, actions = [7, 56, 0, 0], [1, 2, 3, 200]
    p, q, z = [0.1, 0.2, 0.3, 0.4], [0.4, 0.4, 0.1, 0.1], [0.0] * 4
    ring = np.stack([make_record(words, R._mask_words(actions), pol, v, s)
                     for pol, v, s in ((p, 1, 0.5), (z, -1, -0.5), (q, 1, 0.25), (z, 0, 0), (z, 0, 0))])
    slots, sym, order = np.arange(5, dtype=np.int64), np.zeros(5, np.int8), np.arange(5, dtype=np.int64)
    st, out, count, _ = _abi_merge(H, ring, slots, sym, order, np.array([0, 5], np.int64))
    assert st == 0 and count.tolist() == [5]
    want = ((np.array(p, np.float32).astype(np.float64) + np.array(q, np.float32).astype(np.float64)) / 2).astype(np.float32)
    assert _same(out[0][60:76].view(np.float32), want) and not out[0][76:348].any()     # c_p = 2 < c = 5
    assert out[0][348:356].view(np.float32).tolist() == [np.float32(1.0 / 5), np.float32(0.25 / 5)]
    st, out, count, _ = _abi_merge(H, ring, slots, sym, np.array([1, 3, 4, 0, 2], np.int64), np.array([0, 3, 5], np.int64))
    assert count.tolist() == [3, 2] and not out[0][60:348].any()     # c_p = 0: the merged policy is zero
    assert out[0][348:352].view(np.float32)[0] == np.float32(-1.0 / 3)


# ---- the ring: wrapping, repeated and invalid slots ---------------------------------------------------------------------------
def test_a_selection_that_wraps_a_ring_of_16_slots(H):
    rec = R.grid_records(SEED, True)
    ring = np.ascontiguousarray(np.concatenate([rec[:6], rec[:6], rec[100:104]]))     # 16 slots, 6 positions twice
    assert len(ring) == 16
    slots = np.array([13, 14, 15, 0, 1, 2, 3, 3, 5, 3, -1, 16, 7, 1 << 40, -(1 << 62)], np.int64)
    for symmetric in (0, 1):
        want_keys, want_sym, want_bad = R.keys_ref(ring, slots, symmetric)
        st, keys, sym, bad = _abi_keys(H, ring, slots, symmetric)
        assert st == 0 and bad == want_bad == 4 and _same(keys, want_keys) and _same(sym, want_sym)
        for j in (10, 11, 13, 14):
            assert keys[j].tolist() == [R.INT64_MIN + j] + [0] * 7 and sym[j] == 0
        gor, order, begin = PD.group(keys)
        assert gor[6] == gor[7] == gor[9] and gor[4] == gor[12]      # slot 3 three times; slot 1 and its twin in slot 7
        want, want_count, want_over = R.merge_ref(ring, slots, sym, order, begin)
        st, out, count, over = _abi_merge(H, ring, slots, sym, order, begin)
        assert st == 0 and over == want_over and _same(count, want_count) and _same(out, want)
        for j in (10, 11, 13, 14):                                   # a slot outside the ring: a group of its own, zeroed
            assert count[gor[j]] == 0 and not out[gor[j]].any()
    bad = np.zeros(1, np.int32)
    bad[0] = 40                                                      # the counter is add-only
    keys, sym = np.zeros((len(slots), 8), np.int64), np.zeros(len(slots), np.int8)
    assert H.lz_replay_position_keys(_p(ring), 16, _p(slots), len(slots), 1, _p(keys), _p(sym), _p(bad), None) == 0
    assert bad[0] == 44


def test_bad_order_range_and_sym_give_zero_records(H):
    rec = R.grid_records(SEED, True)
    slots = np.arange(len(rec), dtype=np.int64)
    keys, sym, _ = R.keys_ref(rec, slots, 1)
    _, order, begin = PD.group(keys)
    m = len(slots)
    big = int(np.argmax(np.diff(begin)))                             # the 600-member group: an entry of its last chunk
    good = _abi_merge(H, rec, slots, sym, order, begin)
    for bad_value in (m, -1, 1 << 40):
        broken = order.copy()
        broken[begin[big] + 555] = bad_value
        st, out, count, over = _abi_merge(H, rec, slots, sym, broken, begin)
        want, want_count, want_over = R.merge_ref(rec, slots, sym, broken, begin)
        assert st == 0 and count[big] == 0 and not out[big].any() and count.sum() == m - 600
        assert _same(out, want) and _same(count, want_count) and over == want_over
    for where in (0, 3, 599):                                        # a member's slot outside the ring, a sym outside 0..7
        far = slots.copy()
        far[order[begin[big] + where]] = len(rec)
        st, out, count, _ = _abi_merge(H, rec, far, sym, order, begin)
        assert st == 0 and count[big] == 0 and not out[big].any() and _same(np.delete(out, big, 0), np.delete(good[1], big, 0))
        for value in (8, -1, 127, -128):
            odd = sym.copy()
            odd[order[begin[big] + where]] = value
            st, out, count, _ = _abi_merge(H, rec, slots, odd, order, begin)
            assert st == 0 and count[big] == 0 and not out[big].any()
    ranges = begin.copy()                                            # impossible ranges
    ranges[-1] = m + 1
    st, out, count, _ = _abi_merge(H, rec, slots, sym, order, ranges)
    assert st == 0 and count[-1] == 0 and not out[-1].any() and count[:-1].tolist() == np.diff(begin)[:-1].tolist()
    for b, e in ((5, 5), (7, 3), (-1, 2), (m, m + 1)):
        st, out, count, _ = _abi_merge(H, rec, slots, sym, order, np.array([b, e], np.int64))
        assert st == 0 and count.tolist() == [0] and not out.any()
    st, out, count, _ = _abi_merge(H, rec, slots, sym, order, begin, capacity=0)      # an empty ring holds nothing
    assert st == 0 and not count.any() and not out.any()


def test_nothing_to_do_and_every_argument_refusal(H):
    rec = R.edge_records(SEED)[0]
    n = len(rec)
    slots = np.arange(n, dtype=np.int64)
    keys, sym, bad = np.zeros((n, 8), np.int64), np.zeros(n, np.int8), np.zeros(1, np.int32)
    K, M = H.lz_replay_position_keys, H.lz_replay_merge_records
    assert K(None, 0, None, 0, 1, None, None, None, None) == 0       # m == 0: ok without touching anything
    assert K(_p(rec), n, _p(slots), 0, 0, None, None, None, None) == 0
    for args in ((_p(rec), n, _p(slots), -1, 1, _p(keys), _p(sym), _p(bad)), (_p(rec), -1, _p(slots), n, 1, _p(keys), _p(sym), _p(bad)),
                 (_p(rec), n, _p(slots), n, 2, _p(keys), _p(sym), _p(bad)), (_p(rec), n, _p(slots), n, -1, _p(keys), _p(sym), _p(bad)),
                 (None, n, _p(slots), n, 1, _p(keys), _p(sym), _p(bad)), (_p(rec), n, None, n, 1, _p(keys), _p(sym), _p(bad)),
                 (_p(rec), n, _p(slots), n, 1, None, _p(sym), _p(bad)), (_p(rec), n, _p(slots), n, 1, _p(keys), None, _p(bad)),
                 (_p(rec), n, _p(slots), n, 1, _p(keys), _p(sym), None)):
        assert K(*args, None) == ERR_ARG
    order, begin = np.arange(n, dtype=np.int64), np.array([0, n], np.int64)
    out, count = np.full((1, 360), 9, np.uint8), np.full(1, 9, np.int32)
    good = (_p(rec), n, _p(slots), n, _p(sym), _p(order), _p(begin), 1, _p(out), _p(count), _p(bad))
    assert M(None, 0, None, 0, None, None, None, 0, None, None, None, None) == 0
    assert M(*good[:7], 0, None, None, None, None) == 0              # groups == 0
    assert M(*good[:3], 0, *good[4:], None) == 0 and (out == 9).all() and count[0] == 9      # m == 0: no launch
    for i, value in ((1, -1), (3, -1), (7, -1)):                     # capacity, m, groups below zero
        args = list(good)
        args[i] = value
        assert M(*args, None) == ERR_ARG
    for i in (0, 2, 4, 5, 6, 8, 9, 10):                              # every required pointer
        args = list(good)
        args[i] = None
        assert M(*args, None) == ERR_ARG, i
    assert M(*good, None) == 0 and count[0] == n

    def off(a, by):
        return C.c_void_p(a.ctypes.data + by)
    wide = np.zeros(8 * n + 64, np.int64)
    for i, by in ((0, 4), (2, 4), (5, 4)):                           # records, slot, keys: 8 bytes
        args = [_p(rec), n - 1, _p(slots), n - 1, 1, _p(keys), _p(sym), _p(bad)]
        args[i] = off((rec, None, slots, None, None, wide)[i], by)
        assert K(*args, None) == ERR_ALIGN, i
    assert K(_p(rec), n, _p(slots), n, 1, _p(keys), _p(sym), off(wide, 2), None) == ERR_ALIGN
    for i, by in ((0, 4), (2, 4), (5, 4), (6, 4), (8, 4), (9, 2), (10, 2)):
        args = list(good)
        args[3], args[7] = n - 1, 1
        args[i] = off(wide if i >= 8 else (rec, None, slots, None, None, order, begin)[i], by)
        if i == 6:
            args[i] = off(wide, 4)
        assert M(*args, None) == ERR_ALIGN, i


# ---- the weights of the groups ------------------------------------------------------------------------------------------------
def _cpu_window(records, entries, max_generations=4):
    """A ReplayWindow over CPU records: the class refuses CPU devices (the gather kernel has no host build), the two
    merge entry points do not."""
    w = object.__new__(RW.ReplayWindow)
    w.device = torch.device("cpu")
    w.table = RW.GenerationTable(max_generations, len(records))
    for gid, count in entries:
        w.table.add(count, gid)
    w.ring = torch.from_numpy(np.ascontiguousarray(records))
    w._gen = torch.Generator()
    w.last_add = {"generation": None, "rows": 0, "filtered_non_finite_rows": 0, "evicted": []}
    return w


@pytest.mark.parametrize("decay", [0.5, 0.25, 1.0])
@pytest.mark.parametrize("max_weight", [1, 2.5, 1000])
def test_weights_from_group_and_age_counts(decay, max_weight):
    rng = np.random.default_rng(5)
    gor = rng.integers(0, 40, 3000)
    gor[:40] = np.arange(40)
    ages = rng.integers(0, 4, 3000)
    count = np.bincount(gor, minlength=40)
    scale = [decay ** a for a in range(4)]                           # powers of 1/2: exact in every pow
    want = R.merge_weights_ref(gor, ages, scale, max_weight)
    got = RW.merge_weights(torch.from_numpy(gor), torch.from_numpy(count), torch.from_numpy(ages), decay, max_weight)
    assert got.dtype == torch.float64 and _same(got.numpy(), want)
    got = RW.merge_weights(torch.from_numpy(gor), torch.from_numpy(count), torch.from_numpy(ages), decay, max_weight, span=6)
    assert _same(got.numpy(), want)
    if decay == 1.0 and max_weight != 2.5:                           # decay 1 is the capped count of the tensor merge
        assert _same(got.numpy(), D.group_weights(torch.from_numpy(count), max_weight).numpy())
    none = RW.merge_weights(torch.from_numpy(gor), torch.from_numpy(count), None, decay, max_weight)
    assert _same(none.numpy(), np.minimum(count.astype(np.float64), float(max_weight)))


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.3])
def test_no_duplicates_give_the_age_weights_bits(decay):
    ages = torch.from_numpy(np.random.default_rng(2).integers(0, 5, 500))
    rows = torch.arange(500)
    got = RW.merge_weights(rows, torch.ones(500, dtype=torch.int64), ages, decay, 1, span=5)
    assert _same(got.numpy(), W.age_weights(ages, decay).numpy())
    with pytest.raises(ValueError, match="negative"):
        RW.merge_weights(rows, torch.ones(500, dtype=torch.int64), ages - 1, decay, 1)


def test_merge_selection_on_cpu_records():
    rec = R.grid_records(SEED, True)
    n = len(rec)
    first = n - 200
    window = _cpu_window(rec, [(3, first), (4, 200)], max_generations=2)
    slots, ages = window.select(10 ** 6, 0, return_ages=True)         # newest first, every row
    assert slots[:200].tolist() == list(range(first, n)) and ages[:200].eq(0).all() and ages[200:].eq(1).all()
    for mode in PD.MODES:
        merged, weights, info = window.merge_selection(slots, mode=mode, ages=ages, age_decay=0.5, max_weight=3)
        keys, sym, _ = R.keys_ref(rec, slots.numpy(), mode == "symmetric")
        gor, order, begin = PD.group(keys)
        want, want_count, want_over = R.merge_ref(rec, slots.numpy(), sym, order, begin)
        assert _same(merged.numpy(), want) and _same(info["count"].numpy(), want_count)
        assert np.array_equal(info["group_of_row"].numpy(), gor)
        assert _same(weights.numpy(), R.merge_weights_ref(gor, ages.numpy(), [1.0, 0.5], 3))
        size = np.diff(begin)
        assert {k: info[k] for k in D.STAT_KEYS} == {
            "rows_in": n, "rows_out": len(size), "groups": len(size), "merged_groups": int((size > 1).sum()),
            "merged_rows": int(size[size > 1].sum()), "largest_group": int(size.max()), "not_representable": want_over}
        assert info["mode"] == mode and info["max_weight"] == 3.0
        # a group keeps the frame of its newest member: the first member of every group is its first in the selection
        head = decode_records(merged.numpy())[0]
        assert _same(head, decode_records(rec[slots.numpy()[order[begin[:-1]]]])[0])
        plain, w1, _ = window.merge_selection(slots, mode=mode)
        assert _same(plain.numpy(), want) and _same(w1.numpy(), np.ones(len(size)))
        _, w4, _ = window.merge_selection(slots, mode=mode, max_weight=4)
        assert _same(w4.numpy(), D.group_weights(info["count"], 4).numpy())
    with pytest.raises(ValueError, match="exact"):
        window.merge_selection(slots, mode="off")
    for bad in (0, 0.5, True, float("nan"), float("inf"), None, "2"):
        with pytest.raises(ValueError, match="replay_merge_max_weight"):
            window.merge_selection(slots, mode="exact", max_weight=bad)
    with pytest.raises(ValueError, match="ages lie outside"):
        window.merge_selection(slots, mode="exact", ages=ages + 1, age_decay=0.5)
    empty = torch.zeros(0, dtype=torch.int64)
    merged, weights, info = window.merge_selection(empty, mode="symmetric", ages=empty, age_decay=0.5)
    assert tuple(merged.shape) == (0, 360) and weights.numel() == 0 and info["groups"] == 0 and info["largest_group"] == 0


def test_python_functions_validate_their_tensors():
    rec = torch.from_numpy(R.edge_records(SEED)[0])
    slots = torch.arange(4)
    with pytest.raises(ValueError, match="records"):
        RW.record_position_keys(rec[:, :359], slots, symmetric=True)
    with pytest.raises(ValueError, match="slots"):
        RW.record_position_keys(rec, slots.int(), symmetric=True)
    with pytest.raises(TypeError):
        RW.record_position_keys(rec.numpy(), slots, symmetric=True)
    k, s, _ = RW.record_position_keys(rec, slots, symmetric=True)
    _, order, begin, _ = D.group_rows(k)
    with pytest.raises(ValueError, match="sym"):
        RW.merge_record_groups(rec, slots, s.int(), order, begin)
    with pytest.raises(ValueError, match="order"):
        RW.merge_record_groups(rec, slots, s, order[:3], begin)
    with pytest.raises(RuntimeError, match="HIP device"):            # decoding batches stays HIP only
        RW.gather_records(rec, slots)


# ---- the trainer's keywords -----------------------------------------------------------------------------------------------------
def test_trainer_keywords_are_validated_on_and_off():
    from liuzhou_amd import train_bridge as TB

    class Empty:
        num_rows = 0
    nothing = {"epoch_stats": [], "num_samples": 0}
    for kw in ({"replay_merge_positions": "off"}, {"replay_merge_max_weight": 1}, {"replay_merge_positions": "off",
               "replay_merge_max_weight": 1, "replay_age_decay": 1.0}, {"replay_merge_positions": "exact"},
               {"replay_merge_positions": "symmetric", "replay_merge_max_weight": 4, "replay_age_decay": 0.5},
               {"replay_merge_positions": "off", "replay_merge_max_weight": 2.5}):
        assert TB.train_network_from_window(None, Empty(), **kw)[1] == nothing
    for kw in ({"replay_merge": "exact"}, {"replay_merge_position": "exact"}, {"replay_merge_max_copies": 2},
               {"dedup_positions": "exact"}, {"dedup_max_copies": 2}, {"dedup_weighting": "weight"}):
        with pytest.raises(TypeError, match=r"train_network_from_window\(\) got an unexpected keyword argument"):
            TB.train_network_from_window(None, Empty(), **kw)
    for bad in ("on", "", None, 1, "Exact", True):
        with pytest.raises(ValueError, match="replay_merge_positions"):
            TB.train_network_from_window(None, Empty(), replay_merge_positions=bad)
    for mode in ("off", "exact"):
        for bad in (0, -1, 0.999, True, False, float("nan"), float("inf"), None, "2"):
            with pytest.raises(ValueError, match="replay_merge_max_weight"):
                TB.train_network_from_window(None, Empty(), replay_merge_positions=mode, replay_merge_max_weight=bad)
    for kw in ({"policy_draw_weight": 0.5}, {"anti_draw_penalty": 0.1}, {"anti_draw_penalty": -0.1}):
        for mode in ("exact", "symmetric"):
            with pytest.raises(ValueError, match="replay_merge_positions=.*drawn game"):
                TB.train_network_from_window(None, Empty(), replay_merge_positions=mode, **kw)
        assert TB.train_network_from_window(None, Empty(), replay_merge_positions="off", **kw)[1] == nothing


def test_the_defaults_import_nothing_new():
    code = ("import sys; from liuzhou_amd.train_bridge import train_network_from_window as w\n"
            "class Win: num_rows = 0\n"
            "assert w(None, Win())[1]['num_samples'] == 0\n"
            "assert w(None, Win(), replay_merge_positions='off', replay_merge_max_weight=1)[1]['num_samples'] == 0\n"
            "assert not [m for m in ('liuzhou_amd.row_weights', 'liuzhou_amd.position_dedup', 'liuzhou_amd.replay_window') "
            "if m in sys.modules]\n"
            "assert w(None, Win(), replay_merge_positions='exact')[1]['num_samples'] == 0\n"
            "assert 'liuzhou_amd.position_dedup' in sys.modules\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr


# ---- command line -----------------------------------------------------------------------------------------------------------------
def test_staged_loop_flags(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    cli = __import__("staged_loop")
    a = cli.parse_args([])
    assert a.replay_merge_positions == "off" and a.replay_merge_max_weight == 1.0
    a = cli.parse_args(["--replay-generations", "3", "--replay-merge-positions", "symmetric", "--replay-merge-max-weight", "4"])
    assert a.replay_merge_positions == "symmetric" and a.replay_merge_max_weight == 4.0
    a = cli.parse_args(["--replay-generations", "2", "--replay-merge-positions", "exact", "--replay-age-decay", "0.5"])
    assert a.replay_merge_positions == "exact" and a.replay_merge_max_weight == 1.0
    assert cli.parse_args(["--replay-merge-positions", "off", "--replay-merge-max-weight", "1"]).replay_generations == 1
    window = "--replay-merge-positions / --replay-merge-max-weight need a window: --replay-generations > 1"
    for argv, text in ((["--replay-merge-positions", "exact"], window),
                       (["--replay-generations", "1", "--replay-merge-positions", "symmetric"], window),
                       (["--replay-merge-max-weight", "2"], window),
                       (["--replay-generations", "2", "--replay-merge-positions", "fuzzy"], "invalid choice: 'fuzzy'"),
                       (["--replay-generations", "2", "--replay-merge-max-weight", "0.5"], "--replay-merge-max-weight must be a finite number >= 1, got 0.5"),
                       (["--replay-generations", "2", "--replay-merge-max-weight", "nan"], "--replay-merge-max-weight must be a finite number >= 1"),
                       (["--replay-generations", "2", "--replay-merge-max-weight", "inf"], "--replay-merge-max-weight must be a finite number >= 1"),
                       (["--replay-generations", "2", "--dedup-positions", "exact"], "--replay-merge-positions"),
                       (["--replay-generations", "2", "--dedup-positions", "exact", "--replay-merge-positions", "exact"],
                        "--replay-merge-positions")):
        with pytest.raises(SystemExit):                              # refused while parsing: before any process group
            cli.parse_args(argv)
        assert text in capsys.readouterr().err, argv
    base = {"iteration": 1, "positions": 10}
    assert cli.iteration_entry(base) == base and cli.iteration_entry(base, replay={"merge": {}}, row_weights={"s": 1}) == base
    on = cli.iteration_entry(base, replay={"rows": 1, "merge": {"groups": 2}}, window_on=True, row_weights={"source": "replay_merge"},
                             weights_on=True)
    assert list(on) == ["iteration", "positions", "replay", "row_weights"] and on["replay"]["merge"] == {"groups": 2}
    off = cli.iteration_entry(base, replay={"rows": 1}, window_on=True)
    assert list(off) == ["iteration", "positions", "replay"] and "merge" not in off["replay"]


# ---- the host code under the sanitizers -----------------------------------------------------------------------------------------
def test_host_code_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    csrc = os.path.join(ROOT, "liuzhou_amd", "csrc")
    exe = str(tmp_path / "replay_merge_host_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
                           "-I" + csrc, "-o", exe, os.path.join(HERE, "replay_merge_host_check.cpp"),
                           os.path.join(csrc, "lz_dedup_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "replay_merge_host_check: ok" in res.stdout, res.stdout + res.stderr
