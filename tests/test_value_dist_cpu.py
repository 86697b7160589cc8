"""CPU: the distributional value target of merged positions -- the host build of
lz_merge_value_distributions and the Python functions on CPU tensors against the restatement (tests/value_dist_ref.py)
bit for bit, the identities of the restatement, the linearity of the bucket cross entropy in its target (the reason for
the feature) in float64, the keywords of the trainers and the command line, and the host code under the address and
undefined-behaviour sanitizers (tests/value_dist_host_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from liuzhou_amd import _lib as L
from tests import value_dist_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED = 20261022
ERR_ARG, ERR_ALIGN = -1, -4
F = np.float32
SENT = np.array([0x7FC0BEEF], np.uint32).view(F)[0]


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def H():
    return L.host_lib()


@pytest.fixture(scope="module")
def case():
    return R.build_case(SEED, 9)                                    # sizes 2, 3, 1, 2, 3, 300, 1, 2, 3


def _rows_for(G, D_extra=2):
    """dist_row of G groups: a permutation into [0, G), with group 2 -> -1, the last but one -> D and the last -> INT32_MIN;
    the table has G + D_extra rows so that its guard rows and the rows of the skipped groups keep their sentinel."""
    rows = np.random.default_rng(SEED).permutation(G).astype(np.int32)
    D = G + D_extra
    skipped = {2: -1, G - 2: D, G - 1: R.INT32_MIN}
    for g, v in skipped.items():
        rows[g] = v
    return rows, D, skipped


def _abi(H, value_base, soft_base, stride, n, index, m, order, begin, rows, alpha, D, dist=None):
    G = len(begin) - 1
    dist = np.full((D, R.BINS), SENT, F) if dist is None else dist
    st = H.lz_merge_value_distributions(value_base, soft_base, stride, n, _p(index), m, _p(order), _p(begin), G, _p(rows),
                                        C.c_float(alpha), _p(dist), D, None)
    return st, dist


# ---- the host build against the restatement, both addressings -------------------------------------------------------------------
@pytest.mark.parametrize("alpha", R.ALPHAS)
def test_tensor_addressing_is_bit_identical_to_the_restatement(H, case, alpha):
    v, s, order, begin = case["value"], case["soft"], case["order"], case["begin"]
    n, G = len(v), len(begin) - 1
    assert sorted(set(case["sizes"])) == [1, 2, 3, 300]
    rows, D, skipped = _rows_for(G)
    st, got = _abi(H, _p(v), _p(s), 4, n, None, n, order, begin, rows, alpha, D)
    want = R.merge_ref(v, s, n, None, n, order, begin, rows, alpha, np.full((D, R.BINS), SENT, F))
    assert st == 0 and _same(got, want)
    written = {int(r) for g, r in enumerate(rows) if g not in skipped}
    for d in range(D):                                               # guard rows and the skipped groups' rows: the sentinel
        assert (got[d].view(np.uint32) == 0x7FC0BEEF).all() == (d not in written), d
    live = got[sorted(written)]
    assert np.abs(live.astype(np.float64).sum(axis=1) - 1.0).max() <= 101 * 2.0 ** -23      # every row sums to 1


@pytest.mark.parametrize("alpha", R.ALPHAS)
def test_ring_addressing_is_bit_identical_to_the_restatement(H, case, alpha):
    v, s, order, begin = case["value"], case["soft"], case["order"], case["begin"]
    n, G = len(v), len(begin) - 1
    ring, slot = R.ring_of(v, s, guard=3, seed=SEED)
    cap = len(ring)
    rows, D, _ = _rows_for(G)
    flat = ring.reshape(-1)
    vb, sb = C.c_void_p(flat.ctypes.data + R.VALUE_OFF), C.c_void_p(flat.ctypes.data + R.SOFT_OFF)
    st, got = _abi(H, vb, sb, R.REC, cap, slot, n, order, begin, rows, alpha, D)
    tensor = R.merge_ref(v, s, n, None, n, order, begin, rows, alpha, np.full((D, R.BINS), SENT, F))
    value_of, soft_of = R.ring_floats(ring)
    want = R.merge_ref(value_of, soft_of, cap, slot, n, order, begin, rows, alpha, np.full((D, R.BINS), SENT, F))
    assert st == 0 and _same(got, want) and _same(got, tensor)       # the same members through either addressing
    # a slot in the guard records is still inside the ring and is read; a slot outside zeroes its group's row
    far = slot.copy()
    g = 4
    far[order[begin[g]]] = cap
    st, got2 = _abi(H, vb, sb, R.REC, cap, far, n, order, begin, rows, alpha, D)
    assert st == 0 and not got2[rows[g]].any() and _same(np.delete(got2, rows[g], 0), np.delete(got, rows[g], 0))
    far[order[begin[g]]] = -1
    st, got2 = _abi(H, vb, sb, R.REC, cap, far, n, order, begin, rows, alpha, D)
    assert st == 0 and not got2[rows[g]].any()


def test_bad_members_and_ranges_give_zero_rows(H, case):
    v, s, order, begin = case["value"], case["soft"], case["order"], case["begin"]
    n, G = len(v), len(begin) - 1
    rows = np.arange(G, dtype=np.int32)
    big = int(np.argmax(np.diff(begin)))
    st, good = _abi(H, _p(v), _p(s), 4, n, None, n, order, begin, rows, 0.25, G)
    for bad_value in (n, -1, 1 << 40, -(1 << 62)):
        broken = order.copy()
        broken[begin[big] + 299] = bad_value                         # the last member of the 300
        st, got = _abi(H, _p(v), _p(s), 4, n, None, n, broken, begin, rows, 0.25, G)
        want = R.merge_ref(v, s, n, None, n, broken, begin, rows, 0.25, np.full((G, R.BINS), SENT, F))
        assert st == 0 and _same(got, want) and not got[big].any() and _same(np.delete(got, big, 0), np.delete(good, big, 0))
    for b, e in ((5, 5), (7, 3), (-1, 2), (n, n + 1), (0, n + 1)):
        st, got = _abi(H, _p(v), _p(s), 4, n, None, n, order, np.array([b, e], np.int64), np.zeros(1, np.int32), 0.0, 1)
        assert st == 0 and not got.any(), (b, e)
    st, got = _abi(H, _p(v), _p(s), 4, 0, None, n, order, begin, rows, 0.0, G)      # n == 0: no element exists
    assert st == 0 and not got.any()


def test_nothing_to_do_and_every_refusal(H, case):
    v, s, order, begin = case["value"], case["soft"], case["order"], case["begin"]
    n, G = len(v), len(begin) - 1
    rows = np.arange(G, dtype=np.int32)
    dist = np.full((G, R.BINS), SENT, F)
    M = H.lz_merge_value_distributions
    good = [_p(v), _p(s), 4, n, None, n, _p(order), _p(begin), G, _p(rows), C.c_float(0.0), _p(dist), G]
    assert M(None, None, 4, 0, None, 0, None, None, 0, None, C.c_float(0.0), None, 0, None) == 0
    assert M(*good[:8], 0, None, good[10], None, G, None) == 0       # groups == 0
    assert M(*good[:11], None, 0, None) == 0                         # D == 0
    assert (dist.view(np.uint32) == 0x7FC0BEEF).all()
    for i, value in ((3, -1), (5, -1), (8, -1), (12, -1), (2, 3), (2, 0), (2, -4)):      # sizes below zero, stride below 4
        args = list(good)
        args[i] = value
        assert M(*args, None) == ERR_ARG, i
    for i in (0, 1, 6, 7, 9, 11):                                    # every required pointer
        args = list(good)
        args[i] = None
        assert M(*args, None) == ERR_ARG, i
    wide = np.zeros(8 * n + 64, np.int64)

    def off(a, by):
        return C.c_void_p(a.ctypes.data + by)
    for i, by in ((0, 2), (1, 2), (6, 4), (7, 4), (9, 2), (11, 2)):
        args = list(good)
        args[i] = off(wide, by)
        assert M(*args, None) == ERR_ALIGN, i
    args = list(good)
    args[4] = off(wide, 4)                                           # the optional index: 8 bytes when given
    assert M(*args, None) == ERR_ALIGN
    args = list(good)
    args[2] = 6                                                      # a stride that would leave float alignment
    assert M(*args, None) == ERR_ALIGN
    assert (dist.view(np.uint32) == 0x7FC0BEEF).all()                # no refusal wrote anything
    assert M(*good, None) == 0 and not (dist.view(np.uint32) == 0x7FC0BEEF).any()
    assert "lz_merge_value_distributions" in L.HOST_SYMBOLS and "lz_merge_value_distributions" in L.SYMBOLS
    assert "lz_policy_value_loss_dist_fwd_bwd" in L.SYMBOLS and "lz_policy_value_loss_dist_fwd_bwd" not in L.HOST_SYMBOLS
    from liuzhou_amd.build import HOST_SOURCES, SOURCES
    assert "lz_value_dist.hip" in SOURCES and any(p.endswith("lz_value_dist_host.cpp") for p in HOST_SOURCES)


# ---- identities of the restatement ---------------------------------------------------------------------------------------------
def test_two_hot_is_the_loss_restatements_bin_assignment():
    """tests/train_loss_ref.py::value_bins_fp32 (anchored to the reference's golden values) at anti_draw 0, on every
    special value that it is defined for (its .long() of a NaN is not) and on random ones."""
    from tests.train_loss_ref import value_bins_fp32
    rng = np.random.default_rng(SEED)
    sp = R.special_values()
    sp = sp[np.isfinite(sp)]
    v = np.concatenate([np.repeat(sp, len(sp)), rng.uniform(-1.5, 1.5, 4000).astype(F)])
    s = np.concatenate([np.tile(sp, len(sp)), rng.uniform(-1.5, 1.5, 4000).astype(F)])
    for alpha in R.ALPHAS + (0.35,):
        lo, hi, frac = R.two_hot(v, s, alpha)
        _, _, lo2, hi2, frac2 = value_bins_fp32(v, s, alpha, 0.0)
        assert np.array_equal(lo, lo2.numpy()) and np.array_equal(hi, hi2.numpy()) and _same(frac, frac2.numpy())


def test_two_hot_is_total():
    sp = R.special_values()
    for alpha in R.ALPHAS + (float("nan"), float("inf"), -1.0):
        lo, hi, frac = R.two_hot(np.repeat(sp, len(sp)), np.tile(sp, len(sp)), alpha)
        assert lo.min() >= 0 and hi.max() <= 100 and ((hi == lo + 1) | ((hi == lo) & (lo == 100))).all()
        assert (frac >= 0).all() and (frac <= 1).all() and (frac[hi == lo] == 0).all()
    lo, hi, frac = R.two_hot(np.array([np.nan, np.inf, -np.inf, 1.5, -1.5, 0.0, 1.0, -1.0], F), np.zeros(8, F), 0.0)
    assert lo.tolist() == [0, 100, 0, 100, 0, 50, 100, 0] and frac.tolist() == [0.0] * 8
    lo, _, _ = R.two_hot(np.zeros(2, F), np.array([np.inf, -np.inf], F), 0.0)
    assert lo.tolist() == [0, 0]                                     # 0 * inf is a NaN, and a NaN lands on bin 0


def test_identities_of_the_group_distribution():
    rng = np.random.default_rng(SEED)
    for alpha in R.ALPHAS:
        for c in (1, 2, 3, 7, 300):                                  # identical members: exactly the member's two-hot
            v, s = F(rng.uniform(-1, 1)), F(rng.uniform(-1, 1))
            assert _same(R.group_distribution(np.full(c, v, F), np.full(c, s, F), alpha), R.two_hot_row(v, s, alpha))
        for c in (2, 3, 300):                                        # any members: the row sums to one
            row = R.group_distribution(rng.uniform(-1.2, 1.2, c).astype(F), rng.uniform(-1.2, 1.2, c).astype(F), alpha)
            assert abs(float(row.astype(np.float64).sum()) - 1.0) <= 101 * 2.0 ** -23
    # the defect, written down: a position won once and lost once
    dist = R.group_distribution(np.array([1, -1], F), np.array([1, -1], F), 0.0)
    want = np.zeros(R.BINS, F)
    want[[0, 100]] = 0.5
    assert _same(dist, want)
    mean = R.mean_target_row(np.array([1, -1], F), np.array([1, -1], F), 0.0)
    one = np.zeros(R.BINS, F)
    one[50] = 1.0
    assert _same(mean, one)                                          # "certain draw"
    assert float(np.abs(mean - dist).max()) == 1.0                   # the difference of 1.0 on bin 50 is the defect


# ---- linearity: the reason for the feature ---------------------------------------------------------------------------------------
def test_the_bucket_cross_entropy_gradient_is_linear_in_the_target():
    for exact in (True, False):
        c = R.linearity_case(SEED, exact=exact)
        owner, count = c["owner"], c["count"]
        mean64 = R.exact_mean_rows(c)
        table = np.stack([R.group_distribution(c["value"][owner == g], c["soft"][owner == g], c["alpha"])
                          for g in range(len(count))])
        unmerged, merged = R.linearity_sides(c, mean64)
        assert np.abs(unmerged - merged).max() <= 1e-12
        assert np.abs(table.astype(np.float64) - mean64).max() <= 2.0 ** -25      # the table rounds every entry once
        if exact:                                                    # ... and not at all where the mean is k / 2^j
            assert _same(table.astype(np.float64), mean64)
            unmerged, merged = R.linearity_sides(c, table)
            assert np.abs(unmerged - merged).max() <= 1e-12
        # the mean target is not linear: on the (+1, -1) group its gradient is somewhere else entirely
        means = np.stack([R.mean_target_row(c["value"][owner == g], c["soft"][owner == g], c["alpha"])
                          for g in range(len(count))])
        _, wrong = R.linearity_sides(c, means)
        n = len(owner)
        assert np.abs(wrong[0] - unmerged[0]).max() * n / count[0] > 0.1      # per unit of the group's weight: 0.5 and 1.0


# ---- the Python functions on CPU tensors ---------------------------------------------------------------------------------------
def _cpu_rows(n_unique, copies, seed):
    """CPU rows for merge_duplicate_positions: `n_unique` positions of the rules fixture, row i copied copies[i] times
    (copies interleaved), with game results as values."""
    from liuzhou_amd import v0_core
    from tests.golden_utils import load, states, unpack_mask
    z = load("g15_rules_large.npz")
    st = states(z, "s")
    t = [torch.from_numpy(np.ascontiguousarray(st[f])) for f in ("board", "marks_black", "marks_white", "phase", "current_player")]
    planes = v0_core.states_to_model_input(*t).numpy()
    masks = unpack_mask(z["legal_mask"], 220).astype(np.uint8)
    masks[:, 216] = 1
    from tests import position_dedup as PD
    keys, _, bad = PD.keys(planes, masks, False)
    _, first = np.unique(keys, axis=0, return_index=True)
    pick = np.sort(first)[:n_unique]
    rng = np.random.default_rng(seed)
    owner = rng.permutation(np.repeat(np.arange(n_unique), copies))
    n = len(owner)
    policy = (rng.random((n, 220)) * masks[pick][owner]).astype(F)
    policy /= policy.sum(axis=1, keepdims=True, dtype=F)
    return {"planes": planes[pick][owner], "masks": masks[pick][owner], "policy": policy,
            "value": rng.choice(np.array([-1, 0, 1], F), n).astype(F), "soft": rng.uniform(-1, 1, n).astype(F), "owner": owner}


@pytest.mark.parametrize("weighting, max_copies", [("copies", 1), ("copies", 3), ("weight", 3)])
def test_merge_duplicate_positions_on_cpu_tensors(weighting, max_copies):
    from liuzhou_amd import position_dedup as D
    copies = np.array([1, 2, 3, 1, 5, 1, 2, 1, 1, 4])
    rows = _cpu_rows(len(copies), copies, SEED)
    t = [torch.from_numpy(np.ascontiguousarray(rows[k])) for k in ("planes", "masks", "policy", "value", "soft")]
    kw = dict(mode="exact", max_copies=max_copies, weighting=weighting)
    plain, info0 = D.merge_duplicate_positions(*t, **kw)
    for alpha in (0.0, 0.25):
        outs, info = D.merge_duplicate_positions(*t, **kw, value_target="distribution", soft_label_alpha=alpha)
        for a, b in zip(outs, plain):                                # the rows keep their mean value and soft value
            assert torch.equal(a, b)
        assert set(info) - set(info0) == {"value_target", "value_dist", "value_dist_row"} and info["value_target"] == "distribution"
        table, row = info["value_dist"], info["value_dist_row"]
        assert table.dtype == torch.float32 and tuple(table.shape) == (info["merged_groups"], 101) == (5, 101)
        assert row.dtype == torch.int32 and tuple(row.shape) == (info["rows_out"],)
        gor = info["group_of_row"].numpy()
        count = info["count"].numpy()
        reps = np.ones_like(count) if weighting == "weight" else np.minimum(count, max_copies)
        leaving = np.repeat(np.arange(len(count)), reps)             # the group of every row that leaves
        assert len(leaving) == info["rows_out"]
        seen = {}
        for j, g in enumerate(leaving):
            d = int(row[j])
            if count[g] == 1:
                assert d == -1
                continue
            assert 0 <= d < 5 and seen.setdefault(g, d) == d         # every copy of a group points at the group's row
            members = np.flatnonzero(gor == g)                       # ascending: the member order of group_rows
            assert _same(table[d].numpy(), R.group_distribution(rows["value"][members], rows["soft"][members], alpha))
        assert sorted(seen.values()) == list(range(5))
        assert D.stats_of(info) == dict(D.stats_of(info0), value_target="distribution")
    # alpha is clamped as the trainers clamp it
    _, hi = D.merge_duplicate_positions(*t, **kw, value_target="distribution", soft_label_alpha=7.0)
    _, one = D.merge_duplicate_positions(*t, **kw, value_target="distribution", soft_label_alpha=1.0)
    assert torch.equal(hi["value_dist"], one["value_dist"])
    # no duplicates: an empty table, every row -1
    u = [x[:1] for x in t]
    _, info = D.merge_duplicate_positions(*u, mode="exact", value_target="distribution")
    assert tuple(info["value_dist"].shape) == (0, 101) and info["value_dist_row"].tolist() == [-1]
    for bad in ("Mean", "dist", None, 1, True):
        with pytest.raises(ValueError, match="value_target"):
            D.merge_duplicate_positions(*t, mode="exact", value_target=bad)


def test_merge_selection_on_cpu_records_reads_the_ring_through_the_slots():
    from liuzhou_amd import position_dedup as D
    from tests import replay_merge_ref as RM
    from tests.test_replay_merge_cpu import _cpu_window
    rec = RM.grid_records(20261021, True)
    n = len(rec)
    first = n - 200
    window = _cpu_window(rec, [(3, first), (4, 200)], max_generations=2)
    slots, ages = window.select(10 ** 6, 0, return_ages=True)
    value_of, soft_of = R.ring_floats(rec)
    for mode in ("exact", "symmetric"):
        plain, w0, info0 = window.merge_selection(slots, mode=mode, ages=ages, age_decay=0.5, max_weight=3)
        merged, w, info = window.merge_selection(slots, mode=mode, ages=ages, age_decay=0.5, max_weight=3,
                                                 value_target="distribution", soft_label_alpha=0.25)
        assert torch.equal(merged, plain) and torch.equal(w, w0)     # the records keep the mean value and soft value
        assert set(info) - set(info0) == {"value_target", "value_dist", "value_dist_row"}
        table, row = info["value_dist"].numpy(), info["value_dist_row"].numpy()
        count = info["count"].numpy()
        assert table.shape == (info["merged_groups"], 101) and row.dtype == np.int32 and row.shape == count.shape
        assert (row[count == 1] == -1).all() and sorted(row[count > 1].tolist()) == list(range(info["merged_groups"]))
        _, order, begin, _ = D.group_rows(window.position_keys(slots, symmetric=mode == "symmetric")[0])
        want = R.merge_ref(value_of, soft_of, n, slots.numpy(), len(slots), order.numpy(), begin.numpy(), row, 0.25,
                           np.zeros_like(table))
        assert _same(table, want) and info["merged_groups"] > 3 and count.max() > 64
    with pytest.raises(ValueError, match="value_target"):
        window.merge_selection(slots, mode="exact", value_target="median")


# ---- the trainers' keywords and the defaults --------------------------------------------------------------------------------------
def test_trainer_keywords_are_validated_on_and_off():
    from liuzhou_amd import train_bridge as TB

    class Empty:
        num_rows = 0
        num_samples = 0
    nothing = {"epoch_stats": [], "num_samples": 0}
    T, W = TB.train_network_from_tensors, TB.train_network_from_window
    for kw in ({"dedup_value_target": "mean"}, {"dedup_positions": "exact", "dedup_value_target": "distribution"},
               {"dedup_positions": "symmetric", "dedup_max_copies": 3, "dedup_weighting": "weight",
                "dedup_value_target": "distribution"}, {"dedup_positions": "exact", "dedup_value_target": "mean"}):
        assert T(None, Empty(), **kw)[1] == nothing
    for kw in ({"replay_merge_value_target": "mean"}, {"replay_merge_positions": "exact", "replay_merge_value_target": "distribution"},
               {"replay_merge_positions": "symmetric", "replay_merge_max_weight": 4, "replay_age_decay": 0.5,
                "replay_merge_value_target": "distribution"}):
        assert W(None, Empty(), **kw)[1] == nothing
    for bad in ("Distribution", "", None, 1, True):
        with pytest.raises(ValueError, match="dedup_value_target"):
            T(None, Empty(), dedup_positions="exact", dedup_value_target=bad)
        with pytest.raises(ValueError, match="replay_merge_value_target"):
            W(None, Empty(), replay_merge_positions="exact", replay_merge_value_target=bad)
    with pytest.raises(ValueError, match="dedup_value_target='distribution' needs dedup_positions"):
        T(None, Empty(), dedup_value_target="distribution")
    with pytest.raises(ValueError, match="replay_merge_value_target='distribution' needs replay_merge_positions"):
        W(None, Empty(), replay_merge_value_target="distribution")
    with pytest.raises(ValueError, match="replay_merge_value_target='distribution' needs replay_merge_positions"):
        W(None, Empty(), replay_merge_positions="off", replay_merge_max_weight=2, replay_merge_value_target="distribution")
    with pytest.raises(TypeError, match=r"train_network_from_window\(\) got an unexpected keyword argument 'dedup_value_target'"):
        W(None, Empty(), dedup_value_target="distribution")
    with pytest.raises(TypeError, match=r"train_network_from_tensors\(\) got an unexpected keyword argument"):
        T(None, Empty(), replay_merge_value_target="distribution")
    for kw in ({"policy_draw_weight": 0.5}, {"anti_draw_penalty": 0.1}):      # the merge's own refusals still come first
        with pytest.raises(ValueError, match="drawn game"):
            T(None, Empty(), dedup_positions="exact", dedup_value_target="distribution", **kw)
        with pytest.raises(ValueError, match="drawn game"):
            W(None, Empty(), replay_merge_positions="exact", replay_merge_value_target="distribution", **kw)


def test_the_defaults_import_nothing_new():
    code = ("import sys; from liuzhou_amd.train_bridge import train_network_from_window as w, train_network_from_tensors as t\n"
            "import liuzhou_amd\n"
            "class Win: num_rows = 0; num_samples = 0\n"
            "assert w(None, Win())[1]['num_samples'] == 0 and t(None, Win())[1]['num_samples'] == 0\n"
            "assert w(None, Win(), replay_merge_value_target='mean')[1]['num_samples'] == 0\n"
            "assert t(None, Win(), dedup_value_target='mean', dedup_weighting='copies')[1]['num_samples'] == 0\n"
            "assert not [m for m in ('liuzhou_amd.row_weights', 'liuzhou_amd.position_dedup', 'liuzhou_amd.replay_window') "
            "if m in sys.modules]\n"
            "assert t(None, Win(), dedup_positions='exact', dedup_value_target='distribution')[1]['num_samples'] == 0\n"
            "assert 'liuzhou_amd.position_dedup' in sys.modules\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr


def test_fused_loss_validates_the_table_before_it_needs_a_device():
    from liuzhou_amd.train_loss import _check_value_dist
    cpu = torch.device("cpu")
    table, row = torch.zeros(3, 101), torch.zeros(4, dtype=torch.int32)
    _check_value_dist(table, row, 4, cpu, 0.0)
    _check_value_dist(table[:0], row, 4, cpu, 0.0)                   # an empty table: every row is -1 or outside
    for a, b, exc in ((None, row, ValueError), (table, None, ValueError), (table.double(), row, TypeError),
                      (table, row.long(), TypeError), (table.numpy(), row, TypeError), (table[:, :100], row, ValueError),
                      (table.view(-1), row, ValueError), (table, row[:3], ValueError), (table, row.view(4, 1), ValueError)):
        with pytest.raises(exc, match="value_dist"):
            _check_value_dist(a, b, 4, cpu, 0.0)
    with pytest.raises(ValueError, match="anti_draw_penalty"):
        _check_value_dist(table, row, 4, cpu, 0.05)
    with pytest.raises(ValueError, match="must live on"):
        _check_value_dist(table, row, 4, torch.device("cuda:0"), 0.0)


# ---- command line -----------------------------------------------------------------------------------------------------------------
def test_command_line_flags(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    cli = __import__("staged_loop")
    a = cli.parse_args([])
    assert a.dedup_value_target == "mean" and a.replay_merge_value_target == "mean"
    a = cli.parse_args(["--dedup-positions", "exact", "--dedup-value-target", "distribution"])
    assert a.dedup_value_target == "distribution"
    a = cli.parse_args(["--replay-generations", "2", "--replay-merge-positions", "symmetric", "--replay-merge-value-target",
                        "distribution"])
    assert a.replay_merge_value_target == "distribution"
    for argv, text in ((["--dedup-value-target", "distribution"], "--dedup-value-target distribution needs --dedup-positions"),
                       (["--replay-generations", "2", "--replay-merge-value-target", "distribution"],
                        "--replay-merge-value-target distribution needs --replay-merge-positions"),
                       (["--dedup-positions", "exact", "--dedup-value-target", "median"], "invalid choice: 'median'")):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
        assert text in capsys.readouterr().err, argv
    stage = __import__("train_stage")
    need = ["--self_play_input", "x"]
    assert stage.parse(need).dedup_value_target == "mean"
    assert stage.parse(need + ["--dedup_positions", "exact", "--dedup_value_target", "distribution"]).dedup_value_target == "distribution"
    assert stage.parse(need + ["--dedup-value-target", "distribution"]).dedup_value_target == "distribution"


# ---- the host code under the sanitizers -----------------------------------------------------------------------------------------
def test_host_code_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    csrc = os.path.join(ROOT, "liuzhou_amd", "csrc")
    exe = str(tmp_path / "value_dist_host_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe,
                           os.path.join(HERE, "value_dist_host_check.cpp"), os.path.join(csrc, "lz_value_dist_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "value_dist_host_check: ok" in res.stdout, res.stdout + res.stderr
