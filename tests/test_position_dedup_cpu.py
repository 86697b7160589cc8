"""CPU: merging duplicate positions among training rows -- the host build of csrc/lz_dedup.h
(tests/dedup_host_check.cpp) and the host library's two entry points against the numpy restatement
(tests/position_dedup.py), the known group counts of the recorded traces, the properties of the merge, parameter
validation, the trainer's refusals and the command-line flags."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from liuzhou_amd import _lib as L
from liuzhou_amd import position_dedup as D
from liuzhou_amd import symmetry as SY
from tests import position_dedup as PD
from tests.golden_utils import load, states, unpack_mask

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "dedup_host_check.cpp")
LIB = os.path.join(HERE, "_build", "liblz_dedup_hostcheck.so")
SEED = 20261019
FIVE = ("planes", "masks", "policy", "value", "soft")
STATS = D.STAT_KEYS + ("mode", "max_copies")


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def hc():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    deps = [SRC] + [os.path.join(ROOT, "liuzhou_amd", "csrc", h) for h in ("lz_dedup.h", "lz_symmetry.h", "lz_rules.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", LIB, SRC])
    H = C.CDLL(LIB)
    H.lzdedup_row_keys.restype = C.c_int64
    H.lzdedup_row_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    H.lzdedup_choose_sym.restype = C.c_int
    H.lzdedup_choose_sym.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    H.lzdedup_frame_map.restype = C.c_int
    H.lzdedup_frame_map.argtypes = [C.c_int, C.c_int]
    H.lzdedup_merge_group.restype = None
    H.lzdedup_merge_group.argtypes = [C.c_void_p] * 5 + [C.c_int64] + [C.c_void_p] * 3
    return H


@pytest.fixture(scope="module")
def g15():
    """The 5 981 states of the rules fixture as training rows: planes through the host states_to_model_input, masks the
    fixture's own."""
    from liuzhou_amd import v0_core
    z = load("g15_rules_large.npz")
    st = states(z, "s")
    t = {f: torch.from_numpy(np.ascontiguousarray(st[f])) for f in ("board", "marks_black", "marks_white", "phase",
                                                                     "current_player")}
    planes = v0_core.states_to_model_input(t["board"], t["marks_black"], t["marks_white"], t["phase"],
                                           t["current_player"]).numpy()
    return planes, unpack_mask(z["legal_mask"], 220).astype(np.uint8)


def _fixture_rows(name, prefix=""):
    z = load(name)
    planes = unpack_mask(z[prefix + "state_tensors"], 396).astype(np.float32).reshape(-1, 11, 6, 6)
    return {"planes": planes, "masks": unpack_mask(z[prefix + "legal_masks"], 220).astype(np.uint8),
            "policy": z[prefix + "policy_targets"].astype(np.float32), "value": z[prefix + "value_targets"].astype(np.float32),
            "soft": z[prefix + "soft_value_targets"].astype(np.float32)}


def _merge(rows, mode, max_copies=1, masks_bool=False):
    """liuzhou_amd.position_dedup on CPU tensors (the host build through the ABI), back as numpy."""
    mk = torch.from_numpy(rows["masks"])
    outs, info = D.merge_duplicate_positions(torch.from_numpy(rows["planes"]), mk.bool() if masks_bool else mk,
                                             torch.from_numpy(rows["policy"]), torch.from_numpy(rows["value"]),
                                             torch.from_numpy(rows["soft"]), mode=mode, max_copies=max_copies)
    return [o.numpy() for o in outs], info


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_matches_restatement(rows, mode, max_copies=1):
    got, info = _merge(rows, mode, max_copies)
    want, winfo = PD.merge_duplicate_positions(*(rows[f] for f in FIVE), mode=mode, max_copies=max_copies)
    for name, g, w in zip(FIVE, got, want):
        assert _same_bits(g, w.astype(g.dtype)), (mode, max_copies, name)
    assert {k: info[k] for k in STATS} == {k: winfo[k] for k in STATS}
    assert np.array_equal(info["group_of_row"].numpy(), winfo["group_of_row"]) and info["group_of_row"].dtype == torch.int64
    assert np.array_equal(info["count"].numpy(), winfo["count"]) and info["count"].dtype == torch.int32
    return got, info


# ---- the header against numpy --------------------------------------------------------------------------------------------
def test_header_keys_symmetry_and_frame_map_on_every_g15_state(hc, g15):
    planes, masks = g15
    n = len(planes)
    assert n == 5981
    images = [SY.np_transform_samples(planes, masks, np.zeros((n, 220), np.float32), k)[:2] for k in range(8)]
    sym_keys, exact_keys = [], []
    for k, (pl, mk) in enumerate(images):
        pl, mk = np.ascontiguousarray(pl, np.float32), np.ascontiguousarray(mk, np.uint8)
        for symmetric in (0, 1):
            keys, sym = np.zeros((n, 8), np.int64), np.zeros(n, np.int8)
            assert hc.lzdedup_row_keys(_p(pl), _p(mk), n, symmetric, _p(keys), _p(sym)) == 0
            wk, ws, wbad = PD.keys(pl, mk, bool(symmetric))
            assert wbad == 0 and np.array_equal(keys, wk) and np.array_equal(sym, ws), (k, symmetric)
            (sym_keys if symmetric else exact_keys).append(keys)
        # the host library's entry point says the same
        tk, ts, tb = D.position_keys(torch.from_numpy(pl), torch.from_numpy(mk), symmetric=True)
        assert np.array_equal(tk.numpy(), sym_keys[-1]) and int(tb) == 0
    for k in range(1, 8):                                       # the eight images of a state share one symmetric key
        assert np.array_equal(sym_keys[k], sym_keys[0]), k
    for a in range(8):                                          # exact keys differ iff planes or masks differ
        for b in range(a + 1, 8):
            same_rows = (images[a][0].reshape(n, -1) == images[b][0].reshape(n, -1)).all(axis=1) & \
                (images[a][1] == images[b][1]).all(axis=1)
            assert np.array_equal((exact_keys[a] == exact_keys[b]).all(axis=1), same_rows), (a, b)
    for a in range(8):
        for b in range(8):
            assert hc.lzdedup_frame_map(a, b) == PD.frame_map(a, b)
    boards, _, _ = PD.read_rows(planes)                          # k* from bit words, all states
    want_sym, want_img = PD.choose_sym(boards, True)
    for i in range(0, n, 7):
        w, img = np.ascontiguousarray(boards[i]), np.zeros(4, np.uint64)
        assert hc.lzdedup_choose_sym(_p(w), 1, _p(img)) == want_sym[i] and np.array_equal(img, want_img[i])


def test_header_merge_group_matches_numpy(hc):
    rows = PD.grid(SEED, spread=True)
    keys, sym, _ = PD.keys(rows["planes"], rows["masks"], True)
    gor, order, begin = PD.group(keys)
    want = PD.merge_groups(*(rows[f] for f in FIVE), sym, order, begin)
    for g in range(len(begin) - 1):
        mem = np.ascontiguousarray(order[begin[g]:begin[g + 1]])
        pol, val, sof = np.zeros(220, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)
        hc.lzdedup_merge_group(_p(rows["policy"]), _p(rows["value"]), _p(rows["soft"]), _p(sym), _p(mem), len(mem),
                               _p(pol), _p(val), _p(sof))
        assert _same_bits(pol, want[2][g]) and _same_bits(val[0], want[3][g]) and _same_bits(sof[0], want[4][g]), g


# ---- known answers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", PD.MODES)
def test_recorded_traces_give_the_counted_groups(mode):
    for rows, n, groups in ((_fixture_rows("g8_selfplay.npz"), 328, 55), (_fixture_rows("g10_tree_selfplay.npz", "a_"), 144, 48)):
        got, info = _assert_matches_restatement(rows, mode)
        assert (info["rows_in"], info["groups"], info["rows_out"], info["not_representable"]) == (n, groups, groups, 0)
        assert len({rows["planes"][i].tobytes() + rows["masks"][i].tobytes() for i in range(n)}) == groups


# ---- the synthetic grid on the host build ---------------------------------------------------------------------------------
@pytest.mark.parametrize("spread,mode", [(False, "exact"), (True, "symmetric"), (True, "exact"), (False, "symmetric")])
def test_grid_is_bit_identical_to_the_restatement(spread, mode):
    rows = PD.grid(SEED, spread)
    got, info = _assert_matches_restatement(rows, mode)
    assert info["not_representable"] == 6
    if spread == (mode == "symmetric"):
        sizes = sorted(info["count"].tolist())
        assert sizes[-4:] == [255, 256, 257, 600] and info["groups"] == 23 and info["merged_groups"] == 13


@pytest.mark.parametrize("max_copies", [2, 5])
def test_max_copies_repeats_groups_consecutively(max_copies):
    rows = PD.grid(SEED, True)
    got, info = _assert_matches_restatement(rows, "symmetric", max_copies)
    once, _ = _merge(rows, "symmetric", 1)
    reps = np.minimum(info["count"].numpy(), max_copies)
    assert info["rows_out"] == int(reps.sum()) == len(got[3])
    for g, o in zip(got, once):
        assert _same_bits(g, np.repeat(o, reps, axis=0))


def test_bool_masks_and_flat_planes_are_accepted():
    rows = PD.grid(SEED, True)
    a, ia = _merge(rows, "symmetric")
    b, ib = _merge(rows, "symmetric", masks_bool=True)
    assert b[1].dtype == np.bool_ and np.array_equal(a[1] != 0, b[1])
    for i in (0, 2, 3, 4):
        assert _same_bits(a[i], b[i])
    flat = dict(rows, planes=rows["planes"].reshape(-1, 11, 36))
    c, _ = _merge(flat, "symmetric")
    assert c[0].shape[1:] == (11, 36) and _same_bits(c[0].reshape(a[0].shape), a[0])


def test_rows_that_must_not_merge():
    rng = np.random.default_rng(3)
    pl = PD.make_planes([0x123456789, 0x0F0F0F0F0 & 0xFFFFFFFFF, 5, 9 << 20], 3)
    other_phase = PD.make_planes([0x123456789, 0x0F0F0F0F0 & 0xFFFFFFFFF, 5, 9 << 20], 4)
    mk = (rng.random(220) < 0.3).astype(np.uint8)
    mk2 = mk.copy()
    mk2[17] ^= 1
    half, two, ragged, neg = pl.copy(), pl.copy(), pl.copy(), pl.copy()
    half[1, 0] = 0.5
    two[9] = 1.0
    ragged[6, 3] = 0.0
    neg[neg == 0] = -0.0
    planes = np.stack([pl, other_phase, pl, half, half, two, two, ragged, ragged, neg, pl]).reshape(-1, 11, 6, 6)
    masks = np.stack([mk, mk, mk2, mk, mk, mk, mk, mk, mk, mk, mk])
    n = len(planes)
    rows = {"planes": planes, "masks": masks, "policy": (rng.random((n, 220)) * masks).astype(np.float32),
            "value": rng.uniform(-1, 1, n).astype(np.float32), "soft": rng.uniform(-1, 1, n).astype(np.float32)}
    for mode in PD.MODES:
        got, info = _assert_matches_restatement(rows, mode)
        # rows 0, 9 (-0.0 is a zero) and 10 are one position; everything else stands alone
        assert info["group_of_row"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 0]
        assert info["not_representable"] == 6 and info["largest_group"] == 3 and info["merged_rows"] == 3
        keys, sym, bad = D.position_keys(torch.from_numpy(planes), torch.from_numpy(masks), symmetric=mode == "symmetric")
        assert int(bad) == 6 and keys.dtype == torch.int64 and sym.dtype == torch.int8
        for i in range(3, 9):
            assert keys[i].tolist() == [-(1 << 63) + i, 0, 0, 0, 0, 0, 0, 0] and int(sym[i]) == 0


def test_the_policy_count_skips_members_without_a_policy():
    pl = PD.make_planes([7, 56, 0, 0], 1).reshape(1, 11, 6, 6)
    mk = np.zeros((1, 220), np.uint8)
    mk[0, :4] = 1
    p = np.zeros(220, np.float32)
    p[:4] = (0.1, 0.2, 0.3, 0.4)
    q = np.zeros(220, np.float32)
    q[:4] = (0.4, 0.4, 0.1, 0.1)
    zero = np.zeros(220, np.float32)
    rows = {"planes": np.repeat(pl, 5, 0), "masks": np.repeat(mk, 5, 0), "policy": np.stack([p, zero, q, zero, zero]),
            "value": np.array([1, -1, 1, 0, 0], np.float32), "soft": np.array([0.5, -0.5, 0.25, 0, 0], np.float32)}
    got, info = _assert_matches_restatement(rows, "exact")
    assert info["groups"] == 1 and info["count"].tolist() == [5]
    assert np.array_equal(got[2][0], ((p.astype(np.float64) + q.astype(np.float64)) / 2).astype(np.float32))
    assert got[3][0] == np.float32(1.0 / 5) and got[4][0] == np.float32(0.25 / 5)
    rows["policy"][:] = 0                                        # no member has a policy: the merged policy is zero
    got, _ = _assert_matches_restatement(rows, "exact")
    assert not got[2].any() and got[3][0] == np.float32(0.2)


def test_empty_and_single_row():
    for n in (0, 1):
        rows = {k: v[:n] for k, v in PD.grid(SEED, False).items()}
        for mode in PD.MODES:
            got, info = _assert_matches_restatement(rows, mode)
            assert info["rows_in"] == info["rows_out"] == info["groups"] == n and info["merged_groups"] == 0
            assert info["largest_group"] == n and got[0].shape == (n, 11, 6, 6)
            for f, g in zip(FIVE, got):
                assert _same_bits(g, rows[f])


def _abi_merge(lib, rows, sym, order, begin, n=None):
    n = len(rows["value"]) if n is None else n
    G = len(begin) - 1
    outs = [np.full((G, 11, 36), 7, np.float32), np.full((G, 220), 7, np.uint8), np.full((G, 220), 7, np.float32),
            np.full(G, 7, np.float32), np.full(G, 7, np.float32), np.full(G, 7, np.int32)]
    planes = np.ascontiguousarray(rows["planes"].reshape(-1, 396))
    st = lib.lz_dedup_merge_groups(_p(planes), _p(rows["masks"]), _p(rows["policy"]), _p(rows["value"]), _p(rows["soft"]),
                                   n, _p(sym), _p(order), _p(begin), G, *[_p(o) for o in outs], None)
    return st, outs


def test_abi_order_out_of_range_gives_a_zero_row_and_argument_checks():
    H = L.host_lib()
    rows = PD.grid(SEED, True)
    n = len(rows["value"])
    keys, sym, _ = PD.keys(rows["planes"], rows["masks"], True)
    _, order, begin = PD.group(keys)
    big = int(np.argmax(np.diff(begin)))                         # the 600-member group: an entry of its last chunk
    for bad_value in (n, -1, 1 << 40):
        broken = order.copy()
        broken[begin[big] + 555] = bad_value
        st, outs = _abi_merge(H, rows, sym, broken, begin)
        want = PD.merge_groups(*(rows[f] for f in FIVE), sym, broken, begin, check_members=False)
        assert st == 0 and want[5][big] == 0 and want[5].sum() == n - 600
        for o, w in zip(outs, want):
            assert _same_bits(o.reshape(w.shape), w)
        assert not outs[0][big].any() and not outs[2][big].any() and outs[3][big] == 0 and outs[5][big] == 0
    bad_sym = sym.copy()
    bad_sym[order[begin[big] + 3]] = 9
    st, outs = _abi_merge(H, rows, bad_sym, order, begin)
    assert st == 0 and outs[5][big] == 0
    ranges = begin.copy()                                        # an impossible range
    ranges[-1] = n + 1
    st, outs = _abi_merge(H, rows, sym, order, ranges)
    assert st == 0 and outs[5][-1] == 0 and outs[5][:-1].tolist() == np.diff(begin)[:-1].tolist()
    # conventions: nothing to do is ok without touching anything; bad arguments are refused
    assert H.lz_dedup_merge_groups(*[None] * 5, 0, None, None, None, 0, *[None] * 6, None) == 0
    assert H.lz_dedup_position_keys(None, None, 0, 1, None, None, None, None) == 0
    assert H.lz_dedup_position_keys(None, None, 4, 1, None, None, None, None) == -1
    assert H.lz_dedup_position_keys(None, None, -1, 1, None, None, None, None) == -1
    k8, s1, c1 = np.zeros((n, 8), np.int64), np.zeros(n, np.int8), np.zeros(1, np.int32)
    planes = np.ascontiguousarray(rows["planes"].reshape(-1, 396))
    assert H.lz_dedup_position_keys(_p(planes), _p(rows["masks"]), n, 2, _p(k8), _p(s1), _p(c1), None) == -1
    assert H.lz_dedup_merge_groups(*[None] * 5, n, None, None, None, 3, *[None] * 6, None) == -1
    assert H.lz_dedup_merge_groups(*[None] * 5, -1, None, None, None, 3, *[None] * 6, None) == -1
    c1[0] = 40                                                   # the counter is add-only
    assert H.lz_dedup_position_keys(_p(planes), _p(rows["masks"]), n, 1, _p(k8), _p(s1), _p(c1), None) == 0
    assert c1[0] == 46 and np.array_equal(k8, keys) and np.array_equal(s1, sym)


# ---- properties ------------------------------------------------------------------------------------------------------------
def _unique_rows(n, seed):
    rng = np.random.default_rng(seed)
    planes = np.stack([PD.make_planes([int(x) for x in rng.integers(0, 1 << 36, 4, dtype=np.uint64)], int(rng.integers(0, 8)))
                       for _ in range(n)]).reshape(n, 11, 6, 6)
    masks = (rng.random((n, 220)) < 0.2).astype(np.uint8)
    masks[:, 0] = 1
    policy = (rng.random((n, 220)) * masks).astype(np.float32)
    policy /= policy.sum(axis=1, keepdims=True, dtype=np.float32)
    return {"planes": planes, "masks": masks, "policy": policy, "value": rng.integers(-1, 2, n).astype(np.float32),
            "soft": rng.uniform(-1, 1, n).astype(np.float32)}


def test_input_without_duplicates_comes_back_byte_for_byte():
    rows = _unique_rows(300, 5)
    rows["policy"][7] = 0
    rows["policy"][8, ::2] = -0.0
    rows["value"][9] = -0.0
    for mode in PD.MODES:
        got, info = _merge(rows, mode)
        assert info["groups"] == 300 and info["merged_groups"] == 0 and info["largest_group"] == 1
        for f, g in zip(FIVE, got):
            assert _same_bits(g, rows[f]), (mode, f)


def test_three_copies_merge_back_to_the_rows():
    x = _unique_rows(200, 6)
    x["value"][:] = np.random.default_rng(1).integers(-1, 2, 200)
    tripled = {f: np.concatenate([x[f]] * 3) for f in FIVE}
    got, info = _merge(tripled, "exact")
    assert info["rows_out"] == 200 and info["merged_groups"] == 200 and info["largest_group"] == 3
    for f, g in zip(FIVE, got):
        assert _same_bits(g, x[f]), f                            # (x + x + x) / 3 == x in double, exactly


@pytest.mark.parametrize("mode", PD.MODES)
def test_singletons_are_bit_copies_and_policies_keep_their_mass(mode):
    rows = PD.grid(SEED, True)
    got, info = _merge(rows, mode)
    gor, count = info["group_of_row"].numpy(), info["count"].numpy()
    first = np.array([int(np.flatnonzero(gor == g)[0]) for g in range(len(count))])
    for f, g in zip(FIVE, got):
        for grp in np.flatnonzero(count == 1):
            assert _same_bits(g[grp], rows[f][first[grp]]), (f, grp)
    assert _same_bits(got[0], rows["planes"][first]) and _same_bits(got[1], rows["masks"][first])
    for grp in np.flatnonzero(count > 1):
        mem = np.flatnonzero(gor == grp)
        sums = rows["policy"][mem].astype(np.float64).sum(axis=1)
        valid = (rows["policy"][mem] != 0).any(axis=1)
        want = sums[valid].mean() if valid.any() else 0.0
        assert abs(float(got[2][grp].astype(np.float64).sum()) - want) < 1e-6, grp
        assert not got[2][grp][got[1][grp] == 0].any()           # the merged policy stays on the first member's legal actions


# ---- validation and refusals ---------------------------------------------------------------------------------------------
def test_parameters_are_validated_on_and_off():
    assert D.dedup_on("off", 1) is False and D.dedup_on("exact", 1) is True and D.dedup_on("symmetric", 4) is True
    assert D.dedup_on("off", 3) is False
    for mode in ("off", "exact"):
        for bad in (0, -1, True, False, 1.5, float("nan"), float("inf"), None, "2"):
            with pytest.raises(ValueError, match="dedup_max_copies"):
                D.dedup_on(mode, bad)
    for bad in ("on", "", None, 1, "Exact"):
        with pytest.raises(ValueError, match="dedup_positions"):
            D.dedup_on(bad, 1)
    x = _unique_rows(4, 1)
    t = [torch.from_numpy(x[f]) for f in FIVE]
    with pytest.raises(ValueError):
        D.merge_duplicate_positions(*t, mode="off")
    with pytest.raises(TypeError):
        D.merge_duplicate_positions(t[0].double(), *t[1:], mode="exact")
    with pytest.raises(TypeError):
        D.merge_duplicate_positions(t[0], t[1].int(), *t[2:], mode="exact")
    with pytest.raises(ValueError):
        D.merge_duplicate_positions(t[0], t[1][:3], *t[2:], mode="exact")
    with pytest.raises(ValueError):
        D.merge_duplicate_positions(*t[:3], t[3][:2], t[4], mode="exact")


def test_trainer_refuses_draw_options_and_bad_parameters():
    from liuzhou_amd.train_bridge import train_network_from_tensors
    from tests.stage_stub import random_batch
    batch = random_batch(8, 1)
    for kw in ({"policy_draw_weight": 0.5}, {"anti_draw_penalty": 0.1}, {"anti_draw_penalty": -0.1}):
        for mode in ("exact", "symmetric"):
            with pytest.raises(ValueError, match="drawn game"):
                train_network_from_tensors(None, batch, dedup_positions=mode, **kw)
    with pytest.raises(ValueError, match="dedup_positions"):
        train_network_from_tensors(None, batch, dedup_positions="on")
    for bad in (0, True, 1.5):
        for mode in ("off", "exact"):
            with pytest.raises(ValueError, match="dedup_max_copies"):
                train_network_from_tensors(None, batch, dedup_positions=mode, dedup_max_copies=bad)


# ---- command line ---------------------------------------------------------------------------------------------------------
def _train_cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train_stage as cli
    return cli


def test_train_stage_flags_parse():
    cli = _train_cli()
    a = cli.parse(["--self_play_input", "x", "--dedup_positions", "symmetric", "--dedup_max_copies", "3"])
    assert a.dedup_positions == "symmetric" and a.dedup_max_copies == 3 and a.ignored == []
    a = cli.parse(["--self_play_input", "x"])
    assert a.dedup_positions == "off" and a.dedup_max_copies == 1
    with pytest.raises(SystemExit):
        cli.parse(["--self_play_input", "x", "--dedup_positions", "fuzzy"])
    text = open(os.path.join(ROOT, "scripts", "staged_loop.py")).read()
    assert '"--dedup-positions"' in text and '"--dedup-max-copies"' in text


def test_train_stage_passes_the_keywords_only_when_on(monkeypatch, tmp_path):
    cli = _train_cli()
    import liuzhou_amd.self_play_stage as S
    import liuzhou_amd.streaming as ST
    import liuzhou_amd.train_bridge as TB
    from tests.stage_stub import random_batch
    seen = {}

    def train(model, samples, **kw):
        seen.clear()
        seen.update(kw)
        return model, {"epoch_stats": [{"samples": 1}]}

    monkeypatch.setattr(TB, "train_network_from_tensors", train)
    monkeypatch.setattr(TB, "train_network_streaming", lambda model, loader, **kw: train(model, None, streaming=True, **kw))
    monkeypatch.setattr(S, "load_self_play_payload", lambda p, **kw: (random_batch(4, 1), {}))
    monkeypatch.setattr(S, "concat_batches", lambda batches: batches[0])
    monkeypatch.setattr(S, "resolve_shard_specs", lambda *a, **kw: ([], 4))
    monkeypatch.setattr(ST, "build_streaming_dataloader", lambda *a, **kw: [])
    base = ["--model", "b6c64", "--self_play_input", "x.pt", "--checkpoint_dir", str(tmp_path), "--device", "cpu"]
    assert cli.main(base) == 0
    assert "dedup_positions" not in seen and "dedup_max_copies" not in seen
    assert cli.main(base + ["--dedup_positions", "off"]) == 0
    assert "dedup_positions" not in seen and "dedup_max_copies" not in seen
    assert cli.main(base + ["--dedup_positions", "symmetric", "--dedup_max_copies", "4"]) == 0
    assert seen["dedup_positions"] == "symmetric" and seen["dedup_max_copies"] == 4
    assert cli.main(base + ["--dedup_positions", "exact"]) == 0
    assert seen["dedup_positions"] == "exact" and seen["dedup_max_copies"] == 1
    assert cli.main(base + ["--streaming_load", "1"]) == 0 and seen.get("streaming") and "dedup_positions" not in seen
    with pytest.raises(SystemExit, match="one batch at a time"):
        cli.main(base + ["--streaming_load", "1", "--dedup_positions", "exact"])
    with pytest.raises(ValueError, match="dedup_max_copies"):
        cli.main(base + ["--dedup_max_copies", "0"])
