"""CPU: what tests/test_gpu_root_ops.py stands on.  The restatements of tests/root_ops_ref.py are anchored on the reference's
golden values (g4_project.npz, g7_ops.npz) and, on the seeded rows of tests/root_ops_cases.py, on oracle/lz_oracle.py; the
builders are counted class by class, so that the GPU run finds every case it names; and every case goes through the host
build of the same C ABI (csrc/lz_host.cpp) under the checks of tests/root_ops_check.py that the kernels get -- which is
where the two fixes of DESIGN.md section 23 (the NaN-aware argmax, root_value of a row without valid action) are pinned on
the host side."""
import collections

import numpy as np
import pytest

from oracle import lz_oracle as O
from tests import root_ops_cases as K
from tests import root_ops_check as X
from tests import root_ops_ref as Rf
from tests.golden_utils import load, unpack_mask


@pytest.fixture(scope="module")
def host():
    from liuzhou_amd import _lib
    return X.Build(_lib, "cpu")


# =========================================================================================================================
# the restatements against the reference's golden values
# =========================================================================================================================
def test_project_restatement_equals_the_golden_projection():
    z = load("g4_project.npz")
    probs, ml = Rf.ref_project(z["lp1"], z["lp2"], z["lpmc"], unpack_mask(z["mask"], 220))
    X.assert_bits(ml, z["masked_logits"], "masked_logits")               # a copy or one float32 add: bit for bit
    bound, measured = X.project_bound()
    assert np.abs(z["probs"] - probs).max() <= max(measured, 2.0 ** -23), "the reference's float32 softmax is further away than float32 explains"
    assert 0 < bound <= Rf.PROJECT_CAP


def golden_pack(z):
    mask, cap = unpack_mask(z["mask"], 220), 80
    counts, li, pri, codes = Rf.ref_pack_rows(mask, z["probs"], z["meta"].astype(np.int32), cap)
    rank, off, sizes = Rf.ref_pack_plan(counts)
    R, M, N = (int(x) for x in sizes)
    return counts, Rf.ref_pack_fill(counts, li, pri.astype(np.float32), codes, rank, off, R, M, N), pri, rank


def test_pack_restatement_equals_the_golden_pack():
    z = load("g7_ops.npz")
    counts, got, pri64, rank = golden_pack(z)
    for k in Rf.PACK_FILL_OUT:
        want = z[f"pack_{k}"]
        assert got[k].shape == want.shape, k
        if k == "priors_mat":
            n = np.repeat(z["pack_counts"][:, None], want.shape[1], 1)
            live = z["pack_valid_mask"]
            p64 = np.zeros(want.shape)
            p64[rank[rank >= 0]] = pri64[rank >= 0][:, :want.shape[1]]
            rel = np.abs(want[live] - p64[live]) / p64[live]
            assert (rel <= Rf.priors_bound(n[live])).all() and (want[~live] == 0).all()
        else:
            assert np.array_equal(got[k].astype(want.dtype), want), k


def test_finalize_restatement_equals_the_golden_finalize():
    z = load("g7_ops.npz")
    B = z["pack_terminal_mask"].shape[0]
    got = Rf.ref_finalize(z["pack_legal_index_mat"], z["pack_action_code_mat"], z["pack_valid_mask"], z["fin_visits"],
                          z["fin_value_sum"], z["pack_valid_root_indices"], B, 220, z["fin_temps"])
    assert np.array_equal(got["chosen_index"], z["fin_chosen_idx"]) and np.array_equal(got["chosen_codes"], z["fin_chosen_codes"])
    assert np.array_equal(got["chosen_valid"].astype(bool), z["fin_chosen_valid"])
    assert (np.abs(z["fin_root_value"] - got["root_value"]) <= got["root_value_bound"]).all()
    c = dict(lidx=z["pack_legal_index_mat"], valid=z["pack_valid_mask"], temps=z["fin_temps"], roots=z["pack_valid_root_indices"],
             B=B, T=220, R=z["fin_temps"].shape[0])
    assert (np.abs(z["fin_policy_dense"] - got["policy"]) <= X.column_bounds(c, got)).all()    # torch's float32, T in {0.1, 1}
    assert not got["overflow"].any()


def test_trajectory_restatement_equals_the_golden_trajectory():
    z = load("g7_ops.npz")
    S = z["traj_value_out"].shape[0]
    nan = np.full(S, np.nan, np.float32)
    vt, st, keep, fc, co = Rf.ref_finalize_trajectory(nan, nan, z["traj_signs"], z["traj_step_index"], z["traj_counts"], 20,
                                                      z["traj_slots"], z["traj_result"], z["traj_soft"], np.zeros(3, np.int64))
    assert np.array_equal(vt, z["traj_value_out"], equal_nan=True) and np.array_equal(st, z["traj_soft_out"], equal_nan=True)
    k = keep != 0
    assert np.array_equal(z["traj_slots"][k], z["traj_final_slots"]) and np.array_equal(fc[k], z["traj_final_counts"])
    assert np.array_equal(co, z["traj_counts_out"])


# =========================================================================================================================
# the restatements against oracle/lz_oracle.py on the seeded rows
# =========================================================================================================================
@pytest.mark.parametrize("T", (217, 220))
def test_project_restatement_equals_the_oracle(T):
    bound, _ = X.project_bound()
    for B in K.PROJECT_B:
        c = K.project_case(T, B)
        probs, ml = O.project_policy(c["lp1"], c["lp2"], c["lpmc"], c["mask"], ad=T - 216)
        want_p, want_ml = Rf.ref_project(c["lp1"], c["lp2"], c["lpmc"], c["mask"])
        X.assert_bits(ml, want_ml, f"T={T} B={B} masked_logits")
        assert np.abs(probs - want_p).max() <= bound


def test_pack_restatement_equals_the_oracle():
    for c in K.pack_cases():
        counts, li, pri, codes = Rf.ref_pack_rows(c["mask"], c["probs"], c["meta"], c["cap"])
        rank, off, sizes = Rf.ref_pack_plan(counts)
        R, M, N = (int(x) for x in sizes)
        got = Rf.ref_pack_fill(counts, li, pri.astype(np.float32), codes, rank, off, R, M, N)
        want = O.root_pack_sparse_actions(c["mask"], c["probs"], c["meta"])
        for k, w in zip(Rf.PACK_FILL_OUT, want):
            if k == "priors_mat":
                sums = Rf.pack_row_sums(c["mask"], c["probs"])[rank >= 0]
                ok = sums >= 1e-8                                         # under the clamp float32 and float64 1e-8 differ
                np.testing.assert_allclose(w[ok], got[k][ok], rtol=float(Rf.priors_bound(M)), atol=0, err_msg=str(c["B"]))
            else:
                assert np.array_equal(got[k].reshape(w.shape).astype(w.dtype), w), (k, c["B"], c["T"], c["pattern"])


def in_range_columns(c):
    """The oracle scatters with numpy indexing, which has no place for a column of T or -1."""
    return np.where((c["lidx"] < 0) | (c["lidx"] >= c["T"]), 0, c["lidx"])


@pytest.mark.parametrize("M", K.FIN_M)
def test_finalize_restatement_equals_the_oracle(M):
    for R in K.FIN_R:
        c = K.finalize_case(M, R)
        lidx = in_range_columns(c)
        live = (c["valid"] != 0).any(1)                                   # the oracle has no rows without valid action
        sel = np.flatnonzero(live)
        got = Rf.ref_finalize(lidx[sel], c["codes"][sel], c["valid"][sel], c["visits"][sel], c["value_sum"][sel],
                              c["roots"][sel], c["B"], c["T"], c["temps"][sel])
        with np.errstate(all="ignore"):
            want = O.root_finalize_from_visits(lidx[sel], c["codes"][sel], c["valid"][sel] != 0, c["visits"][sel],
                                               c["value_sum"][sel], c["roots"][sel], c["B"], c["T"], c["temps"][sel])
        assert np.array_equal(got["chosen_index"], want[1]), (M, R, np.flatnonzero(got["chosen_index"] != want[1]))
        assert np.array_equal(got["chosen_codes"], want[2]) and np.array_equal(got["chosen_valid"].astype(bool), want[3])
        assert np.array_equal(np.isnan(got["policy"]), np.isnan(want[0])), "the overflow rows: NaN where the oracle has NaN"
        cc = dict(c, lidx=lidx[sel], valid=c["valid"][sel], temps=c["temps"][sel], roots=c["roots"][sel], R=sel.size)
        err = np.where(np.isnan(want[0]), 0, np.abs(want[0] - got["policy"]))
        assert (err <= X.column_bounds(cc, got)).all()
        assert (np.abs(want[4] - got["root_value"]) <= got["root_value_bound"]).all()


def test_trajectory_restatement_equals_the_oracle():
    for c in K.traj_cases():
        inside = (c["slots"] >= 0) & (c["slots"] < c["G"])                # the oracle indexes with the slot
        nan = np.full(c["S"], np.nan, np.float32)
        vt, st, keep, fc, co = Rf.ref_finalize_trajectory(nan, nan, c["signs"], c["step_index"], c["step_counts"],
                                                          c["max_steps"], c["slots"], c["result"], c["softv"], np.zeros(3))
        wv, ws = nan.copy(), nan.copy()
        fs, fcw, cow = O.finalize_trajectory_inplace(wv, ws, c["signs"], c["step_index"],
                                                     np.minimum(c["step_counts"], c["max_steps"]), c["slots"][inside],
                                                     c["result"][inside], c["softv"][inside])
        X.assert_bits(vt, wv, "value_targets"); X.assert_bits(st, ws, "soft_value_targets")
        k = keep != 0
        assert np.array_equal(c["slots"][k], fs) and np.array_equal(fc[k], fcw) and np.array_equal(co, cow)
        assert not keep[~inside].any() and not fc[~inside].any()


# =========================================================================================================================
# the builders reach every class they name
# =========================================================================================================================
def test_projection_cases_cover_their_classes():
    n = collections.Counter()
    for c in K.project_cases():
        n.update(c["cls"].tolist())
        x = Rf.ref_logits(c["lp1"], c["lp2"], c["lpmc"], c["T"])
        legal = c["mask"] != 0
        assert not (legal & (np.isnan(x) | np.isposinf(x))).any(), "a NaN or +inf on a legal entry has no defined answer"
        for b, k in enumerate(c["cls"]):
            lx = x[b, legal[b]]
            if k == "none":
                assert lx.size == 0
            elif k.startswith("one_") and k != "one_ninf_head":
                seg = np.searchsorted([36, 180, 216], np.flatnonzero(legal[b])[0], side="right")
                assert lx.size == 1 and np.isfinite(lx).all() and seg == ["one_placement", "one_movement", "one_selection", "one_auxiliary"].index(k)
            elif k in ("offboard_only", "all_ninf"):
                assert lx.size >= 2 and np.isneginf(lx).all()
                assert k == "all_ninf" or ((np.flatnonzero(legal[b]) >= 36) & (np.flatnonzero(legal[b]) < 180)).all()
            elif k == "one_ninf_head":
                assert np.isneginf(lx).any() and np.isfinite(lx).any()
            elif k == "underflow":
                assert (lx <= -9000).any()
            elif k == "board_full":
                assert legal[b, :216].all()
            elif k == "auxiliary_only":
                assert np.flatnonzero(legal[b]).min() >= 216
            elif k == "nan_illegal":
                assert np.isnan(x[b]).sum() >= 3 and np.isfinite(lx).any()
    assert {c["B"] for c in K.project_cases()} == set(K.PROJECT_B) and {c["T"] for c in K.project_cases()} == set(K.PROJECT_T)
    assert all(n[k] >= 4 for k in K.PROJECT_CLASSES), n
    print(dict(n))


def test_pack_cases_cover_their_classes():
    n = collections.Counter()
    for c in K.pack_cases():
        counts = (c["mask"] != 0).sum(1)
        assert counts.max(initial=0) <= c["cap"], "more legal entries than cap is outside the operator's contract"
        sums = Rf.pack_row_sums(c["mask"], c["probs"])
        for b, k in enumerate(c["cls"]):
            n[k] += 1
            if k.startswith("count_"):
                assert counts[b] == (c["cap"] if k == "count_cap" else int(k[6:]))
                n[f"count_cap_{c['cap']}"] += k == "count_cap"
            elif k == "clamp":
                assert 0 < sums[b] < 1e-8
            elif k == "zeros":
                assert sums[b] == 0 and counts[b] > 0
            elif k == "negative_meta":
                assert (c["meta"][b] < 0).all()
        n[c["pattern"]] += 1
        if c["pattern"] == "all_terminal":
            assert counts.sum() == 0
        if c["pattern"] == "ends_terminal":
            assert counts[0] == 0 and counts[-1] == 0
    assert all(n[k] >= 1 for k in K.PACK_CLASSES + K.PACK_PATTERNS), n
    assert n["count_cap_80"] >= 4 and n["count_cap_72"] >= 4, n
    assert {(c["B"], c["T"]) for c in K.pack_cases()} >= {(B, T) for B in K.PACK_B for T in K.PACK_T}
    print(dict(n))


def test_plan_cases_cover_the_scan():
    seen = set()
    for c in K.plan_cases():
        seen.add((c["B"], c["pattern"]))
        if c["pattern"] == "runs" and c["B"] > 1024:
            assert c["per"] > 1                                           # every thread scans several rows
            per = c["per"]
            kinds = set()
            for lo, hi in c["runs"]:
                assert (c["counts"][lo:hi] == 0).all()
                kinds.add("thread" if lo // per != (hi - 1) // per else "")
                kinds.add("wave" if lo // (64 * per) != (hi - 1) // (64 * per) else "")
            assert {"thread", "wave"} <= kinds
    assert seen == {(B, p) for B in K.PLAN_B for p in ("mixed", "all_terminal", "ends_terminal", "runs")}


def test_finalize_cases_cover_their_classes():
    n = collections.Counter()
    groups = collections.defaultdict(set)
    for c in K.finalize_cases():
        M, R = c["M"], c["R"]
        valid = c["valid"] != 0
        inv_t = Rf.finalize_inv_t(c["temps"])
        assert c["B"] > R and (np.diff(c["roots"]) > 0).all() and (np.diff(c["roots"]) > 1).any() | (R == 1)
        assert not np.array_equal(c["roots"], np.arange(R))
        assert (c["visits"][~valid] == 0).all()                           # an overflow on a slot that is not valid stays out
        for r in range(R):
            k = c["cls"][r]
            n[k] += 1
            n[f"T={c['temps'][r]:g}"] += 1
            pol, over = Rf.ref_row_policy(c["visits"][r], valid[r], inv_t[r])
            with np.errstate(over="ignore"):
                p64 = np.where(valid[r], np.power(np.maximum(c["visits"][r].astype(np.float64), 1e-8), float(inv_t[r])), 0)
            lim = float(np.finfo(np.float32).max)                         # no power, and no sum, sits near the overflow
            assert not ((p64 > lim / 4) & (p64 < lim * 2)).any() and (over or p64.sum() < lim / 4)
            if over:
                first = int(np.flatnonzero(np.isnan(pol))[0])
                n["overflow"] += 1
                n["overflow_away_from_slot_0"] += first > 0
                n["overflow_slot_0_invalid"] += first > 0 and not valid[r, 0]
                n[f"overflow_inv_t={inv_t[r]:g}"] += 1
                n[f"overflow_{k}"] += 1
            if k == "all_zero":
                assert (c["visits"][r][valid[r]] == 0).all() and valid[r].any()
            elif k == "single_last" and M > 1:
                assert np.flatnonzero(valid[r]).tolist() == [M - 1]
            elif k == "no_valid":
                assert not valid[r].any()
                n[f"no_valid_at_{'first' if r == 0 else 'last' if r == R - 1 else 'middle'}"] += 1
            elif k == "dup_cols" and M > 1:
                cols = c["lidx"][r][valid[r]]
                assert np.unique(cols).size < cols.size
            elif k == "col_T_and_neg":
                cols = c["lidx"][r][valid[r]]
                assert (cols == c["T"]).any()
                n["col_neg"] += (cols == -1).any()
            elif k == "mixed_value":
                assert (c["value_sum"][r] > 0).any() and (c["value_sum"][r] < 0).any() or valid[r].sum() < 2
            elif k == "tiny_visits":
                assert 0 < c["visits"][r].sum() < 1
            n["zero_visits_on_valid_slot"] += bool((c["visits"][r][valid[r]] == 0).any())
            # ---- the sampled pick: the builder aimed, the restatement must land there with room to spare ----------------
            kind = c["kinds"][r]
            if kind == "none":
                continue
            pick, width, w, live = Rf.ref_sampled_pick(c["visits"][r], valid[r], inv_t[r], c["uniforms"][r])
            assert pick == c["target"][r], (M, R, r, kind)
            assert width > K.MIN_WIDTH, f"M={M} R={R} row {r}: interval {width:.2e} of the total would need a candidate set"
            assert not (valid[r] & (w >= K.DENORMAL_BAND[0]) & (w <= K.DENORMAL_BAND[1])).any(), "a weight float32 may flush"
            cum = np.cumsum(w)
            if kind == "u_zero":
                assert c["uniforms"][r] == 0 and pick == np.flatnonzero(live)[0]
            elif kind == "u_top":
                assert c["uniforms"][r] == np.nextafter(np.float32(1), np.float32(0)) and pick == np.flatnonzero(live)[-1]
            else:                                                         # the midpoint: half a width to either edge
                u = float(c["uniforms"][r])
                assert min(cum[pick] - u, u - (cum[pick] - w[pick])) > K.MIN_WIDTH / 2.5
            if kind == "after_invalid_run":
                assert not valid[r, pick - 3:pick].any()
            n[f"pick_{kind}"] += 1
            groups[M].add(pick // 64)
    assert all(n[k] >= 1 for k in K.FIN_CLASSES), n
    assert all(n[f"pick_{k}"] >= 1 for k in K.PICK_KINDS), n
    assert all(n[f"T={t:g}"] >= 1 for t in K.FIN_TEMPS), n
    assert n["overflow"] >= 4 and n["overflow_dominant_8192"] >= 4 and n["overflow_dominant_65536"] >= 4, n
    assert n["overflow_inv_t=10"] >= 4 and n["overflow_inv_t=1e+06"] >= 4, n       # T = 0.1, and the clamp (1e-6, 0, -1)
    assert n["overflow_away_from_slot_0"] >= 4 and n["overflow_slot_0_invalid"] >= 4, n
    assert all(n[f"no_valid_at_{p}"] >= 1 for p in ("first", "middle", "last")), n
    assert n["col_neg"] >= 1 and n["zero_visits_on_valid_slot"] >= 1
    assert all(groups[M] == set(range(-(-M // 64))) for M in K.FIN_M if M > 1), dict(groups)   # a sampled pick in every 64-wide group
    print(dict(n))


def test_trajectory_cases_cover_their_classes():
    n = collections.Counter()
    for c in K.traj_cases():
        G, ms = c["G"], c["max_steps"]
        inside = (c["slots"] >= 0) & (c["slots"] < G)
        games = c["slots"][inside]
        assert np.unique(games).size == games.size, "two finished slots of one game would race"
        assert np.unique(c["step_index"]).size == c["step_index"].size and c["step_index"].max() < c["S"]
        n["slot_-1"] += (c["slots"] == -1).any(); n["slot_G"] += (c["slots"] == G).any()
        for g in games:
            k = int(c["step_counts"][g])
            n["count_0"] += k == 0; n["count_1"] += k == 1; n["count_64"] += k == 64 <= ms; n["count_65"] += k == 65 <= ms
            n["count_max"] += k == ms; n["count_past_max"] += k > ms; n["stride_iterates"] += min(k, ms) > 64
        for v, name in ((-1.0, "loss"), (1.0, "win")):
            n[name] += (c["result"] == v).any()
        n["zero"] += ((c["result"] == 0) & ~np.signbit(c["result"])).any(); n["minus_zero"] += ((c["result"] == 0) & np.signbit(c["result"])).any()
        n["both_signs"] += set(c["signs"].tolist()) == {-1, 1}
        written = np.zeros(c["S"], bool)
        for g in games:
            written[c["step_index"][g, :min(int(c["step_counts"][g]), ms)]] = True
        n["untouched_rows"] += (~written).any()
        assert (np.asarray(K.TRAJ_COUNTS_IN) != 0).all()
    assert all(v >= 1 for v in n.values()) and len(n) == 15, n
    assert {(c["F"], c["G"], c["max_steps"]) for c in K.traj_cases()} == {(F, G, s) for F in K.TRAJ_F for G in K.TRAJ_G for s in K.TRAJ_STEPS}
    print(dict(n))


# =========================================================================================================================
# every case through the host build
# =========================================================================================================================
@pytest.mark.parametrize("T", K.PROJECT_T)
def test_host_projection_equals_the_restatement(host, T):
    for B in K.PROJECT_B:
        X.check_project(host, K.project_case(T, B))


@pytest.mark.parametrize("B", K.PACK_B)
def test_host_pack_equals_the_restatement(host, B):
    for c in K.pack_cases():
        if c["B"] == B:
            X.check_pack_chain(host, c)


@pytest.mark.parametrize("B", K.PLAN_B)
def test_host_plan_equals_the_restatement(host, B):
    for c in K.plan_cases():
        if c["B"] == B:
            X.check_pack_plan(host, c["counts"], f"B={B} {c['pattern']}")


@pytest.mark.parametrize("sampled", (False, True), ids=("argmax", "sampled"))
@pytest.mark.parametrize("M", K.FIN_M)
def test_host_finalize_equals_the_restatement(host, M, sampled):
    for R in K.FIN_R:
        X.check_finalize(host, K.finalize_case(M, R), sampled)


@pytest.mark.parametrize("max_steps", K.TRAJ_STEPS)
def test_host_trajectory_equals_the_restatement(host, max_steps):
    for c in K.traj_cases():
        if c["max_steps"] == max_steps:
            X.check_traj(host, c)


def test_host_argmax_takes_the_overflowed_action_not_slot_0(host):
    """visits^(1/T) overflows float32 from about 7132 visits at T = 0.1: the reference's policy is NaN there and 0
    elsewhere, and torch's max takes the first NaN.  Slot 0 is padding here; it used to be returned as a valid choice."""
    X.check_finalize(host, K.overflow_pin_case(), False)
    got = X.run_finalize(host, K.overflow_pin_case(), False)
    assert got["chosen_index"].tolist() == [-1, 9, 11] and got["chosen_valid"].tolist() == [0, 1, 1]


def test_host_root_value_is_written_for_a_row_without_valid_action(host):
    c = K.no_valid_pin_case()
    got, _, _ = X.check_finalize(host, c, False)
    assert got["root_value"].tolist() == [0.5, -0.25, 2.0] and got["chosen_valid"].tolist() == [0, 0, 1, 0]
