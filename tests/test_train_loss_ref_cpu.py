"""CPU: the restatements tests/train_loss_ref.py against the reference's golden values (g11, g21), the float32 oracle and
literal records, and the coverage of the cases tests/train_loss_cases.py that tests/test_gpu_train_kernels.py runs."""
import struct

import numpy as np
import pytest
import torch

from tests import train_loss_cases as K
from tests.golden_utils import load, unpack_mask
from tests.train_loss_ref import (MOVE_DEST, MOVE_FROM, ON_BOARD, ref_loss, ref_pack, ref_representable, ref_unpack,
                                  run_oracle, value_bins_fp32, wide_class_factors)

ALL_SETTINGS = K.SETTINGS + K.EXTRA_SETTINGS


def run_ref(c, setting, grad_scale=1.0, weight_sum=None):
    ws = K.weight_sum_of(c["value"], setting[2]) if weight_sum is None else weight_sum
    return ref_loss(*(c[k] for k in K.INPUT_KEYS), alpha=setting[0], anti_draw=setting[1], draw_weight=setting[2],
                    weight_sum=ws, grad_scale=grad_scale)


@pytest.fixture(scope="module")
def edge():
    return K.edge_batch(K.EDGE_B)


@pytest.fixture(scope="module")
def edge_refs(edge):
    return [run_ref(edge, s) for s in ALL_SETTINGS]


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


# =========================================================================================================================
# the loss restatement
# =========================================================================================================================
def test_ref_loss_matches_the_reference_golden_values_and_gradients_g11():
    z = load("g11_loss.npz")
    heads = [torch.log_softmax(torch.from_numpy(z[k]), 1).numpy() for k in ("raw1", "raw2", "raw3")]
    for tag in ("a", "b"):
        alpha, anti, dw = (float(x) for x in z[f"{tag}_params"])
        ws = K.weight_sum_of(z["value"], dw)
        r = ref_loss(*heads, z["value_logits"], z["mask"], z["target"], z["value"], z["soft"], alpha=alpha,
                     anti_draw=anti, draw_weight=dw, weight_sum=ws)
        t = r["terms"]
        np.testing.assert_allclose((t[:, 0] * t[:, 1]).sum() / (ws + 1e-8), z[f"{tag}_policy_loss"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(t[:, 2].mean(), z[f"{tag}_bucket_loss"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(t[:, 3], z[f"{tag}_wdl_aux"], rtol=1e-5, atol=1e-6)
        for key in ("g1", "g2", "g3", "gv"):
            np.testing.assert_allclose(r[key], z[f"{tag}_{key}"], rtol=1e-5, atol=1e-7, err_msg=f"{tag} {key}")


def test_ref_loss_matches_the_reference_on_the_edge_batch_g21(edge, edge_refs):
    z = load("g21_loss_edges.npz")
    for k in K.INPUT_KEYS:                                # the fixture holds the inputs the tests rebuild
        want = unpack_mask(z["mask"], 220) if k == "mask" else z[k]
        got = edge[k] != 0 if k == "mask" else edge[k]
        assert np.array_equal(bits(got), bits(want)), k
    for tag, setting, r in zip(K.SETTING_TAGS, K.SETTINGS, edge_refs):
        assert tuple(np.float32(setting)) == tuple(z[f"{tag}_params"])
        t = r["terms"]
        np.testing.assert_allclose(t[:, 0], z[f"{tag}_kl"], rtol=1e-5, atol=1e-6, err_msg=tag)
        assert np.array_equal(t[:, 1].astype(np.float32), z[f"{tag}_weight"])
        np.testing.assert_allclose(t[:, 2], z[f"{tag}_ce_value"], rtol=1e-5, atol=1e-6, err_msg=tag)
        np.testing.assert_allclose(t[:, 3], z[f"{tag}_wdl_aux"], rtol=1e-5, atol=1e-6, err_msg=tag)
        for key in ("g1", "g2", "g3", "gv"):
            assert np.isfinite(z[f"{tag}_{key}"]).all()
            np.testing.assert_allclose(r[key], z[f"{tag}_{key}"], rtol=1e-5, atol=1e-7, err_msg=f"{tag} {key}")


@pytest.mark.parametrize("B", [64, 257])
def test_ref_loss_matches_the_fp32_oracle_on_every_class(B):
    """Base classes within the bounds of the kernel comparison; for the wide classes the distance is what sets the kernel's
    bound (tests/train_loss_ref.py::wide_class_factors): printed, and held to a sanity limit only."""
    c = K.edge_batch(B)
    for setting in ALL_SETTINGS:
        for gs in (1.0, 65536.0):
            want = run_ref(c, setting, gs)
            factors, measured = wide_class_factors(c, K.policy_class(c), K.value_class(c), want, setting, gs)
            for (name, cls), m in sorted(measured.items()):
                print(f"B={B} setting={setting} grad_scale={gs:g} {name:>3} {cls:>8}: oracle distance {m:8.3f} x bound, "
                      f"factor {factors[(name, cls)]:.2f}")
                assert m <= (1.0 if cls == "base" else 64.0), (name, cls, m)
            got = run_oracle(c, setting, gs)
            assert np.array_equal(got["terms"][:, 1], want["terms"][:, 1].astype(np.float32))


def test_hand_written_gradients_equal_autograd_at_every_scale_and_with_weight_sum_zero(edge):
    """ref_loss asserts hand == autograd to 1e-12 (per unit of grad_scale) on every call; the calls the other tests do not make."""
    for gs in K.GRAD_SCALES:
        run_ref(edge, K.SETTINGS[1], gs)
    c = K.draws_only_batch()
    assert K.weight_sum_of(c["value"], 0.0) == 0.0
    r = run_ref(c, (0.35, -0.15, 0.0), 3.0)
    assert (r["terms"][:, 1] == 0).all()
    for key in ("g1", "g2", "g3"):
        assert (r[key] == 0).all()
    assert np.isfinite(r["terms"]).all() and np.isfinite(r["gv"]).all() and np.abs(r["gv"]).max() > 0
    # the reference's policy loss of such a batch is 0
    t = r["terms"]
    assert (t[:, 0] * t[:, 1]).sum() / (0.0 + 1e-8) == 0.0


def test_draw_class_of_the_wdl_term_is_empty():
    centres = torch.linspace(-1.0, 1.0, steps=101)
    assert (centres[50:] > 1e-8).all() and (centres[:50] < -1e-8).all()


# =========================================================================================================================
# coverage of the loss cases
# =========================================================================================================================
def test_edge_batch_holds_every_class(edge, edge_refs):
    c, B = edge, K.EDGE_B
    legal = c["mask"] != 0
    count = lambda key, kind: int((c[key] == kind).sum())
    for s in K.HEAD_SCALES:
        assert int((c["head_scale"] == s).sum()) >= 3, s
    for kind in K.MASK_KINDS:
        assert count("mask_kind", kind) >= 3, kind
    for kind in K.VLOGIT_KINDS:
        assert count("vlogit_kind", kind) >= 3, kind
    for a in K.BORDER_ACTIONS:
        assert int(legal[:, a].sum()) >= 3, a
    nlegal = legal.sum(axis=1)
    on, off = list(K.ON_BOARD_ACTIONS), list(K.OFF_BOARD_ACTIONS)
    assert int((legal[:, on].all(axis=1)).sum()) >= 3                       # every on-board action
    assert int((nlegal == 1).sum()) >= 3 and int((nlegal == 0).sum()) >= 3
    assert int(((nlegal == 1) & legal[:, 216]).sum()) >= 3                  # only the auxiliary action
    assert int((legal[:, off].any(axis=1) & legal[:, on].any(axis=1)).sum()) >= 3
    assert int((legal[:, off].any(axis=1) & (nlegal == 1)).sum()) >= 3      # an off-board move alone
    # the -inf head cell: legal, with finite company (one row)
    i = int(c["inf_row"])
    assert i >= 0 and c["lp1"][i, 0] == -np.inf and legal[i, 0] and np.isfinite(c["lp1"][i, 35]) and legal[i, 35]
    # movement-only rows: every on-board (from, direction) pair carries target mass at least once
    mv = c["mask_kind"] == "movement"
    assert not legal[mv][:, :36].any() and not legal[mv][:, 180:].any()
    covered = ((c["target"][mv][:, 36:180] > 0) & legal[mv][:, 36:180]).any(axis=0)
    assert covered[ON_BOARD].all() and int(ON_BOARD.sum()) == 120 and not covered[~ON_BOARD].any()
    kinds = {"corner": 0, "edge": 0, "interior": 0}
    for m in np.flatnonzero(ON_BOARD):
        for cell in (MOVE_FROM[m], MOVE_DEST[m]):
            r, col = divmod(int(cell), 6)
            kinds[("interior", "edge", "corner")[(r in (0, 5)) + (col in (0, 5))]] += 1
    assert min(kinds.values()) > 0
    # targets
    t = c["target"]
    tsum, on_mask = t.sum(axis=1), (t * legal).sum(axis=1)
    lp, live = edge_refs[0]["lp"], edge_refs[0]["live"]
    assert int(((np.abs(tsum - 1) < 1e-5) & (np.abs(on_mask - 1) < 1e-5)).sum()) >= 3
    assert int((tsum == 0).sum()) >= 3
    assert int((np.abs(tsum - 0.5) < 1e-5).sum()) >= 3
    assert int(((t > 0) & live & (lp < -50)).any(axis=1).sum()) >= 3        # mass on an entry below the gate
    assert int(((t[:, off] > 0) & legal[:, off]).any(axis=1).sum()) >= 3    # mass on the off-board legal entry
    assert int(((t > 0) & ~legal).any(axis=1).sum()) >= 3                   # mass off the mask
    # values
    for v in K.VALUES:
        same = (c["value"] == np.float32(v)) & (np.signbit(c["value"]) == np.signbit(np.float32(v)))
        assert int(same.sum()) >= 3, v
    assert int((c["soft"] == np.float32(1.7)).sum()) >= 3 and int((c["soft"] == np.float32(-1.7)).sum()) >= 3
    assert int((np.abs(c["soft"]) <= 1).sum()) >= 3
    assert {s[0] for s in ALL_SETTINGS} == {0.0, 0.35, 1.0} and {s[1] for s in ALL_SETTINGS} == {0.0, 5e-10, -0.15, -1.5}
    # value logits: the classes as data
    v = c["vlogits"]
    assert int(((v == v[:, :1]).all(axis=1)).sum()) >= 3
    assert int(((v.max(axis=1) == 60000) & (v.min(axis=1) == -60000) & ((v == 0).sum(axis=1) == 99)).sum()) >= 3
    assert int((np.abs(v).max(axis=1) > 60).sum()) >= 3 + 16


def test_gate_margin_and_both_sides_of_the_gate():
    """No legal entry's float64 log-probability within 1e-3 of -50: the fp32 error of c - lse at |c| <= 250 is a few 1e-5,
    so both precisions put every entry on the same side and no entry needs to be left out of any comparison."""
    for B in K.BATCH_SIZES:
        c = K.edge_batch(B)
        r = run_ref(c, K.SETTINGS[0])
        lp = r["lp"][r["live"]]
        comb = np.stack([K._combined_np(c["lp1"][i], c["lp2"][i], c["lpm"][i]) for i in range(B)])
        assert np.abs(comb[r["live"]]).max(initial=0) <= 250
        assert lp.size == 0 or np.abs(lp + 50).min() > 1e-3, B
        if B >= 64:
            rows = (r["live"] & (r["lp"] < -50)).any(axis=1) & (r["live"] & (r["lp"] > -50)).any(axis=1)
            assert int(rows.sum()) >= 3


def test_value_bins_of_the_edge_batch(edge):
    """mixed exactly -1, 0, +1, on bin centres, and the (lo, hi) pairs, by the fp32 chain."""
    seen_pairs, seen_mixed, centres = {}, {}, 0
    for setting in ALL_SETTINGS:
        _, mixed, lo, hi, frac = value_bins_fp32(edge["value"], edge["soft"], setting[0], setting[1])
        for p in K.LO_HI_PAIRS:
            seen_pairs[p] = max(seen_pairs.get(p, 0), int(((lo == p[0]) & (hi == p[1])).sum()))
        for m in (-1.0, 0.0, 1.0):
            seen_mixed[m] = max(seen_mixed.get(m, 0), int((mixed == m).sum()))
        centres = max(centres, int(((frac == 0) & (lo > 0) & (lo < 100) & (lo != 50)).sum()))
        if setting[0] == 0.0:                             # the straddle of the two register slots, with weight on both
            assert int(((lo == 63) & (hi == 64) & (frac > 0.25) & (frac < 0.75)).sum()) >= 3
        if setting[0] == 1.0:
            assert int((mixed.abs() == 1).sum()) >= 6     # soft = +-1.7 clamps
    assert all(n >= 3 for n in seen_pairs.values()), seen_pairs
    assert all(n >= 3 for n in seen_mixed.values()), seen_mixed
    assert centres >= 3
    # literal points of the chain
    _, mixed, lo, hi, frac = value_bins_fp32([0.27, 0.29, 0.99, 1.0, -1.0, 0.0, 5.0], [0.0] * 7, 0.0, 0.0)
    assert list(zip(lo.tolist(), hi.tolist())) == [(63, 64), (64, 65), (99, 100), (100, 100), (0, 1), (50, 51), (100, 100)]
    assert frac[3] == 0 and frac[4] == 0 and frac[5] == 0 and abs(float(frac[0]) - 0.5) < 1e-4


def test_weight_sum_is_the_wrappers(edge):
    assert K.weight_sum_of(edge["value"], 1.0) == 64.0
    draws = int((np.abs(edge["value"]) < 1e-8).sum())
    assert draws >= 12
    np.testing.assert_allclose(K.weight_sum_of(edge["value"], 0.4), 64 - draws + 0.4 * draws, rtol=1e-6)


# =========================================================================================================================
# the codec restatement
# =========================================================================================================================
def test_ref_pack_on_three_literal_records():
    planes = np.zeros((3, 11, 6, 6), np.float32)
    legal = np.zeros((3, 220), np.uint8)
    policy = np.zeros((3, 220), np.float32)
    value, soft = np.array([1.0, -1.0, 0.5], np.float32), np.array([0.25, -0.5, 0.0], np.float32)
    # row 0: own on cells 0 and 35, opp on cell 1, own-marked cell 7, opp-marked cell 8, phase 3; actions 0 and 219
    planes[0, 0, 0, 0] = planes[0, 0, 5, 5] = planes[0, 1, 0, 1] = planes[0, 2, 1, 1] = planes[0, 3, 1, 2] = 1
    planes[0, 6] = 1
    legal[0, [0, 219]] = 1
    policy[0, 0], policy[0, 219] = 0.75, 0.25
    # row 1: nothing on the board, no phase plane, no legal action
    # row 2: phase 7, actions 31, 32 and 64 (word borders), the policy in ascending action order
    planes[2, 10] = 1
    legal[2, [31, 32, 64]] = (1, 2, 255)
    policy[2, 31], policy[2, 32], policy[2, 64] = 0.5, 0.125, 0.375
    rec, bad = ref_pack((planes, legal, policy, value, soft))
    assert bad == 0 and rec.shape == (3, 360) and rec.dtype == np.uint8
    want0 = struct.pack("<4Q7I72f2f4x", (1 | 1 << 35) | 3 << 36, 2, 1 << 7, 1 << 8, 1, 0, 0, 0, 0, 0, 1 << 27,
                        0.75, 0.25, *([0.0] * 70), 1.0, 0.25)
    want1 = struct.pack("<4Q7I72f2f4x", 0, 0, 0, 0, *([0] * 7), *([0.0] * 72), -1.0, -0.5)
    want2 = struct.pack("<4Q7I72f2f4x", 7 << 36, 0, 0, 0, 1 << 31, 1, 1, 0, 0, 0, 0, 0.5, 0.125, 0.375, *([0.0] * 69),
                        0.5, 0.0)
    for got, want in zip(rec, (want0, want1, want2)):
        assert len(want) == 360 and got.tobytes() == want
    back = ref_unpack(rec)
    legal01 = (legal != 0).astype(np.uint8)
    for got, want in zip(back, (planes, legal01, policy, value, soft)):
        assert np.array_equal(bits(got), bits(want))


def test_ref_codec_round_trip_and_counts():
    for n in K.CODEC_N:
        rows, labels = K.codec_rows(n, seed=n)
        ok = ref_representable(rows)
        assert np.array_equal(ok, np.isin(labels, ("ok", "minus_zero")))
        rec, bad = ref_pack(rows)
        assert bad == int((~ok).sum())
        back = ref_unpack(rec)
        exact = labels == "ok"
        planes, legal, policy, value, soft = rows
        for got, want in zip(back, (planes, (legal != 0).astype(np.uint8), policy, value, soft)):
            assert np.array_equal(bits(got[exact]), bits(want[exact]))
        # the -0.0 exception: equal as numbers, +0.0 where the row had -0.0 in a plane or off the legal set
        mz = labels == "minus_zero"
        for got, want in ((back[0], planes), (back[2], policy)):
            assert np.array_equal(got[mz], want[mz]) and not np.signbit(got[mz][want[mz] == 0]).any()
        if mz.any():
            off = legal[mz] == 0
            assert np.signbit(planes[mz]).any() and np.signbit(policy[mz][off]).any()
        assert np.array_equal(bits(back[2][mz][legal[mz] != 0]), bits(policy[mz][legal[mz] != 0]))
        assert not rec[ok][:, 356:].any()                 # the pad


def test_codec_rows_hold_every_class():
    rows, labels = K.codec_rows(257, seed=257)
    planes, legal, policy, value, soft = rows
    ok = np.isin(labels, ("ok", "minus_zero"))
    counts = (legal != 0).sum(axis=1)
    for k in K.LEGAL_COUNTS_OK:
        assert int((counts[ok] == k).sum()) >= 3, k
    for k in K.LEGAL_COUNTS_BAD:
        assert int((counts == k).sum()) >= 3, k
    for d in K.DEFECTS:
        assert int((labels == d).sum()) >= 3, d
    phase = np.where(planes[:, 4:].any(axis=(2, 3)), np.arange(1, 8), 0).max(axis=1)
    for ph in range(8):
        assert int((phase[labels == "ok"] == ph).sum()) >= 3, ph
    for a in K.BORDER_ACTIONS:
        assert int((legal[ok][:, a] != 0).sum()) >= 3, a
    for byte in (1, 2, 255):
        assert int((legal[ok] == byte).any(axis=1).sum()) >= 3
    pb = policy.view(np.uint32)
    for b in K.SPECIAL_POLICY_BITS:
        assert int(((pb == b) & (legal != 0))[ok].any(axis=1).sum()) >= 3, hex(b)
    assert int((value.view(np.uint32)[ok] == K.NAN_VALUE_BITS).sum()) >= 3
    assert int((soft.view(np.uint32)[ok] == K.NAN_SOFT_BITS).sum()) >= 3
    # small n: the first rows are representable, so every n of CODEC_N has rows whose bytes are compared
    for n in K.CODEC_N:
        assert np.isin(K.codec_rows(n, seed=n)[1][:min(n, 9)], ("ok",)).all()


def test_random_records_stay_within_72_mask_bits_and_overfull_ones_have_neighbours():
    for n in K.CODEC_N:
        rec = K.random_records(n, seed=n)
        assert K.mask_bits_of(rec).max() <= 72
    assert (K.mask_bits_of(K.random_records(257, seed=257)) == 72).sum() >= 3
    rec, rows = K.overfull_records()
    nbits = K.mask_bits_of(rec)
    for row, count in rows.items():
        assert nbits[row] == count and len(rec) - 1 - row >= 3 and 60 + 4 * 220 <= 3 * 360
    assert sorted(rows.values()) == [73, 220] and (np.delete(nbits, list(rows)) <= 72).all()
    # the restatement gives policy 0 past slot 71 and the record's own values before it
    planes, legal, policy, value, soft = ref_unpack(rec)
    for row in rows:
        acts = np.flatnonzero(legal[row])
        assert (policy[row, acts[72:]].view(np.uint32) == 0).all()
        assert np.array_equal(policy[row, acts[:72]].view(np.uint32), rec[row, 60:348].copy().view(np.uint32))
        # what an unpack without the bound would fetch for the slots past 71 lies inside the buffer and is not zero,
        # so the comparison in tests/test_gpu_train_kernels.py tells the two apart by value
        flat = rec.reshape(-1)
        last = row * 360 + 60 + 4 * (len(acts) - 1) + 4
        assert last <= flat.size
        beyond = flat[row * 360 + 60 + 4 * 72:last].copy().view(np.uint32)
        assert (beyond != 0).any()
