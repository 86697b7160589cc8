"""Restatement of csrc/lz_valid.hip and csrc/lz_valid.h for the tests (numpy on the CPU).

`ref_rows`: the twelve row columns in float64 and the four integers of `cls`.  Like tests/train_loss_ref.py, only the
scalar chain that assigns the value bins is taken in float32 (it is the specification of the bin assignment, not
rounding); the combined logits, the masked log-sum-exp with its conventions (no legal entry or a non-finite lse => 0,
non-finite log-probabilities => -50), CE, both entropies, the value softmax and its expectation are float64.  The
classification takes float32 inputs where the kernel does: the calibration bin is a function of a float32 v_hat
(`calib_bin`), policy_valid of the float32 sum of the target.

`ref_reduce`: the sums into acc f64[18,14] (+ zsum f64[18]) with the association of csrc/lz_valid.h, exact in double:
lane l adds its rows l, l + 64, ... in order from 0.0, the 64 partials are combined by the butterfly
v[l] = v[l] + v[l ^ d], d = 32 .. 1, and the total is added to acc."""
import numpy as np

from tests.train_loss_ref import BINS, MOVE_DEST, MOVE_FROM, ON_BOARD, TOTAL, value_bins_fp32

ROW_COLS = 12
GROUPS = 18
ACC_COLS = 14
KL, CE, H_TARGET, H_NET, TOP1, P_TOP, BUCKET_CE, V_HAT, SQ_ERR, SIGN_OK, DECISIVE, POLICY_VALID = range(12)
CENTRES = -1.0 + np.arange(BINS) / 50.0


def combined(lp1, lp2, lpm):
    l1, l2, l3 = (np.asarray(a, np.float32).astype(np.float64).reshape(-1, 36) for a in (lp1, lp2, lpm))
    with np.errstate(invalid="ignore"):
        moves = l2[:, MOVE_FROM] + l1[:, np.where(ON_BOARD, MOVE_DEST, 0)]
    moves = np.where(ON_BOARD[None, :], moves, -np.inf)
    return np.concatenate([l1, moves, l3, np.zeros((len(l1), 4))], axis=1)


def argmax_legal(x, legal):
    """Lowest index among the legal entries with the largest key (NaN as -inf); -1 without a legal entry."""
    x = np.asarray(x, np.float64)
    idx = np.flatnonzero(legal)
    if idx.size == 0:
        return -1
    key = np.where(np.isnan(x[idx]), -np.inf, x[idx])
    return int(idx[np.flatnonzero(key == key.max())[0]])


def calib_bin(v_hat):
    """min(9, max(0, (int)floorf((v_hat + 1) * 5))) in float32; NaN -> 0."""
    v = np.asarray(v_hat, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.floor((v + np.float32(1.0)) * np.float32(5.0))
    return np.where(u >= 9, 9, np.where(u >= 0, u, 0)).astype(np.int32)     # NaN fails both comparisons


def phase_of(planes):
    cell0 = np.asarray(planes, np.float32).reshape(-1, 11, 36)[:, 4:, 0]
    nz = cell0 != 0                                                          # NaN is not zero
    return np.where(nz.any(axis=1), nz.argmax(axis=1), -1).astype(np.int32)


def twohot(value, soft, alpha):
    _, _, lo, hi, frac = value_bins_fp32(value, soft, alpha, 0.0)
    lo, hi, frac = lo.numpy(), hi.numpy(), frac.numpy().astype(np.float64)
    t = np.zeros((len(lo), BINS))
    np.add.at(t, (np.arange(len(lo)), lo), 1.0 - frac)
    np.add.at(t, (np.arange(len(lo)), hi), frac)
    return t


def ref_rows(lp1, lp2, lpm, vlogits, legal, target, value, soft, planes, *, alpha):
    """-> rows float64[B,12], cls int32[B,4], v_hat64 (the expectation before any float32 rounding)."""
    comb = combined(lp1, lp2, lpm)
    B = len(comb)
    legal = np.asarray(legal).reshape(B, TOTAL) != 0
    t32 = np.asarray(target, np.float32).reshape(B, TOTAL)
    t = t32.astype(np.float64)
    z = np.asarray(value, np.float32).reshape(B).astype(np.float64)
    vl = np.asarray(vlogits, np.float32).astype(np.float64).reshape(B, BINS)
    rows = np.zeros((B, ROW_COLS))
    cls = np.zeros((B, 4), np.int32)
    tv = twohot(value, soft, alpha)
    with np.errstate(all="ignore"):
        for s in range(B):
            lg, c = legal[s], comb[s]
            live = lg & (c > -np.inf)                                        # NaN is not live either
            any_legal = bool(lg.any())
            if live.any():
                mx = np.max(c[live])
                lse = mx + np.log(np.sum(np.exp(c[live] - mx)))
            else:
                lse = -np.inf
            lse_ok = any_legal and np.isfinite(lse)
            if not lse_ok:
                lse = 0.0
            lp = np.where(lg, c - lse, 0.0)
            lp = np.where(np.isfinite(lp), lp, -50.0)
            lp = np.maximum(lp, -50.0)
            ce = -np.sum(t[s] * lp)
            ent = -np.sum(t[s] * np.log(np.maximum(t[s], 1e-8)))
            p = np.where(live & lse_ok, np.exp(np.where(live, c, 0.0) - lse), 0.0)
            h_net = -np.sum(np.where(p > 0, p * (np.where(live, c, 0.0) - lse), 0.0))
            net_top = argmax_legal(c, lg)
            tgt_arg = argmax_legal(t[s], lg)
            valid = bool(np.float32(t32[s].sum(dtype=np.float64)) > np.float32(1e-8)) and any_legal
            if valid:
                rows[s, :6] = (ce - ent, ce, ent, h_net, 1.0 if net_top == tgt_arg else 0.0, p[tgt_arg])
            m = vl[s].max()
            e = np.exp(vl[s] - m)
            sm = e / e.sum()
            vlog = vl[s] - (m + np.log(e.sum()))
            rows[s, BUCKET_CE] = -np.sum(tv[s] * vlog)
            v_hat = np.sum(sm * CENTRES)
            rows[s, V_HAT] = v_hat
            rows[s, SQ_ERR] = (v_hat - z[s]) ** 2
            hard_draw = abs(z[s]) < 1e-8
            rows[s, SIGN_OK] = 1.0 if (not hard_draw and v_hat * z[s] > 0) else 0.0
            rows[s, DECISIVE] = 0.0 if hard_draw else 1.0
            rows[s, POLICY_VALID] = 1.0 if valid else 0.0
            cls[s] = (0, 0, net_top, tgt_arg if valid else -1)
    cls[:, 0] = phase_of(planes)
    cls[:, 1] = calib_bin(rows[:, V_HAT].astype(np.float32))
    return rows, cls


# ---- the reduction, exact ------------------------------------------------------------------------------------------------------
def in_group(g, phase, bin_):
    if g == 0:
        return np.ones(len(phase), bool)
    if g <= 7:
        return phase == g - 1
    return bin_ == g - 8


def butterfly64(v):
    v = np.array(v, np.float64)
    d = 32
    while d >= 1:
        v = v + v[np.arange(64) ^ d]
        d >>= 1
    return v


def ref_reduce(rows, cls, value=None, acc=None, zsum=None):
    """acc f64[18,14] (+= in place when given), zsum f64[18]: one call of lz_valid_reduce."""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, ROW_COLS)
    cls = np.ascontiguousarray(cls, np.int32).reshape(-1, 4)
    B = len(rows)
    acc = np.zeros((GROUPS, ACC_COLS)) if acc is None else acc
    zsum = np.zeros(GROUPS) if zsum is None else zsum
    if B == 0:
        return acc, zsum
    z = None if value is None else np.ascontiguousarray(value, np.float32).reshape(B).astype(np.float64)
    counted = np.isfinite(rows).all(axis=1)
    r64 = rows.astype(np.float64)
    with np.errstate(all="ignore"):
        for g in range(GROUPS):
            member = in_group(g, cls[:, 0], cls[:, 1])
            part = np.zeros((64, ACC_COLS + 1))
            for lane in range(64):
                for i in range(lane, B, 64):
                    if not member[i]:
                        continue
                    if counted[i]:
                        part[lane, :ROW_COLS] = part[lane, :ROW_COLS] + r64[i]
                        part[lane, ROW_COLS] += 1.0
                        if z is not None:
                            part[lane, ACC_COLS] = part[lane, ACC_COLS] + z[i]
                    else:
                        part[lane, ROW_COLS + 1] += 1.0
            total = np.array([butterfly64(part[:, c])[0] for c in range(ACC_COLS + 1)])
            acc[g] = acc[g] + total[:ACC_COLS]
            if z is not None:
                zsum[g] = zsum[g] + total[ACC_COLS]
    return acc, zsum
