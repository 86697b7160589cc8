"""One case of tests/root_ops_cases.py through one build of the C ABI -- the gfx950 kernels (`_lib.lib()`, device memory) or
the host twin (`_lib.host_lib()`, host memory) -- held to the restatements of tests/root_ops_ref.py.  Shared by
tests/test_gpu_root_ops.py and tests/test_root_ops_ref_cpu.py, so that both builds answer to the same checks.

Every output is allocated with 8 guard rows on both sides and starts as a sentinel (0xA5 bytes for integers, a quiet NaN
with a marked payload for floats); the guards, and every element the contract leaves alone, must come back bit for bit."""
import functools

import numpy as np
import torch

from oracle import lz_oracle as O
from tests import root_ops_cases as K
from tests import root_ops_ref as Rf

GUARD = K.GUARD_ROWS
_NP = {torch.float32: np.float32, torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8}


def host_sentinel(shape, dtype):
    if dtype == np.float32:
        return np.full(shape, K.SENT_F32, np.int32).view(np.float32)
    return np.full(tuple(np.atleast_1d(shape)) + (np.dtype(dtype).itemsize,), K.SENT_BYTE, np.uint8).view(dtype)[..., 0]


def assert_bits(got, want, name):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (name, got.shape, want.shape)
    a, b = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        e = int(bad[0]) // got.dtype.itemsize
        raise AssertionError(f"{name}: {bad.size} bytes differ, first at element {e}: got {got.reshape(-1)[e]!r}, "
                             f"want {want.reshape(-1)[e]!r}")


class Build:
    """A library handle plus the memory it works on."""

    def __init__(self, L, dev):
        self.L, self.dev = L, dev
        self.lib = L.host_lib() if dev == "cpu" else L.lib()
        self.stream = L.stream_ptr(torch.device(dev))

    def dv(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def out(self, rows, tail=(), dtype=torch.float32, init=None):
        """A guarded output of `rows` rows: (whole tensor, the view the call gets).  `init` pre-loads the body."""
        whole = torch.from_numpy(host_sentinel((rows + 2 * GUARD,) + tuple(tail), _NP[dtype]).copy())
        if init is not None:
            whole[GUARD:GUARD + rows] = torch.from_numpy(np.ascontiguousarray(init))
        whole = whole.to(self.dev)
        return whole, whole[GUARD:]

    def take(self, whole, rows, name):
        """The body as numpy, after the guard rows on both sides were found untouched."""
        self.sync()
        a = whole.cpu().numpy()
        g = host_sentinel((GUARD,) + a.shape[1:], a.dtype.type)
        assert_bits(a[:GUARD], g, f"{name}: guard rows in front")
        assert_bits(a[GUARD + rows:], g, f"{name}: guard rows behind")
        return a[GUARD:GUARD + rows]

    def sync(self):
        if self.dev != "cpu":
            torch.cuda.synchronize()

    def ptr(self, t):
        return self.L.ptr(t)

    def ok(self, status, op):
        self.sync()
        self.L.check(status, op)


# =========================================================================================================================
# bounds that come from the float32 oracle's own distance to the float64 restatement
# =========================================================================================================================
@functools.lru_cache(maxsize=None)
def project_bound():
    """-> (bound, measured): the largest error of a float32 softmax (numpy throughout; for T = 217, 220 also the oracle's C
    restatement) against ref_project over every projection case; the kernel gets 4 x that, never more than 1e-6."""
    worst = 0.0
    for c in K.project_cases():
        want, _ = Rf.ref_project(c["lp1"], c["lp2"], c["lpmc"], c["mask"])
        worst = max(worst, float(np.abs(Rf.f32_project_probs(c["lp1"], c["lp2"], c["lpmc"], c["mask"]) - want).max()))
        if c["T"] in (217, 220):
            got, _ = O.project_policy(c["lp1"], c["lp2"], c["lpmc"], c["mask"], ad=c["T"] - 216)
            worst = max(worst, float(np.abs(got - want).max()))
    return min(4.0 * worst, Rf.PROJECT_CAP), worst


def slot_policy_oracle(c):
    """The float32 oracle's per-slot policy [R, M]: oracle.lz_oracle.root_finalize_from_visits scattering slot a of row r
    to column a of row r."""
    R, M = c["valid"].shape
    with np.errstate(all="ignore"):
        return O.root_finalize_from_visits(np.tile(np.arange(M), (R, 1)), c["codes"], c["valid"] != 0, c["visits"],
                                           c["value_sum"], np.arange(R), R, M, c["temps"])[0]


@functools.lru_cache(maxsize=None)
def finalize_bounds():
    """-> {1 / T as float32: (bound, measured)}: the float32 oracle against the float64 policy over every finalize case, one
    figure per exponent (powf's error grows with it); rows whose power overflows hold NaN and exact zeros and are not
    measured.  The kernel gets 4 x that, never more than 1e-5."""
    worst = {}
    for c in K.finalize_cases():
        inv_t = Rf.finalize_inv_t(c["temps"])
        got = slot_policy_oracle(c)
        for r in range(c["R"]):
            valid = c["valid"][r] != 0
            pol, over = Rf.ref_row_policy(c["visits"][r], valid, inv_t[r])
            if over or not valid.any():
                continue
            worst[float(inv_t[r])] = max(worst.get(float(inv_t[r]), 0.0), float(np.abs(got[r] - pol).max()))
    return {k: (min(4.0 * v, Rf.FINALIZE_CAP), v) for k, v in worst.items()}


# =========================================================================================================================
# lz_project_policy_logits_fast
# =========================================================================================================================
def run_project(bd, c):
    B, T = c["B"], c["T"]
    probs, probs_v = bd.out(B, (T,))
    ml, ml_v = bd.out(B, (T,))
    ins = [bd.dv(c[k]) for k in ("lp1", "lp2", "lpmc", "mask")]
    i64 = bd.L.i64
    bd.ok(bd.lib.lz_project_policy_logits_fast(*(bd.ptr(t) for t in ins), i64(B), i64(36), i64(144), i64(36), i64(T - 216),
                                               bd.ptr(probs_v), bd.ptr(ml_v), bd.stream), "project_policy_logits_fast")
    return bd.take(probs, B, "probs"), bd.take(ml, B, "masked_logits")


def check_project(bd, c):
    """-> the largest error of the probabilities."""
    probs, ml = run_project(bd, c)
    want_p, want_ml = Rf.ref_project(c["lp1"], c["lp2"], c["lpmc"], c["mask"])
    where = f"project T={c['T']} B={c['B']}"
    assert_bits(ml, want_ml, f"{where} masked_logits")
    assert np.isfinite(probs).all(), f"{where}: a non-finite probability (a NaN head of an illegal cell leaked?)"
    assert_bits(probs[want_p == 0], np.zeros(int((want_p == 0).sum()), np.float32), f"{where} probabilities outside the legal finite set")
    err = np.abs(probs.astype(np.float64) - want_p)
    bound, _ = project_bound()
    b, a = np.unravel_index(np.argmax(err), err.shape)
    print(f"{where}: worst |p - ref| {err.max():.3e} (bound {bound:.3e}) at row {b} ({c['cls'][b]}) column {a}")
    assert err.max() <= bound, f"{where}: {err.max():.3e} > {bound:.3e} at row {b} ({c['cls'][b]}) column {a}"
    return float(err.max())


# =========================================================================================================================
# lz_root_pack_rows / _plan / _fill
# =========================================================================================================================
def run_pack_rows(bd, c):
    B, T, cap = c["B"], c["T"], c["cap"]
    counts, counts_v = bd.out(B, (), torch.int32)
    li, li_v = bd.out(B, (cap,), torch.int32)
    pri, pri_v = bd.out(B, (cap,))
    codes, codes_v = bd.out(B, (cap, 4), torch.int32)
    ins = [bd.dv(c[k]) for k in ("mask", "probs", "meta")]
    i64 = bd.L.i64
    bd.ok(bd.lib.lz_root_pack_rows(*(bd.ptr(t) for t in ins), i64(B), i64(T), i64(cap), bd.ptr(counts_v), bd.ptr(li_v),
                                   bd.ptr(pri_v), bd.ptr(codes_v), bd.stream), "root_pack_rows")
    return (bd.take(counts, B, "counts"), bd.take(li, B, "legal_index"), bd.take(pri, B, "priors"),
            bd.take(codes, B, "codes"))


def check_pack_rows(bd, c):
    """-> (the four outputs, largest prior error as a multiple of its bound)."""
    got = run_pack_rows(bd, c)
    counts, li, pri, codes = got
    w_counts, w_li, w_pri, w_codes = Rf.ref_pack_rows(c["mask"], c["probs"], c["meta"], c["cap"])
    where = f"pack_rows B={c['B']} T={c['T']} cap={c['cap']} {c['pattern']}"
    assert_bits(counts, w_counts, f"{where} counts")
    assert_bits(li, w_li, f"{where} legal_index")
    assert_bits(codes, w_codes, f"{where} codes")
    assert_bits(pri[w_li < 0], np.zeros(int((w_li < 0).sum()), np.float32), f"{where} priors padding")
    sums = Rf.pack_row_sums(c["mask"], c["probs"])
    worst = 0.0
    for b in range(c["B"]):
        n = int(w_counts[b])
        if n == 0:
            continue
        if sums[b] < 1e-8:                                  # under the clamp the denominator is the constant: exact
            idx = w_li[b, :n]
            assert_bits(pri[b, :n], c["probs"][b, idx] / Rf.F32_TINY, f"{where} row {b} (clamp)")
            continue
        rel = np.abs(pri[b, :n].astype(np.float64) - w_pri[b, :n]) / w_pri[b, :n]
        ratio = float(rel.max() / Rf.priors_bound(n))
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{where} row {b} ({c['cls'][b]}, count {n}): prior off by {rel.max():.3e}, {ratio:.2f} x the bound"
    print(f"{where}: worst prior error {worst:.3f} x bound")
    return got, worst


def run_pack_plan(bd, counts):
    B = len(counts)
    rank, rank_v = bd.out(B, (), torch.int32)
    off, off_v = bd.out(B, (), torch.int64)
    sizes, sizes_v = bd.out(3, (), torch.int64)
    bd.ok(bd.lib.lz_root_pack_plan(bd.ptr(bd.dv(counts)), bd.L.i64(B), bd.ptr(rank_v), bd.ptr(off_v), bd.ptr(sizes_v),
                                   bd.stream), "root_pack_plan")
    return bd.take(rank, B, "rank"), bd.take(off, B, "child_off"), bd.take(sizes, 3, "sizes")


def check_pack_plan(bd, counts, where):
    got = run_pack_plan(bd, counts)
    for g, w, name in zip(got, Rf.ref_pack_plan(counts), ("rank", "child_off", "sizes")):
        assert_bits(g, w, f"pack_plan {where} {name}")
    return got


def run_pack_fill(bd, counts, li, pri, codes, rank, off, R, M, N):
    """Empty outputs (R = 0 / N = 0) are passed as NULL."""
    B, cap = li.shape
    spec = dict(terminal_mask=(B, (), torch.uint8), valid_root_indices=(R, (), torch.int64), counts=(R, (), torch.int64),
                valid_mask=(R, (M,), torch.uint8), legal_index_mat=(R, (M,), torch.int64), priors_mat=(R, (M,), torch.float32),
                action_code_mat=(R, (M, 4), torch.int32), pack_flat_idx=(N, (), torch.int64),
                action_codes_all=(N, (4,), torch.int32), parent_indices_all=(N, (), torch.int64))
    outs = {k: bd.out(*v) for k, v in spec.items()}
    args = [None if spec[k][0] * int(np.prod(spec[k][1])) == 0 else outs[k][1] for k in Rf.PACK_FILL_OUT]
    ins = [bd.dv(a) for a in (counts, li, pri, codes, rank, off)]
    i64 = bd.L.i64
    bd.ok(bd.lib.lz_root_pack_fill(*(bd.ptr(t) for t in ins), i64(B), i64(cap), i64(R), i64(M), i64(N),
                                   *(bd.ptr(t) for t in args), bd.stream), "root_pack_fill")
    return {k: bd.take(outs[k][0], spec[k][0], k) for k in Rf.PACK_FILL_OUT}


def check_pack_chain(bd, c):
    """rows -> plan -> fill on one case: every stage against the restatement of that stage on the same inputs; the fill
    copies, so all ten outputs are bit for bit."""
    (counts, li, pri, codes), worst = check_pack_rows(bd, c)
    where = f"B={c['B']} T={c['T']} cap={c['cap']} {c['pattern']}"
    rank, off, sizes = check_pack_plan(bd, counts, where)
    R, M, N = (int(x) for x in sizes)
    got = run_pack_fill(bd, counts, li, pri, codes, rank, off, R, M, N)
    want = Rf.ref_pack_fill(counts, li, pri, codes, rank, off, R, M, N)
    for k in Rf.PACK_FILL_OUT:
        assert_bits(got[k], want[k], f"pack_fill {where} {k}")
    return got, worst


# =========================================================================================================================
# lz_root_finalize_from_visits
# =========================================================================================================================
FIN_OUT = ("policy", "chosen_index", "chosen_codes", "chosen_valid", "root_value")


def run_finalize(bd, c, sampled):
    R, M, B, T = c["R"], c["M"], c["B"], c["T"]
    spec = dict(policy=(B, (T,), torch.float32), chosen_index=(B, (), torch.int64), chosen_codes=(B, (4,), torch.int32),
                chosen_valid=(B, (), torch.uint8), root_value=(R, (), torch.float32))
    outs = {k: bd.out(*v) for k, v in spec.items()}
    ins = [bd.dv(c[k]) for k in ("lidx", "codes", "valid", "visits", "value_sum", "roots")]
    temps, uni = bd.dv(c["temps"]), (bd.dv(c["uniforms"]) if sampled else None)
    i64 = bd.L.i64
    bd.ok(bd.lib.lz_root_finalize_from_visits(*(bd.ptr(t) for t in ins), i64(R), i64(M), i64(B), i64(T), bd.ptr(temps),
                                              bd.ptr(uni), *(bd.ptr(outs[k][1]) for k in FIN_OUT), bd.stream),
          "root_finalize_from_visits")
    return {k: bd.take(outs[k][0], spec[k][0], k) for k in FIN_OUT}


def column_bounds(c, want):
    """[B, T] bound of policy_dense: a column that n valid slots of the row scatter to carries n slot errors, and the n - 1
    float32 additions of the scatter round once each (relative to a sum that is at most the column's value)."""
    bounds = finalize_bounds()
    inv_t = Rf.finalize_inv_t(c["temps"])
    out = np.zeros((c["B"], c["T"]))
    for r in range(c["R"]):
        cols = c["lidx"][r][(c["valid"][r] != 0) & (c["lidx"][r] >= 0) & (c["lidx"][r] < c["T"])]
        n = np.bincount(cols, minlength=c["T"])
        b = int(c["roots"][r])
        slot = bounds.get(float(inv_t[r]), (0.0, 0.0))[0]
        out[b] = np.maximum(n, 1) * slot + np.maximum(n - 1, 0) * Rf.F32_EPS * np.abs(np.nan_to_num(want["policy"][b]))
    return out


def check_finalize(bd, c, sampled):
    """-> (outputs, largest policy error per 1 / T, largest root_value error as a multiple of its bound)."""
    got = run_finalize(bd, c, sampled)
    want = Rf.ref_finalize(c["lidx"], c["codes"], c["valid"], c["visits"], c["value_sum"], c["roots"], c["B"], c["T"],
                           c["temps"], c["uniforms"] if sampled else None)
    where = f"finalize M={c['M']} R={c['R']} {'sampled' if sampled else 'argmax'}"
    row_of = {int(b): r for r, b in enumerate(c["roots"])}
    fails = []                                              # every row is looked at, so that a failure names all its classes
    for b in range(c["B"]):
        r = row_of.get(b, -1)
        kind = "no row" if r < 0 else ("overflow" if want["overflow"][r] else str(c["cls"][r]))
        for name in ("chosen_index", "chosen_codes", "chosen_valid"):
            if not np.array_equal(got[name][b], want[name][b]):
                fails.append((kind, f"root {b} row {r} ({c['cls'][r] if r >= 0 else None}, T={c['temps'][r] if r >= 0 else None}, "
                                    f"{c['kinds'][r] if r >= 0 else None}): {name} {got[name][b]!r}, want {want[name][b]!r} "
                                    f"(slot {want['pick'][r] if r >= 0 else None})"))
    assert not fails, f"{where}: {len(fails)} picks differ, classes {sorted({k for k, _ in fails})}; first: {fails[0][1]}"
    gp, wp = got["policy"].astype(np.float64), want["policy"]
    assert np.array_equal(np.isnan(gp), np.isnan(wp)), f"{where}: NaN entries of policy_dense differ from the reference's"
    err = np.where(np.isnan(wp), 0.0, np.abs(gp - wp))
    bound = column_bounds(c, want)
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (f"{where}: {len(bad)} policy entries past the bound, first at root {bad[0][0]} column {bad[0][1]}: "
                           f"got {gp[tuple(bad[0])]!r}, want {wp[tuple(bad[0])]!r}, bound {bound[tuple(bad[0])]:.3e}")
    inv_t = Rf.finalize_inv_t(c["temps"])
    worst = {}
    for r in range(c["R"]):
        worst[float(inv_t[r])] = max(worst.get(float(inv_t[r]), 0.0), float(err[int(c["roots"][r])].max()))
    rv = np.abs(got["root_value"].astype(np.float64) - want["root_value"])
    over = np.flatnonzero(~(rv <= want["root_value_bound"]))               # a sentinel NaN left in place counts
    assert over.size == 0, (f"{where}: root_value of {over.size} rows, classes {sorted(set(c['cls'][over]))}; row {over[0]}: got "
                            f"{got['root_value'][over[0]]!r}, want {want['root_value'][over[0]]!r}, bound "
                            f"{want['root_value_bound'][over[0]]:.3e}")
    with np.errstate(invalid="ignore", divide="ignore"):
        rv_ratio = float(np.nan_to_num(rv / want["root_value_bound"]).max())
    print(f"{where}: policy error per 1/T {({k: f'{v:.2e}' for k, v in worst.items()})}, root_value {rv_ratio:.3f} x bound")
    return got, worst, rv_ratio


# =========================================================================================================================
# lz_finalize_trajectory_inplace
# =========================================================================================================================
def run_traj(bd, c):
    F, G, S = c["F"], c["G"], c["S"]
    vt, vt_v = bd.out(S)
    st, st_v = bd.out(S)
    keep, keep_v = bd.out(F, (), torch.uint8)
    fc, fc_v = bd.out(F, (), torch.int64)
    co, co_v = bd.out(3, (), torch.int64, init=c["counts_in"])
    ins = {k: bd.dv(c[k]) for k in ("signs", "step_index", "step_counts", "slots", "result", "softv")}
    i64 = bd.L.i64
    bd.ok(bd.lib.lz_finalize_trajectory_inplace(
        bd.ptr(vt_v), bd.ptr(st_v), bd.ptr(ins["signs"]), bd.ptr(ins["step_index"]), bd.ptr(ins["step_counts"]), i64(G),
        i64(c["max_steps"]), bd.ptr(ins["slots"]), bd.ptr(ins["result"]), bd.ptr(ins["softv"]), i64(F), bd.ptr(keep_v),
        bd.ptr(fc_v), bd.ptr(co_v), bd.stream), "finalize_trajectory_inplace")
    return (bd.take(vt, S, "value_targets"), bd.take(st, S, "soft_value_targets"), bd.take(keep, F, "keep"),
            bd.take(fc, F, "final_counts"), bd.take(co, 3, "counts_out"))


def check_traj(bd, c):
    got = run_traj(bd, c)
    sent = host_sentinel((c["S"],), np.float32)
    want = Rf.ref_finalize_trajectory(sent, sent, c["signs"], c["step_index"], c["step_counts"], c["max_steps"], c["slots"],
                                      c["result"], c["softv"], c["counts_in"])
    where = f"trajectory F={c['F']} G={c['G']} max_steps={c['max_steps']}"
    for g, w, name in zip(got, want, ("value_targets", "soft_value_targets", "keep", "final_counts", "counts_out")):
        assert_bits(g, w, f"{where} {name}")              # multiplications by +-1: exact, -0.0 included; untouched rows too
    return got
