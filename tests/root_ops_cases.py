"""Inputs of tests/test_gpu_root_ops.py (numpy only, seeded): what the root operators of csrc/lz_ops.hip are given, built
from named classes.  Every builder tags its rows with the class they belong to; tests/test_root_ops_ref_cpu.py builds the
same inputs on the host alone and counts the classes there, so that a GPU run never finds a case missing."""
import functools
import itertools

import numpy as np

from tests.root_ops_ref import finalize_inv_t, ref_logits, ref_sampled_pick

GUARD_ROWS = 8
SENT_F32 = 0x7FC12345                                     # a quiet NaN with a marked payload: "nobody wrote here"
SENT_BYTE = 0xA5
NINF = np.float32(-np.inf)


def heads(r, B):
    """Three log-softmax heads float32[B, 36], as the network hands them over."""
    out = []
    for _ in range(3):
        x = 2.0 * r.standard_normal((B, 36))
        x = x - x.max(1, keepdims=True)
        out.append((x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32))
    return out


# =========================================================================================================================
# lz_project_policy_logits_fast
# =========================================================================================================================
PROJECT_T = (216, 217, 220, 256)
PROJECT_B = (1, 3, 4, 5, 257)
PROJECT_CLASSES = ("random", "none", "one_placement", "one_movement", "one_selection", "one_auxiliary", "offboard_only",
                   "all_ninf", "one_ninf_head", "underflow", "board_full", "auxiliary_only", "nan_illegal")
OFFBOARD = (36 + 4 * 0 + 0, 36 + 4 * 0 + 2, 36 + 4 * 35 + 1, 36 + 4 * 35 + 3, 36 + 4 * 17 + 3, 36 + 4 * 18 + 2)


@functools.lru_cache(maxsize=None)
def project_case(T, B, seed=0):
    """-> dict(lp1, lp2, lpmc float32[B, 36], mask uint8[B, T], cls [B] of PROJECT_CLASSES).  The classes rotate over the
    rows, starting at a different one for every (T, B), so that the small batches reach all of them between them."""
    r = np.random.default_rng([seed, T, B, 4])
    lp1, lp2, lpmc = heads(r, B)
    mask = (r.random((B, T)) < 0.12).astype(np.uint8)
    classes = [c for c in PROJECT_CLASSES if T > 216 or c not in ("one_auxiliary", "auxiliary_only")]
    start = (PROJECT_T.index(T) * 5 + PROJECT_B.index(B) * 3) % len(classes) if B < 100 else 0
    cls = []
    for b in range(B):
        c = classes[(start + b) % len(classes)]
        cls.append(c)
        cell = int(r.integers(0, 36))
        if c == "random":
            mask[b, int(r.integers(0, T))] = 1                        # at least one
        elif c == "none":
            mask[b] = 0
        elif c.startswith("one_") and c != "one_ninf_head":
            mask[b] = 0
            a = {"one_placement": cell, "one_movement": 36 + 4 * 14 + int(r.integers(0, 4)), "one_selection": 180 + cell,
                 "one_auxiliary": 216 + int(r.integers(0, T - 216)) if T > 216 else 0}[c]
            mask[b, a] = 1
        elif c == "offboard_only":                                    # legal by the mask, -inf by the board's edge
            mask[b] = 0
            mask[b, list(OFFBOARD[:2 + b % 4])] = 1
        elif c == "all_ninf":                                         # every legal logit is -inf: masked_logits 0 there
            mask[b] = 0
            cells = r.choice(36, 3, replace=False)
            lp1[b, cells[0]] = NINF
            lpmc[b, cells[1]] = NINF
            lp2[b, 14] = NINF
            mask[b, [cells[0], 180 + cells[1], 36 + 4 * 14 + 3, OFFBOARD[0]]] = 1
        elif c == "one_ninf_head":                                    # one -inf head among finite ones
            lp1[b, cell] = NINF
            mask[b, cell] = 1
            mask[b, 180 + (cell + 1) % 36] = 1
        elif c == "underflow":                                        # exp(-1e4 - max) is 0
            cells = r.choice(36, 4, replace=False)
            lp1[b, cells[:2]] = np.float32(-1e4)
            lpmc[b, cells[2]] = np.float32(-1e4) if b % 2 else lpmc[b, cells[2]]
            mask[b, [cells[0], cells[1], 180 + cells[2]]] = 1
            if b % 2 == 0:                                            # ... and a row whose legal heads are ALL down there
                mask[b] = 0
                lp1[b, cells[:3]] = np.float32([-1e4, -1e4 - 1.5, -1e4 + 0.25])
                mask[b, cells[:3]] = 1
        elif c == "board_full":
            mask[b, :216] = 1
        elif c == "auxiliary_only":
            mask[b] = 0
            mask[b, 216 + r.choice(T - 216, min(2, T - 216), replace=False)] = 1
        elif c == "nan_illegal":                                      # a NaN head reaches illegal entries only
            lp1[b, cell] = np.float32(np.nan)
            lp2[b, (cell + 7) % 36] = np.float32(np.nan)
            lpmc[b, (cell + 11) % 36] = np.float32(np.nan)
            mask[b, np.isnan(ref_logits(lp1[b:b + 1], lp2[b:b + 1], lpmc[b:b + 1], T)[0])] = 0
            mask[b, 180 + (cell + 12) % 36] = 1
    return dict(T=T, B=B, lp1=lp1, lp2=lp2, lpmc=lpmc, mask=mask, cls=np.array(cls))


def project_cases():
    return [project_case(T, B) for T in PROJECT_T for B in PROJECT_B]


# =========================================================================================================================
# lz_root_pack_rows / _plan / _fill
# =========================================================================================================================
PLAN_B = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
PLAN_THREADS = 1024                                       # the plan is one workgroup of this size
PACK_B = (1, 5, 257)
PACK_T = (220, 217, 64, 65)
PACK_CAPS = (80, 72)
PACK_PATTERNS = ("mixed", "all_terminal", "ends_terminal")
PACK_CLASSES = ("count_0", "count_1", "count_64", "count_65", "count_cap", "clamp", "zeros", "negative_meta", "random")


@functools.lru_cache(maxsize=None)
def plan_case(B, pattern, seed=0):
    """Counts only.  "runs": terminal rows in runs that cross a boundary between two threads' chunks and between two
    waves' chunks of the plan (chunk = ceil(B / 1024) rows)."""
    r = np.random.default_rng([seed, B, PACK_PATTERNS.index(pattern) if pattern in PACK_PATTERNS else 7])
    counts = r.choice(np.array([1, 2, 64, 65, 72, 80, 17], np.int32), B)
    counts[r.random(B) < 0.2] = 0
    per = -(-B // PLAN_THREADS)
    runs = []
    if pattern == "all_terminal":
        counts[:] = 0
    elif pattern == "ends_terminal":
        counts[0] = counts[-1] = 0
        if B > 2:
            counts[1] = 3
    elif pattern == "runs":
        for edge in (per * 5, per * 64, per * 64 * 7 + per, B - 1):
            lo, hi = max(edge - 2, 0), min(edge + 2, B)
            if lo < hi:
                counts[lo:hi] = 0
                runs.append((lo, hi))
        if B > 4:
            counts[B // 2] = 80                                       # something lives between the runs
    return dict(B=B, pattern=pattern, counts=counts.astype(np.int32), per=per, runs=runs)


def plan_cases():
    return [plan_case(B, p) for B in PLAN_B for p in ("mixed", "all_terminal", "ends_terminal", "runs")]


@functools.lru_cache(maxsize=None)
def pack_case(B, T, cap, pattern, seed=0):
    """-> dict(mask uint8[B, T], probs float32[B, T], meta int32[B, T, 4], cap, cls [B]).  No row exceeds cap."""
    r = np.random.default_rng([seed, B, T, cap, PACK_PATTERNS.index(pattern)])
    mask = np.zeros((B, T), np.uint8)
    probs = r.random((B, T)).astype(np.float32)
    probs /= probs.sum(1, keepdims=True, dtype=np.float32)
    meta = r.integers(0, 36, (B, T, 4)).astype(np.int32)
    classes = [c for c in PACK_CLASSES if not (c == "count_cap" and T < cap) and not (c == "count_65" and T < 65)]
    start = (PACK_B.index(B) * 2 + PACK_T.index(T) * 3 + PACK_CAPS.index(cap)) % len(classes)
    cls = []
    for b in range(B):
        c = classes[(start + b) % len(classes)]
        n = {"count_0": 0, "count_1": 1, "count_64": 64, "count_65": 65, "count_cap": cap}.get(c)
        if n is None:
            n = int(r.integers(2, min(T, cap) + 1))
        if pattern == "all_terminal" or (pattern == "ends_terminal" and b in (0, B - 1)):
            c, n = "count_0", 0
        mask[b, r.choice(T, n, replace=False)] = 1 + int(r.integers(0, 255)) * (b % 3 == 0)   # any non-zero byte is legal
        if c == "clamp":                                              # the legal probabilities sum below 1e-8
            probs[b] = (probs[b] * np.float32(1e-9)).astype(np.float32)
        elif c == "zeros":
            probs[b] = 0
        elif c == "negative_meta":
            meta[b] = -meta[b] - 1
        cls.append(c)
    return dict(B=B, T=T, cap=cap, pattern=pattern, mask=mask, probs=probs, meta=meta, cls=np.array(cls))


def pack_cases():
    out = [pack_case(B, T, cap, "mixed") for B in PACK_B for T in PACK_T for cap in PACK_CAPS]
    out += [pack_case(B, 220, 80, p) for B in PACK_B for p in ("all_terminal", "ends_terminal")]
    return out


# =========================================================================================================================
# lz_root_finalize_from_visits
# =========================================================================================================================
FIN_M = (1, 2, 35, 64, 65, 128, 129, 256)
FIN_R = (1, 4, 5, 130)
FIN_T = 220
FIN_TEMPS = (1.0, 0.5, 0.1, 1e-6, 0.0, -1.0)
FIN_CLASSES = ("random", "dominant_8192", "dominant_65536", "all_zero", "single_last", "no_valid", "dup_cols",
               "col_T_and_neg", "mixed_value", "tiny_visits")
PICK_KINDS = ("first_live", "last_live", "group", "after_invalid_run", "u_zero", "u_top")
MIN_WIDTH = 1e-3                                          # of the row's total: the narrowest interval a sampled case aims at
DENORMAL_BAND = (1e-50, 1e-30)                            # weights a float32 exp may or may not flush: no case has one


@functools.lru_cache(maxsize=None)
def finalize_case(M, R, seed=0):
    """-> the inputs of one call plus, per row, its class, its temperature, the kind of sampled pick it aims at, the
    target slot and the uniform that aims at it (the midpoint of the slot's float64 CDF interval, 0, or the float32 below
    1).  `uniforms` may be passed or left out: the same rows then test the argmax."""
    r = np.random.default_rng([seed, M, R, 23])
    steps = r.integers(1, 4, R)
    steps[R // 2] = 2
    roots = np.cumsum(steps).astype(np.int64)                         # ascending, with gaps, never the identity
    B = int(roots[-1]) + 3
    T = FIN_T
    lidx = np.stack([r.choice(T, M, replace=(M > T)) for _ in range(R)]).astype(np.int64)
    codes = r.integers(-1, 36, (R, M, 4)).astype(np.int32)
    valid = (r.random((R, M)) < 0.7).astype(np.uint8)
    visits = r.integers(0, 21, (R, M)).astype(np.float32)
    value_sum = (visits * r.uniform(-1, 1, (R, M))).astype(np.float32)
    shift = (FIN_M.index(M) * 3 + FIN_R.index(R)) % len(FIN_CLASSES)
    temps = np.array([FIN_TEMPS[(r_ + shift // 2 + (r_ // 6)) % 6] for r_ in range(R)], np.float32)
    no_valid_rows = {0, R // 2, R - 1} if R >= 4 else ({0} if (M + R) % 2 else set())
    cls, kinds, target = [], [], np.full(R, -1, np.int64)
    for i in range(R):
        c = FIN_CLASSES[(shift + i) % len(FIN_CLASSES)]
        if i in no_valid_rows:
            c = "no_valid"
        elif c == "no_valid":
            c = "random"
        far = int(r.integers(1, M)) if M > 1 else 0                   # a slot away from slot 0
        if c in ("dominant_8192", "dominant_65536"):
            big = 8192 if c == "dominant_8192" else 65536
            visits[i] = np.where(r.random(M) < 0.5, 0, r.integers(big // 64, big // 64 + 41, M)).astype(np.float32)
            visits[i, far] = big
            valid[i, far] = 1
            if M > 1 and i % 2 == 0:
                valid[i, 0] = 0                                       # slot 0 is padding in some rows
            if temps[i] in (np.float32(1.0), np.float32(0.5)) and i % 3 == 0:
                temps[i] = np.float32(0.1)                            # most of them overflow
        elif c == "all_zero":
            visits[i] = np.where(valid[i] != 0, 0, visits[i]).astype(np.float32)
            valid[i, far] = 1
            visits[i, far] = 0
        elif c == "single_last":
            valid[i] = 0
            valid[i, M - 1] = 1
        elif c == "no_valid":
            valid[i] = 0
        elif c == "dup_cols":
            valid[i, [0, far, M // 2]] = 1
            lidx[i, far] = lidx[i, 0]
            lidx[i, M // 2] = lidx[i, 0]
        elif c == "col_T_and_neg":
            valid[i, [0, far]] = 1
            lidx[i, 0] = T
            lidx[i, far] = -1 if far else T
        elif c == "mixed_value":
            valid[i, far] = 1
            value_sum[i] = (np.where(np.arange(M) % 2 == 0, 1, -1) * r.uniform(0.5, 40, M)).astype(np.float32)
        elif c == "tiny_visits":                                      # sum(visits) < 1: the denominator clamp
            visits[i] = 0
            valid[i, far] = 1
            visits[i, far] = 0.25
            value_sum[i] = (r.uniform(-1, 1, M) * 0.1).astype(np.float32)
        if not valid[i].any() and c != "no_valid":
            valid[i, far] = 1
        value_sum[i] = np.where(valid[i] != 0, value_sum[i], 0).astype(np.float32)
        visits[i] = np.where(valid[i] != 0, visits[i], 0).astype(np.float32)           # padding holds no visits
        cls.append(c)
        # ---- the sampled pick this row aims at: the target slot first, then the uniform --------------------------------
        vs = np.flatnonzero(valid[i])
        kind = PICK_KINDS[(i + shift) % len(PICK_KINDS)]
        if c == "single_last":
            kind = "last_live"                                        # the one valid slot stays the only one
        if c == "no_valid" or M == 1:
            kinds.append("none")
            continue
        if kind == "after_invalid_run" and M >= 5:
            k = int(r.integers(3, M))
            valid[i, k - 3:k] = 0
            visits[i, k - 3:k] = 0
            value_sum[i, k - 3:k] = 0
            valid[i, k] = 1
        elif kind == "group":
            grp = vs[vs // 64 == (i // len(PICK_KINDS)) % (-(-M // 64))]
            k = int(r.choice(grp if grp.size else vs))
        elif kind in ("last_live", "u_top"):
            k = int(vs[-1])
        else:
            k = int(vs[0])
        if kind == "after_invalid_run" and M < 5:
            kind = "first_live"
        visits[i, k] = visits[i].max()                                # the target's weight is the row's largest: width >= 1 / M
        if c == "tiny_visits":
            visits[i] = 0                                             # keep 0 < sum(visits) < 1
            visits[i, k] = 0.25
        kinds.append(kind)
        target[i] = k
    inv_t = finalize_inv_t(temps)
    uniforms = np.zeros(R, np.float32)
    for i in range(R):
        if target[i] < 0:
            uniforms[i] = 0.5
            continue
        _, _, w, live = ref_sampled_pick(visits[i], valid[i] != 0, inv_t[i], 0.0)
        cum = np.cumsum(w)
        k = int(target[i])
        if kinds[i] == "u_zero":
            uniforms[i] = 0.0
            target[i] = int(np.flatnonzero(live)[0])
        elif kinds[i] == "u_top":
            uniforms[i] = np.nextafter(np.float32(1), np.float32(0))
            target[i] = int(np.flatnonzero(live)[-1])
        else:
            uniforms[i] = np.float32((cum[k] - w[k] / 2))
    return dict(M=M, R=R, B=B, T=T, lidx=lidx, codes=codes, valid=valid, visits=visits, value_sum=value_sum, roots=roots,
                temps=temps, uniforms=uniforms, cls=np.array(cls), kinds=np.array(kinds), target=target)


def finalize_cases():
    return [finalize_case(M, R) for M in FIN_M for R in FIN_R]


def small_finalize_case(visits, valid, value_sum, temps, roots, B, first_col):
    visits, valid = np.array(visits, np.float32), np.array(valid, np.uint8)
    R, M = visits.shape
    lidx = (np.array(first_col, np.int64)[:, None] + np.arange(M)[None, :])
    codes = (lidx[:, :, None] * 4 + np.arange(4)).astype(np.int32) % 36
    return dict(M=M, R=R, B=B, T=FIN_T, lidx=lidx, codes=codes, valid=valid, visits=visits,
                value_sum=np.array(value_sum, np.float32), roots=np.array(roots, np.int64), temps=np.array(temps, np.float32),
                uniforms=np.full(R, 0.5, np.float32), cls=np.array(["pin"] * R), kinds=np.array(["none"] * R),
                target=np.full(R, -1, np.int64))


def overflow_pin_case():
    """Row 0: 8000^10 and 9000^10 overflow float32 (T = 0.1), slot 0 is padding: the reference picks slot 2 (column 9).
    Row 1: at the temperature clamp every action with 2 visits or more overflows: slot 3 (column 11)."""
    return small_finalize_case([[0, 5, 8000, 9000, 3], [1, 0, 1, 2, 3]], [[0, 1, 1, 1, 1], [1, 1, 1, 1, 1]],
                               [[0, 1, -2, 3, 0.5], [0.5, 0, -1, 1, 1]], [0.1, 0.0], [1, 2], 3, [7, 8])


def no_valid_pin_case():
    """Rows 0 and 2 have no valid action (terminal roots of a padded layout): root_value is sum(value_sum) /
    max(sum(visits), 1) all the same, the other four outputs keep their fill."""
    return small_finalize_case([[1, 1, 2, 0], [1, 2, 1, 0], [0.25, 0.25, 0, 0]], [[0, 0, 0, 0], [1, 1, 1, 0], [0, 0, 0, 0]],
                               [[1, 1, 0.5, -0.5], [-2, 0.5, 0.5, 0], [1, 1, 0, 0]], [1.0, 1.0, 1.0], [1, 2, 3], 4, [3, 30, 60])


# =========================================================================================================================
# lz_finalize_trajectory_inplace
# =========================================================================================================================
TRAJ_F = (1, 4, 5, 300)
TRAJ_G = (1, 12, 300)
TRAJ_STEPS = (1, 20, 64, 65, 200)
TRAJ_RESULTS = np.array([-1.0, 0.0, 1.0, -0.0], np.float32)
TRAJ_COUNTS_IN = (7, 11, 13)


@functools.lru_cache(maxsize=None)
def traj_case(F, G, max_steps, seed=0):
    """-> one call.  Games' recorded counts rotate over 0, 1, 64, 65, max_steps, max_steps + 3 (past the clamp: the matrix
    has no column for them, and the rows beyond must stay untouched); every game's rows are a slice of one permutation
    of twice as many target rows, so that untouched rows lie between the written ones; the finished slots are distinct
    games, mixed with -1 and G."""
    r = np.random.default_rng([seed, F, G, max_steps, 5])
    rot = (TRAJ_F.index(F) + TRAJ_G.index(G) * 2 + TRAJ_STEPS.index(max_steps)) % 6
    step_counts = np.array([(0, 1, 64, 65, max_steps, max_steps + 3)[(g + rot) % 6] for g in range(G)], np.int64)
    S = 2 * G * max_steps + 5
    step_index = r.permutation(S)[:G * max_steps].reshape(G, max_steps).astype(np.int64)
    games = r.permutation(G)
    slots = np.full(F, -1, np.int64)
    slots[1::2] = G
    pos = np.sort(r.choice(F, min(F, G), replace=False)) if F > 2 else np.arange(min(F, G))
    slots[pos] = games[:pos.size]
    if F >= 4:                                                        # out-of-range slots also where games would fit
        slots[0], slots[F - 1] = -1, G
    return dict(F=F, G=G, max_steps=max_steps, S=S, step_counts=step_counts, step_index=step_index, slots=slots,
                signs=r.choice(np.array([-1, 1], np.int8), S), result=TRAJ_RESULTS[(np.arange(F) + rot) % 4],
                softv=r.uniform(-1, 1, F).astype(np.float32), counts_in=np.array(TRAJ_COUNTS_IN, np.int64))


def traj_cases():
    return [traj_case(F, G, s) for F, G, s in itertools.product(TRAJ_F, TRAJ_G, TRAJ_STEPS)]
