"""Plain restatements of the root operators of csrc/lz_ops.hip (numpy, per-row loops, float64 wherever arithmetic is
involved): lz_project_policy_logits_fast, lz_root_pack_rows / _plan / _fill, lz_root_finalize_from_visits and
lz_finalize_trajectory_inplace.  tests/test_root_ops_ref_cpu.py anchors every one of them on the committed golden values
of the reference (g4_project.npz, g7_ops.npz) and on oracle/lz_oracle.py; tests/test_gpu_root_ops.py holds the kernels to
them.  DESIGN.md section 23 has the bounds.

Inputs that stay out because the reference gives no single defined answer for them: a NaN or +inf head on a LEGAL entry of
the projection (torch's softmax makes the whole row NaN, the kernel's maximum skips a NaN), NaN visits, and visits whose
power overflows on a slot that is NOT valid (the reference multiplies inf by the mask's 0)."""
import numpy as np

F32_EPS = 2.0 ** -24                                        # unit roundoff of float32
F32_TINY = np.float32(1e-8)                                 # the reference's clamps, as the float32 it compares with
PROJECT_CAP = 1e-6                                          # what tests/test_gpu_ops.py allows the projection ...
FINALIZE_CAP = 1e-5                                         # ... and the finalize policy: never more than these


# =========================================================================================================================
# project_policy_logits_fast.cpp:16-164
# =========================================================================================================================
def movement_tables():
    """Column 36 + 4 * from + dir: (from, destination, on_board) of the 144 movement entries; dir = up, down, left, right."""
    frm = np.repeat(np.arange(36), 4)
    d = np.tile(np.arange(4), 36)
    r, c = frm // 6, frm % 6
    on = ~(((d == 0) & (r == 0)) | ((d == 1) & (r == 5)) | ((d == 2) & (c == 0)) | ((d == 3) & (c == 5)))
    dest = np.where(on, frm + np.array([-6, 6, -1, 1])[d], 0)
    return frm, dest, on


def ref_logits(lp1, lp2, lpmc, T):
    """float32[B, T]: placement | movement = float32 sum lp2[from] + lp1[dest], off-board -inf | selection | auxiliary 0."""
    lp1, lp2, lpmc = (np.asarray(a, np.float32) for a in (lp1, lp2, lpmc))
    B = lp1.shape[0]
    frm, dest, on = movement_tables()
    x = np.zeros((B, T), np.float32)
    x[:, :36] = lp1
    with np.errstate(invalid="ignore"):
        mv = (lp2[:, frm] + lp1[:, dest]).astype(np.float32)
    x[:, 36:180] = np.where(on[None, :], mv, np.float32(-np.inf))
    x[:, 180:216] = lpmc
    return x


def ref_project(lp1, lp2, lpmc, mask):
    """-> probs float64[B, T], masked_logits float32[B, T] (exact: a copy, one float32 add, -inf or 0)."""
    mask = np.asarray(mask).astype(bool)
    B, T = mask.shape
    x = ref_logits(lp1, lp2, lpmc, T)
    ml = np.where(mask, x, np.float32(-np.inf)).astype(np.float32)
    probs = np.zeros((B, T), np.float64)
    for b in range(B):
        legal = mask[b]
        if not legal.any():                                 # no legal entry: zeros, every logit -inf
            continue
        fin = legal & np.isfinite(ml[b])
        if not fin.any():                                   # :153-160: the legal entries of such a row read 0
            ml[b, legal] = 0.0
            continue
        z = ml[b, fin].astype(np.float64)
        e = np.exp(z - z.max())
        probs[b, fin] = e / e.sum()
    return probs, ml


def f32_project_probs(lp1, lp2, lpmc, mask):
    """The same softmax carried out in float32 throughout: the yardstick for what float32 can reach (its distance from
    ref_project, times 4, is the kernel's bound)."""
    mask = np.asarray(mask).astype(bool)
    B, T = mask.shape
    ml = np.where(mask, ref_logits(lp1, lp2, lpmc, T), np.float32(-np.inf)).astype(np.float32)
    probs = np.zeros((B, T), np.float32)
    for b in range(B):
        fin = np.isfinite(ml[b])
        if fin.any():
            e = np.exp(ml[b, fin] - ml[b, fin].max(), dtype=np.float32)
            probs[b, fin] = e / e.sum(dtype=np.float32)
    return probs


# =========================================================================================================================
# root_pack_sparse_actions (module.cpp:247-363) behind the three-call protocol
# =========================================================================================================================
def ref_pack_rows(mask, probs, meta, cap):
    """-> counts int32[B], legal_index int32[B, cap] (-1), priors float64[B, cap] (0), codes int32[B, cap, 4] (0).
    Precondition of the operator: no row has more than `cap` legal entries."""
    mask = np.asarray(mask).astype(bool)
    B, T = mask.shape
    counts = np.zeros(B, np.int32)
    legal_index = np.full((B, cap), -1, np.int32)
    priors = np.zeros((B, cap), np.float64)
    codes = np.zeros((B, cap, 4), np.int32)
    for b in range(B):
        idx = np.flatnonzero(mask[b])
        n = idx.size
        assert n <= cap
        p = np.asarray(probs[b], np.float32)[idx].astype(np.float64)
        counts[b] = n
        legal_index[b, :n] = idx
        priors[b, :n] = p / max(p.sum(), 1e-8)
        codes[b, :n] = np.asarray(meta, np.int32)[b, idx]
    return counts, legal_index, priors, codes


def pack_row_sums(mask, probs):
    """float64 sum of the legal probabilities of every row (which rows sit under the 1e-8 clamp)."""
    return (np.asarray(probs, np.float32).astype(np.float64) * np.asarray(mask).astype(bool)).sum(1)


def ref_pack_plan(counts):
    """-> rank int32[B] (-1 for a row without legal action), child_off int64[B], sizes int64[3] = {R, Amax, N}."""
    B = len(counts)
    rank = np.full(B, -1, np.int32)
    child_off = np.zeros(B, np.int64)
    r = k = mx = 0
    for b in range(B):
        c = int(counts[b])
        child_off[b] = k
        if c > 0:
            rank[b] = r
            r += 1
            k += c
        mx = max(mx, c)
    return rank, child_off, np.array([r, mx, k], np.int64)


PACK_FILL_OUT = ("terminal_mask", "valid_root_indices", "counts", "valid_mask", "legal_index_mat", "priors_mat",
                 "action_code_mat", "pack_flat_idx", "action_codes_all", "parent_indices_all")


def ref_pack_fill(counts, legal_index, priors, codes, rank, child_off, R, M, N):
    """The reference's 10-tuple from the fixed-capacity rows: copies only, so `priors` (float32) comes back bit for bit."""
    B, cap = legal_index.shape
    o = dict(terminal_mask=np.zeros(B, np.uint8), valid_root_indices=np.zeros(R, np.int64), counts=np.zeros(R, np.int64),
             valid_mask=np.zeros((R, M), np.uint8), legal_index_mat=np.zeros((R, M), np.int64),
             priors_mat=np.zeros((R, M), np.float32), action_code_mat=np.zeros((R, M, 4), np.int32),
             pack_flat_idx=np.zeros(N, np.int64), action_codes_all=np.zeros((N, 4), np.int32),
             parent_indices_all=np.zeros(N, np.int64))
    for b in range(B):
        c, r = int(counts[b]), int(rank[b])
        o["terminal_mask"][b] = c == 0
        if r < 0:
            continue
        o["valid_root_indices"][r] = b
        o["counts"][r] = c
        for k in range(min(c, M)):
            o["valid_mask"][r, k] = 1
            o["legal_index_mat"][r, k] = max(int(legal_index[b, k]), 0)
            o["priors_mat"][r, k] = priors[b, k]
            o["action_code_mat"][r, k] = codes[b, k]
            o["pack_flat_idx"][child_off[b] + k] = r * M + k
            o["action_codes_all"][child_off[b] + k] = codes[b, k]
            o["parent_indices_all"][child_off[b] + k] = b
    return o


def priors_bound(counts):
    """Relative error of a float32 prior against float64: a float32 sum of `count` non-negative terms in any order is
    within (count - 1) u of the exact sum (relative; every partial sum is at most the total), rounding the inputs' quotient
    adds u, and first-order slack 2 u covers the products of these: (count + 2) * 2^-24."""
    return (np.asarray(counts, np.float64) + 2.0) * F32_EPS


# =========================================================================================================================
# root_finalize_from_visits (module.cpp:441-535) + the sampled pick of mcts_gpu.py:853-898
# =========================================================================================================================
def finalize_inv_t(temps):
    """1 / max(T, 1e-6) as the float32 the reference and the kernel raise to."""
    t = np.maximum(np.asarray(temps, np.float32), np.float32(1e-6))
    return (np.float32(1.0) / t).astype(np.float32)


def ref_row_policy(visits, valid, inv_t):
    """One row: (policy float64[M], overflow bool).  pow(max(v, 1e-8), 1/T) on the valid slots, normalised with the 1e-8
    clamp.  Whether a power overflows is decided in float32, as the reference computes it: then the overflowed entries
    are inf / inf = NaN and every other entry is x / inf = 0."""
    v = np.maximum(np.asarray(visits, np.float32), F32_TINY)
    with np.errstate(over="ignore"):
        p32 = np.power(v, np.float32(inv_t), dtype=np.float32)
        p64 = np.power(v.astype(np.float64), float(inv_t))
    over = valid & np.isinf(p32)
    if over.any():
        return np.where(over, np.nan, 0.0), True
    p64 = np.where(valid, p64, 0.0)
    return p64 / max(p64.sum(), 1e-8), False


def torch_argmax(pol):
    """torch's max over a row: a NaN is the maximum; the lowest index wins."""
    p = np.asarray(pol, np.float64).astype(np.float32)      # the comparison the reference makes is one of float32 values
    nan = np.flatnonzero(np.isnan(p))
    return int(nan[0]) if nan.size else int(np.argmax(p))


def ref_sampled_pick(visits, valid, inv_t, u):
    """The documented rule (header; mcts_gpu.py:853-898), float64: sanitise, log / T, subtract the finite maximum, exp,
    uniform over the legal set when the sum is not positive and finite; the first live slot whose inclusive sum exceeds
    u * sum, else the last live slot.  A slot is live when it is valid and its weight is positive as a float32 (weights
    below the float32 range are 0 to the kernel).  -> (pick or -1, width of the pick's interval / sum, weights, live)."""
    v = np.asarray(visits, np.float32).astype(np.float64)
    v = np.where(np.isfinite(v), v, 0.0)
    with np.errstate(divide="ignore"):
        lg = np.where(valid, np.log(np.maximum(v, float(F32_TINY))) * float(inv_t), -np.inf)
    mx = lg.max() if lg.size else -np.inf
    if not np.isfinite(mx):
        mx = 0.0
    ex = np.where(valid, np.exp(lg - mx), 0.0)
    ex = np.where(np.isfinite(ex), ex, 0.0)
    total = ex.sum()
    if not (total > 0 and np.isfinite(total)):
        ex = valid.astype(np.float64)
        total = float(max(int(valid.sum()), 1))
    live = valid & (ex.astype(np.float32) > 0)
    cum = np.cumsum(ex)
    hit = np.flatnonzero(live & (cum > float(np.float32(u)) * total))
    pick = int(hit[0]) if hit.size else (int(np.flatnonzero(live)[-1]) if live.any() else -1)
    width = ex[pick] / total if pick >= 0 else 0.0
    return pick, width, ex / total, live


def ref_finalize(lidx, codes, valid, visits, value_sum, roots, B, T, temps, uniforms=None):
    """-> dict: policy float64[B, T] (NaN where the reference has NaN), chosen_index int64[B], chosen_codes int32[B, 4],
    chosen_valid uint8[B], root_value float64[R], pick int[R] (local slot, -1: row without valid action), overflow bool[R],
    dup bool[R] (two valid slots of the row share a column)."""
    valid = np.asarray(valid).astype(bool)
    visits = np.asarray(visits, np.float32)
    R, M = valid.shape
    inv_t = finalize_inv_t(temps)
    out = dict(policy=np.zeros((B, T), np.float64), chosen_index=np.full(B, -1, np.int64),
               chosen_codes=np.full((B, 4), -1, np.int32), chosen_valid=np.zeros(B, np.uint8),
               root_value=np.zeros(R, np.float64), pick=np.full(R, -1, np.int64), overflow=np.zeros(R, bool),
               dup=np.zeros(R, bool), root_value_bound=np.zeros(R, np.float64))
    for r in range(R):
        v64, w64 = visits[r].astype(np.float64), np.asarray(value_sum[r], np.float32).astype(np.float64)
        den = max(v64.sum(), 1.0)
        out["root_value"][r] = w64.sum() / den              # every row, also one without a valid action
        # float32 sums of M terms in any order: |error| <= (M - 1) u sum|w| and (M - 1) u sum(v).  To first order the
        # quotient moves by err_w / den + |sum w| err_v / den^2 <= (M - 1) u (sum|w| / den) (1 + sum(v) / den); the
        # division's own rounding adds u |q| <= u sum|w| / den, and 2 u of slack covers the second-order terms:
        out["root_value_bound"][r] = (M + 2) * F32_EPS * (np.abs(w64).sum() / den) * (1.0 + v64.sum() / den)
        if not valid[r].any():
            continue
        b = int(roots[r])
        pol, out["overflow"][r] = ref_row_policy(visits[r], valid[r], inv_t[r])
        pick = torch_argmax(pol)
        if uniforms is not None and M > 1:
            s, _, _, _ = ref_sampled_pick(visits[r], valid[r], inv_t[r], uniforms[r])
            pick = s if s >= 0 else pick
        cols = np.asarray(lidx[r], np.int64)
        ok = valid[r] & (cols >= 0) & (cols < T)
        np.add.at(out["policy"][b], cols[ok], pol[ok])      # duplicates accumulate, columns outside [0, T) are dropped
        out["dup"][r] = np.unique(cols[ok]).size < int(ok.sum())
        out["pick"][r] = pick
        out["chosen_index"][b] = cols[pick]
        out["chosen_codes"][b] = codes[r, pick]
        out["chosen_valid"][b] = 1
    return out


# =========================================================================================================================
# finalize_trajectory_inplace (module.cpp:547-630) as the C ABI has it
# =========================================================================================================================
def ref_finalize_trajectory(value_t, soft_t, signs, step_index, step_counts, max_steps, slots, result, softv, counts_in):
    """Per finished slot f (no compaction): a slot outside [0, G) has n = 0, n is clamped to max_steps; keep[f] = n > 0,
    final_counts[f] = n, counts_out += [black wins, white wins, draws] over the kept ones, and the game's first n rows get
    sign * result / sign * soft.  -> (value_t, soft_t, keep uint8[F], final_counts int64[F], counts_out int64[3])."""
    value_t, soft_t = np.array(value_t, np.float32), np.array(soft_t, np.float32)
    G, F = len(step_counts), len(slots)
    keep, final_counts = np.zeros(F, np.uint8), np.zeros(F, np.int64)
    counts_out = np.array(counts_in, np.int64)
    for f in range(F):
        g = int(slots[f])
        n = int(step_counts[g]) if 0 <= g < G else 0
        n = min(n, max_steps)
        keep[f], final_counts[f] = n > 0, n
        if n == 0:
            continue
        res = np.float32(result[f])
        counts_out[0 if res > 0 else (1 if res < 0 else 2)] += 1
        idx = np.asarray(step_index, np.int64).reshape(G, max_steps)[g, :n]
        sg = np.asarray(signs)[idx].astype(np.float32)
        value_t[idx] = sg * res
        soft_t[idx] = sg * np.float32(softv[f])
    return value_t, soft_t, keep, final_counts, counts_out
