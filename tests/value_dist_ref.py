"""Restatement of the distributional value target of merged positions, for the tests only (numpy
on the CPU): `two_hot` and `group_distribution` of csrc/lz_value_dist.h, `merge_ref` = lz_merge_value_distributions, the
float64 bucket cross entropy and its gradient against any target distribution, and the inputs the CPU and GPU tests
share.

Every float32 step of `two_hot` is a numpy float32 operation of its own (no fused multiply-add exists in numpy), in the
order the header writes them; the sums of `group_distribution` are Python floats (doubles) added member after member."""
import numpy as np

BINS = 101
REC = 360
VALUE_OFF, SOFT_OFF = 348, 352
INT32_MIN = -(1 << 31)
F = np.float32


def two_hot(value, soft, alpha):
    """float32 arrays (or scalars) -> (lo int64, hi int64, frac float32), elementwise."""
    v = np.asarray(value, F)
    s = np.asarray(soft, F)
    al = F(alpha)
    with np.errstate(all="ignore"):
        a = (F(1.0) - al) * v
        b = al * s
        mixed = (a + b).astype(F)
        mixed = np.fmin(np.fmax(mixed, F(-1.0)), F(1.0)).astype(F)          # fmax / fmin return the other operand of a NaN
        step = F(2.0) / F(BINS - 1)
        u = ((mixed + F(1.0)).astype(F) / step).astype(F)
        fl = np.floor(u)
        lo = np.where(fl >= 0, np.where(fl < BINS - 1, fl, BINS - 1), 0).astype(np.int64)
        hi = np.minimum(lo + 1, BINS - 1)
        frac = np.fmin(np.fmax((u - lo.astype(F)).astype(F), F(0.0)), F(1.0)).astype(F)
        frac = np.where(hi == lo, F(0.0), frac).astype(F)
    return lo, hi, frac


def two_hot_row(value, soft, alpha):
    """float32[101]: the target the loss kernel forms for one row (tg0 / tg1 of every lane)."""
    lo, hi, frac = (x.reshape(()) for x in two_hot(value, soft, alpha))
    row = np.zeros(BINS, F)
    for b in range(BINS):
        row[b] = (F(1.0) - frac if b == lo else F(0.0)) + (frac if b == hi else F(0.0))
    return row


def group_distribution(values, softs, alpha):
    """float32[101] of the members in order: per bin a double summed sequentially from 0.0, / c, rounded once."""
    values, softs = np.asarray(values, F).reshape(-1), np.asarray(softs, F).reshape(-1)
    c = len(values)
    lo, hi, frac = two_hot(values, softs, alpha)
    S = [0.0] * BINS
    for i in range(c):                                               # only the two bins a member touches change
        l, h, f = int(lo[i]), int(hi[i]), frac[i]
        if l == h:
            S[l] += float((F(1.0) - f) + f)
        else:
            S[l] += float(F(1.0) - f)
            S[h] += float(f)
    return np.array([F(np.float64(x) / np.float64(c)) for x in S], F)


def mean_target_row(values, softs, alpha):
    """What the merges did before: the two-hot of the members' mean value and mean soft value (double sums, one rounding)."""
    v = F(np.asarray(values, F).astype(np.float64).sum() / len(values))
    s = F(np.asarray(softs, F).astype(np.float64).sum() / len(softs))
    return two_hot_row(v, s, alpha)


def merge_ref(value_of, soft_of, n, index, m, order, begin, dist_row, alpha, dist):
    """lz_merge_value_distributions: value_of / soft_of float32[n] by element; index int64[m] or None; -> a copy of `dist`
    [rows,101] with the rows of the groups written (D = len(dist))."""
    out = np.array(dist, F, copy=True)
    D = len(out)
    for g in range(len(begin) - 1):
        d = int(dist_row[g])
        if d < 0 or d >= D:
            continue
        b, e = int(begin[g]), int(begin[g + 1])
        bad = b < 0 or e <= b or e > m
        elems = []
        for i in range(b, e) if not bad else ():
            p = int(order[i])
            if p < 0 or p >= m:
                bad = True
                break
            el = p if index is None else int(index[p])
            if el < 0 or el >= n:
                bad = True
                break
            elems.append(el)
        out[d] = 0 if bad else group_distribution(value_of[elems], soft_of[elems], alpha)
    return out


# ---- float64 bucket cross entropy ----------------------------------------------------------------------------------------------
def ce_and_grad(logits, target, scale):
    """logits [rows,101], target [rows,101], scale [rows] (or a scalar), all taken to float64 ->
    (ce [rows], (softmax - target) * scale [rows,101]).  The gradient is that of a target that sums to one, as the loss
    kernel and tests/train_loss_ref.py::ref_loss write it; both are linear in the target."""
    x = np.asarray(logits, np.float64)
    t = np.asarray(target, np.float64)
    mx = x.max(axis=1, keepdims=True)
    lse = mx + np.log(np.exp(x - mx).sum(axis=1, keepdims=True))
    logp = x - lse
    ce = -(t * logp).sum(axis=1)
    sc = np.broadcast_to(np.asarray(scale, np.float64).reshape(-1, 1), (x.shape[0], 1))
    grad = (np.exp(logp) - t) * sc
    return ce, grad


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
def special_values():
    """The values of the issue: +-1, 0, bin centres +-0.02 k, their float32 neighbours, +-1.5, NaN, +-inf, denormals."""
    k = np.arange(0, 51, 7)
    centres = np.concatenate([F(0.02) * k.astype(F), -(F(0.02) * k.astype(F))]).astype(F)
    near = np.concatenate([np.nextafter(centres, F(2.0)), np.nextafter(centres, F(-2.0))]).astype(F)
    odd = np.array([-1.0, 1.0, 0.0, -0.0, 1.5, -1.5, np.nan, np.inf, -np.inf], F)
    den = np.array([1, 0x80000001, 0x007FFFFF, 0x807FFFFF], np.uint32).view(F)
    nan_payload = np.array([0x7FC00123, 0xFFC00001, 0x7F800001], np.uint32).view(F)      # quiet, negative quiet, signalling
    return np.concatenate([odd, centres, near, den, nan_payload]).astype(F)


GROUP_SIZES = (1, 2, 3, 300)
ALPHAS = (0.0, 0.25, 1.0)


def build_case(seed, groups_wanted=None):
    """-> dict(value, soft float32[n]; order int64[m], begin int64[G+1], sizes): groups of sizes 1, 2, 3, 300 (repeated
    until `groups_wanted` groups exist), every special value a member of some group, one group of identical members, one
    (+1, -1) pair, members listed in a shuffled `order` so that member order differs from element order."""
    rng = np.random.default_rng(seed)
    sp = special_values()
    sizes = [2, 3] + list(GROUP_SIZES)                               # group 0: the (+1, -1) pair; group 1: identical members
    while groups_wanted is not None and len(sizes) < groups_wanted:
        sizes.append(GROUP_SIZES[len(sizes) % 3])                    # small ones: 1, 2, 3
    if groups_wanted is not None:
        sizes = sizes[:groups_wanted]
    n = sum(sizes)
    value = rng.choice(np.array([-1.0, 0.0, 1.0], F), n).astype(F)
    soft = rng.uniform(-1.2, 1.2, n).astype(F)
    where = rng.permutation(n)
    k = min(len(sp), n)
    value[where[:k]] = sp[:k]                                        # the specials as values ...
    soft[where[::-1][:k]] = sp[:k]                                   # ... and, elsewhere, as soft values
    begin = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    elems = rng.permutation(n).astype(np.int64)                      # order[i]: the element of place i
    if len(sizes) >= 1 and sizes[0] == 2:
        value[elems[0:2]] = (1.0, -1.0)
        soft[elems[0:2]] = (1.0, -1.0)
    if len(sizes) >= 2:
        value[elems[begin[1]:begin[2]]] = F(0.3)
        soft[elems[begin[1]:begin[2]]] = F(-0.7)
    return {"value": value, "soft": soft, "order": elems, "begin": begin, "sizes": sizes}


def ring_of(value, soft, guard, seed):
    """-> (ring uint8[guard + n + guard, 360] of junk with the two floats of element e in record slot[e], slot int64[n]):
    the elements scattered over the ring, `guard` records of junk at either end and junk in every other byte."""
    rng = np.random.default_rng(seed)
    n = len(value)
    cap = n + 2 * guard
    ring = rng.integers(0, 256, (cap, REC), dtype=np.uint8)
    ring[:, VALUE_OFF:VALUE_OFF + 8].view(F)[:] = F(1e30)            # a value nobody may read: bin 100, visibly wrong
    slot = (guard + rng.permutation(n)).astype(np.int64)
    ring[slot, VALUE_OFF:VALUE_OFF + 4] = np.ascontiguousarray(value).view(np.uint8).reshape(n, 4)
    ring[slot, SOFT_OFF:SOFT_OFF + 4] = np.ascontiguousarray(soft).view(np.uint8).reshape(n, 4)
    return np.ascontiguousarray(ring), slot


def ring_floats(ring):
    """(value_of, soft_of) float32[capacity] of a ring, by slot."""
    return (np.ascontiguousarray(ring[:, VALUE_OFF:VALUE_OFF + 4]).view(F).reshape(-1),
            np.ascontiguousarray(ring[:, SOFT_OFF:SOFT_OFF + 4]).view(F).reshape(-1))


def linearity_case(seed, exact=True):
    """Groups that share their logits: -> dict(logits float32[G,101], value / soft float32[n], owner int64[n] (the group of
    every unmerged row), count [G], alpha).  Group 0 is a (+1, -1) pair.
    exact: game results -1 / 0 / +1 at alpha 0 in groups of 1, 2, 4 and 8 -- every two-hot is a one-hot of 1.0 and every
    group mean k / 2^j, so the float32 table holds the mean without rounding and the linearity is testable to 1e-12 on the
    table itself.  Otherwise: odd counts, random soft values, alpha 0.25 -- the table rounds each entry once (<= 2^-25),
    and the linearity holds to 1e-12 for the unrounded mean only."""
    rng = np.random.default_rng(seed)
    count = np.array([2, 1, 4, 8, 2, 1, 4, 2, 8] if exact else [2, 1, 3, 5, 2, 1, 4, 2, 7], np.int64)
    G = len(count)
    owner = np.repeat(np.arange(G), count)
    n = len(owner)
    value = rng.choice(np.array([-1.0, 0.0, 1.0], F), n).astype(F)
    soft = value.copy() if exact else rng.uniform(-1, 1, n).astype(F)
    value[:2] = (1.0, -1.0)
    soft[:2] = (1.0, -1.0)
    logits = (3.0 * rng.standard_normal((G, BINS))).astype(F)
    return {"logits": logits, "value": value, "soft": soft, "owner": owner, "count": count, "alpha": 0.0 if exact else 0.25}


def exact_mean_rows(c):
    """float64[G,101]: the unrounded mean of the members' float32 two-hot rows."""
    rows = np.stack([two_hot_row(v, s, c["alpha"]) for v, s in zip(c["value"], c["soft"])]).astype(np.float64)
    out = np.zeros((len(c["count"]), BINS))
    np.add.at(out, c["owner"], rows)
    return out / c["count"].reshape(-1, 1)


def linearity_sides(c, merged_target):
    """The two float64 sides of the linearity argument for a case of `linearity_case`:
    unmerged: the n rows with their own two-hot, B = n, grad_scale 1, gradients summed per group;
    merged: one row per group against merged_target [G,101] with weight count, B = G, grad_scale G / n.
    -> (unmerged [G,101], merged [G,101])."""
    owner, count = c["owner"], c["count"]
    n, G = len(owner), len(count)
    rows = np.stack([two_hot_row(v, s, c["alpha"]) for v, s in zip(c["value"], c["soft"])])
    _, g_rows = ce_and_grad(c["logits"][owner], rows, 1.0 / n)
    unmerged = np.zeros((G, BINS))
    np.add.at(unmerged, owner, g_rows)
    _, merged = ce_and_grad(c["logits"], merged_target, (G / n) / G * count.astype(np.float64))
    return unmerged, merged
