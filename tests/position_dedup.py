"""Numpy restatement of merging duplicate positions among training rows (liuzhou_amd/position_dedup.py,
csrc/lz_dedup.h): the reading of a row, the row's symmetry k*, the key words, the exact grouping,
the frame map and the merged row with the fixed association of its sums.  Built on the (r, c) formulas of
`symmetry.np_*`, not on the compiled tables; the kernels and the host build are checked against it bit for bit."""
import numpy as np

from liuzhou_amd import symmetry as SY

CHUNK = 256
MODES = ("exact", "symmetric")
CELL = np.stack([SY.np_cell_perm(k) for k in range(8)])               # [8,36]  sigma_k(cell)
ACTION = np.stack([SY.np_action_perm(k) for k in range(8)])           # [8,220] P_k(action)
COMPOSE = np.array([[SY.np_compose(a, b) for b in range(8)] for a in range(8)])
INVERSE = np.array([int(np.flatnonzero(COMPOSE[a] == 0)[0]) for a in range(8)])
_SHIFT = np.arange(36, dtype=np.uint64)


def frame_map(sym_f: int, sym_m: int) -> int:
    """e_m: from member m's frame to the first member f's frame."""
    return int(COMPOSE[INVERSE[int(sym_f)], int(sym_m)])


def read_rows(planes):
    """boards uint64[n,4], phase int64[n], representable bool[n] of planes float32[n,11,36]."""
    pl = np.asarray(planes, np.float32).reshape(-1, 11, 36)
    good = ((pl == 0) | (pl == 1)).all(axis=(1, 2))                  # -0.0 == 0; NaN is neither
    nz = pl != 0
    boards = (nz[:, :4].astype(np.uint64) << _SHIFT).sum(axis=2, dtype=np.uint64)
    some, every = nz[:, 4:].any(axis=2), nz[:, 4:].all(axis=2)       # [n,7]
    ok = good & (some == every).all(axis=1) & (some.sum(axis=1) <= 1)
    phase = np.where(some.any(axis=1), some.argmax(axis=1) + 1, 0).astype(np.int64)
    return boards, phase, ok


def sym_boards(k: int, boards):
    """Bit x of every board moved to bit sigma_k(x)."""
    b = np.asarray(boards, np.uint64)
    bits = (b[..., None] >> _SHIFT) & np.uint64(1)
    return (bits << CELL[k].astype(np.uint64)).sum(axis=-1, dtype=np.uint64)


def _lex_less(a, b):
    less = np.zeros(len(a), bool)
    open_ = np.ones(len(a), bool)
    for j in range(a.shape[1]):
        less |= open_ & (a[:, j] < b[:, j])
        open_ &= a[:, j] == b[:, j]
    return less


def choose_sym(boards, symmetric: bool):
    """(k* int8[n], the image of the boards under it)."""
    best = np.asarray(boards, np.uint64).copy()
    sym = np.zeros(len(best), np.int8)
    if symmetric:
        for k in range(1, 8):
            img = sym_boards(k, boards)
            lt = _lex_less(img, best)                                # strictly smaller: the lowest k wins a tie
            best[lt], sym[lt] = img[lt], k
    return sym, best


def keys(planes, masks, symmetric: bool):
    """(keys int64[n,8], sym int8[n], the number of rows that are not representable)."""
    boards, phase, ok = read_rows(planes)
    n = len(ok)
    mk = np.asarray(masks).reshape(n, 220) != 0
    sym, img = choose_sym(boards, symmetric)
    out = np.zeros((n, 8), np.uint64)
    out[:, :4] = img
    out[:, 0] |= phase.astype(np.uint64) << np.uint64(36)
    moved = np.zeros_like(mk)
    for k in range(8):
        rows = np.flatnonzero(sym == k)
        moved[rows[:, None], ACTION[k][None, :]] = mk[rows]
    b = np.arange(220)
    for w in range(4):
        cols = b[(b >> 6) == w]
        out[:, 4 + w] = (moved[:, cols].astype(np.uint64) << (cols & 63).astype(np.uint64)).sum(axis=1, dtype=np.uint64)
    bad = np.flatnonzero(~ok)
    out[bad] = 0
    out[bad, 0] = np.uint64(1 << 63) | bad.astype(np.uint64)
    sym[bad] = 0
    return out.view(np.int64), sym, int(len(bad))


def group(key_words):
    """Exact grouping: (group_of_row int64[n], order int64[n], group_begin int64[groups+1]); groups by ascending first
    member, members by ascending row."""
    k = np.ascontiguousarray(key_words, np.int64).reshape(-1, 8)
    ids = {}
    gor = np.array([ids.setdefault(k[i].tobytes(), len(ids)) for i in range(len(k))], np.int64).reshape(-1)
    order = np.argsort(gor, kind="stable").astype(np.int64)
    begin = np.concatenate([[0], np.cumsum(np.bincount(gor, minlength=len(ids)))]).astype(np.int64)
    return gor, order, begin


def chunked_sum(terms):
    """Sum over axis 0 in the fixed association: chunks of 256, each accumulated in order from 0.0, added in order."""
    terms = np.asarray(terms, np.float64)
    total = np.zeros(terms.shape[1:], np.float64)
    for c0 in range(0, len(terms), CHUNK):
        part = np.zeros(terms.shape[1:], np.float64)
        for t in terms[c0:c0 + CHUNK]:
            part = part + t
        total = total + part
    return total


def merge_groups(planes, masks, policy, value, soft, sym, order, group_begin, check_members: bool = True):
    """The merge entry point: (planes, masks, policy, value, soft, count) of the groups.  A group with an empty or
    impossible range, an `order` entry outside [0, n) or a sym outside 0..7 is an all-zero row with count 0."""
    pl = np.ascontiguousarray(planes, np.float32).reshape(-1, 11, 36)
    n = len(pl)
    mk = np.ascontiguousarray(masks).reshape(n, 220)
    pol = np.ascontiguousarray(policy, np.float32).reshape(n, 220)
    val, sof = np.ascontiguousarray(value, np.float32).reshape(-1), np.ascontiguousarray(soft, np.float32).reshape(-1)
    G = len(group_begin) - 1
    o_pl, o_mk = np.zeros((G, 11, 36), np.float32), np.zeros((G, 220), mk.dtype)
    o_pol, o_val, o_sof = np.zeros((G, 220), np.float32), np.zeros(G, np.float32), np.zeros(G, np.float32)
    count = np.zeros(G, np.int32)
    for g in range(G):
        b, e = int(group_begin[g]), int(group_begin[g + 1])
        if b < 0 or e <= b or e > n:
            continue
        mem = np.asarray(order[b:e], np.int64)
        if (mem < 0).any() or (mem >= n).any() or (np.asarray(sym)[mem] < 0).any() or (np.asarray(sym)[mem] > 7).any():
            continue
        f, c = int(mem[0]), len(mem)
        o_pl[g], o_mk[g], count[g] = pl[f], mk[f], c
        if c == 1:                                                   # a bit copy
            o_pol[g], o_val[g], o_sof[g] = pol[f], val[f], sof[f]
            continue
        moved = np.zeros((c, 220), np.float64)
        for i, m in enumerate(mem):
            e_m = frame_map(sym[f], sym[m])
            moved[i, ACTION[e_m]] = pol[m].astype(np.float64)
            if check_members:                                        # sigma_e of the member IS the first member
                img = np.zeros((11, 36), np.float32)
                img[:, CELL[e_m]] = pl[m]
                im = np.zeros(220, bool)
                im[ACTION[e_m]] = mk[m] != 0
                assert np.array_equal(img, pl[f]) and np.array_equal(im, mk[f] != 0), (g, int(m), f, e_m)
        c_p = int((pol[mem] != 0).any(axis=1).sum())
        valid = (pol[mem] != 0).any(axis=1)
        S = chunked_sum(np.where(valid[:, None], moved, 0.0))
        o_pol[g] = (S / c_p).astype(np.float32) if c_p else 0.0
        o_val[g] = np.float32(chunked_sum(val[mem].astype(np.float64)) / c)
        o_sof[g] = np.float32(chunked_sum(sof[mem].astype(np.float64)) / c)
    return o_pl, o_mk, o_pol, o_val, o_sof, count


def merge_duplicate_positions(planes, masks, policy, value, soft, *, mode: str, max_copies: int = 1):
    """((planes, masks, policy, value, soft), info) as liuzhou_amd.position_dedup.merge_duplicate_positions returns."""
    assert mode in MODES and int(max_copies) >= 1
    shape = np.asarray(planes).shape
    k, sym, bad = keys(planes, masks, mode == "symmetric")
    gor, order, begin = group(k)
    o_pl, o_mk, o_pol, o_val, o_sof, count = merge_groups(planes, masks, policy, value, soft, sym, order, begin)
    reps = np.minimum(count, int(max_copies)).astype(np.int64)
    take = np.repeat(np.arange(len(count)), reps)
    merged = count > 1
    info = {"rows_in": int(len(sym)), "rows_out": int(len(take)), "groups": int(len(count)),
            "merged_groups": int(merged.sum()), "merged_rows": int(count[merged].sum()),
            "largest_group": int(count.max()) if len(count) else 0, "not_representable": bad, "mode": mode,
            "max_copies": int(max_copies), "group_of_row": gor, "count": count}
    return (o_pl[take].reshape((-1,) + tuple(shape[1:])), o_mk[take], o_pol[take], o_val[take], o_sof[take]), info


# ---- the synthetic grid of the tests ---------------------------------------------------------------------------------------
GROUP_SIZES = (1, 2, 3, 255, 256, 257, 600)                           # every chunk boundary; 600 = 2 chunks + 88


def make_planes(boards, phase):
    """float32[11,36] of four bit boards and a phase 0..7."""
    pl = np.zeros((11, 36), np.float32)
    for p in range(4):
        pl[p] = (int(boards[p]) >> np.arange(36)) & 1
    if phase:
        pl[3 + phase] = 1.0
    return pl


def _random_policy(rng, mask):
    p = np.zeros(220, np.float32)
    on = np.flatnonzero(mask)
    w = rng.random(len(on)).astype(np.float32) + np.float32(0.01)
    p[on] = w / w.sum(dtype=np.float32)
    return p


def grid(seed: int, spread: bool):
    """The rows of the synthetic grid, shuffled so that the members of every group interleave: a dict of planes
    float32[n,11,6,6], masks uint8[n,220], policy float32[n,220], value, soft float32[n].  `spread`: the members of a
    group stand under all eight symmetries (they merge in symmetric mode); otherwise they are the same row image."""
    rng = np.random.default_rng(seed)
    rows = []

    def add(pl, mk, pol=None, k=0):
        tp, tm, tq = SY.np_transform_samples(pl[None], mk[None].astype(np.uint8),
                                             (_random_policy(rng, mk) if pol is None else pol)[None], k)
        if pol is None:                                              # a member's own policy, on its own legal actions
            tq = _random_policy(rng, tm[0])[None]
        rows.append((tp[0].reshape(11, 36), tm[0], tq[0], np.float32(rng.integers(-1, 2)),
                     np.float32(rng.uniform(-1, 1))))

    def position():
        boards = [int(x) for x in rng.integers(0, 1 << 36, 4, dtype=np.uint64)]
        mk = rng.random(220) < 0.25
        mk[int(rng.integers(0, 220))] = True
        return make_planes(boards, int(rng.integers(0, 8))), mk

    for c in GROUP_SIZES:
        pl, mk = position()
        for i in range(c):
            add(pl, mk, k=i % 8 if spread else 0)
    empty = make_planes([0, 0, 0, 0], 1)                              # the stabiliser is the whole group
    place = np.arange(220) < 36
    for i in range(5):
        add(empty, place, k=(3 * i) % 8 if spread else 0)
    mirror = make_planes([(1 << 1) | (1 << 4), 1 << 14 | 1 << 15, 0, 0], 2)   # fixed by flip left-right alone
    mk = np.zeros(220, bool)
    mk[[2, 3, 180 + 1, 180 + 4]] = True
    for k in range(8):
        add(mirror, mk, k=k if spread else 0)
    pl, mk = position()                                              # equal boards, another phase
    other = pl.copy()
    other[4:] = 0
    other[4 + (int(pl[4:, 0].argmax()) + 1) % 7] = 1.0
    pl[4:] = 0
    pl[4] = 1.0
    add(pl, mk), add(other, mk), add(pl, mk)
    pl, mk = position()                                              # equal planes, another legal mask
    mk2 = mk.copy()
    mk2[int(np.flatnonzero(~mk)[0])] = True
    add(pl, mk), add(pl, mk2), add(pl, mk2)
    pl, mk = position()                                              # not representable: they never join a group
    half = pl.copy()
    half[1, 7] = 0.5
    add(half, mk), add(half, mk)
    two = pl.copy()
    two[4:] = 0
    two[5] = two[8] = 1.0
    add(two, mk), add(two, mk)
    ragged = pl.copy()
    ragged[4:] = 0
    ragged[6, :35] = 1.0
    add(ragged, mk), add(ragged, mk)
    pl, mk = position()                                              # -0.0 is a zero: representable, merges
    neg = pl.copy()
    neg[neg == 0] = -0.0
    add(pl, mk), add(neg, mk), add(pl, mk)
    pl, mk = position()                                              # members without a policy: the c_p rule
    zero = np.zeros(220, np.float32)
    add(pl, mk), add(pl, mk, pol=zero), add(pl, mk)
    pl, mk = position()
    add(pl, mk, pol=zero), add(pl, mk, pol=zero)
    pl, mk = position()                                              # a lone row with an odd policy: a bit copy
    odd = zero.copy()
    odd[::3] = -0.0
    add(pl, mk, pol=odd)
    order = rng.permutation(len(rows))
    cols = [np.stack([rows[i][j] for i in order]) for j in range(5)]
    return {"planes": np.ascontiguousarray(cols[0].reshape(-1, 11, 6, 6)), "masks": np.ascontiguousarray(cols[1], np.uint8),
            "policy": np.ascontiguousarray(cols[2], np.float32), "value": cols[3].astype(np.float32),
            "soft": cols[4].astype(np.float32)}
