"""Numpy restatement of merging duplicate positions across the replay window, record to record
(liuzhou_amd/replay_window.py, csrc/lz_replay_merge.h).  Nothing new is restated: the records are
decoded (`replay_ref.decode_records`), keyed, grouped and merged as rows (`tests/position_dedup.py`) and the merged rows
written as records again (`replay_ref.make_record`).  Plus the records of the tests: the synthetic grid as records and a
ring of hand-built edge records."""
import numpy as np

from liuzhou_amd import symmetry as SY
from tests import position_dedup as PD
from tests.replay_ref import RECORD_BYTES, decode_records, make_record

INT64_MIN = -(1 << 63)
FULL = (1 << 36) - 1


# ---- rows -> records (what lz_pack_trajectory_rows writes) ------------------------------------------------------------
def pack_row(planes, mask, policy_bits, value_bits, soft_bits):
    """(record uint8[360], representable) of one row: planes float32[11,36], mask [220], policy as u32 bit patterns
    [220], value / soft as u32 bit patterns.  The first 72 legal actions' slots; more than 72 legal actions, planes that
    are not 0/1 or policy mass off the legal set make the row not representable."""
    pl = np.asarray(planes, np.float32).reshape(11, 36)
    nz = pl != 0
    words = [sum(1 << c for c in range(36) if nz[p, c]) for p in range(4)]
    phase = 0
    for ph in range(1, 8):
        if nz[3 + ph].any():
            phase = ph
    words[0] |= phase << 36
    legal = np.flatnonzero(np.asarray(mask).reshape(220) != 0)
    mask_words = [0] * 7
    for a in legal:
        mask_words[a // 32] |= 1 << (a % 32)
    bits = np.asarray(policy_bits, np.uint32).reshape(220)
    rec = make_record(words, mask_words, [int(bits[a]) for a in legal[:72]], 0.0, 0.0)
    rec[348:352] = np.frombuffer(np.uint32(value_bits).tobytes(), np.uint8)
    rec[352:356] = np.frombuffer(np.uint32(soft_bits).tobytes(), np.uint8)
    _, _, ok = PD.read_rows(pl[None])
    off = np.ones(220, bool)
    off[legal] = False
    representable = bool(ok[0]) and len(legal) <= 72 and not (bits.view(np.float32)[off] != 0).any()
    return rec, representable


def pack_rows(rows):
    """uint8[n,360] of a dict of rows (planes, masks, policy, value, soft as tests/position_dedup.grid returns them)."""
    n = len(rows["value"])
    pol = np.ascontiguousarray(rows["policy"], np.float32).view(np.uint32)
    val = np.ascontiguousarray(rows["value"], np.float32).view(np.uint32)
    sof = np.ascontiguousarray(rows["soft"], np.float32).view(np.uint32)
    pl = np.asarray(rows["planes"], np.float32).reshape(n, 11, 36)
    return np.stack([pack_row(pl[i], rows["masks"][i], pol[i], val[i], sof[i])[0] for i in range(n)])


# ---- the two entry points -----------------------------------------------------------------------------------------------
def _decode_positions(records, slots):
    """The rows of the positions in `slots` (an all-zero row where the slot is outside the ring) and which are inside."""
    records = np.asarray(records, np.uint8).reshape(-1, RECORD_BYTES)
    slots = np.asarray(slots, np.int64).reshape(-1)
    m = len(slots)
    inside = (slots >= 0) & (slots < len(records))
    planes = np.zeros((m, 11, 36), np.float32)
    masks = np.zeros((m, 220), np.uint8)
    policy = np.zeros((m, 220), np.uint32)
    value, soft = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
    pos = np.flatnonzero(inside)
    if len(pos):
        uniq, inverse = np.unique(slots[pos], return_inverse=True)
        dp, dm, dq, dv, ds = decode_records(records[uniq])
        planes[pos], masks[pos], policy[pos] = dp.reshape(-1, 11, 36)[inverse], dm[inverse], dq[inverse]
        value[pos], soft[pos] = dv[inverse], ds[inverse]
    return planes, masks, policy, value, soft, inside


def keys_ref(records, slots, symmetric):
    """(keys int64[m,8], sym int8[m], count) that lz_replay_position_keys writes: the keys of the decoded rows; a slot
    outside the ring gives {INT64_MIN | j, 0, ...}, sym 0 and is counted."""
    planes, masks, _, _, _, inside = _decode_positions(records, slots)
    keys, sym, bad = PD.keys(planes, masks, bool(symmetric))
    assert bad == 0                                                  # a record is always representable
    out = np.ascontiguousarray(keys).copy()
    for j in np.flatnonzero(~inside):
        out[j] = 0
        out[j, 0] = INT64_MIN | int(j)
        sym[j] = 0
    return out, sym, int((~inside).sum())


def merge_ref(records, slots, sym, order, begin):
    """(out uint8[groups,360], count int32[groups], not_representable) that lz_replay_merge_records writes: row g of
    `position_dedup.merge_groups` on the decoded rows, packed.  A group with a member outside the ring is a zero record
    like every other bad group."""
    planes, masks, policy, value, soft, inside = _decode_positions(records, slots)
    m, G = len(inside), len(begin) - 1
    sym, order = np.asarray(sym, np.int8), np.asarray(order, np.int64)
    out = np.zeros((G, RECORD_BYTES), np.uint8)
    count = np.zeros(G, np.int32)
    over = 0
    for g in range(G):
        b, e = int(begin[g]), int(begin[g + 1])
        if b < 0 or e <= b or e > m:
            continue
        mem = order[b:e]
        if (mem < 0).any() or (mem >= m).any() or not inside[mem].all():
            continue
        o_pl, o_mk, o_pol, o_val, o_sof, cnt = PD.merge_groups(planes, masks, policy.view(np.float32), value.view(np.float32),
                                                               soft.view(np.float32), sym, order, np.array([b, e], np.int64),
                                                               check_members=False)
        if cnt[0] == 0:
            continue
        legal = np.flatnonzero(o_mk[0])
        bits = np.zeros(220, np.uint32)                              # what pack keeps: the legal actions' entries
        bits[legal] = o_pol[0].view(np.uint32)[legal]
        out[g], _ = pack_row(o_pl[0], o_mk[0], bits, o_val.view(np.uint32)[0], o_sof.view(np.uint32)[0])
        over += len(legal) > 72
        count[g] = cnt[0]
    return out, count, over


def merge_weights_ref(group_of_row, ages, scale, max_weight):
    """w_g = min(sum over the members of scale[age], max_weight) with scale[a] = decay ** a given as float64: members
    counted per (group, age), the products added in ascending age in float64, one Python float at a time."""
    gor = [int(g) for g in group_of_row]
    G = max(gor) + 1 if gor else 0
    ages = [0] * len(gor) if ages is None else [int(a) for a in ages]
    out = np.zeros(G, np.float64)
    for g in range(G):
        total = 0.0
        for a in range(len(scale)):
            total = total + float(sum(1 for j in range(len(gor)) if gor[j] == g and ages[j] == a)) * float(scale[a])
        out[g] = min(total, float(max_weight))
    return out


# ---- the records of the tests ---------------------------------------------------------------------------------------------
def grid_records(seed, spread):
    """tests/position_dedup.grid as records (group sizes 1, 2, 3, 255, 256, 257, 600; members under all eight
    symmetries with `spread`; members without a policy; a lone row with -0.0 entries)."""
    return pack_rows(PD.grid(seed, spread))


def _mask_words(actions):
    words = [0] * 7
    for a in actions:
        words[a // 32] |= 1 << (a % 32)
    return words


def _junk(rec, rng, legal_count):
    """Set every bit the layout does not own: above bit 38 of word 0, above bit 35 of words 1..3, mask bits 220..223,
    the pad bytes and the policy slots at or past the legal count."""
    rec = rec.copy()
    w = rec[:32].view(np.uint64)
    w[0] |= np.uint64(int(rng.integers(0, 1 << 25)) << 39)
    for p in (1, 2, 3):
        w[p] |= np.uint64(int(rng.integers(1, 1 << 28)) << 36)
    rec[32:60].view(np.uint32)[6] |= np.uint32(0xF0000000)
    rec[356:360] = rng.integers(1, 256, 4, dtype=np.uint8)
    slots = rec[60:348].view(np.uint32)
    for r in range(min(legal_count, 72), 72):
        slots[r] = np.uint32(rng.integers(1, 1 << 32))
    return rec


ODD_BITS = (0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7FA00000)


def edge_records(seed):
    """(records, notes): hand-built records.  For every legal count in (0, 1, 71, 72, 73, 220): a lone junk record whose
    legal slots hold -0.0 / NaN payloads / infinities / subnormals, and a position held three times under junk, one copy
    without a policy.  Then for every symmetry k: a position whose first copy stands under k and whose other copies stand
    under all eight; a position whose copies all have a zero policy; and a pair of records that differ in the phase."""
    rng = np.random.default_rng(seed)
    recs, notes = [], []

    def position(n_legal):
        boards = [int(x) for x in rng.integers(0, 1 << 36, 4, dtype=np.uint64)]
        actions = sorted(rng.choice(220, n_legal, replace=False).tolist())
        return boards, int(rng.integers(0, 8)), actions

    def record(boards, phase, actions, policy, value, soft):
        words = list(boards)
        words[0] |= phase << 36
        return make_record(words, _mask_words(actions), policy[:72], value, soft)

    for n_legal in (0, 1, 71, 72, 73, 220):
        boards, phase, actions = position(n_legal)
        odd = [ODD_BITS[i % len(ODD_BITS)] for i in range(min(n_legal, 72))]
        lone = record(boards, phase, actions, odd, 0.0, 0.0)
        lone[348:352] = np.frombuffer(np.uint32(0x7FC0ABCD).tobytes(), np.uint8)
        lone[352:356] = np.frombuffer(np.uint32(0x80000000).tobytes(), np.uint8)
        recs.append(_junk(lone, rng, n_legal))
        notes.append(("lone", n_legal))
        boards, phase, actions = position(n_legal)
        for copy in range(3):
            pol = [float(x) for x in rng.random(min(n_legal, 72)).astype(np.float32)] if copy != 1 else [0.0] * min(n_legal, 72)
            recs.append(_junk(record(boards, phase, actions, pol, float(rng.integers(-1, 2)), float(rng.uniform(-1, 1))),
                              rng, n_legal))
            notes.append(("triple", n_legal))
    for k in range(8):                                               # every symmetry as the first member's frame
        boards, phase, actions = position(40)
        pl = PD.make_planes(boards, phase)
        mk = np.zeros(220, np.uint8)
        mk[actions] = 1
        for member in [k] + list(range(8)):
            tp, tm, _ = SY.np_transform_samples(pl.reshape(1, 11, 6, 6), mk[None], np.zeros((1, 220), np.float32), member)
            pol = np.zeros(220, np.float32)
            on = np.flatnonzero(tm[0])
            pol[on] = rng.random(len(on)).astype(np.float32)
            rec, ok = pack_row(tp[0].reshape(11, 36), tm[0], pol.view(np.uint32), np.float32(rng.integers(-1, 2)).view(np.uint32),
                               np.float32(rng.uniform(-1, 1)).view(np.uint32))
            assert ok
            recs.append(rec)
            notes.append(("frames", k))
    boards, phase, actions = position(9)                             # no copy has a policy: c_p = 0
    for _ in range(3):
        recs.append(record(boards, phase, actions, [0.0] * 9, 1.0, 0.5))
        notes.append(("no policy", 9))
    boards, phase, actions = position(5)                             # equal boards and legal set, another phase
    for ph in (phase, (phase + 1) % 8):
        recs.append(record(boards, ph, actions, [0.2] * 5, -1.0, -0.25))
        notes.append(("phase", ph))
    order = rng.permutation(len(recs))
    return np.stack([recs[i] for i in order]), [notes[i] for i in order]
