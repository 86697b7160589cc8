"""Seeded inputs of the loss and trajectory-codec kernel tests (tests/test_gpu_train_kernels.py), built from classes.
tests/test_train_loss_ref_cpu.py counts every class on the host, so that a GPU run never finds its cases missing, and
oracle/gen_golden.py::gen_loss_edges puts the batch of 64 through the reference's own functions (g21_loss_edges.npz).
Nothing here needs a GPU, the reference or the oracle."""
import numpy as np
import torch

TOTAL = 220
POLICY_SLOTS = 72
# (oracle/gen_golden.py loads this file by its path: it imports no other module of the tests)
MOVE_FROM = np.repeat(np.arange(36), 4)                   # action 36 + 4 * from + direction; up, down, left, right
_R, _C = MOVE_FROM // 6 + np.tile([-1, 1, 0, 0], 36), MOVE_FROM % 6 + np.tile([0, 0, -1, 1], 36)
ON_BOARD = (_R >= 0) & (_R < 6) & (_C >= 0) & (_C < 6)
MOVE_DEST = np.where(ON_BOARD, _R * 6 + _C, -1)

SENT_F32 = 0x7FC12345                                     # a quiet NaN with a marked payload: "nobody wrote here"
GUARD_ROWS = 8

# (soft_label_alpha, anti_draw_penalty, policy_draw_weight): the three of g21, and one with an anti-draw penalty below
# the 1e-9 threshold of the substitution
SETTINGS = ((0.0, 0.0, 1.0), (0.35, -0.15, 0.4), (1.0, -1.5, 0.0))
EXTRA_SETTINGS = ((0.35, 5e-10, 0.4),)
SETTING_TAGS = ("a", "b", "c")
BATCH_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 64, 257)
GRAD_SCALES = (1.0, 3.0, 65536.0)
EDGE_B = 64

BORDER_ACTIONS = (0, 35, 36, 63, 64, 127, 128, 179, 180, 191, 192, 215, 216, 219)   # section and 64-lane slot borders
OFF_BOARD_ACTIONS = tuple(int(36 + m) for m in np.flatnonzero(~ON_BOARD))
ON_BOARD_ACTIONS = tuple(a for a in range(TOTAL) if a not in OFF_BOARD_ACTIONS)
assert 36 in OFF_BOARD_ACTIONS and 179 in OFF_BOARD_ACTIONS and len(ON_BOARD_ACTIONS) == 196

HEAD_SCALES = (1.0, 8.0, 25.0)
MASK_KINDS = ("border", "all_on_board", "single", "none", "aux216", "off_board_company", "off_board_only", "movement",
              "random")
TARGET_KINDS = ("normalised", "empty", "half", "below_gate", "off_board_mass", "off_mask")
VALUES = (0.0, -0.0, 5e-9, -5e-9, 2e-8, -2e-8, 0.37, -0.37, 1.0, -1.0)
PLACED = (0.27, 0.29, 0.99, -0.74, 0.54)                  # u = 63.5, 64.5, 99.5 and the bin centres 13 / 50 - 1, 77 / 50 - 1
SOFT_KINDS = ("as_value", "random", "+1.7", "-1.7", "random")
VLOGIT_KINDS = ("randn2", "randn30", "equal", "pm60000")
WIDE_VLOGITS = ("randn30", "pm60000")
LO_HI_PAIRS = ((63, 64), (64, 65), (99, 100), (100, 100))


def _cycle(kinds, B, rng):
    """Every kind floor(B / len) times at least, in a seeded order."""
    return [kinds[i % len(kinds)] for i in rng.permutation(B)]


def edge_batch(B=EDGE_B, seed=None):
    """-> dict of float32 / uint8 numpy inputs of B rows, and per-row labels (head_scale, mask_kind, target_kind,
    vlogit_kind, value_kind).  Rows are independent: a batch size changes which rows there are, not what a row is like."""
    rng = np.random.default_rng(2100 + B if seed is None else seed)
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    scale = _cycle(HEAD_SCALES, B, rng)
    mkind = _cycle(MASK_KINDS, B, rng)
    tkind = _cycle(TARGET_KINDS, B, rng)
    vkind = _cycle(VALUES + PLACED, B, rng)
    skind = _cycle(SOFT_KINDS, B, rng)
    lkind = _cycle(VLOGIT_KINDS, B, rng)
    big = ("border", "all_on_board", "movement", "random", "off_board_company")
    for i in range(B):                                    # classes that need company
        if tkind[i] == "below_gate":                      # mass on an entry below -50: sharp heads, several legal entries
            scale[i] = 25.0
            if mkind[i] not in big:
                mkind[i] = big[i % len(big)]
        if tkind[i] == "off_board_mass" and mkind[i] not in ("border", "off_board_company", "off_board_only"):
            mkind[i] = ("border", "off_board_company", "off_board_only")[i % 3]
        if mkind[i] == "movement" and tkind[i] == "empty":           # every pair of a movement row carries mass
            tkind[i] = "normalised"

    raw = torch.randn((3, B, 36), generator=g, dtype=torch.float32) * torch.tensor(scale, dtype=torch.float32).view(1, B, 1)
    inf_row = next((i for i in range(B) if mkind[i] == "border" and tkind[i] != "below_gate"), None)
    if inf_row is not None:
        raw[0, inf_row, 0] = float("-inf")                # a head cell that is legal (action 0), next to finite legal entries
    heads = torch.log_softmax(raw, dim=2).numpy()
    lp1, lp2, lpm = heads[0], heads[1], heads[2]

    mask = np.zeros((B, TOTAL), np.uint8)
    target = np.zeros((B, TOTAL), np.float32)
    movement_rows = [i for i in range(B) if mkind[i] == "movement"]
    pairs = np.flatnonzero(ON_BOARD)                      # the 120 on-board (from, direction) pairs
    for i in range(B):
        k = mkind[i]
        if k == "border":
            mask[i, list(BORDER_ACTIONS)] = 1
            mask[i, rng.random(TOTAL) < 0.08] = 1
        elif k == "all_on_board":
            mask[i, list(ON_BOARD_ACTIONS)] = 1
        elif k == "single":
            mask[i, ON_BOARD_ACTIONS[int(rng.integers(len(ON_BOARD_ACTIONS)))]] = 1
        elif k == "aux216":
            mask[i, 216] = 1
        elif k == "off_board_company":
            mask[i, OFF_BOARD_ACTIONS[int(rng.integers(len(OFF_BOARD_ACTIONS)))]] = 1
            mask[i, rng.choice(ON_BOARD_ACTIONS, size=9, replace=False)] = 1
        elif k == "off_board_only":
            mask[i, OFF_BOARD_ACTIONS[int(rng.integers(len(OFF_BOARD_ACTIONS)))]] = 1
        elif k == "movement":                             # shares of the 120 pairs, dealt out over the movement rows
            j = movement_rows.index(i)
            mask[i, 36 + pairs[j::len(movement_rows)]] = 1
        elif k == "random":
            mask[i, rng.random(TOTAL) < 0.12] = 1
            mask[i, 0] = 1
        legal = mask[i] != 0
        t = (rng.random(TOTAL) * 0.98 + 0.02) * legal     # every legal entry carries mass (movement rows: every pair)
        t = t / max(t.sum(), 1e-8)
        k = tkind[i]
        if k == "empty":
            t[:] = 0
        elif k == "half":
            t *= 0.5
        elif k == "below_gate" and legal.any():           # the legal entry with the lowest finite combined logit
            comb = _combined_np(lp1[i], lp2[i], lpm[i])
            cand = np.where(legal & np.isfinite(comb), comb, np.inf)
            t = t * 0.7
            t[int(np.argmin(cand))] += 0.3
        elif k == "off_board_mass":
            off = [a for a in OFF_BOARD_ACTIONS if legal[a]]
            t = t * 0.75
            t[off[0]] += 0.25
        elif k == "off_mask":
            t = t * 0.8
            t[rng.choice(np.flatnonzero(~legal), size=3, replace=False)] += 0.2 / 3
        target[i] = t

    value = np.array(vkind, np.float32)
    soft = (rng.random(B) * 2 - 1).astype(np.float32)
    for i in range(B):
        if skind[i] == "as_value" or vkind[i] in PLACED:
            soft[i] = value[i]                            # mixed = value for alpha 0 and alpha 1 alike
        elif skind[i] in ("+1.7", "-1.7"):
            soft[i] = float(skind[i])

    vlog = np.zeros((B, 101), np.float32)
    for i in range(B):
        if lkind[i] == "randn2":
            vlog[i] = 2 * rng.standard_normal(101)
        elif lkind[i] == "randn30":
            vlog[i] = 30 * rng.standard_normal(101)
        elif lkind[i] == "equal":
            vlog[i] = np.float32(rng.standard_normal() * 3)
        else:                                             # the fp16 range under AMP, on two bins
            a, b = rng.choice(101, size=2, replace=False)
            vlog[i, a], vlog[i, b] = 60000.0, -60000.0
    return dict(lp1=lp1, lp2=lp2, lpm=lpm, vlogits=vlog, mask=mask, target=target, value=value, soft=soft,
                head_scale=np.array(scale, np.float32), mask_kind=np.array(mkind), target_kind=np.array(tkind),
                vlogit_kind=np.array(lkind), soft_kind=np.array(skind), inf_row=-1 if inf_row is None else inf_row)


def _combined_np(l1, l2, l3):
    moves = np.where(ON_BOARD, l2[MOVE_FROM] + l1[np.where(ON_BOARD, MOVE_DEST, 0)], -np.inf)
    return np.concatenate([l1, moves, l3, np.zeros(4, np.float32)]).astype(np.float64)


INPUT_KEYS = ("lp1", "lp2", "lpm", "vlogits", "mask", "target", "value", "soft")


def draws_only_batch(B=5):
    """Hard draws only: with policy_draw_weight 0 the weight sum is 0."""
    c = edge_batch(B, seed=77)
    c["value"] = np.array([0.0, -0.0, 5e-9, -5e-9, 0.0], np.float32)[np.arange(B) % 5]
    return c


def weight_sum_of(value, draw_weight):
    """As liuzhou_amd/train_loss.py forms it: a float32 sum of float32 weights."""
    v = torch.from_numpy(np.asarray(value, np.float32))
    return float(torch.where(v.abs() < 1e-8, float(draw_weight), 1.0).to(torch.float32).sum())


def policy_class(c):
    """Per row: 's25' for the heads of log_softmax(25 * randn), else 'base'."""
    return np.where(c["head_scale"] > 8.0, "s25", "base")


def value_class(c):
    return np.where(np.isin(c["vlogit_kind"], WIDE_VLOGITS), c["vlogit_kind"], "base")


# =========================================================================================================================
# trajectory rows for the codec
# =========================================================================================================================
CODEC_N = (1, 2, 3, 4, 5, 9, 257)
LEGAL_COUNTS_OK = (0, 1, 36, 60, 63, 64, 65, 71, 72)
LEGAL_COUNTS_BAD = (73, 100, 220)
SPECIAL_POLICY_BITS = (0x00000001, 0x7F800000, 0xFF800000, 0x80000000, 0x7FC0BEEF, 0xFFC00001)   # subnormal, +-inf, -0.0, NaNs
NAN_VALUE_BITS, NAN_SOFT_BITS = 0x7FC0CAFE, 0xFFC0F00D
DEFECTS = ("two_phases", "partial_phase", "plane_half", "plane_two", "plane_nan", "policy_off_mask", "two_defects",
           "legal_73", "legal_100", "legal_220")


def _legal_set(count, rng):
    """`count` actions: the slot borders first, the rest at random."""
    first = list(BORDER_ACTIONS)[:count]
    rest = [a for a in rng.permutation(TOTAL) if a not in first]
    return sorted(first + [int(a) for a in rest[:count - len(first)]])


def codec_rows(n, seed=0, defects=True):
    """-> ((planes, legal, policy, value, soft), labels): row r follows recipe r of a fixed cycle; `defects`: include the
    rows that are not representable.  labels[r] is 'ok', 'minus_zero' or the name of the defect."""
    rng = np.random.default_rng(4200 + seed)
    planes = np.zeros((n, 11, 6, 6), np.float32)
    legal = np.zeros((n, TOTAL), np.uint8)
    policy = np.zeros((n, TOTAL), np.float32)
    value = (rng.random(n) * 2 - 1).astype(np.float32)
    soft = (rng.random(n) * 2 - 1).astype(np.float32)
    labels = []
    recipes = ["ok"] * 9 + ["minus_zero"] + (list(DEFECTS) if defects else [])
    for r in range(n):
        label = recipes[r % len(recipes)]
        turn = r // len(recipes)
        planes[r, :4] = rng.random((4, 6, 6)) < 0.4
        phase = (r + turn) % 8                            # 0: no phase plane at all
        if phase:
            planes[r, 3 + phase] = 1.0
        count = LEGAL_COUNTS_OK[(r + turn) % len(LEGAL_COUNTS_OK)]
        if label.startswith("legal_"):
            count = int(label[6:])
        acts = _legal_set(count, rng)
        legal[r, acts] = (1, 2, 255)[r % 3]
        pol = rng.random(len(acts)).astype(np.float32) + np.float32(1e-3)
        pol /= max(pol.sum(), 1)
        bits = pol.view(np.uint32).copy()
        for j, b in enumerate(SPECIAL_POLICY_BITS):       # on legal entries: carried bit for bit
            if len(acts) > j and r % 2 == 0:
                bits[(j * 11 + r) % len(acts)] = b
        policy[r].view(np.uint32)[acts] = bits
        if r % 5 == 3:
            value[r:r + 1].view(np.uint32)[:] = NAN_VALUE_BITS
            soft[r:r + 1].view(np.uint32)[:] = NAN_SOFT_BITS
        off = [a for a in range(TOTAL) if a not in acts]
        if label == "minus_zero":                         # equal to zero: packed as zero, comes back as +0.0, no count
            planes[r, 1, 2, 3] = -0.0
            planes[r, 5 if phase != 2 else 6, 0, 0] = -0.0
            if off:
                policy[r, off[0]] = -0.0
        elif label == "two_phases":
            planes[r, 4 + (phase % 7)] = 1.0
            planes[r, 4 + ((phase + 2) % 7)] = 1.0
        elif label == "partial_phase":
            planes[r, 4:] = 0
            planes[r, 4 + r % 7, :3] = 1.0
        elif label == "plane_half":
            planes[r, 2, 1, 1] = 0.5
        elif label == "plane_two":
            planes[r, 0, 5, 5] = 2.0
        elif label == "plane_nan":
            planes[r, 3, 0, 4] = np.nan
        elif label == "policy_off_mask":
            policy[r, off[len(off) // 2]] = 0.25
        elif label == "two_defects":                      # counts once
            planes[r, 1, 0, 0] = 0.5
            policy[r, off[0]] = 1e-30
        labels.append(label)
    return (planes, legal, policy, value, soft), np.array(labels)


def random_records(n, seed=0):
    """Seeded random bytes with the mask words drawn so that every record has at most 72 of its 224 mask bits set."""
    rng = np.random.default_rng(4300 + seed)
    rec = rng.integers(0, 256, size=(n, 360), dtype=np.uint8)
    for s in range(n):
        bits = np.zeros(224, np.uint8)
        bits[rng.choice(224, size=int(rng.integers(0, POLICY_SLOTS + 1)), replace=False)] = 1
        if s % 4 == 0:
            bits[:] = 0
            bits[rng.choice(224, size=POLICY_SLOTS, replace=False)] = 1
        rec[s, 32:60] = np.packbits(bits, bitorder="little")
    return rec


def mask_bits_of(records):
    """Number of set bits among the 224 mask bits of each record."""
    return np.unpackbits(np.ascontiguousarray(records[:, 32:60]), axis=1).sum(axis=1)


def overfull_records(n=9, seed=0):
    """Random records of which rows 0 and 3 hold 73 and 220 legal bits.  Each is followed by at least three more records of
    the same buffer (n - 1 - row >= 3): an unpack without the slot bound reads at most 220 * 4 + 60 = 940 < 3 * 360 bytes
    past the start of its record's policy, that is a neighbouring record, never outside the buffer."""
    rec = random_records(n, seed=100 + seed)
    rows = {0: 73, 3: 220}
    rng = np.random.default_rng(4400 + seed)
    for row, count in rows.items():
        assert n - 1 - row >= 3
        bits = np.zeros(224, np.uint8)
        bits[rng.choice(220, size=count, replace=False)] = 1
        rec[row, 32:60] = np.packbits(bits, bitorder="little")
    return rec, rows
