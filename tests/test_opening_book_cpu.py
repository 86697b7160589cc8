"""CPU: the opening book without a device -- tests/opening_book_ref.py (numpy / Python integers on the host scalar rule
engine) against the host build of lz_opening_book_keys / lz_states_from_packed (csrc/lz_opening_book_host.cpp over
csrc/lz_opening_book.h, the header the kernels include), each validity clause on its own, `OpeningBook`,
`assign_openings` and `paired_statistics`.  Everything but the statistics is integers and bytes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import opening_book_ref as R
from tests import start_bank_ref as S

@pytest.fixture(scope="module")
def L():
    from liuzhou_amd import _lib
    _lib.host_lib()
    return _lib


def one(L, rec, lo=0, hi=143):
    """(valid, key, sym) of one record from the host build, checked against the restatement on the way."""
    v, k, s = R.run_keys(L, L.host_lib(), "cpu", [rec], lo, hi)
    return int(v[0]), tuple(int(x) for x in k[0]), int(s[0])


# ---- the pool ------------------------------------------------------------------------------------------------------------------
def test_the_walks_cover_the_phases_and_pack_like_the_numpy_codec():
    p = R.pool()
    assert len(p) > 400 and {R.meta_of(r[0])["phase"] for r in p} >= {1, 2, 3, 4, 5}
    packed = R.to_bytes(p)
    assert np.array_equal(S.pack_states(S.unpack_states(packed)), packed)          # canonical under the other codec too
    assert all(R.valid_ref(r, 0, 143) for r in p)                                  # every walked position is playable


# ---- keys ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.SIZES)
def test_host_keys_equal_the_restatement(L, m):
    words = R.mixed_records(m)
    v, _k, _s = R.run_keys(L, L.host_lib(), "cpu", words)
    if m >= 63:
        assert 0 < int(v.sum()) < m                                                # the mix is mixed
    R.run_keys(L, L.host_lib(), "cpu", words, 10, 40)


def test_the_eight_images_share_one_key_and_their_sym_carries_each_to_the_same_image(L):
    from liuzhou_amd.symmetry import transform_packed
    for rec in R.playable()[::53][:8]:
        base = torch.from_numpy(R.to_bytes([rec]).view(np.int64).reshape(1, 4).copy())
        images = transform_packed(base.repeat(8, 1), torch.arange(8, dtype=torch.int8))
        words = R.to_words(images.numpy().view(np.uint8).reshape(8, 32))
        assert words == [R.sym_record(k, rec) for k in range(8)]                   # the library's images are the restatement's
        v, k, s = R.run_keys(L, L.host_lib(), "cpu", words)
        assert v.tolist() == [1] * 8 and len({tuple(row) for row in k.tolist()}) == 1
        carried = transform_packed(images, torch.from_numpy(s.copy()))
        boards = carried.numpy().view(np.uint64) & np.uint64(R.FULL)
        assert (boards == boards[0]).all()
        assert [int(x) for x in boards[0]] == [int(k[0, 0]) & R.FULL] + [int(x) for x in k[0, 1:]]


def test_what_is_and_is_not_part_of_the_key(L):
    rec = next(r for r in R.playable() if R.meta_of(r[0])["phase"] == 4)
    m = R.meta_of(rec[0])
    v0, k0, s0 = one(L, rec)
    assert v0 == 1
    for other in (R.with_fields(rec, move_count=m["move_count"] + 3), R.with_fields(rec, msc=(m["msc"] + 5) % 30),
                  R.with_fields(rec, move_count=m["move_count"] - 2, msc=0)):
        assert one(L, other) == (1, k0, s0)                                        # how it was reached: one opening
    v, k, _ = one(L, R.with_fields(rec, player=-m["player"]))
    assert v == 1 and k != k0 and k[1:] == k0[1:] and (k[0] ^ k0[0]) == 1 << (36 + 3)          # the player bit alone
    v, k, _ = one(L, R.with_fields(rec, phase=7))
    assert v == 1 and k != k0 and k[1:] == k0[1:] and (k[0] ^ k0[0]) >> 36 == (4 ^ 7)          # the phase alone


# ---- each validity clause on its own -----------------------------------------------------------------------------------------------
def invalid(row):
    return (0, (R.NO_KEY | row, 0, 0, 0), 0)


def test_a_zero_record_is_invalid(L):
    assert one(L, (0, 0, 0, 0)) == invalid(0)


def test_an_unowned_bit_makes_a_record_invalid(L):
    """Words 1..3 own bits 0..35.  Word 0 owns all 64 of its bits (36 cells, 8 + 6 counter bits, 14 bits of metadata), so it
    has no bit to set: packing the unpacked record returns every word 0 unchanged."""
    rec = R.playable()[40]
    assert one(L, rec)[0] == 1
    for w in (1, 2, 3):
        for bit in (36, 50, 63):
            bad = list(rec)
            bad[w] |= 1 << bit
            assert one(L, tuple(bad)) == invalid(0), (w, bit)
    r = np.random.default_rng(3)
    w0 = r.integers(0, 1 << 63, 64, dtype=np.uint64) * np.uint64(2) + r.integers(0, 2, 64, dtype=np.uint64)
    raw = np.zeros((64, 4), np.uint64)
    raw[:, 0] = w0
    packed = np.ascontiguousarray(raw.astype("<u8")).view(np.uint8).reshape(64, 32)
    assert np.array_equal(S.pack_states(S.unpack_states(packed)), packed)


def test_overlapping_boards_are_invalid(L):
    rec = next(r for r in R.playable() if r[0] & R.FULL)
    low = (rec[0] & R.FULL) & -(rec[0] & R.FULL)
    assert one(L, rec)[0] == 1 and one(L, (rec[0], rec[1] | low, rec[2], rec[3])) == invalid(0)


def test_a_finished_game_of_each_status_is_invalid(L):
    fin = R.finished_records()
    assert [R.status(R.cstate(fin[k])) for k in (1, -1, 2, "msc")] == [1, -1, 2, 2]
    for k in (1, -1, 2, "msc"):
        assert one(L, fin[k], 0, 255) == invalid(0), k                             # the move range admits all of them


def test_a_position_without_a_legal_action_is_invalid(L):
    """The walks never stop at one (a player without a movement removes a piece instead), so this one is hand-built: a mark
    selection with no mark left to make."""
    rec = R.no_legal_record()
    cs = R.cstate(rec)
    assert R.status(cs) == 0 and R.legal_moves(cs) == []
    assert one(L, rec) == invalid(0)
    assert one(L, R.with_fields(rec, pm_rem=1))[0] == 1                            # with a mark to make it is playable


def test_move_count_one_outside_each_end_of_the_range(L):
    rec = next(r for r in R.playable() if R.meta_of(r[0])["move_count"] == 12)
    assert one(L, rec, 12, 12)[0] == 1 and one(L, rec, 0, 12)[0] == 1 and one(L, rec, 12, 143)[0] == 1
    assert one(L, rec, 13, 143) == invalid(0) and one(L, rec, 0, 11) == invalid(0)
    assert one(L, R.with_fields(rec, move_count=11), 12, 20) == invalid(0)
    assert one(L, R.with_fields(rec, move_count=21), 12, 20) == invalid(0)
    assert one(L, R.with_fields(rec, move_count=20), 12, 20)[0] == 1


def test_invalid_records_get_keys_of_their_own_rows(L):
    _v, k, _s = R.run_keys(L, L.host_lib(), "cpu", [(0, 0, 0, 0)] * 5)
    assert k[:, 0].tolist() == [R.NO_KEY | i for i in range(5)] and not k[:, 1:].any()


# ---- lz_states_from_packed -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
def test_host_states_from_packed_equals_the_restatement(L, n):
    words = R.playable(0)[:97]
    r = np.random.default_rng(n)
    index = r.integers(0, len(words), n)
    outside = r.random(n) < 0.2
    index[outside] = r.choice([-1, len(words), -(1 << 40), 1 << 40], int(outside.sum()))
    if n >= 2:
        index[0], index[-1] = -1, len(words)
    ts, hit = R.run_from_packed(L, L.host_lib(), "cpu", words, [int(i) for i in index], rows=n + 3)
    if hit:                                                                        # the pack round trip, byte for byte
        rows = torch.tensor(hit)
        st = dict(zip(S.FIELDS, (t.index_select(0, rows).numpy() for t in ts)))
        assert np.array_equal(S.pack_states(st), R.to_bytes([words[int(index[g])] for g in hit]))


def test_host_states_from_packed_with_more_rows_than_records_and_fewer(L):
    words = R.playable(0)[:5]
    R.run_from_packed(L, L.host_lib(), "cpu", words, [4, 0, 0, 5, 3, -1, 2, 1, 4, 4, 6], rows=11)
    R.run_from_packed(L, L.host_lib(), "cpu", R.playable(0)[:64], [63, 7], rows=2)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_host_argument_refusals(L):
    R.check_argument_refusals(L, L.host_lib(), "cpu")


def test_the_abi_declares_both_entry_points(L):
    for name in ("lz_opening_book_keys", "lz_states_from_packed"):
        assert name in L.SYMBOLS and name in L.HOST_SYMBOLS
    assert len(L.DECLS["lz_opening_book_keys"][1]) == 8 and len(L.DECLS["lz_states_from_packed"][1]) == 6
    from liuzhou_amd.build import HOST_SOURCES, SOURCES
    assert "lz_opening_book.hip" in SOURCES and any(p.endswith("lz_opening_book_host.cpp") for p in HOST_SOURCES)


# ---- OpeningBook ---------------------------------------------------------------------------------------------------------------
def bank_words():
    """A bank with duplicates, symmetric duplicates, copies reached another way and invalid rows; A..D are distinct
    openings at move counts >= 6."""
    p = R.playable()
    a, b, c, d = p[3], p[90], p[200], p[333]
    ma = R.meta_of(a[0])
    return [a, b, a, R.sym_record(3, a), (0, 0, 0, 0), c, R.with_fields(b, msc=(R.meta_of(b[0])["msc"] + 1) % 30),
            (c[0], c[1] | 1 << 40, c[2], c[3]), R.sym_record(6, c), d, R.with_fields(a, move_count=ma["move_count"] + 2),
            R.finished_records()[1]]


def test_from_packed_keeps_the_predicted_rows_in_order_and_its_counts_add_up():
    from liuzhou_amd.opening_book import OpeningBook
    words = bank_words()
    rows, counts = R.book_rows_ref(words, 6, 143)
    assert rows == [0, 1, 5, 9] and counts == dict(seen=12, invalid=3, duplicate=5, truncated=0, kept=4)
    book = OpeningBook.from_packed(torch.from_numpy(R.to_bytes(words)), min_move=6)
    assert len(book) == 4 and book.positions.dtype == torch.uint8 and tuple(book.positions.shape) == (4, 32)
    assert np.array_equal(book.positions.numpy(), R.to_bytes([words[i] for i in rows]))
    assert book.move_counts.tolist() == [R.meta_of(words[i][0])["move_count"] for i in rows]
    m = book.meta
    assert {k: m[k] for k in counts} == counts and m["seen"] == m["invalid"] + m["duplicate"] + m["truncated"] + m["kept"]
    assert m["format"] == "lz_opening_book_v1" and (m["min_move"], m["max_move"], m["max_positions"]) == (6, 143, None)
    # the move window is part of validity: a window that admits only some rows
    lo = sorted(R.meta_of(words[i][0])["move_count"] for i in rows)[2]
    rows2, counts2 = R.book_rows_ref(words, lo, 143)
    book2 = OpeningBook.from_packed(torch.from_numpy(R.to_bytes(words)), min_move=lo)
    assert np.array_equal(book2.positions.numpy(), R.to_bytes([words[i] for i in rows2])) and 0 < len(book2) < 4
    assert {k: book2.meta[k] for k in counts2} == counts2


def test_max_positions_truncates_and_an_empty_input_gives_an_empty_book():
    from liuzhou_amd.opening_book import OpeningBook
    words = bank_words()
    book = OpeningBook.from_packed(torch.from_numpy(R.to_bytes(words)), min_move=6, max_positions=3)
    assert np.array_equal(book.positions.numpy(), R.to_bytes([words[i] for i in (0, 1, 5)]))
    assert (book.meta["kept"], book.meta["truncated"], book.meta["duplicate"], book.meta["invalid"]) == (3, 1, 5, 3)
    empty = OpeningBook.from_packed(torch.zeros((0, 32), dtype=torch.uint8))
    assert len(empty) == 0 and empty.meta["seen"] == 0 and empty.meta["kept"] == 0
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            OpeningBook.from_packed(torch.from_numpy(R.to_bytes(words)), max_positions=bad)
    with pytest.raises(ValueError):
        OpeningBook.from_packed(torch.zeros((3, 31), dtype=torch.uint8))
    with pytest.raises(ValueError):
        OpeningBook.from_packed(torch.from_numpy(R.to_bytes(words)), min_move=9, max_move=8)


def test_from_bank_reads_the_filled_rows_only():
    from liuzhou_amd.opening_book import OpeningBook
    from liuzhou_amd.start_bank import StartBank
    words = bank_words()
    bank = StartBank(32, "cpu")
    bank.append_packed(torch.from_numpy(R.to_bytes(words)))
    book = OpeningBook.from_bank(bank, min_move=6)
    assert np.array_equal(book.positions.numpy(), R.to_bytes([words[i] for i in (0, 1, 5, 9)]))
    assert book.meta["seen"] == 12                                                 # not the 20 zero rows behind them
    assert len(OpeningBook.from_bank(StartBank(8, "cpu"))) == 0


def test_save_and_load_round_trip_and_a_wrong_file_is_refused(tmp_path):
    from liuzhou_amd.opening_book import OpeningBook
    book = OpeningBook.from_packed(torch.from_numpy(R.to_bytes(bank_words())), min_move=6)
    path = str(tmp_path / "book.pt")
    book.save(path)
    back = OpeningBook.load(path, "cpu")
    assert torch.equal(back.positions, book.positions) and torch.equal(back.move_counts, book.move_counts)
    assert back.meta == book.meta
    good = torch.load(path, weights_only=True)
    assert set(good) == {"format", "positions", "move_counts", "meta"}
    for name, bad in (("tag", {**good, "format": "lz_opening_book_v0"}), ("no tag", {k: v for k, v in good.items() if k != "format"}),
                      ("shape", {**good, "positions": good["positions"][:, :31].contiguous()}),
                      ("dtype", {**good, "positions": good["positions"].to(torch.int16)}),
                      ("counts", {**good, "move_counts": good["move_counts"][:3]}),
                      ("count values", {**good, "move_counts": good["move_counts"] + 1}),
                      ("count dtype", {**good, "move_counts": good["move_counts"].to(torch.int32)}),
                      ("meta", {**good, "meta": [1, 2]}), ("not a dict", good["positions"])):
        other = str(tmp_path / "bad.pt")
        torch.save(bad, other)
        with pytest.raises(ValueError):
            OpeningBook.load(other, "cpu")


# ---- assign_openings -----------------------------------------------------------------------------------------------------------
def test_assign_openings_is_a_pure_function_that_uses_every_opening_before_it_repeats_one():
    from liuzhou_amd.opening_book import assign_openings
    for B, P in ((4, 6), (7, 7), (5, 3), (1, 4), (100, 100), (9, 40), (3, 0)):
        torch.manual_seed(B)                                                       # the global generator plays no part
        a = assign_openings(B, P, 11)
        torch.manual_seed(P + 100)
        assert a.dtype == torch.int64 and tuple(a.shape) == (P,) and torch.equal(a, assign_openings(B, P, 11))
        counts = torch.bincount(a, minlength=B)
        assert int(counts.sum()) == P and set(counts.tolist()) <= {P // B, -(-P // B)}
        if P <= B:
            assert len(set(a.tolist())) == P
        for lo in range(0, P - B + 1, B):                                          # every full cycle is a permutation
            assert sorted(a[lo:lo + B].tolist()) == list(range(B))
    assert not torch.equal(assign_openings(100, 100, 1), assign_openings(100, 100, 2))
    assert torch.equal(assign_openings(9, 40, 5)[:9], assign_openings(9, 9, 5))
    with pytest.raises(ValueError):
        assign_openings(0, 4, 0)


# ---- paired_statistics ---------------------------------------------------------------------------------------------------------
def stats_ref(first, second):
    """The same statistics from the per-pair scores: mean and population variance of (x + y) / 2 over the pairs."""
    s = (np.asarray(first, np.float64) + np.asarray(second, np.float64)) / 2.0
    P = s.size
    score, se = float(s.mean()), float(math.sqrt(((s - s.mean()) ** 2).mean() / P))
    elo = lambda x: None if not 0.0 < x < 1.0 else -400.0 * math.log10(1.0 / x - 1.0)
    g = np.concatenate([np.asarray(first, np.float64), np.asarray(second, np.float64)])
    los = 0.5 * (1.0 + math.erf((score - 0.5) / (se * math.sqrt(2.0)))) if se > 0 else (1.0 if score > 0.5 else 0.0 if score < 0.5 else 0.5)
    return dict(pairs=P, pentanomial=np.bincount(np.rint(4 * s).astype(int), minlength=5).tolist(), score=score, score_stderr=se,
                elo=elo(score), elo_ci95=[elo(score - 1.959964 * se), elo(score + 1.959964 * se)], los=los,
                trinomial_stderr=float(math.sqrt(((g - g.mean()) ** 2).mean() / g.size)))


def close(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        if isinstance(w, list):
            assert len(g) == len(w) and all((a is None) == (b is None) and (a is None or abs(a - b) <= 1e-9 * max(1.0, abs(b)))
                                            for a, b in zip(g, w)), (k, g, w)
        elif w is None or isinstance(w, int):
            assert g == w, (k, g, w)
        else:
            assert abs(g - w) <= 1e-12 * max(1.0, abs(w)), (k, g, w)


def test_paired_statistics_of_all_wins_all_losses_and_all_split_pairs():
    from liuzhou_amd.opening_book import paired_statistics
    win = paired_statistics([1.0] * 5, [1.0] * 5)
    assert win["pentanomial"] == [0, 0, 0, 0, 5] and win["score"] == 1.0 and win["score_stderr"] == 0.0
    assert win["elo"] is None and win["elo_ci95"] == [None, None] and win["los"] == 1.0 and win["trinomial_stderr"] == 0.0
    loss = paired_statistics(torch.zeros(5), torch.zeros(5))
    assert loss["pentanomial"] == [5, 0, 0, 0, 0] and loss["score"] == 0.0 and loss["elo"] is None and loss["los"] == 0.0
    # every pair split 1 - 0: each opening is won by the side it favours -- the pairing cancels it, independent games do not
    split = paired_statistics([1.0, 0.0, 1.0, 1.0], [0.0, 1.0, 0.0, 0.0])
    assert split["pentanomial"] == [0, 0, 4, 0, 0] and split["score"] == 0.5 and split["score_stderr"] == 0.0
    assert split["los"] == 0.5 and split["elo"] == 0.0 and split["elo_ci95"] == [0.0, 0.0]
    assert split["trinomial_stderr"] == math.sqrt(0.25 / 8) > 0
    for first, second in (([1.0] * 5, [1.0] * 5), ([0.0] * 5, [0.0] * 5), ([1.0, 0.0, 1.0, 1.0], [0.0, 1.0, 0.0, 0.0])):
        close(paired_statistics(first, second), stats_ref(first, second))


def test_paired_statistics_of_a_mixed_case_worked_by_hand():
    """Pairs (1, 1), (1, 1/2), (1/2, 1/2), (0, 1): sums 2, 3/2, 1, 1 -> N = [0, 0, 2, 1, 1], P = 4.
    score = (2 * 1/2 + 3/4 + 1) / 4 = 11/16.  Squared deviations: 2 * (3/16)^2 + (1/16)^2 + (5/16)^2 = 44/256;
    score_stderr = sqrt(44/256 / 4 / 4) = sqrt(11) / 32.  The eight games 1, 1, 1/2, 0, 1, 1/2, 1/2, 1 have mean 11/16 and
    squared deviations 4 * (5/16)^2 + 3 * (3/16)^2 + (11/16)^2 = 248/256; trinomial_stderr = sqrt(248/256 / 8 / 8) =
    sqrt(62) / 64.  elo = -400 log10(16/11 - 1) = 400 log10(11/5)."""
    from liuzhou_amd.opening_book import paired_statistics
    first, second = [1.0, 1.0, 0.5, 0.0], [1.0, 0.5, 0.5, 1.0]
    got = paired_statistics(first, second)
    assert got["pairs"] == 4 and got["pentanomial"] == [0, 0, 2, 1, 1] and sum(got["pentanomial"]) == 4
    assert got["score"] == 11 / 16
    assert abs(got["score_stderr"] - math.sqrt(11) / 32) < 1e-15 and abs(got["trinomial_stderr"] - math.sqrt(62) / 64) < 1e-15
    assert abs(got["elo"] - 400 * math.log10(11 / 5)) < 1e-9
    lo, hi = 11 / 16 - 1.959964 * math.sqrt(11) / 32, 11 / 16 + 1.959964 * math.sqrt(11) / 32
    assert 0 < lo and hi < 1
    assert abs(got["elo_ci95"][0] + 400 * math.log10(1 / lo - 1)) < 1e-9 and abs(got["elo_ci95"][1] + 400 * math.log10(1 / hi - 1)) < 1e-9
    assert abs(got["los"] - 0.5 * (1 + math.erf((3 / 16) / (math.sqrt(11) / 32 * math.sqrt(2))))) < 1e-15
    close(got, stats_ref(first, second))
    r = np.random.default_rng(8)
    for P in (1, 2, 9, 200):
        a, b = r.choice([0.0, 0.5, 1.0], P), r.choice([0.0, 0.5, 1.0], P)
        got = paired_statistics(a, b)
        close(got, stats_ref(a, b))
        assert sum(got["pentanomial"]) == P
    one_sided = paired_statistics([1.0, 1.0, 1.0, 0.5], [1.0, 1.0, 1.0, 1.0])           # the upper end reaches the clip
    assert one_sided["elo_ci95"][1] is None and one_sided["elo_ci95"][0] is not None
    for bad in (([], []), ([1.0], [1.0, 0.0]), ([0.25], [1.0])):
        with pytest.raises(ValueError):
            paired_statistics(*bad)


# ---- the replay the GPU tests judge the arena's games with ---------------------------------------------------------------------------
def test_replay_follows_a_walked_game_to_its_result_and_refuses_a_wrong_log():
    rng = np.random.default_rng(6)
    for rec in R.playable()[::70][:4]:
        cs, log = R.cstate(rec), []
        for _ in range(40):
            moves = R.legal_moves(cs)
            if not moves:
                break
            mv = moves[int(rng.integers(len(moves)))]
            log.append(R.action_index(mv))
            cs = R.apply_move(cs, mv)
        st = R.status(cs)
        want = 0 if st in (0, 2) else st
        assert R.replay(rec, log + [-1, -1], 40) == want
        with pytest.raises(AssertionError):
            R.replay(rec, log[:3] + [217] + log[3:], 40)                           # not an action of any phase
        with pytest.raises(AssertionError):
            R.replay(rec, log[:5] + [-1] + log[5:], 40)                            # a move after the end
        if st == 0:
            with pytest.raises(AssertionError):
                R.replay(rec, log[:5], 40)                                         # stopped while running with a move to make
