"""GPU: the opening book -- lz_opening_book_keys and lz_states_from_packed (csrc/lz_opening_book.hip) through the C ABI
against tests/opening_book_ref.py at wave and block edges, and the arena playing colour-swapped pairs from a book: the
games are replayed move by move from their openings with the host scalar rules."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import opening_book_ref as R
from tests import start_bank_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLIES = 60


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def L():
    from liuzhou_amd import _lib
    return _lib


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.SIZES)
def test_keys_kernel_equals_the_restatement(L, m):
    _need_gpu()
    words = R.mixed_records(m)
    v, _k, _s = R.run_keys(L, L.lib(), DEV, words)
    if m >= 63:
        assert 0 < int(v.sum()) < m
    R.run_keys(L, L.lib(), DEV, words, 10, 40)


def test_keys_kernel_on_each_kind_of_invalid_record(L):
    _need_gpu()
    fin, rec = R.finished_records(), R.playable()[40]
    low = (rec[0] & R.FULL) & -(rec[0] & R.FULL)
    words = [(0, 0, 0, 0), (rec[0], rec[1] | 1 << 36, rec[2], rec[3]), (rec[0], rec[1], rec[2] | 1 << 63, rec[3]),
             (rec[0], rec[1], rec[2], rec[3] | 1 << 50), (rec[0], rec[1] | low, rec[2], rec[3]), fin[1], fin[-1], fin[2],
             fin["msc"], R.no_legal_record(), R.with_fields(rec, move_count=100), rec]
    v, k, _s = R.run_keys(L, L.lib(), DEV, words, 0, 255)
    assert v.tolist() == [0] * 10 + [1, 1] and k[:10, 0].tolist() == [R.NO_KEY | i for i in range(10)]
    v, _k, _s = R.run_keys(L, L.lib(), DEV, words, 0, 99)                          # one past the range's end
    assert v.tolist() == [0] * 11 + [1]


def test_keys_kernel_gives_the_eight_images_one_key(L):
    _need_gpu()
    words = [R.sym_record(k, rec) for rec in R.playable()[::61][:9] for k in range(8)]
    v, k, s = R.run_keys(L, L.lib(), DEV, words)
    assert v.all()
    for i in range(0, len(words), 8):
        assert len({tuple(row) for row in k[i:i + 8].tolist()}) == 1
        carried = [R.sym_record(int(s[i + j]), words[i + j]) for j in range(8)]
        assert len({tuple(w & R.FULL for w in c) for c in carried}) == 1


@pytest.mark.parametrize("n", R.SIZES)
def test_states_from_packed_kernel_equals_the_restatement_and_packs_back(L, n):
    _need_gpu()
    words = R.playable(0)[:97]
    r = np.random.default_rng(n)
    index = r.integers(0, len(words), n)
    outside = r.random(n) < 0.2
    index[outside] = r.choice([-1, len(words), -(1 << 40), 1 << 40], int(outside.sum()))
    if n >= 2:
        index[0], index[-1] = -1, len(words)
    ts, hit = R.run_from_packed(L, L.lib(), DEV, words, [int(i) for i in index], rows=n + 3)
    if hit:                                                                        # lz_pack_states is its inverse
        packed = torch.full((n + 3, 4), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device=DEV)
        L.check(L.lib().lz_pack_states(C.byref(L.soa(ts)), L.i64(n + 3), L.ptr(packed), L.stream_ptr(torch.device(DEV))),
                "pack_states")
        got = packed.cpu().numpy().view(np.uint8).reshape(n + 3, 32)[hit]
        assert np.array_equal(got, R.to_bytes([words[int(index[g])] for g in hit]))


def test_states_from_packed_kernel_with_more_rows_than_records_and_fewer(L):
    _need_gpu()
    R.run_from_packed(L, L.lib(), DEV, R.playable(0)[:5], [4, 0, 0, 5, 3, -1, 2, 1, 4, 4, 6] * 30, rows=331)
    R.run_from_packed(L, L.lib(), DEV, R.playable(0)[:300], [299, 7], rows=2)


def test_kernel_argument_refusals(L):
    _need_gpu()
    R.check_argument_refusals(L, L.lib(), DEV)


# ---- the arena -----------------------------------------------------------------------------------------------------------------
def _model(seed, config="b6c64"):
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    m = ChessNet(**MODEL_CONFIGS[config])
    stable_resnet_init(m, seed)
    return m.eval()


def book_words():
    return R.playable()[::70][:4]


@pytest.fixture(scope="module")
def book():
    _need_gpu()
    from liuzhou_amd.opening_book import OpeningBook
    b = OpeningBook.from_packed(torch.from_numpy(R.to_bytes(book_words())).to(DEV), min_move=6)
    assert len(b) == 4 and b.device.type == "cuda" and int(b.move_counts.min()) >= 6
    assert np.array_equal(b.positions.cpu().numpy(), R.to_bytes(book_words()))
    return b


@pytest.fixture(scope="module")
def tree_agents():
    _need_gpu()
    from liuzhou_amd.eval_arena import TreeSearchAgent
    return [TreeSearchAgent(_model(s), DEV, 8) for s in (20260314, 7, 8)]


def _trim(log):
    keep = (log >= 0).any(dim=0).nonzero().view(-1)
    return log[:, : int(keep.max()) + 1] if keep.numel() else log[:, :0]


def check_match(stats, games, seed, max_plies=PLIES):
    """Seating, colours, legality, results and pair statistics of one match played from book_words()."""
    from liuzhou_amd.opening_book import assign_openings, paired_statistics
    half, words = games // 2, book_words()
    want = assign_openings(4, half, seed)
    assert stats.openings.dtype == torch.int64 and stats.openings.tolist() == want.tolist() * 2
    log = stats.move_log.cpu().numpy()
    assert log.shape[0] == games
    black = [R.replay(words[int(stats.openings[g])], log[g], max_plies) for g in range(games)]
    # the challenger is black in the first game of a pair and white in the second
    res = [black[g] if g < half else -black[g] for g in range(games)]
    assert (stats.wins, stats.losses, stats.draws) == (res.count(1), res.count(-1), res.count(0))
    cb = stats.color_breakdown
    assert cb["black"]["games"] == cb["white"]["games"] == half
    assert cb["black"]["wins"] == res[:half].count(1) and cb["white"]["wins"] == res[half:].count(1)
    points = [(r + 1) / 2 for r in res]
    p = stats.paired
    assert sum(p["pentanomial"]) == half == p["pairs"]
    counts = [0] * 5
    for g in range(half):
        counts[int(2 * (points[g] + points[g + half]))] += 1
    assert p["pentanomial"] == counts
    want_stats = paired_statistics(points[:half], points[half:])
    assert {k: p[k] for k in want_stats} == want_stats
    assert p["book_size"] == 4 and p["openings_used"] == min(4, half)
    mc = [R.meta_of(words[int(e)][0])["move_count"] for e in want.tolist()]
    assert abs(p["opening_move_mean"] - sum(mc) / len(mc)) < 1e-12
    assert set(stats.to_payload("x")) >= {"paired", "wins", "color_breakdown"}
    return res


def test_tree_arena_plays_colour_swapped_pairs_from_the_book(book, tree_agents):
    _need_gpu()
    from liuzhou_amd.eval_arena import play_matches
    a, b = tree_agents[:2]
    kw = dict(max_game_plies=PLIES, record_moves=True, opening_book=book, opening_seed=3)
    joint = play_matches(a, b, 12, DEV, joint=True, **kw)
    check_match(joint, 12, 3)
    # 6 pairs on 4 entries: every entry is used, two of them twice
    assert sorted(torch.bincount(joint.openings[:6], minlength=4).tolist()) == [1, 1, 2, 2]
    # deterministic agents: games of one opening and one colour assignment are one game, other openings other games
    first = [bytes(row) for row in joint.move_log[:6].cpu().numpy()]
    assert len(set(first)) == 4 and all((first[p] == first[q]) == (int(joint.openings[p]) == int(joint.openings[q]))
                                        for p in range(6) for q in range(6))
    alone = play_matches(a, b, 12, DEV, joint=False, **kw)
    assert torch.equal(_trim(joint.move_log), _trim(alone.move_log)) and alone.paired == joint.paired
    again = play_matches(a, b, 12, DEV, joint=True, **kw)
    assert torch.equal(_trim(joint.move_log), _trim(again.move_log)) and again.paired == joint.paired
    assert torch.equal(again.openings, joint.openings)
    # without a book the same call starts from the empty board: placements only at first, and no pair statistics
    plain = play_matches(a, b, 4, DEV, max_game_plies=8, record_moves=True)
    assert plain.paired is None and plain.openings is None and "paired" not in plain.to_payload("x")
    assert int(plain.move_log[:, 0].max()) < 36


def test_the_arena_seats_its_games_with_one_launch(book):
    _need_gpu()
    from liuzhou_amd.eval_arena import _seat_openings
    from liuzhou_amd.mcts_gpu import GpuStateBatch
    openings = torch.tensor([2, 0, 3, 3, 1, 2], dtype=torch.int64)
    states = GpuStateBatch.initial(DEV, 6)
    _seat_openings(states, book, openings)
    S.assert_states(list(states.tensors()), S.unpack_states(R.to_bytes([book_words()[i] for i in openings.tolist()])), "seated")
    cpu_book = book.to("cpu")                                  # a book on another device is moved, not refused
    states = GpuStateBatch.initial(DEV, 6)
    _seat_openings(states, cpu_book, openings)
    S.assert_states(list(states.tensors()), S.unpack_states(R.to_bytes([book_words()[i] for i in openings.tolist()])), "seated")


def test_v1_arena_seats_the_same_pairs(book):
    _need_gpu()
    from liuzhou_amd.eval_arena import RandomAgent, RootSearchAgent, play_matches
    stats = play_matches(RootSearchAgent(_model(5), DEV, 8), RandomAgent(), 8, DEV, max_game_plies=PLIES, seed=4,
                         record_moves=True, opening_book=book, opening_seed=9)
    check_match(stats, 8, 9)
    assert sorted(stats.openings[:4].tolist()) == [0, 1, 2, 3]


def test_round_robin_with_a_book_equals_the_pairwise_matches(book, tree_agents):
    _need_gpu()
    from liuzhou_amd.eval_arena import play_matches, play_round_robin
    kw = dict(max_game_plies=40, record_moves=True, opening_book=book, opening_seed=5)
    rr = play_round_robin(tree_agents, 4, DEV, **kw)
    assert rr.pairs == [(0, 1), (0, 2), (1, 2)]
    for (i, j) in rr.pairs:
        st = rr.pair_stats[(i, j)]
        ref = play_matches(tree_agents[i], tree_agents[j], 4, DEV, **kw)
        assert torch.equal(_trim(st.move_log), _trim(ref.move_log)) and torch.equal(st.openings, ref.openings)
        assert (st.wins, st.losses, st.draws, st.color_breakdown, st.paired) == \
               (ref.wins, ref.losses, ref.draws, ref.color_breakdown, ref.paired)
        check_match(st, 4, 5, max_plies=40)
        assert "paired" in rr.to_payload()["pairs"][rr.pairs.index((i, j))]


def test_evaluate_checkpoint_payload_has_paired_only_with_a_book(tmp_path, book):
    _need_gpu()
    from liuzhou_amd.eval_arena import evaluate_checkpoint
    path = str(tmp_path / "model.pt")
    torch.save({"model_state_dict": _model(11).state_dict()}, path)
    keys = {"name", "wins", "losses", "draws", "total_games", "win_rate", "loss_rate", "draw_rate", "color_breakdown", "seed"}
    kw = dict(num_games=5, device=DEV, mcts_simulations=4, max_game_plies=20, seed=1)
    off = evaluate_checkpoint(path, None, **kw)
    assert set(off) == keys and off["total_games"] == 4
    on = evaluate_checkpoint(path, None, opening_book=book, opening_seed=2, **kw)
    assert set(on) == keys | {"paired"} and on["total_games"] == 4
    assert {"pairs", "pentanomial", "score", "score_stderr", "elo", "elo_ci95", "los", "trinomial_stderr", "book_size",
            "openings_used", "opening_move_mean"} == set(on["paired"])
    assert on["paired"]["pairs"] == 2 and sum(on["paired"]["pentanomial"]) == 2


def test_build_opening_book_plays_games_and_keeps_their_positions(tmp_path, capsys):
    """scripts/build_opening_book.py --checkpoint: tree self-play with a private bank that only captures."""
    _need_gpu()
    import importlib.util
    import json
    import os
    from liuzhou_amd.opening_book import OpeningBook
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("lz_script_build_opening_book", os.path.join(root, "scripts", "build_opening_book.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ckpt, out = str(tmp_path / "model.pt"), str(tmp_path / "book.pt")
    torch.save({"model_state_dict": _model(11).state_dict()}, ckpt)
    assert cli.main(["--checkpoint", ckpt, "--games", "8", "--concurrent_games", "8", "--mcts_simulations", "4", "--capture_prob", "1.0",
                     "--bank_capacity", "4096", "--min_move", "2", "--max_move", "30", "--out", out]) == 0
    meta = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    # every searched root of moves 2..30 was captured: running positions with a move, so none is invalid
    assert meta["seen"] >= 8 and meta["invalid"] == 0 and meta["kept"] >= 8 and meta["seen"] == meta["duplicate"] + meta["kept"]
    book = OpeningBook.load(out)
    assert len(book) == meta["kept"] and 2 <= int(book.move_counts.min()) and int(book.move_counts.max()) <= 30
    words = R.to_words(book.positions.numpy())
    rows, counts = R.book_rows_ref(words, 2, 30)
    assert rows == list(range(len(words))) and counts["invalid"] == 0 and counts["duplicate"] == 0
