"""CPU: the opening book at the command line and at the arena's door -- the flags of scripts/eval_arena.py and
scripts/build_opening_book.py, the refusals that need no device, and a book built from a file of records."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import opening_book_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def script(name):
    spec = importlib.util.spec_from_file_location("lz_script_" + name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def small_book():
    from liuzhou_amd.opening_book import OpeningBook
    words = [r for r in R.pool() if R.valid_ref(r, 6, 143)][::70][:4]
    return OpeningBook.from_packed(torch.from_numpy(R.to_bytes(words)), min_move=6)


def test_eval_arena_flags_parse():
    cli = script("eval_arena")
    args = cli.parse(["--challenger_checkpoint", "a.pt"])
    assert args.opening_book is None and args.opening_seed == 0 and cli.opening_book_of(args) is None
    args = cli.parse(["--challenger_checkpoint", "a.pt", "--opening_book", "book.pt", "--opening_seed", "7"])
    assert args.opening_book == "book.pt" and args.opening_seed == 7


def test_eval_arena_loads_the_book_and_refuses_it_with_random_openings(tmp_path):
    cli = script("eval_arena")
    book = small_book()
    path = str(tmp_path / "book.pt")
    book.save(path)
    got = cli.opening_book_of(cli.parse(["--challenger_checkpoint", "a.pt", "--opening_book", path, "--device", "cpu"]))
    assert torch.equal(got.positions, book.positions)
    with pytest.raises(ValueError, match="cannot be combined"):
        cli.main(["--challenger_checkpoint", "a.pt", "--opening_book", path, "--v1_opening_random_moves", "2",
                  "--eval_games_vs_random", "4"])


def test_the_arena_refuses_what_a_book_cannot_be_combined_with():
    from liuzhou_amd.eval_arena import RandomAgent, evaluate_checkpoint, play_matches, play_round_robin
    book = small_book()
    a, b = RandomAgent(), RandomAgent()
    with pytest.raises(ValueError, match="must be even"):
        play_matches(a, b, 7, "cuda:0", opening_book=book)
    with pytest.raises(ValueError, match="must be even"):
        play_round_robin([a, b, a], 5, "cuda:0", opening_book=book)
    with pytest.raises(ValueError, match="opening_random_moves"):
        play_matches(a, b, 8, "cuda:0", opening_book=book, opening_random_moves=2)
    with pytest.raises(ValueError, match="opening_random_moves"):
        play_round_robin([a, b], 8, "cuda:0", opening_book=book, opening_random_moves=1)
    with pytest.raises(ValueError, match="opening_random_moves"):
        evaluate_checkpoint("missing.pt", None, num_games=8, opening_book=book, opening_random_moves=3)
    with pytest.raises(ValueError, match="OpeningBook"):
        play_matches(a, b, 8, "cuda:0", opening_book=book.positions)
    from liuzhou_amd.opening_book import OpeningBook
    with pytest.raises(ValueError, match="at least one position"):
        play_matches(a, b, 8, "cuda:0", opening_book=OpeningBook(torch.zeros((0, 32), dtype=torch.uint8)))


def test_a_payload_without_a_book_keeps_its_keys():
    from liuzhou_amd.eval_arena import EvaluationStats
    keys = {"name", "wins", "losses", "draws", "total_games", "win_rate", "loss_rate", "draw_rate", "color_breakdown"}
    assert set(EvaluationStats(1, 1, 0, 2).to_payload("x")) == keys
    with_book = EvaluationStats(1, 1, 0, 2, paired={"pairs": 1})
    assert set(with_book.to_payload("x")) == keys | {"paired"}


def test_build_opening_book_from_a_file_of_records(tmp_path, capsys):
    from liuzhou_amd.opening_book import OpeningBook
    from liuzhou_amd.start_bank import StartBank
    cli = script("build_opening_book")
    words = [r for r in R.pool() if R.valid_ref(r, 0, 143)][::25]
    words = words + [R.sym_record(2, w) for w in words[:5]] + [(0, 0, 0, 0)]
    rows, counts = R.book_rows_ref(words, 8, 60, 12)
    raw, out = str(tmp_path / "raw.pt"), str(tmp_path / "out" / "book.pt")
    torch.save(torch.from_numpy(R.to_bytes(words)), raw)
    args = ["--min_move", "8", "--max_move", "60", "--max_positions", "12", "--out", out]
    assert cli.main(["--records", raw] + args) == 0
    meta = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert {k: meta[k] for k in counts} == counts and meta["format"] == "lz_opening_book_v1"
    book = OpeningBook.load(out)
    assert np.array_equal(book.positions.numpy(), R.to_bytes([words[i] for i in rows])) and book.meta == meta
    # the same records as a saved StartBank: its filled rows, not the zero rows behind them
    bank = StartBank(len(words) + 9, "cpu")
    bank.append_packed(torch.from_numpy(R.to_bytes(words)))
    state = str(tmp_path / "bank.pt")
    torch.save(bank.state_dict(), state)
    assert cli.main(["--records", state] + args) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == meta
    assert torch.equal(OpeningBook.load(out).positions, book.positions)
    bad = str(tmp_path / "bad.pt")
    torch.save(torch.zeros((4, 31), dtype=torch.uint8), bad)
    with pytest.raises(ValueError):
        cli.main(["--records", bad, "--out", out])


def test_build_opening_book_flags_parse():
    cli = script("build_opening_book")
    a = cli.parse(["--checkpoint", "ck.pt", "--games", "64", "--mcts_simulations", "32", "--capture_prob", "0.1", "--out", "b.pt"])
    assert (a.checkpoint, a.games, a.mcts_simulations, a.capture_prob, a.records) == ("ck.pt", 64, 32, 0.1, None)
    assert (a.min_move, a.max_move, a.max_positions) == (0, 143, None)
    with pytest.raises(SystemExit):
        cli.parse(["--out", "b.pt"])                                               # one source is required
    with pytest.raises(SystemExit):
        cli.parse(["--records", "r.pt", "--checkpoint", "ck.pt", "--out", "b.pt"])
