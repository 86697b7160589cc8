"""CPU: the resignation rule's checker (tests/resign_rule.py), the parameters' validation, the refusals that need no device,
the counters' arithmetic and the C ABI of the two entry points."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.resign_rule import (PHASE_CAPTURE_SELECTION, PHASE_COUNTER_REMOVAL, PHASE_MOVEMENT, PHASE_PLACEMENT,
                               resign_rule)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PHASES = (PHASE_PLACEMENT, 2, 3, PHASE_MOVEMENT, PHASE_CAPTURE_SELECTION, 6, PHASE_COUNTER_REMOVAL)


def _random_games(n=200, length=40):
    rng = np.random.default_rng(20261019)
    for _ in range(n):
        movers = np.where(rng.random(length) < 0.8, np.where(np.arange(length) % 2 == 0, 1, -1), rng.choice([-1, 1], length))
        start = int(rng.integers(0, 12))                      # placement-like phases first, then the movement phases
        phases = [int(rng.choice(PHASES[:3])) if t < start else int(rng.choice(PHASES)) for t in range(length)]
        values = rng.choice([F(-0.9), F(-0.5), F(-0.2), F(0.3), F("nan")], length, p=[0.35, 0.25, 0.2, 0.15, 0.05])
        term = rng.random(length) < 0.02
        yield [(int(m), p, F(v), bool(t)) for m, p, v, t in zip(movers, phases, values, term)]


# ---- the checker -------------------------------------------------------------------------------------------------------
def test_a_hand_computed_game():
    mv = PHASE_MOVEMENT
    game = [(1, mv, F(-0.9), False), (-1, mv, F(0.9), False), (1, mv, F(-0.9), False), (-1, mv, F(0.9), False),
            (1, mv, F(-0.9), False), (-1, mv, F(0.9), False)]
    # Black is low on its own plies 0, 2, 4: "side" resigns at its third, "ply" never sees two low plies in a row
    assert resign_rule(game, -0.5, min_moves=0, consecutive=3, streak="side") == (4, 0, -1)
    assert resign_rule(game, -0.5, min_moves=0, consecutive=2, streak="side") == (2, 0, -1)
    assert resign_rule(game, -0.5, min_moves=0, consecutive=2, streak="ply") == (None, 0, -1)
    assert resign_rule(game, -0.5, min_moves=0, consecutive=1, streak="ply") == (0, 0, -1)
    assert resign_rule(game, -0.5, min_moves=1, consecutive=2, streak="side") == (4, 0, -1)
    assert resign_rule(game, -0.5, min_moves=0, consecutive=2, streak="side", playthrough=True) == (None, 1, 2)
    # a good value of the same side breaks its streak; the other side's does not
    game[2] = (1, mv, F(0.0), False)
    assert resign_rule(game, -0.5, min_moves=0, consecutive=2, streak="side") == (None, 0, -1)
    # the threshold itself is low, one ulp above it is not; a NaN never is
    at, above = F(-0.5), np.nextafter(F(-0.5), F(0))
    assert resign_rule([(1, mv, at, False)], -0.5, 0, 1) == (0, 0, -1)
    assert resign_rule([(1, mv, above, False)], -0.5, 0, 1) == (None, 0, -1)
    assert resign_rule([(1, mv, F("nan"), False)], -0.5, 0, 1) == (None, 0, -1)
    # the threshold is rounded to float32 before the comparison
    assert resign_rule([(1, mv, F(-0.1), False)], -0.1, 0, 1) == (0, 0, -1)
    # a terminal root is not eligible
    assert resign_rule([(1, mv, F(-1), True)], -0.5, 0, 1) == (None, 0, -1)
    assert resign_rule([], -0.5) == (None, 0, -1)


def test_consecutive_one_both_streak_modes_agree():
    hits = 0
    for game in _random_games():
        for pt in (False, True):
            a = resign_rule(game, -0.4, min_moves=5, consecutive=1, streak="side", playthrough=pt)
            assert a == resign_rule(game, -0.4, min_moves=5, consecutive=1, streak="ply", playthrough=pt)
            hits += a != (None, 0, -1)
    assert hits > 100


def test_never_before_min_moves_or_in_placement():
    seen = 0
    for game in _random_games():
        for streak in ("side", "ply"):
            for cons in (1, 2, 3):
                for mm in (0, 7, 20):
                    ply, _, _ = resign_rule(game, -0.4, min_moves=mm, consecutive=cons, streak=streak)
                    _, would, wply = resign_rule(game, -0.4, min_moves=mm, consecutive=cons, streak=streak, playthrough=True)
                    assert (ply is None) == (would == 0) and (ply is None or ply == wply)     # the same event, latched
                    if ply is None:
                        continue
                    seen += 1
                    mover, phase, value, term = game[ply]
                    assert ply >= mm and ply >= cons - 1 and not term
                    assert phase in (PHASE_MOVEMENT, PHASE_CAPTURE_SELECTION, PHASE_COUNTER_REMOVAL)
                    assert value <= F(-0.4) and would == (1 if mover >= 0 else -1)
    assert seen > 500
    placement = [(1 if t % 2 == 0 else -1, PHASE_PLACEMENT, F(-1), False) for t in range(30)]
    assert resign_rule(placement, -0.1, 0, 1) == (None, 0, -1)


def test_play_through_never_resigns():
    for game in _random_games():
        for streak in ("side", "ply"):
            assert resign_rule(game, -0.2, min_moves=0, consecutive=1, streak=streak, playthrough=True)[0] is None


# ---- validation and refusals -------------------------------------------------------------------------------------------
def test_validation():
    from liuzhou_amd.resign import resign_kwargs, resign_on
    assert resign_on() is False and resign_on(0.0) is False and resign_on(0) is False and resign_on(-0.0) is False
    assert resign_on(-0.9) is True and resign_on(-1) is True and resign_on(np.float32(-0.5)) is True
    assert resign_on(-0.9, 0, 1, 0.0, "ply") is True and resign_on(-0.9, 10, 3, 1.0, "side") is True
    for bad in (math.nan, math.inf, -math.inf, 0.1, -1.5, "x", None, True):
        with pytest.raises(ValueError, match="resign_threshold"):
            resign_on(bad)
    for thr in (0.0, -0.9):                                 # the other four are checked on or off
        for bad in (-1, 1.5, math.nan, "x", None, True):
            with pytest.raises(ValueError, match="resign_min_moves"):
                resign_on(thr, resign_min_moves=bad)
        for bad in (0, -1, 2.5, math.inf, None, False):
            with pytest.raises(ValueError, match="resign_consecutive"):
                resign_on(thr, resign_consecutive=bad)
        for bad in (-0.1, 1.1, math.nan, math.inf, "x", None, True):
            with pytest.raises(ValueError, match="resign_playthrough_fraction"):
                resign_on(thr, resign_playthrough_fraction=bad)
        for bad in ("both", "", None, 1):
            with pytest.raises(ValueError, match="resign_streak"):
                resign_on(thr, resign_streak=bad)
    assert resign_kwargs() == {} and resign_kwargs(0.0, 5, 2, 0.5, "ply") == {}
    assert resign_kwargs(-0.9, 5, 2, 0.5, "ply") == {
        "resign_threshold": -0.9, "resign_min_moves": 5, "resign_consecutive": 2, "resign_playthrough_fraction": 0.5,
        "resign_streak": "ply"}


def test_self_play_refuses_the_host_loop_before_it_touches_a_device():
    from liuzhou_amd.tree_engine import self_play_tree_gpu
    module = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="device_tail"):
        self_play_tree_gpu(module, 2, 16, 1.0, 0.1, 10, 1.0, "cpu", evaluator="module", device_tail=False,
                           resign_threshold=-0.9)
    for bad in (math.nan, math.inf, 0.5, -1.5):
        with pytest.raises(ValueError, match="resign_threshold"):
            self_play_tree_gpu(module, 2, 16, 1.0, 0.1, 10, 1.0, "cpu", evaluator="module", resign_threshold=bad)
    with pytest.raises(ValueError, match="resign_streak"):
        self_play_tree_gpu(module, 2, 16, 1.0, 0.1, 10, 1.0, "cpu", evaluator="module", resign_threshold=-0.9,
                           resign_streak="game")


def test_tail_refuses_the_in_kernel_reseat_before_it_touches_a_device():
    from liuzhou_amd.wave_tail import WaveTail
    with pytest.raises(ValueError, match="reseat"):
        WaveTail(None, 4, 16, "cpu", reseat=True, resign_threshold=-0.9)
    for bad in (math.nan, 0.5, -1.5):
        with pytest.raises(ValueError, match="resign_threshold"):
            WaveTail(None, 4, 16, "cpu", resign_threshold=bad)
    with pytest.raises(ValueError, match="resign_consecutive"):
        WaveTail(None, 4, 16, "cpu", resign_threshold=-0.9, resign_consecutive=0)
    with pytest.raises(RuntimeError, match="HIP device"):          # off: the tail it always was
        WaveTail(None, 4, 16, "cpu", reseat=True, resign_threshold=0.0)


# ---- counters -----------------------------------------------------------------------------------------------------------
def test_counters_derive_and_merge():
    from liuzhou_amd.resign import COUNTER_KEYS, DERIVED_KEYS, counters_from_block
    from liuzhou_amd.self_play_worker import merge_self_play_stats
    from liuzhou_amd.self_play_types import SelfPlayV1Stats
    a = counters_from_block([4, 3, 1, 2, 2, 1, 100, 30])
    assert [a[k] for k in COUNTER_KEYS] == [4, 3, 1, 2, 2, 1, 100, 30]
    assert a["resign_avg_ply"] == 25 and a["resign_plies_saved_estimate"] == 60
    b = counters_from_block([0, 0, 0, 1, 0, 0, 0, 0])
    assert b["resign_avg_ply"] == 0 and b["resign_plies_saved_estimate"] == 0
    assert set(a) == set(COUNTER_KEYS) | set(DERIVED_KEYS)
    keys = ("root_puct_ms", "pack_writeback_ms", "self_play_step_ms", "finalize_ms")
    st = lambda c: SelfPlayV1Stats(num_games=8, num_positions=80, black_wins=4, white_wins=3, draws=1, avg_game_length=10.0,
                                   elapsed_sec=1.0, positions_per_sec=80.0, games_per_sec=8.0,
                                   step_timing_ms={k: 1.0 for k in keys}, step_timing_ratio={k: 0.25 for k in keys},
                                   step_timing_calls={k: 1 for k in keys}, mcts_counters=dict(c), piece_delta_buckets={})
    c = counters_from_block([6, 2, 4, 2, 1, 0, 60, 50])
    m = merge_self_play_stats([st(a), st(c)], 2.0).mcts_counters
    assert [m[k] for k in COUNTER_KEYS] == [10, 5, 5, 4, 3, 1, 160, 80]
    assert m["resign_avg_ply"] == 16 and m["resign_plies_saved_estimate"] == round(10 * 80 / 3)     # not 25 + 10
    plain = merge_self_play_stats([st({"leaf_eval_count": 5}), st({"leaf_eval_count": 7})], 2.0).mcts_counters
    assert plain == {"leaf_eval_count": 12}                 # without the feature the merged counters gain nothing


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def _args(name):
    text = open(os.path.join(ROOT, "include", "liuzhou_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"LZ_API\s+int\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_two_entry_points():
    from liuzhou_amd import _lib as L
    assert _args("lz_wave_resign") == [
        "const uint8_t* done", "int64_t num_slots", "const int64_t* plies", "const int64_t* phase",
        "const int64_t* current_player", "const float* root_value", "const uint8_t* terminal_mask",
        "const int64_t* slot_game", "int64_t game_base", "uint64_t seed", "float threshold", "int64_t min_moves",
        "int32_t consecutive", "float playthrough_fraction", "int per_ply", "int32_t* streak", "int32_t* would",
        "int32_t* would_ply", "uint8_t* terminal_out", "uint8_t* was_live", "uint8_t* resigned", "void* stream"]
    assert _args("lz_wave_resign_book") == [
        "const LzStateSoA* states", "int64_t num_slots", "const uint8_t* done", "const uint8_t* was_live",
        "const int64_t* plies", "const uint8_t* terminal_out", "const uint8_t* chosen_valid_mask",
        "const uint8_t* resigned", "const int32_t* would", "const int32_t* would_ply", "const int64_t* slot_game",
        "int64_t game_base", "uint64_t seed", "float playthrough_fraction", "int64_t* counters", "void* stream"]
    for name, scalars in (("lz_wave_resign", {1: C.c_int64, 8: C.c_int64, 9: C.c_uint64, 10: C.c_float, 11: C.c_int64,
                                              12: C.c_int32, 13: C.c_float, 14: C.c_int32}),
                          ("lz_wave_resign_book", {1: C.c_int64, 11: C.c_int64, 12: C.c_uint64, 13: C.c_float})):
        assert name in L.SYMBOLS
        ret, types = L.DECLS[name]
        assert ret is C.c_int and len(types) == len(_args(name))
        for i, t in enumerate(types):
            if i in scalars:
                assert issubclass(t, scalars[i]), (name, i)
            else:
                assert t is C.c_void_p, (name, i)
    src = open(os.path.join(ROOT, "liuzhou_amd", "csrc", "lz_ops.hip")).read()
    for name in ("lz_wave_resign", "lz_wave_resign_book"):             # defined with the declared parameter types
        m = re.search(r"\nint " + name + r"\(([^{]*?)\)\s*\{", src, flags=re.S)
        assert m, name
        strip = lambda a: " ".join(a.split()).rsplit(" ", 1)[0]
        assert [strip(a) for a in m.group(1).split(",")] == [strip(a) for a in _args(name)]


# ---- the scripted wave of the kernels' GPU test --------------------------------------------------------------------------
def test_scripted_wave_covers_its_cases():
    """tests/resign_wave.py on the host alone: every run of the GPU test meets the cases it was built for, and the
    play-through set is a function of the game id only."""
    from tests.resign_wave import CONFIGS, GAME_BASE, KSEED, ScriptedWave, plays_through
    for cons, streak, fraction in CONFIGS:
        wave = ScriptedWave(cons, streak, fraction)
        last = None
        for last in wave.plies():
            assert len(last["expected"]) == wave.G
        assert last["tally"] == wave.tally.tolist()
        wave.check_coverage()
    ids = np.arange(4096, dtype=np.int64) + GAME_BASE
    a = plays_through(KSEED, ids, 0.5)
    assert np.array_equal(a, plays_through(KSEED, ids[::-1], 0.5)[::-1]) and 0.45 < a.mean() < 0.55
    assert not plays_through(KSEED, ids, 0.0).any() and plays_through(KSEED, ids, 1.0).all()
    assert (plays_through(KSEED, ids, 0.1) <= a).all()                      # u < 0.1 implies u < 0.5
