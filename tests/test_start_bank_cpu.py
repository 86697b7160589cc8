"""CPU: the start bank (game forking) without a device -- tests/start_bank_ref.py, the numpy restatement of
lz_start_bank_capture / lz_start_bank_seed on oracle/rng_oracle.draw, against the host build of the same entry points
(csrc/lz_start_bank_host.cpp over csrc/lz_start_bank.h, the header the kernels include) on the cases the GPU tests use;
the coverage those cases must reach; `StartBank`; and the rule in `SearchRules`.  Everything is integers and bytes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import start_bank_ref as S
from tests.golden_utils import load, states, states_equal

SIMS = 16
ON = dict(start_fork_prob=0.5, start_capture_prob=0.25, start_bank_capacity=4096, start_min_move=4, start_max_move=90)
ERR_ARG, ERR_ALIGN = -1, -4


@pytest.fixture(scope="module")
def L():
    from liuzhou_amd import _lib
    _lib.host_lib()
    return _lib


# ---- the record ------------------------------------------------------------------------------------------------------------
def test_pack_unpack_is_the_identity_on_the_fixtures_reachable_states():
    for name in ("g1_rules.npz", "g15_rules_large.npz"):
        st = states(load(name), "s")
        packed = S.pack_states(st)
        assert packed.shape == (st["phase"].shape[0], 32) and packed.dtype == np.uint8
        ok, field = states_equal(S.unpack_states(packed), st)
        assert ok, (name, field)
    assert set(np.unique(S.pool()["phase"])) == set(range(1, 8))             # every phase is among them


def test_the_host_build_unpacks_what_the_restatement_packs(L):
    """seed with fork_prob 1 on a bank of the pool's own packed states: every slot becomes some pool state, bit for bit."""
    r = np.random.default_rng(5)
    want = S.pool_states(r, 257)
    ref = S.BankRef(257, 257)
    ref.entries[:] = S.pack_states(want)
    c = S.seed_case(65)
    c["fresh"][:] = 1
    j = S.run_seed(L, L.host_lib(), "cpu", c, ref, 1.0)
    assert (j >= 0).all() and np.unique(j).size > 40


# ---- the fixed-seed coverage the GPU cases rely on ---------------------------------------------------------------------------
def test_fork_draws_of_seed_12345():
    j = S.fork_entries(12345, np.arange(40), 0.5, 7)
    assert int((j >= 0).sum()) == 19 and int((j < 0).sum()) == 21
    assert int((j[:8] >= 0).sum()) == 5
    assert set(j[j >= 0].tolist()) == set(range(7))                           # each of the 7 entries is picked
    assert (S.fork_entries(12345, np.arange(40), 0.5, 0) == -1).all()         # an empty bank forks nothing
    assert (S.fork_entries(12345, np.arange(40), 0.0, 7) == -1).all()
    one = S.fork_entries(12345, np.arange(40), 1.0, 1)
    assert (one == 0).all()


def test_capture_draws_of_seed_12345():
    games, plies = np.meshgrid(np.arange(8), np.arange(12), indexing="ij")
    d = S.capture_draws(12345, games.reshape(-1), plies.reshape(-1), 0.25).reshape(8, 12)
    assert int(d.sum()) == 24
    assert int(d[:, 3].sum()) == 4 and int(d[:, 6].sum()) == 4                # more than a capacity of 3 in one launch


def test_the_playout_positions_cover_the_phases():
    st, packed = S.playout_positions()
    assert st["phase"].tolist() == [1, 1, 2, 3, 4, 4, 5] and (st["move_count"] >= 1).all()
    assert len({bytes(p) for p in packed}) == 7
    ok, field = states_equal(S.unpack_states(packed), st)
    assert ok, field


# ---- host build == restatement on the GPU cases ------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [3, 7, 4096])
@pytest.mark.parametrize("G", S.CAPTURE_G)
def test_host_capture_equals_the_restatement(L, G, capacity):
    H = L.host_lib()
    most = 0
    for total in S.capture_totals(capacity):
        n = S.run_capture(L, H, "cpu", S.capture_case(G, "mixed"), capacity, total)
        assert S.run_capture(L, H, "cpu", S.capture_case(G, "all"), capacity, total) == G
        assert S.run_capture(L, H, "cpu", S.capture_case(G, "none"), capacity, total) == 0
        assert S.run_capture(L, H, "cpu", S.capture_case(G, "all"), capacity, total, capture_prob=0.0) == 0
        most = max(most, n)
    if G >= 64:
        assert 0 < most < G                                  # the mixed case is mixed
    if G >= 1030:                                            # a run of several slots per scan thread, several wave totals
        per = -(-G // S.SCAN_THREADS)
        c = S.capture_case(G, "mixed")
        cand = S.BankRef(capacity).capture(c["states"], c["done"], c["terminal"], c["cvalid"], c["plies"], c["slot_game"],
                                           c["game_base"], c["seed"], c["capture_prob"], c["min_move"], c["max_move"])
        runs = np.add.reduceat(cand, np.arange(0, G, per))
        assert per >= 2 and runs.max() >= 2 and (cand[64 * per:].sum() > 0)
    assert S.run_capture(L, H, "cpu", S.capture_case(G, "mixed"), capacity, 0, with_slot_game=False) >= 0


@pytest.mark.parametrize("G", S.CAPTURE_G)
def test_host_seed_equals_the_restatement(L, G):
    H = L.host_lib()
    c = S.seed_case(G)
    forks = {}
    for filled in (0, 1, 7):
        for prob in (0.0, 0.5, 1.0):
            j = S.run_seed(L, H, "cpu", c, S.seed_bank(7, filled), prob)
            forks[filled, prob] = int((j >= 0).sum())
    fresh = int((c["fresh"] != 0).sum())
    assert all(forks[0, p] == 0 for p in (0.0, 0.5, 1.0)) and forks[1, 0.0] == forks[7, 0.0] == 0
    assert forks[1, 1.0] == forks[7, 1.0] == fresh
    if G >= 64:
        assert 0 < forks[7, 0.5] < fresh
    # a ring that has wrapped: filled = capacity whatever the total
    S.run_seed(L, H, "cpu", c, S.seed_bank(7, 7, total=5 * 7 + 2), 0.5)
    # a non-zero game_base gives what a shifted slot_game gives; without slot_game the slot is the game
    base = (1 << 35) + 3
    a = S.run_seed(L, H, "cpu", c, S.seed_bank(7, 7), 0.5, game_base=base)
    b = S.run_seed(L, H, "cpu", c, S.seed_bank(7, 7), 0.5, slot_game=c["slot_game"] + base)
    assert np.array_equal(a, b)
    a = S.run_seed(L, H, "cpu", c, S.seed_bank(7, 7), 0.5, game_base=base, slot_game=None)
    b = S.run_seed(L, H, "cpu", c, S.seed_bank(7, 7), 0.5, slot_game=np.arange(G, dtype=np.int64) + base)
    assert np.array_equal(a, b)


def check_argument_refusals(L, lib, device):
    """Null, range and alignment refusals of both entry points return without touching a buffer; num_slots == 0 is ok."""
    c, s = S.capture_case(4, "all"), S.seed_case(4)
    ts = S.to_device(c["states"], device)
    d = {k: S.tensor(c[k], device) for k in ("done", "terminal", "cvalid", "plies", "slot_game")}
    fresh = S.tensor(np.ones(4, np.uint8), device)
    ref = S.seed_bank(7, 7)
    raw = S.tensor(np.concatenate([ref.entries.reshape(-1), np.full(16, S.SENT, np.uint8)]), device)
    entries, cursor = raw[:7 * 32].view(7, 32), S.tensor(np.array([7], np.int64), device)
    counters = S.tensor(np.array([3, 5, 7], np.int64), device)

    def capture(ts=ts, entries=entries, cursor=cursor, counters=counters, capacity=7, prob=1.0, lo=0, hi=143, G=4, **kw):
        a = {**d, **kw}
        return S.call_capture(L, lib, device, ts, a["done"], a["terminal"], a["cvalid"], a["plies"], a["slot_game"], 0, 1, prob,
                              lo, hi, entries, capacity, cursor, counters, G=G)

    def seed(ts=ts, fresh=fresh, entries=entries, cursor=cursor, counters=counters, capacity=7, prob=1.0, G=4):
        return S.call_seed(L, lib, device, ts, fresh, d["slot_game"], 0, 1, prob, entries, capacity, cursor, counters, G=G)

    for call in (capture, seed):
        assert call(G=-1) == ERR_ARG and call(capacity=0) == ERR_ARG and call(capacity=(1 << 24) + 1) == ERR_ARG
        assert call(prob=-0.5) == ERR_ARG and call(prob=1.5) == ERR_ARG and call(prob=math.nan) == ERR_ARG
        assert call(ts=None) == ERR_ARG and call(entries=None) == ERR_ARG and call(cursor=None) == ERR_ARG
        assert call(counters=None) == ERR_ARG
        assert call(entries=raw[8:8 + 7 * 32].view(7, 32)) == ERR_ALIGN
        assert call(G=0, ts=None, entries=None, cursor=None, counters=None) == 0
    assert capture(lo=-1) == ERR_ARG and capture(lo=9, hi=8) == ERR_ARG
    assert capture(done=None) == ERR_ARG and capture(terminal=None) == ERR_ARG and capture(cvalid=None) == ERR_ARG
    assert capture(plies=None) == ERR_ARG and seed(fresh=None) == ERR_ARG
    S.assert_bytes(raw[:7 * 32].view(7, 32), ref.entries, "entries")          # nothing ran
    S.assert_bytes(raw[7 * 32:], np.full(16, S.SENT, np.uint8), "guard")
    assert int(cursor.item()) == 7 and counters.tolist() == [3, 5, 7]
    S.assert_states(ts, c["states"], "states")


def test_host_argument_refusals(L):
    check_argument_refusals(L, L.host_lib(), "cpu")


def test_the_abi_declares_both_entry_points(L):
    for name in ("lz_start_bank_capture", "lz_start_bank_seed"):
        assert name in L.SYMBOLS and name in L.HOST_SYMBOLS
    # capture_prob / fork_prob are floats, the seed is a 64-bit unsigned, sizes are 64-bit
    args = L.DECLS["lz_start_bank_capture"][1]
    assert len(args) == 17 and issubclass(args[8], C.c_uint64) and issubclass(args[9], C.c_float)
    args = L.DECLS["lz_start_bank_seed"][1]
    assert len(args) == 12 and issubclass(args[5], C.c_uint64) and issubclass(args[6], C.c_float)


def test_scripted_wave_on_the_host_reaches_its_coverage(L):
    """The 8-slot scripted wave of the GPU test, with the host build of capture and seed beside the restatement after
    every ply (the tail's own kernels have no host build: their restatement advances the wave)."""
    H = L.host_lib()
    w = S.scripted_bank_tail()
    entries = S.tensor(w.bank.entries, "cpu")
    cursor, counters = torch.zeros(1, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    for ply in range(w.PLIES):
        x = w.inputs()
        ts = S.to_device(w.st, "cpu")
        L.check(S.call_capture(L, H, "cpu", ts, S.tensor(w.done, "cpu"), S.tensor(x["terminal"], "cpu"), S.tensor(x["cvalid"], "cpu"),
                               S.tensor(w.plies, "cpu"), S.tensor(w.slot_game, "cpu"), w.GAME_BASE, w.RUN_SEED, w.CAPTURE_PROB,
                               w.MIN_MOVE, w.MAX_MOVE, entries, w.CAPACITY, cursor, counters), "start_bank_capture")
        w.capture(x)
        w.advance(x)
        ts = S.to_device(w.st, "cpu")
        L.check(S.call_seed(L, H, "cpu", ts, S.tensor(w.reseated, "cpu"), S.tensor(w.slot_game, "cpu"), w.GAME_BASE, w.RUN_SEED,
                            w.FORK_PROB, entries, w.CAPACITY, cursor, counters), "start_bank_seed")
        w.seed()
        where = f"ply {ply}: "
        S.assert_states(ts, w.st, where + "states")
        S.assert_bytes(entries, w.bank.entries, where + "entries")
        assert int(cursor.item()) == w.bank.cursor and counters.tolist() == w.bank.counters.tolist(), where
    w.check_bank_coverage()


# ---- StartBank --------------------------------------------------------------------------------------------------------------
def test_start_bank_appends_with_the_ring_rule_and_round_trips():
    from liuzhou_amd.start_bank import StartBank
    packed = S.pack_states(S.pool_states(np.random.default_rng(9), 12))
    bank, ref = StartBank(5, "cpu"), S.BankRef(5)
    ref.entries[:] = 0
    assert bank.filled() == 0 and bank.entries.shape == (5, 32) and bank.entries.dtype == torch.uint8
    assert bank.cursor.dtype == torch.int64 and bank.cursor.shape == (1,)
    for lo, hi in ((0, 2), (2, 2), (2, 6), (6, 12), (0, 12)):                 # a wrap, and more records than rows
        bank.append_packed(torch.from_numpy(packed[lo:hi]))
        ref.append(packed[lo:hi])
        assert np.array_equal(bank.entries.numpy(), ref.entries) and bank.total() == ref.cursor
        assert bank.filled() == ref.filled()
    other = StartBank(5, "cpu")
    other.load_state_dict(bank.state_dict())
    assert torch.equal(other.entries, bank.entries) and other.total() == bank.total() == 24
    with pytest.raises(ValueError):
        StartBank(6, "cpu").load_state_dict(bank.state_dict())
    with pytest.raises(ValueError):
        bank.append_packed(torch.zeros((2, 31), dtype=torch.uint8))
    for bad in (0, -1, (1 << 24) + 1, 2.5, True):
        with pytest.raises(ValueError):
            StartBank(bad, "cpu")


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def test_parse_kwargs_meta_round_trip_and_one_off_value():
    from liuzhou_amd.search_rules import SearchRules
    off = SearchRules.parse(SIMS)
    assert off.start == () and "start_bank" not in off.meta() and not any(k.startswith("start_") for k in off.kwargs())
    for kw in (dict(start_bank_capacity=7), dict(start_min_move=3, start_max_move=9), dict(start_fork_prob=0.0),
               dict(start_capture_prob=0, start_bank_capacity=1 << 24)):
        assert SearchRules.parse(SIMS, **kw) == off and hash(SearchRules.parse(SIMS, **kw)) == hash(SearchRules())
    on = SearchRules.parse(SIMS, **ON)
    assert on.kwargs() == ON and on.start_kwargs() == ON and SearchRules.parse(SIMS, **on.kwargs()) == on
    assert on.meta() == {"start_bank": {"fork_prob": 0.5, "capture_prob": 0.25, "capacity": 4096, "min_move": 4, "max_move": 90}}
    assert all(type(on.kwargs()[k]) is type(v) for k, v in ON.items())
    # capture alone and fork alone are both the rule, with the defaults of the rest
    cap = SearchRules.parse(SIMS, start_capture_prob=1)
    assert cap.start == (0.0, 1.0, 65536, 1, 143) and SearchRules.parse(SIMS, start_fork_prob=1.0).start[0] == 1.0
    # its group comes last, after every other rule's
    both = SearchRules.parse(SIMS, policy_surprise_weight=0.5, eval_symmetry="random", **ON)
    assert list(both.kwargs())[-5:] == list(ON) and list(both.meta())[-1] == "start_bank"
    # a rule of the per-ply tail: the engine does not see it
    assert on.engine() == off and both.engine() == SearchRules.parse(SIMS, eval_symmetry="random")
    with pytest.raises(TypeError):
        SearchRules.parse_engine(SIMS, start_fork_prob=0.5)
    import pickle
    assert pickle.loads(pickle.dumps(on)) == on


def test_every_invalid_value_is_a_value_error():
    from liuzhou_amd.search_rules import SearchRules
    bads = [dict(start_fork_prob=p) for p in (-0.1, 1.5, math.nan, math.inf, True)] + \
           [dict(start_capture_prob=p) for p in (-0.1, 1.5, math.nan, True)] + \
           [dict(start_bank_capacity=c) for c in (0, -1, (1 << 24) + 1, 2.5, True)] + \
           [dict(start_min_move=-1), dict(start_min_move=1.5), dict(start_max_move=144), dict(start_max_move=2.5),
            dict(start_min_move=10, start_max_move=9)]
    for bad in bads:
        for more in ({}, dict(start_fork_prob=0.5)):         # on or off, every value is validated
            if set(bad) & set(more):
                continue
            with pytest.raises(ValueError):
                SearchRules.parse(SIMS, **bad, **more)


ROOT_TEXT = ("the start bank needs the tree backend, not the root-PUCT search ('cuda_root'): its capture and seed kernels run "
             "in the tree backend's per-ply device tail")
NO_TAIL_TEXT = ("the start bank is not supported with the host loop (device_tail=False): the bank is filled and read by the "
                "per-ply device tail")
RESEAT_TEXT = ("the start bank is not supported with the in-kernel re-seat (reseat=True): the step kernel starts the next "
               "game there, and no kernel runs between its fresh state and the search")
RUN = dict(num_games=2, mcts_simulations=SIMS, temperature_init=1.0, temperature_final=0.1, temperature_threshold=4,
           exploration_weight=1.0, device="cuda:0")
WORKER = dict(worker_idx=0, shard_device="cuda:0", shard_games=4, seed=1, model_state_path="none.pt", output_path="none",
              mcts_simulations=SIMS, temperature_init=1.0, temperature_final=0.1, temperature_threshold=4,
              exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
              opening_random_moves=0, max_game_plies=8, concurrent_games_per_device=4)


def test_the_three_refusals_at_the_layers_that_know_them(tmp_path):
    from liuzhou_amd.search_rules import SearchRules
    from liuzhou_amd.self_play_stage import run_self_play_stage
    from liuzhou_amd.self_play_worker import run_self_play_worker
    from liuzhou_amd.tree_engine import PriorEvaluator, self_play_tree_gpu
    from liuzhou_amd.wave_tail import WaveTail
    from tests.stage_stub import stub_worker
    for kw in (dict(start_fork_prob=0.5), dict(start_capture_prob=0.5)):
        rules = SearchRules.parse(SIMS, **kw)
        assert rules.refusal(search_backend="cuda_root") == ROOT_TEXT
        assert rules.refusal(device_tail=False) == NO_TAIL_TEXT and rules.refusal(reseat=True) == RESEAT_TEXT
        assert rules.refusal(search_backend="tree", device_tail=True, reseat=False, prior_evaluator=True, batch_k=2,
                             fused=False, several_networks=True) is None
    assert SearchRules.parse(SIMS).refusal(search_backend="cuda_root", device_tail=False, reseat=True) is None
    # the backend: the stage and the worker, before a process is spawned or a device touched
    with pytest.raises(ValueError) as err:
        run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                            output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=SIMS,
                            concurrent_games_per_device=4, worker_fn=stub_worker, in_process=True,
                            search_backend="cuda_root", start_fork_prob=0.5)
    assert str(err.value) == ROOT_TEXT
    with pytest.raises(ValueError) as err:
        run_self_play_worker(search_backend="cuda_root", start_capture_prob=0.5, **WORKER)
    assert str(err.value) == ROOT_TEXT
    # the host loop: the runner; the in-kernel re-seat: the tail -- both before anything is allocated
    prior = PriorEvaluator(lambda planes, packed: None)
    with pytest.raises(ValueError) as err:
        self_play_tree_gpu(prior, device_tail=False, start_fork_prob=0.5, **RUN)
    assert str(err.value) == NO_TAIL_TEXT
    with pytest.raises(ValueError) as err:
        WaveTail(None, 4, 8, "cuda:0", reseat=True, start_bank=object.__new__(_Bank), start_fork_prob=0.5)
    assert str(err.value) == RESEAT_TEXT


class _Bank:
    capacity = 16


def test_the_runner_refuses_a_bank_that_does_not_fit_the_rule():
    from liuzhou_amd.start_bank import StartBank
    from liuzhou_amd.tree_engine import PriorEvaluator, self_play_tree_gpu
    prior = PriorEvaluator(lambda planes, packed: None)
    bank = StartBank(16, "cpu")
    with pytest.raises(ValueError, match="the rule is off"):
        self_play_tree_gpu(prior, start_bank=bank, **RUN)
    with pytest.raises(ValueError, match="the rule is off"):
        self_play_tree_gpu(prior, start_bank=bank, start_bank_capacity=16, **RUN)
    with pytest.raises(ValueError, match="start_bank_capacity is 65536"):
        self_play_tree_gpu(prior, start_bank=bank, start_fork_prob=0.5, **RUN)
