"""A scripted wave for the resignation kernels' test, played on the host (numpy only).

About 70 slots are driven ply by ply for 12 plies: every slot holds a list of scripted games (a finished slot with games
left is re-seated at the top of the next ply, as lz_wave_reseat does).  For every ply `ScriptedWave.plies()` yields the
inputs of lz_wave_resign, what the kernel has to leave for every slot (from tests/resign_rule.py over the game so far and
the play-through set of the host Philox, oracle/rng_oracle.py), the effect of the step kernel (restated here: a terminal
root or a resignation ends the game where it stands, a scripted ending ends it after its move) and the running tally of
lz_wave_resign_book's counter block."""
import numpy as np

from oracle import rng_oracle
from tests.resign_rule import (PHASE_CAPTURE_SELECTION, PHASE_COUNTER_REMOVAL, PHASE_MOVEMENT, PHASE_PLACEMENT,
                               resign_rule)

F = np.float32
THR = -0.3                                                  # not a float32: the kernel compares with float32(-0.3)
AT = F(THR)
ABOVE = np.nextafter(AT, F(0))
LOW, GOOD, NAN = F(-0.9), F(0.3), F("nan")
MIN_MOVES, T = 4, 12
KSEED = 0x9E3779B97F4A7C15
GAME_BASE = (1 << 33) + 7                                   # game ids with a high word
MV, CS, CR, PL = PHASE_MOVEMENT, PHASE_CAPTURE_SELECTION, PHASE_COUNTER_REMOVAL, PHASE_PLACEMENT
ALT = [1 if t % 2 == 0 else -1 for t in range(T)]
TRIPLES = [1 if (t // 3) % 2 == 0 else -1 for t in range(T)]
# (resign_consecutive, resign_streak, resign_playthrough_fraction) of the runs
CONFIGS = [(1, "side", 0.5), (2, "side", 0.5), (3, "side", 0.5), (1, "ply", 0.5), (2, "ply", 0.5), (3, "ply", 0.0),
           (2, "side", 0.0), (2, "side", 1.0), (1, "ply", 1.0)]


def plays_through(seed, games, fraction):
    """The play-through draw restated on the host: Philox at purpose 3, ply 0, index 1023; u < float32(fraction)."""
    games = np.asarray(games, np.int64).reshape(-1)
    return rng_oracle.u01(rng_oracle.draw(int(seed), games, 0, 3, 1023, 0)[:, 0]) < F(fraction)


def _game(values, movers=ALT, phases=MV, end=None, terminal_at=None):
    """One game's script: T plies of (mover, phase, value, terminal root) and how it ends by itself: `end` = (ply, kind),
    kind in black / white / draw_limit / draw_novalid (the move of that ply ends it), or a terminal root at a ply."""
    values = [values] * T if not isinstance(values, (list, tuple)) else list(values)
    phases = [phases] * T if not isinstance(phases, (list, tuple)) else list(phases)
    plies = [(movers[t], phases[t], F(values[t]), terminal_at == t) for t in range(T)]
    return {"plies": plies, "end": (terminal_at, "terminal") if terminal_at is not None else end}


def scripted_slots():
    s = []
    two = lambda g: [g, g]                                  # the same script under two game ids
    s += two([_game(LOW)])                                  # alternating movers, low from ply 0: first eligible ply = MIN_MOVES
    s += two([_game(AT)])                                   # exactly the threshold: low
    s += two([_game(ABOVE)])                                # one ulp above: never
    s += two([_game(NAN)])                                  # NaN: never
    s += two([_game(LOW, phases=PL)])                       # placement: never
    s += two([_game(LOW, phases=[PL] * 6 + [MV] * 6)])      # movement starts at ply 6
    s += two([_game(LOW, phases=[PL] * 3 + [MV] * 9)])      # ... at ply 3 = MIN_MOVES - 1: ply 3 must not count
    s += two([_game(LOW, movers=TRIPLES, phases=CS)])       # same-mover capture sequences
    s += two([_game(LOW, movers=TRIPLES, phases=[MV, CS, CR] * 4)])
    s += two([_game([LOW] * 6 + [GOOD] + [LOW] * 5)])       # a streak broken by one good value
    s += two([_game([LOW] * 7 + [GOOD] + [LOW] * 4)])       # ... of the other side
    s += two([_game([LOW, GOOD] * 6)])                      # Black low, White fine
    s += two([_game([GOOD, LOW] * 6)])                      # White low, Black fine
    s += two([_game([LOW] * 5 + [LOW, LOW, NAN, LOW, LOW, ABOVE, LOW])])
    s += two([_game(LOW, phases=[MV] * 6 + [PL] + [MV] * 5)])      # an ineligible ply in between clears both sides
    s += two([_game(LOW, terminal_at=7)])                   # a terminal root passes through (and is no resignation)
    s += two([_game(GOOD, terminal_at=5)])
    s += two([_game(LOW, terminal_at=MIN_MOVES)])           # terminal at the first eligible ply: not low
    for kind in ("black", "white", "draw_limit", "draw_novalid"):   # natural endings, with and without a wish to resign
        s += two([_game(LOW, end=(9, kind))])
        s += [[_game(GOOD, end=(6, kind))]]
        s += [[_game([GOOD, LOW] * 6, end=(10, kind))]]
    s += two([None])                                        # finished from the start
    for kind in ("black", "draw_limit"):                    # re-seated to ply 0 mid-run, then low
        s += two([_game(GOOD, end=(4, kind)), _game(LOW, phases=MV)])
    s += [[_game(LOW, end=(2, "white")), _game(LOW, end=(3, "black")), _game(LOW)]]
    rng = np.random.default_rng(20261019)
    while len(s) < 70:                                      # and random ones
        vals = list(rng.choice([LOW, AT, ABOVE, GOOD, NAN], T, p=[0.45, 0.15, 0.15, 0.2, 0.05]))
        ph = [int(x) for x in rng.choice([PL, 2, MV, CS, CR], T, p=[0.1, 0.05, 0.45, 0.2, 0.2])]
        mv = [int(x) for x in np.where(rng.random(T) < 0.7, ALT, rng.choice([-1, 1], T))]
        end = (int(rng.integers(5, T)), str(rng.choice(["black", "white", "draw_limit", "draw_novalid"]))) \
            if rng.random() < 0.5 else None
        s.append([_game(vals, movers=mv, phases=ph, end=end)])
    return s


def _board(kind):
    """Post-move boards of the natural endings: a side with 3 pieces has lost; 5 against 5 is a draw by a limit."""
    b = np.zeros(36, np.int8)
    nb, nw = {"black": (5, 3), "white": (3, 5)}.get(kind, (5, 5))
    b[:nb] = 1
    b[18:18 + nw] = -1
    return b.reshape(6, 6)


class ScriptedWave:
    def __init__(self, consecutive, streak, fraction):
        self.consecutive, self.streak, self.fraction = int(consecutive), streak, float(fraction)
        self.slots = scripted_slots()
        self.G = len(self.slots)
        assert 64 < self.G <= 80                            # more than one wave of lanes
        # every game of every slot has its own id; slot_game holds id - GAME_BASE, as the runner's slot_game does
        self.ids = [[1000 * k + g for k in range(len(self.slots[g]))] for g in range(self.G)]
        every = np.array([i for row in self.ids for i in row], np.int64) + GAME_BASE
        self.pt = dict(zip(every.tolist(), plays_through(KSEED, every, fraction).tolist()))
        self.seen = {"resigned": 0, "latched": 0, "fp_draw": 0, "true_positive": 0, "terminal": 0, "reseated": 0,
                     "endings": set(), "first_eligible": 0}
        self.tally = np.zeros(8, np.int64)

    def plies(self):
        G, slots, ids, seen, tally = self.G, self.slots, self.ids, self.seen, self.tally
        game_no = [0] * G                                   # which of the slot's games is seated
        live = [slots[g][0] is not None for g in range(G)]
        ply = [0] * G
        ended_prev = [False] * G
        for t in range(T):
            for g in range(G):                              # top of the ply: re-seat
                if not live[g] and ended_prev[g] and game_no[g] + 1 < len(slots[g]):
                    game_no[g] += 1
                    live[g], ply[g] = True, 0
                    seen["reseated"] += 1
            ended_prev = [False] * G
            cur = [slots[g][game_no[g]]["plies"][ply[g]] if live[g] else (1, PL, F(0), False) for g in range(G)]
            out = {"done": np.array([not x for x in live], np.uint8), "plies": np.array(ply, np.int64),
                   "slot_game": np.array([ids[g][game_no[g]] for g in range(G)], np.int64),
                   "phase": np.array([c[1] for c in cur], np.int64), "player": np.array([c[0] for c in cur], np.int64),
                   "root_value": np.array([c[2] for c in cur], np.float32),
                   "terminal": np.array([c[3] for c in cur], np.uint8)}
            expected, rule = [None] * G, [None] * G
            for g in range(G):
                if not live[g]:
                    continue
                gid = ids[g][game_no[g]] + GAME_BASE
                r, wd, wp = resign_rule(slots[g][game_no[g]]["plies"][:ply[g] + 1], THR, MIN_MOVES, self.consecutive,
                                        self.streak, playthrough=self.pt[gid])
                assert r is None or r == ply[g]
                rule[g] = (r is not None, wd, wp)
                expected[g] = (int(r is not None), int(r is not None or cur[g][3]), wd, wp)
                seen["first_eligible"] += int(r is not None and ply[g] == MIN_MOVES)
            out["expected"] = expected
            cvalid = np.ones(G, np.uint8)
            board = np.zeros((G, 6, 6), np.int8)
            board[:, 0, :5] = 1
            board[:, 3, :5] = -1
            ended = [False] * G
            for g in range(G):
                if not live[g]:
                    continue
                end = slots[g][game_no[g]]["end"]
                mover = 1 if cur[g][0] >= 0 else -1
                resign_now, wd, wp = rule[g]
                result = None
                if resign_now or cur[g][3]:
                    result = -mover
                    seen["resigned" if resign_now else "terminal"] += 1
                elif end is not None and end[0] == ply[g]:
                    kind = end[1]
                    seen["endings"].add(kind)
                    if kind == "draw_novalid":
                        cvalid[g], result = 0, 0
                    else:
                        board[g] = _board(kind)
                        result = {"black": 1, "white": -1, "draw_limit": 0}[kind]
                        ply[g] += 1
                else:
                    ply[g] = min(ply[g] + 1, T - 1)         # the scripts are T plies long
                if result is None:
                    continue
                live[g], ended_prev[g], ended[g] = False, True, True
                if resign_now:
                    tally[0] += 1
                    tally[1 if mover > 0 else 2] += 1
                    tally[6] += ply[g]
                if self.pt[ids[g][game_no[g]] + GAME_BASE]:
                    assert not resign_now
                    tally[3] += 1
                    if wd != 0:
                        seen["latched"] += 1
                        tally[4] += 1
                        tally[5] += int(result != -wd)
                        tally[7] += ply[g] - wp
                        seen["fp_draw"] += int(result == 0)
                        seen["true_positive"] += int(result == -wd)
            out.update(board_after=board, cvalid=cvalid,
                       # (a movement phase where a game ended: the winner rule only looks at the board in those phases)
                       phase_after=np.array([MV if ended[g] else cur[g][1] for g in range(G)], np.int64),
                       done_after=np.array([not x for x in live], np.uint8), plies_after=np.array(ply, np.int64),
                       tally=[int(x) for x in tally])
            yield out

    def check_coverage(self):
        """The run went through the cases it was built for."""
        seen, tally, frac = self.seen, self.tally, self.fraction
        assert seen["terminal"] > 0 and seen["reseated"] >= 4
        assert seen["endings"] == {"black", "white", "draw_limit", "draw_novalid"}
        if frac < 1.0:
            assert seen["resigned"] > 0 and tally[0] == seen["resigned"] and tally[6] >= MIN_MOVES * tally[0]
            if self.consecutive == 1:
                assert seen["first_eligible"] > 0           # p = MIN_MOVES resigns, p = MIN_MOVES - 1 never did
            if self.consecutive == 1 or self.streak == "side":
                assert tally[1] > 0 and tally[2] > 0        # both colours resign
        else:
            assert seen["resigned"] == 0 and tally[0] == 0
        if frac > 0.0:
            assert tally[3] > 0 and seen["latched"] > 0 and tally[5] > 0 and tally[7] > 0
            assert seen["fp_draw"] > 0                      # a would-be resigner that drew is a false positive
            if frac == 1.0:
                assert seen["true_positive"] > 0            # ... and one that lost is not
        else:
            assert tally[3] == 0 and tally[4] == 0
        if frac == 0.5:
            share = np.mean(list(self.pt.values()))
            assert 0.25 < share < 0.75
        else:
            assert set(self.pt.values()) == {frac == 1.0}
