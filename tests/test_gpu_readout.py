"""GPU: the tree read-out kernels of csrc/lz_engine.hip -- lz_tree_finish, lz_tree_finish_pruned, lz_tree_finish_gumbel,
lz_tree_solver_pick, lz_tree_move_pick, lz_tree_kld_check -- called through the C ABI on the hand-built roots of
tests/readout_cases.py (written into the arena by tests/hand_roots.py) and held to the restatements of
tests/readout_ref.py, which tests/test_readout_ref_cpu.py anchors on the reference.

Every output buffer starts as 0xA5 bytes and carries 8 guard rows on both sides; they, and every word the contract leaves
alone (child_* beyond a root's children, everything of a root a variant skips), must come back bit for bit.  Compared bit
for bit: integers, masks, codes, child_*, N', pruned_visits, picks, root_value, the Gumbel scores and vmix.  policy_dense of
the visit-count targets: 4 x the float32 oracle's own distance from the float64 restatement, measured in this run per
1 / T over all finish cases, never more than the 2e-6 of tests/test_gpu_tree.py (the 4: the kernel sums over a wave
butterfly and takes the device's logf / expf); one-hot rows bit for bit.  The Gumbel target is formed in double on both
sides and rounded once: at most 1 float32 ulp.  No network and no search anywhere in this file."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import hand_roots as H
from tests import kld_stop as kld
from tests import move_pick as mp
from tests import readout_cases as K
from tests import readout_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, FILL = 8, 0xA5
F32 = np.float32
CAP = 2e-6


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from liuzhou_amd import _lib
    return _lib


_BOUNDS = {}


def bounds():
    """Per 1 / T (0: one-hot): (the oracle's own distance, the kernel's bound)."""
    if not _BOUNDS:
        for key, d in K.oracle_distance(K.finish_launches()).items():
            _BOUNDS[key] = (d, min(4.0 * d, CAP))
    return _BOUNDS


class Buffers:
    """Named output buffers of B rows with guard rows, as the device sees them and as the restatement expects them."""

    def __init__(self, B, spec):
        self.B, self.spec, self.dev, self.want = B, spec, {}, {}
        for name, (dt, w) in spec.items():
            n = (B + 2 * GUARD) * w * np.dtype(dt).itemsize
            self.dev[name] = torch.full((n,), FILL, dtype=torch.uint8, device=DEV)
            self.want[name] = np.full(n, FILL, np.uint8).view(dt).reshape(B + 2 * GUARD, w)

    def ptr(self, name):
        dt, w = self.spec[name]
        return C.c_void_p(self.dev[name].data_ptr() + GUARD * w * np.dtype(dt).itemsize)

    def rows(self, name):
        return self.want[name][GUARD:GUARD + self.B]

    def got(self, name):
        dt, w = self.spec[name]
        return self.dev[name].cpu().numpy().view(dt).reshape(self.B + 2 * GUARD, w)

    def assert_bits(self, name, what):
        got, want = self.got(name), self.want[name]
        same = (got.view(np.uint8).reshape(len(got), -1) == want.view(np.uint8).reshape(len(want), -1)).all(1)
        assert same.all(), f"{what}: {name} differs in rows {(np.nonzero(~same)[0] - GUARD).tolist()[:12]} " \
                           f"(got {got[~same][:3].tolist()}, want {want[~same][:3].tolist()})"


def finish_spec(cap, pruned=False, gumbel=False):
    s = dict(policy=("<f4", 220), chosen_index=("<i4", 1), chosen_code=("<i4", 4), chosen_valid=("u1", 1), terminal=("u1", 1),
             root_value=("<f4", 1), child_count=("<i4", 1), child_action=("<i4", cap), child_visits=("<i4", cap),
             child_prior=("<f4", cap))
    if pruned:
        s.update(child_target_visits=("<i4", cap), pruned_visits=("<i4", 1))
    if gumbel:
        s.update(score=("<f8", cap), vmix=("<f8", 1))
    return s


def options(L):
    o = {}
    if "forced_k" in L:
        o.update(forced_k=L["forced_k"], root_noise=L["root_noise"])
        if L["table"] is not None:
            o["cpuct_table"] = L["table"]
    if "gl" in L:
        o.update(gumbel_m=L["m"], gumbel_gl=L["gl"], gumbel_base=L["base"], gumbel_root_value=L["v0"], root_noise=L["root_noise"],
                 gumbel_root_base=np.array([r["root_visits"] for r in L["roots"]], np.int32),
                 gumbel_c_visit=L["c_visit"], gumbel_c_scale=L["c_scale"])
    if "overrides" in L:
        o["root_proven"] = np.zeros(L["B"], np.int32)
    return o


def engine(L):
    return H.HandEngine(H.layout(L["roots"], options=options(L)), DEV, c_puct=L.get("c_puct", 1.0))


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def call_finish(lib, he, L, buf, variant="plain"):
    """One call of lz_tree_finish / _pruned / _gumbel into `buf`; returns the input tensors (kept alive by the caller)."""
    keep = [_up(L["temps"]), _up(L["target_temps"]), _up(L["force"]), _up(L["uniforms"])]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    args = [C.byref(he.engine.desc), p(keep[0]), p(keep[1]), C.c_float(float(L["beta"])), p(keep[2]),
            C.c_int(int(L["sample_moves"])), p(keep[3])] + \
           [buf.ptr(n) for n in ("policy", "chosen_index", "chosen_code", "chosen_valid", "terminal", "root_value", "child_count",
                                 "child_action", "child_visits", "child_prior")] + [C.c_int64(L["out_cap"])]
    stream = lib.stream_ptr(torch.device(DEV))
    if variant == "pruned":
        given = L["outputs"]
        rc = lib.lib().lz_tree_finish_pruned(*args, buf.ptr("child_target_visits") if given else None,
                                             buf.ptr("pruned_visits") if given else None, stream)
    elif variant == "gumbel":
        rc = lib.lib().lz_tree_finish_gumbel(*args, buf.ptr("score"), buf.ptr("vmix"), stream)
    else:
        rc = lib.lib().lz_tree_finish(*args, stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return keep


def expect_finish(L, buf, target_visits=None):
    """Fill `buf.want` with what lz_tree_finish writes; returns per game (float64 target row or None, bound key)."""
    rows = []
    for g, r in enumerate(L["roots"]):
        forced = bool(L["force"] is not None and L["force"][g])
        Tt = None if L["target_temps"] is None else L["target_temps"][g]
        o = R.ref_finish(r, temperature=L["temps"][g], target_temperature=Tt, beta=L["beta"], force_uniform=forced,
                         sample_moves=L["sample_moves"], uniform=None if L["uniforms"] is None else L["uniforms"][g],
                         out_cap=L["out_cap"], target_visits=None if target_visits is None else target_visits[g])
        buf.rows("terminal")[g] = int(o["terminal"])
        buf.rows("chosen_valid")[g] = int(o["chosen_valid"])
        buf.rows("chosen_index")[g] = o["chosen_index"]
        buf.rows("chosen_code")[g] = o["chosen_code"]
        buf.rows("child_count")[g] = o["child_count"]
        buf.rows("root_value")[g] = o["root_value"]
        buf.rows("policy")[g] = 0
        if o["terminal"]:
            rows.append((None, None))
            continue
        m = len(o["child_action"])
        buf.rows("child_action")[g, :m] = o["child_action"]
        buf.rows("child_visits")[g, :m] = o["child_visits"]
        buf.rows("child_prior")[g, :m] = o["child_prior"]
        t = L["temps"][g] if Tt is None else Tt
        rows.append((o["policy"], 0.0 if F32(t) <= R.T_EDGE else float(1.0 / np.float64(t))))
    return rows


def check_policy_row(what, row, pol, key, worst):
    if pol is None:
        assert not row.view(np.uint32).any(), (what, "a terminal root's row must be zeros")
    elif key == 0.0:
        assert np.array_equal(row, pol.astype(F32)), (what, "one-hot target")
    else:
        d = float(np.abs(row.astype(np.float64) - pol).max())
        worst[key] = max(worst.get(key, 0.0), d)
        assert d <= bounds()[key][1], (what, key, d, bounds()[key])
        assert not row[pol == 0].any(), (what, "mass outside the live children")


def check_policy(L, buf, rows, worst):
    got = buf.got("policy")
    assert (got[:GUARD].view(np.uint8) == FILL).all() and (got[-GUARD:].view(np.uint8) == FILL).all(), "policy guard rows"
    for g, (pol, key) in enumerate(rows):
        check_policy_row((L["name"], g), got[GUARD + g], pol, key, worst)


BIT_EXACT = ("chosen_index", "chosen_code", "chosen_valid", "terminal", "root_value", "child_count", "child_action",
             "child_visits", "child_prior")


@pytest.mark.parametrize("B", K.BATCHES)
def test_finish_equals_the_restatement(gpu, B):
    """ne 1 .. 72 mixed within a launch, both lane slots, every phase and mover, roots without edges and terminal roots in
    the first, a middle and the last slot; deterministic, sampled and forced-uniform picks; NULL / equal / different target
    temperatures; pseudocount 0, 0.5, 8; out_cap 72 and 36.  B = 1, 3 leave waves of the workgroup idle, 5 and 257 end
    inside one."""
    worst = {}
    for L in K.finish_launches():
        if L["B"] != B:
            continue
        he = engine(L)
        buf = Buffers(B, finish_spec(L["out_cap"]))
        rows = expect_finish(L, buf)
        keep = call_finish(gpu, he, L, buf)
        for name in BIT_EXACT:
            buf.assert_bits(name, L["name"])
        check_policy(L, buf, rows, worst)
        del keep
    print(f"B={B}: kernel's worst policy distance per 1/T {({k: f'{v:.3e}' for k, v in sorted(worst.items())})}; "
          f"oracle's own and bound {({k: (f'{a:.3e}', f'{b:.3e}') for k, (a, b) in sorted(bounds().items())})}")


def test_finish_twice_gives_the_same_bits(gpu):
    """No atomics and no order dependence in the stage: a second call writes the same bytes, policy_dense included."""
    L = K.finish_launches()[4]
    he = engine(L)
    a, b = Buffers(L["B"], finish_spec(L["out_cap"])), Buffers(L["B"], finish_spec(L["out_cap"]))
    k1, k2 = call_finish(gpu, he, L, a), call_finish(gpu, he, L, b)
    for name in a.spec:
        assert np.array_equal(a.got(name).view(np.uint8), b.got(name).view(np.uint8)), name


def _pruned_visits(L):
    out = []
    for g, r in enumerate(L["roots"]):
        if not K.prune_on(L, g):
            out.append(None)
            continue
        N = np.asarray(r["N"])
        q = R.child_q(r["W"], N, (np.asarray(r["info"]) & 1) != 0, r["player"])
        out.append(R.prune_targets(N, r["P"], q, r["root_visits"], L["forced_k"], K.prune_c(L, g)))
    return out


@pytest.mark.parametrize("B", (1, 3, 4, 5, 257))
def test_pruned_finish_equals_the_restatement(gpu, B):
    """Dyadic priors, forced_k and table entries: N * N at, one below and one above the threshold, gap <= 0, x < 0, x >= N, N'
    of exactly 1 and 2, c* tied and in the second slot, T = 0 / 1, the table index at and beyond its last entry, root_noise
    off, forced_k = 0 (then the plain finish's bytes), child_target_visits / pruned_visits NULL and given."""
    worst = {}
    for L in K.prune_launches():
        if L["B"] != B:
            continue
        he = engine(L)
        buf = Buffers(B, finish_spec(L["out_cap"], pruned=True))
        tv = _pruned_visits(L)
        rows = expect_finish(L, buf, tv)
        if L["outputs"]:
            for g, r in enumerate(L["roots"]):
                buf.rows("pruned_visits")[g] = 0 if tv[g] is None else int((np.asarray(r["N"]) - tv[g]).sum())
                if K.live(r):
                    m = min(r["ne"], L["out_cap"])
                    buf.rows("child_target_visits")[g, :m] = (np.asarray(r["N"]) if tv[g] is None else tv[g])[:m]
        keep = call_finish(gpu, he, L, buf, "pruned")
        for name in BIT_EXACT + ("child_target_visits", "pruned_visits"):
            buf.assert_bits(name, L["name"])
        check_policy(L, buf, rows, worst)
        del keep
    print(f"pruned B={B}: kernel's worst policy distance per 1/T {({k: f'{v:.3e}' for k, v in sorted(worst.items())})}")


@pytest.mark.parametrize("B", (1, 3, 5, 257))
def test_solver_pick_equals_the_restatement(gpu, B):
    """Behind a deterministic lz_tree_finish: wins by terminal and by proven bit through both mover combinations, several wins
    with tied visits across the slots, the picked child lost with and without another child, every child lost, no decided
    child, force_uniform set, `overrides` NULL and pre-loaded.  Everything but the three pick arrays stays as the finish
    wrote it."""
    for L in K.solver_launches():
        if L["B"] != B:
            continue
        he = engine(L)
        spec = dict(finish_spec(L["out_cap"]), overrides=("<i4", 1))
        buf = Buffers(B, spec)
        expect_finish(L, buf)
        keep = call_finish(gpu, he, L, buf)
        before = {n: buf.got(n).copy() for n in spec if n not in ("chosen_index", "chosen_code", "chosen_valid", "overrides")}
        changed = 0
        for g, r in enumerate(L["roots"]):
            buf.rows("overrides")[g] = 1000 + g
            if not K.live(r) or L["force"][g]:
                continue
            fin = int(buf.rows("chosen_index")[g, 0])
            a = R.solver_pick(r["act"], r["N"], K.solver_xs(r), fin)
            if a != fin:
                buf.rows("chosen_index")[g] = a
                buf.rows("chosen_code")[g] = R.index_to_code(r["phase"], a)
                buf.rows("chosen_valid")[g] = 1
                buf.rows("overrides")[g] += 1
                changed += 1
        if L["overrides"]:
            buf.dev["overrides"].view(torch.int32)[GUARD:GUARD + B] = torch.arange(1000, 1000 + B, dtype=torch.int32, device=DEV)
        rc = gpu.lib().lz_tree_solver_pick(C.byref(he.engine.desc), C.c_void_p(keep[2].data_ptr()), buf.ptr("chosen_index"),
                                           buf.ptr("chosen_code"), buf.ptr("chosen_valid"),
                                           buf.ptr("overrides") if L["overrides"] else None, gpu.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        assert rc == 0
        for name in ("chosen_index", "chosen_code", "chosen_valid") + (("overrides",) if L["overrides"] else ()):
            buf.assert_bits(name, L["name"])
        for n, was in before.items():
            assert np.array_equal(buf.got(n).view(np.uint8), was.view(np.uint8)), (L["name"], n)
        assert changed > 0 or B < 5
        print(f"{L['name']}: picks changed {changed}")


def _ulp_diff(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("B", (1, 3, 4, 5, 257))
def test_gumbel_finish_equals_the_restatement(gpu, B):
    """P = 0 children, all N = 0 (vmix = v0), Pv <= 0, L ties decided by the score and then by the index across the slots,
    force_uniform keeps the plain pick, games whose switch is off keep the plain finish's bytes, m below and above ne.
    Scores, vmix and picks bit for bit; the target within 1 float32 ulp."""
    for L in K.gumbel_launches():
        if L["B"] != B:
            continue
        he = engine(L)
        buf = Buffers(B, finish_spec(L["out_cap"], gumbel=True))
        rows = expect_finish(L, buf)
        buf.rows("score")[:] = 0
        buf.rows("vmix")[:] = 0
        targets = {}
        for g, r in enumerate(L["roots"]):
            if not K.live(r) or L["root_noise"][g] == 0:
                continue
            N, q, (pick, probs, score, vmix) = K.gumbel_row(L, g)
            buf.rows("score")[g, :r["ne"]] = score
            buf.rows("vmix")[g] = vmix
            if probs is not None:
                targets[g] = probs
            if not L["force"][g]:
                a = int(r["act"][pick])
                buf.rows("chosen_index")[g] = a
                buf.rows("chosen_code")[g] = R.index_to_code(r["phase"], a)
        keep = call_finish(gpu, he, L, buf, "gumbel")
        for name in BIT_EXACT + ("score", "vmix"):
            buf.assert_bits(name, L["name"])
        got = buf.got("policy")
        differ = total = 0
        for g, probs in targets.items():
            r = L["roots"][g]
            want = np.zeros(220, F32)
            want[r["act"]] = probs
            d = _ulp_diff(got[GUARD + g], want)
            assert d.max() <= 1, (L["name"], g, int(d.max()))
            differ += int((d > 0).sum()); total += r["ne"]
        assert (got[:GUARD].view(np.uint8) == FILL).all() and (got[-GUARD:].view(np.uint8) == FILL).all(), "policy guard rows"
        for g, (pol, key) in enumerate(rows):                    # games the rule leaves alone: the plain finish's row
            if g not in targets:
                check_policy_row((L["name"], g), got[GUARD + g], pol, key, {})
        print(f"{L['name']}: Gumbel target entries differing by 1 ulp: {differ} of {total}")
        del keep


def test_move_pick_on_wide_roots_equals_the_checker(gpu):
    """The checker's rule (tests/move_pick.py) on hand-built roots of 37, 60, 64, 65 and 72 children."""
    L = K.wide_launch(61)
    he = engine(L)
    B = L["B"]
    rng = np.random.default_rng(5)
    wide = 0
    for o, c in ((1.0, 0.0), (0.5, 0.25), (3.0, 1.0)):
        u = L["uniforms"].copy()
        res = {}
        for g, r in enumerate(L["roots"]):
            if not (K.live(r) and mp.applies(terminal=False, sample_moves=True, temperature=L["temps"][g],
                                             force_uniform=bool(L["force"][g]), offset=o, cutoff=c)):
                continue
            N = np.asarray(r["N"])
            q = R.child_q(r["W"], N, (np.asarray(r["info"]) & 1) != 0, r["player"])
            for _ in range(64):
                res[g] = mp.pick(N, q, L["temps"][g], u[g], o, c)
                if mp.margin_ok(res[g]):
                    break
                u[g] = F32(rng.uniform(0.001, 0.999))
            assert mp.margin_ok(res[g])
        Lc = dict(L, uniforms=u)
        buf = Buffers(B, dict(finish_spec(72), counters=("<i8", 4)))
        keep = call_finish(gpu, he, Lc, buf)
        fin = buf.got("chosen_index")[GUARD:GUARD + B, 0].copy()
        buf.want["chosen_index"][:] = buf.got("chosen_index")
        buf.want["chosen_code"][:] = buf.got("chosen_code")
        cnt = np.zeros(4, np.int64)
        for g, r_ in res.items():
            r = L["roots"][g]
            a = int(r["act"][r_["pick"]])
            cnt += [1, r_["cut_visits"], r_["cut_value"], int(a != fin[g])]
            if a != fin[g]:
                buf.rows("chosen_index")[g] = a
                buf.rows("chosen_code")[g] = R.index_to_code(r["phase"], a)
        buf.dev["counters"].view(torch.int64)[GUARD * 4:GUARD * 4 + 4] = 1000
        rc = gpu.lib().lz_tree_move_pick(C.byref(he.engine.desc), C.c_void_p(keep[0].data_ptr()), C.c_void_p(keep[2].data_ptr()),
                                         C.c_void_p(keep[3].data_ptr()), 1, C.c_double(o), C.c_double(c), buf.ptr("chosen_index"),
                                         buf.ptr("chosen_code"), buf.ptr("counters"), gpu.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        assert rc == 0
        buf.assert_bits("chosen_index", f"move pick o={o} c={c}")
        buf.assert_bits("chosen_code", f"move pick o={o} c={c}")
        got = buf.got("counters")
        assert (got[GUARD, :] - 1000).tolist() == cnt.tolist(), (o, c, got[GUARD].tolist(), cnt.tolist())
        assert (np.delete(got, GUARD, 0).view(np.uint8) == FILL).all()
        print(f"move pick o={o} c={c}: counters {cnt.tolist()}, wide picks {sum(r_['pick'] >= 64 for r_ in res.values())}")
        wide += sum(r_["pick"] >= 64 for r_ in res.values())
        assert cnt[0] > 0
    assert wide > 0


def test_kld_check_on_wide_roots_equals_the_checker(gpu):
    """One check of the rule (tests/kld_stop.py) on hand-built roots of 37 .. 72 children: the snapshot rows, the budgets and
    the counters; an inactive game, a game whose budget is spent and a terminal root are left alone."""
    L = K.wide_launch(62)
    B = L["B"]
    rng = np.random.default_rng(9)
    snap = np.full((B, 72), 7, np.int32)
    for g, r in enumerate(L["roots"]):
        N = np.asarray(r["N"])
        snap[g, :r["ne"]] = np.maximum(N - rng.integers(0, 3, r["ne"]), 0) if g % 3 else N        # (g % 3 == 0: no new visits)
    budget = np.array([3 if g % 9 == 4 else 40 for g in range(B)], np.int32)
    active = np.array([0 if g % 10 == 7 else 1 for g in range(B)], np.uint8)
    step, min_sims, theta = 8, 4, 2e-4
    o = dict(kld_snapshot=snap, kld_budget=budget, active=active, kld_threshold=theta, kld_interval=4, kld_min_sims=min_sims)
    he = H.HandEngine(H.layout(L["roots"], options=o), DEV)
    e = he.engine
    stops = torch.full((B,), 100, dtype=torch.int64, device=DEV)
    saved = torch.full((B,), 200, dtype=torch.int64, device=DEV)
    trace = torch.full((B,), -5.0, dtype=torch.float64, device=DEV)
    e.desc.kld_stops, e.desc.kld_saved, e.desc.kld_trace = stops.data_ptr(), saved.data_ptr(), trace.data_ptr()
    rc = gpu.lib().lz_tree_kld_check(C.byref(e.desc), C.c_int64(step), gpu.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    got_snap, got_budget = he.keep["kld_snapshot"].cpu().numpy(), he.keep["kld_budget"].cpu().numpy()
    got_stops, got_saved, got_trace = stops.cpu().numpy(), saved.cpu().numpy(), trace.cpu().numpy()
    n_stop = n_gain = 0
    for g, r in enumerate(L["roots"]):
        ne = r["ne"]
        if not active[g] or budget[g] <= step + 1:
            assert np.array_equal(got_snap[g], snap[g]) and got_budget[g] == budget[g] and got_stops[g] == 100, g
            continue
        # (a root marked terminal still has its edges: the rule reads nedges only)
        per, stop, new = kld.check(snap[g, :ne], r["N"], step, min_sims, theta)
        want_snap = np.zeros(72, np.int32)
        want_snap[:ne] = new
        assert np.array_equal(got_snap[g], want_snap), g
        assert got_budget[g] == (step + 1 if stop else budget[g]) and got_stops[g] == 100 + int(stop), g
        assert got_saved[g] == 200 + (int(budget[g]) - (step + 1) if stop else 0), g
        if per is None:
            assert got_trace[g] == -5.0, g
        else:
            assert abs(got_trace[g] - per) <= 1e-12 * max(1.0, abs(per)), (g, got_trace[g], per)
            n_gain += 1
        n_stop += int(stop)
    print(f"kld check on wide roots: gains formed {n_gain}, stops {n_stop}")
    assert n_gain >= 8 and 0 < n_stop < n_gain
