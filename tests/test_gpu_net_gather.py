"""GPU: the gathering network launch (lz_net_forward_packed_gather_f16) against the plain packed forward, and the list
search on that launch (LZ_TREE_GATHER=1) against the same search on the scan path (LZ_TREE_GATHER=0)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.golden_utils import FIELDS, load, states
from tests.live_patterns import PATTERNS, SIZES, live_pattern
from tests.tree_parity import to_gpu_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (0, 2, 3, 4)                      # the LeafKind values that are not "leaf to expand" (1)
SENTINEL = -12345.5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


_cache = {}


def _packed(n):
    """n packed states from the rule fixtures (the same ones for every test)."""
    if "packed" not in _cache:
        from liuzhou_amd import _lib as L
        st_all = states(load("g1_rules.npz"), "s")
        idx = np.random.default_rng(11).integers(0, st_all["board"].shape[0], max(SIZES))
        batch = to_gpu_batch({f: np.ascontiguousarray(np.asarray(st_all[f])[idx]) for f in FIELDS}, DEV)
        out = torch.zeros((max(SIZES), 4), dtype=torch.int64, device=DEV)
        s = L.soa([t.contiguous() for t in batch.tensors()])
        with torch.cuda.device(DEV):
            L.check(L.lib().lz_pack_states(C.byref(s), L.i64(max(SIZES)), L.ptr(out), L.stream_ptr(DEV)), "pack_states")
        _cache["packed"] = out
    return _cache["packed"][:n]


def _net(model, shape):
    """(network, its plain forward of all the states: the reference, computed once per network and left alone)"""
    key = (model, shape)
    if key not in _cache:
        from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
        from liuzhou_amd.net_hip import FusedNet
        torch.manual_seed(20260314)
        net = FusedNet(ChessNet(**MODEL_CONFIGS[model]).eval().to(DEV), half_workgroups=shape == "half",
                       wide_tiles=shape == "wide")
        n = max(SIZES)
        ref = {"lp1": torch.empty((n, 36), device=DEV), "lp2": torch.empty((n, 36), device=DEV),
               "lpm": torch.empty((n, 36), device=DEV), "vl": torch.empty((n, 101), device=DEV), "v": torch.empty((n,), device=DEV)}
        from liuzhou_amd import _lib as L
        with torch.cuda.device(DEV):
            L.check(L.lib().lz_net_forward_packed_f16(C.byref(net.desc), L.ptr(_packed(n)), L.i64(n), L.ptr(ref["lp1"]),
                                                      L.ptr(ref["lp2"]), L.ptr(ref["lpm"]), L.ptr(ref["vl"]), L.ptr(ref["v"]),
                                                      L.stream_ptr(DEV)), "net_forward_packed_f16")
        torch.cuda.synchronize()
        _cache[key] = (net, ref)
    return _cache[key]


def _kinds(live, seed):
    """int32[B] leaf kinds: 1 where live, one of the four other kinds elsewhere."""
    other = np.asarray(KINDS)[np.random.default_rng(seed).integers(0, len(KINDS), len(live))]
    return np.where(live, 1, other).astype(np.int32)


def _gather(net, max_blocks, packed, kind_np):
    """One gathering launch over sentinel-filled outputs -> (outputs, count)."""
    import copy
    from liuzhou_amd import _lib as L
    from liuzhou_amd.net_hip import LzNetDesc
    B = len(kind_np)
    desc = LzNetDesc()
    C.memmove(C.byref(desc), C.byref(net.desc), C.sizeof(LzNetDesc))
    desc.max_blocks = max_blocks
    kind = torch.from_numpy(kind_np).to(DEV)
    out = {"lp1": torch.full((B, 36), SENTINEL, device=DEV), "lp2": torch.full((B, 36), SENTINEL, device=DEV),
           "lpm": torch.full((B, 36), SENTINEL, device=DEV), "vl": torch.full((B, 101), SENTINEL, device=DEV),
           "v": torch.full((B,), SENTINEL, device=DEV)}
    count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    with torch.cuda.device(DEV):
        L.check(L.lib().lz_net_forward_packed_gather_f16(C.byref(desc), L.ptr(packed), L.ptr(kind), L.i64(B), L.ptr(count),
                                                         L.ptr(out["lp1"]), L.ptr(out["lp2"]), L.ptr(out["lpm"]),
                                                         L.ptr(out["vl"]), L.ptr(out["v"]), L.stream_ptr(DEV)),
                "net_forward_packed_gather_f16")
    return out, count


def _check(net, ref, max_blocks, B, live, what):
    kind_np = _kinds(live, B)
    out, count = _gather(net, max_blocks, _packed(B), kind_np)
    lv = torch.from_numpy(live).to(DEV)
    assert int(count.item()) == int(live.sum()), what
    for name, got in out.items():
        want = ref[name][:B]
        g, w = got.view(torch.int32), want.view(torch.int32)       # byte for byte
        assert torch.equal(g[lv], w[lv]), (what, name, "live slots differ from the plain forward")
        assert bool((got[~lv] == SENTINEL).all()), (what, name, "a slot that is not live was written")


@pytest.mark.parametrize("model,shape,max_blocks", [("b6c64", "full", 0), ("b6c64", "full", 2), ("b10c128", "full", 0),
                                                     ("b10c128", "full", 2), ("b6c64", "half", 0), ("b6c64", "half", 2),
                                                     ("b10c128", "wide", 0), ("b10c128", "wide", 2)])
def test_gather_entry_equals_plain_forward_on_live_slots(model, shape, max_blocks):
    """Every size and pattern of tests/test_live_gather_cpu.py, kinds drawn from all five LeafKind values: live slots equal
    lz_net_forward_packed_f16 of the same states byte for byte on all five outputs, every other slot keeps its sentinel,
    count_out is the number of live flags (0 included).  max_blocks = 2: several rounds per workgroup, and workgroups
    without a pass, at these sizes."""
    _need_gpu()
    net, ref = _net(model, shape)
    for B in SIZES:
        for pattern in PATTERNS:
            _check(net, ref, max_blocks, B, live_pattern(pattern, B), (model, shape, max_blocks, B, pattern))


@pytest.mark.parametrize("even", ["1", "0"])
@pytest.mark.parametrize("model,shape,S", [("b6c64", "full", 16), ("b10c128", "full", 8), ("b6c64", "half", 8),
                                            ("b10c128", "wide", 8)])
def test_gather_entry_around_one_pass(monkeypatch, model, shape, S, even):
    """Live counts of S - 1, S and S + 1 (S = samples per pass), of 2 S +- 1 and of 7 S + 1, scattered over 513 slots, on
    all, 2 and 5 workgroups; with even rounds (LZ_NET_EVEN_ROUNDS, the default: 8 passes on 5 workgroups run on 4) and
    without."""
    _need_gpu()
    monkeypatch.setenv("LZ_NET_EVEN_ROUNDS", even)
    net, ref = _net(model, shape)
    B = 513
    for n in (S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 7 * S + 1):
        for max_blocks in (0, 2, 5):
            live = np.zeros(B, dtype=bool)
            live[np.random.default_rng(100 + n).choice(B, n, replace=False)] = True
            _check(net, ref, max_blocks, B, live, (model, shape, max_blocks, n))


def test_gather_entry_values_only_and_refusals():
    """Values only (no policy outputs) works like the plain forward; the parity networks and a batch beyond the kernel's
    LDS are refused with LZ_ERR_UNSUPPORTED, bad arguments with LZ_ERR_ARG, and nothing is launched."""
    _need_gpu()
    from liuzhou_amd import _lib as L
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    net, ref = _net("b6c64", "full")
    B = 65
    live = live_pattern("random75", B)
    kind = torch.from_numpy(_kinds(live, 3)).to(DEV)
    v = torch.full((B,), SENTINEL, device=DEV)
    count = torch.zeros((1,), dtype=torch.int64, device=DEV)
    fn = L.lib().lz_net_forward_packed_gather_f16
    with torch.cuda.device(DEV):
        args = (L.ptr(_packed(B)), L.ptr(kind), L.i64(B), L.ptr(count), None, None, None, None, L.ptr(v), L.stream_ptr(DEV))
        assert fn(C.byref(net.desc), *args) == 0
        lv = torch.from_numpy(live).to(DEV)
        assert torch.equal(v[lv].view(torch.int32), ref["v"][:B][lv].view(torch.int32)) and bool((v[~lv] == SENTINEL).all())
        assert int(count.item()) == int(live.sum())
        torch.manual_seed(1)
        net32 = FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV), precision="fp32")
        assert fn(C.byref(net32.desc), *args) == -2
        assert fn(C.byref(net.desc), L.ptr(_packed(B)), L.ptr(kind), L.i64(1 << 20), L.ptr(count), None, None, None, None,
                  L.ptr(v), L.stream_ptr(DEV)) == -2
        assert fn(C.byref(net.desc), L.ptr(_packed(B)), None, L.i64(B), L.ptr(count), None, None, None, None, L.ptr(v),
                  L.stream_ptr(DEV)) == -1
        assert fn(C.byref(net.desc), L.ptr(_packed(B)), L.ptr(kind), L.i64(B), None, None, None, None, None, L.ptr(v),
                  L.stream_ptr(DEV)) == -1
    torch.cuda.synchronize()


# ---- the search: gathering launch against the scan path, each in a fresh child process ---------------------------------
@pytest.fixture(scope="module")
def children(tmp_path_factory):
    _need_gpu()
    d = tmp_path_factory.mktemp("gather")
    procs = {}
    for flag in ("1", "0"):                                          # both at once: two processes on the device
        env = dict(os.environ)
        env["LZ_TREE_GATHER"] = flag
        env.pop("LZ_TREE_SPLIT", None)
        procs[flag] = subprocess.Popen([sys.executable, "-m", "tests.gather_search_child", str(d / f"g{flag}.npz")], cwd=ROOT,
                                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for flag, p in procs.items():
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0, (flag, se[-3000:])
        out[flag] = dict(np.load(d / f"g{flag}.npz"))
    return out["1"], out["0"]


def _same(a, b, prefix):
    keys = sorted(k for k in a if k.startswith(prefix + ".") and not k.endswith("live_row_touched"))
    assert keys and keys == sorted(k for k in b if k.startswith(prefix + ".") and not k.endswith("live_row_touched"))
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("scenario", ["plain", "split", "forced", "gumbel"])
def test_search_on_the_gathering_launch_equals_the_scan_path(children, scenario):
    """70 games, 24 simulations, kept subtrees over 3 moves, LZ_TREE_GATHER=1 against 0: the same trees (every node's state
    and parent, every edge run's visits, value sums, priors; root values, policies and chosen moves after every move) and
    the same live_count[: sims + 1].  "plain": the one-wave step; "split": the two-wave step and the 128-channel network.
    "forced": forced playouts at the root; "gumbel": the Gumbel root search over 8 considered moves.
    The gathering side never ran the scan (live_row and live_state untouched), the other side did."""
    got, ref = children
    _same(got, ref, scenario)
    assert not bool(got[scenario + ".live_row_touched"]) and bool(ref[scenario + ".live_row_touched"])
    assert int(got[scenario + ".lists"]) == 3 and bool(got[scenario + ".graph"])
    counts = np.stack([got[f"{scenario}.m{m}.live_count"] for m in range(3)])
    assert (counts > 0).any() and (counts <= 70).all()
    assert int(got[f"{scenario}.m2.n_nodes"].max()) > 1
    assert int(got[scenario + ".leaf_evals"]) == int(counts.sum())    # what tree_engine.py sums into leaf_evals


def test_search_with_the_playout_cap_on_the_gathering_launch(children):
    """Budgets of 6 and 24 simulations mixed: the games whose budget is spent leave the launches mid-search on both paths
    alike."""
    got, ref = children
    _same(got, ref, "cap")
    assert not bool(got["cap.live_row_touched"])
    full, fast = (int(x) for x in got["cap.cap_counts"])
    assert full > 0 and fast > 0
    c = got["cap.m0.live_count"]
    assert c[8:].max() < c[:6].max()                                 # the fast searches have left


def test_search_with_kld_stopping_on_the_gathering_launch(children):
    """The playout cap's budgets with KLD-gain early stopping on top (a check every 4 simulations): the checks lower the
    budgets between the launches on both paths alike."""
    got, ref = children
    _same(got, ref, "kld")


def test_search_of_finished_games_launches_nothing(children):
    """Every root a finished game: every launch's count is 0 on both paths, nothing is evaluated, nothing is picked."""
    got, ref = children
    _same(got, ref, "terminal")
    for m in range(3):
        assert (got[f"terminal.m{m}.live_count"] == 0).all()
        assert (got[f"terminal.m{m}.chosen"] == -1).all()
    assert int(got["terminal.leaf_evals"]) == 0


def test_captured_search_replayed_twice_equals_direct_launches(children):
    """The gathering search as a hipGraph (the continued search is captured at the second move and replayed again at the
    third) and with direct launches: identical trees and counts."""
    got, _ = children
    assert bool(got["plain.graph"]) and not bool(got["direct.graph"])
    keys = sorted(k[len("plain."):] for k in got if k.startswith("plain.") and not k.endswith(".graph"))
    assert keys == sorted(k[len("direct."):] for k in got if k.startswith("direct.") and not k.endswith(".graph"))
    for k in keys:
        assert got["plain." + k].tobytes() == got["direct." + k].tobytes(), k
