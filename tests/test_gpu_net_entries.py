"""GPU: the plumbing around the network kernel's arithmetic -- the packed-state entry against the planes entry on states
that separate the 11 planes, the rows a launch may write (sentinels behind the last row, several passes per workgroup, the
device-counted entry), values-only mode, and the depth limits of the descriptor (0, 1 and 47 residual blocks) against the
module in float64.  The arithmetic itself is pinned by tests/test_gpu_net.py; everything here that compares two launches
is exact (bit equality on int32 views, untouched sentinel bytes)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lz_oracle as O
from tests.golden_utils import FIELDS, load, perturb_bn, states
from tests.test_gpu_net import PROB_TOL, VALUE_TOL, VLOGIT_TOL, _planes
from tests.tree_parity import to_gpu_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.5
SENTINEL_BITS = int(np.float32(SENTINEL).view(np.int32))
OUTPUTS = (("lp1", 36), ("lp2", 36), ("lpm", 36), ("vl", 101), ("v", 0))

# (id, precision, MODEL_CONFIGS name, FusedNet arguments, samples per pass of that kernel shape)
CONFIGS = [("fp16-64x16", "fp16", "b6c64", {}, 16), ("fp16-64x8-half", "fp16", "b6c64", {"half_workgroups": True}, 8),
           ("fp16-128x8", "fp16", "b10c128", {"wide_tiles": False}, 8), ("fp16-128x8-wide", "fp16", "b10c128", {"wide_tiles": True}, 8),
           ("fp32-64", "fp32", "b6c64", {}, 4), ("fp32-128", "fp32", "b10c128", {}, 2),
           ("fp16x3-64", "fp16x3", "b6c64", {}, 4), ("fp16x3-128", "fp16x3", "b10c128", {}, 2)]
CONFIG_IDS = [c[0] for c in CONFIGS]

_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _net(cid):
    """(FusedNet, samples per pass) of a configuration, packed once."""
    if ("net", cid) not in _cache:
        from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
        from liuzhou_amd.net_hip import FusedNet
        _, precision, name, kw, S = CONFIGS[CONFIG_IDS.index(cid)]
        if ("model", name) not in _cache:
            torch.manual_seed(20260314)
            _cache[("model", name)] = perturb_bn(ChessNet(**MODEL_CONFIGS[name]).eval(), 5).to(DEV)
        _cache[("net", cid)] = (FusedNet(_cache[("model", name)], precision=precision, **kw), S)
    return _cache[("net", cid)]


def _state_set():
    """g1 (2 320 reachable states) + g2 (163 edge states) + g3 (1 500 garbage states) = 3 983 rows: the state fields, the
    expected planes from no kernel of this project (g2 / g3: the reference's own `model_input`; g1: the C oracle), the
    packed records and the planes on the device."""
    if "set" not in _cache:
        from liuzhou_amd import _lib as L
        parts, planes = [], []
        for name in ("g1_rules.npz", "g2_edges.npz", "g3_garbage.npz"):
            z = load(name)
            st = {f: np.asarray(v) for f, v in states(z, "s").items()}
            parts.append(st)
            planes.append(z["model_input"].astype(np.float32) if "model_input" in z.files else O.states_to_model_input(st))
        st = {f: np.ascontiguousarray(np.concatenate([p[f] for p in parts])) for f in FIELDS}
        want = np.ascontiguousarray(np.concatenate(planes))
        n = st["board"].shape[0]
        batch = to_gpu_batch(st, DEV)
        tensors = [t.contiguous() for t in batch.tensors()]
        packed = torch.zeros((n, 4), dtype=torch.int64, device=DEV)
        with torch.cuda.device(DEV):
            L.check(L.lib().lz_pack_states(C.byref(L.soa(tensors)), L.i64(n), L.ptr(packed), L.stream_ptr(DEV)), "pack_states")
        torch.cuda.synchronize()
        _cache["set"] = {"st": st, "want": want, "packed": packed, "planes": torch.from_numpy(want).to(DEV),
                         "sizes": [p["board"].shape[0] for p in parts]}
    return _cache["set"]


def _rows(n, seed=7):
    """n rows drawn from all over the state set (the same rows for every configuration) -> (planes, packed)."""
    s = _state_set()
    idx = torch.from_numpy(np.random.default_rng(seed).permutation(s["packed"].shape[0])[:n]).to(DEV)
    return s["planes"].index_select(0, idx).contiguous(), s["packed"].index_select(0, idx).contiguous()


def _launch(net, n, planes=None, packed=None, rows=None, max_blocks=0, count=None, heads=True, logits=True):
    """One launch through the C ABI over sentinel-filled outputs of `rows` rows (default n) -> {name: tensor}.
    `planes` -> lz_net_forward_f16, `packed` -> lz_net_forward_packed_f16, `packed` and `count` (a device int64) ->
    lz_net_forward_packed_counted_f16 with capacity n.  `heads` False: the three policy pointers are NULL; `logits` False:
    value_logits is NULL."""
    from liuzhou_amd import _lib as L
    from liuzhou_amd.net_hip import LzNetDesc
    rows = n if rows is None else rows
    desc = LzNetDesc()
    C.memmove(C.byref(desc), C.byref(net.desc), C.sizeof(LzNetDesc))
    desc.max_blocks = max_blocks
    out = {k: torch.full((rows, w) if w else (rows,), SENTINEL, device=DEV) for k, w in OUTPUTS}
    p = lambda k, on: L.ptr(out[k]) if on else None
    tail = (p("lp1", heads), p("lp2", heads), p("lpm", heads), p("vl", logits), L.ptr(out["v"]), L.stream_ptr(DEV))
    lib = L.lib()
    with torch.cuda.device(DEV):
        if planes is not None:
            rc = lib.lz_net_forward_f16(C.byref(desc), L.ptr(planes), L.i64(n), *tail)
        elif count is None:
            rc = lib.lz_net_forward_packed_f16(C.byref(desc), L.ptr(packed), L.i64(n), *tail)
        else:
            rc = lib.lz_net_forward_packed_counted_f16(C.byref(desc), L.ptr(packed), L.i64(n), L.ptr(count), *tail)
    L.check(rc, "net forward")
    torch.cuda.synchronize()
    if not heads:
        for k in ("lp1", "lp2", "lpm"):
            del out[k]
    if not logits:
        del out["vl"]
    return out


def _bits(t):
    return t.view(torch.int32)


def _same(got, want, n, what):
    """Rows below n of every output of `got` equal `want` bit for bit."""
    for k, g in got.items():
        assert torch.equal(_bits(g[:n]), _bits(want[k][:n])), (what, k)


def _untouched(got, n, what):
    """Rows at or beyond n of every output keep the sentinel's bytes."""
    for k, g in got.items():
        assert bool((_bits(g[n:]) == SENTINEL_BITS).all()), (what, k, "a row outside the call was written")


def _written(got, n, what):
    """Rows below n hold results (finite, and not the sentinel: the comparison of two launches is not vacuous)."""
    for k, g in got.items():
        assert bool(torch.isfinite(g[:n]).all()) and not bool((_bits(g[:n]) == SENTINEL_BITS).any()), (what, k)


# ---- A. packed entry == planes entry on states that separate the planes ------------------------------------------------
def test_state_set_separates_the_planes_and_ends_every_shape_on_a_partial_pass():
    """What the bit-equality below is worth: 3 983 rows (15 mod 16, 7 mod 8: the last pass of every shape is partial), all
    14 (phase, mover) pairs, for each mover states with black marks only, white marks only and both (a swap of the own /
    opponent mark planes shows), marks on empty cells and both colours' marks on one cell (the garbage states)."""
    _need_gpu()
    s = _state_set()
    st = s["st"]
    n = st["board"].shape[0]
    assert s["sizes"] == [2320, 163, 1500] and n == 3983 and n % 16 == 15 and n % 8 == 7 and n % 4 == 3 and n % 2 == 1
    phase, mover = st["phase"].astype(np.int64), st["current_player"].astype(np.int64)
    assert set(zip(phase.tolist(), mover.tolist())) == {(p, c) for p in range(1, 8) for c in (1, -1)}
    board = st["board"].reshape(n, 36)
    mb, mw = st["marks_black"].reshape(n, 36).astype(bool), st["marks_white"].reshape(n, 36).astype(bool)
    for c in (1, -1):
        m = mover == c
        assert (m & mb.any(1) & ~mw.any(1)).any() and (m & ~mb.any(1) & mw.any(1)).any() and (m & mb.any(1) & mw.any(1)).any()
        assert (m & (mb != mw).any(1)).any()
    assert ((mb | mw) & (board == 0)).any() and (mb & mw).any()
    assert (s["want"][:, 2] != s["want"][:, 3]).any() and (s["want"][:, 0] != s["want"][:, 1]).any()
    assert s["want"][:, 10].any()                                   # the last phase plane is set somewhere


def test_pack_then_unpack_to_planes_reproduces_the_reference_planes():
    """lz_pack_states followed by lz_packed_to_model_input gives the reference's own `model_input` of the edge and garbage
    states (and the C oracle's planes of the reachable ones): the packed records the entries below read are right."""
    _need_gpu()
    from liuzhou_amd import _lib as L
    s = _state_set()
    n = s["packed"].shape[0]
    out = torch.full((n, 11, 6, 6), SENTINEL, device=DEV)
    with torch.cuda.device(DEV):
        L.check(L.lib().lz_packed_to_model_input(L.ptr(s["packed"]), L.i64(n), L.ptr(out), L.stream_ptr(DEV)),
                "packed_to_model_input")
    got = out.cpu().numpy()
    lo = 0
    for name, k in zip(("g1", "g2", "g3"), s["sizes"]):
        assert np.array_equal(got[lo:lo + k], s["want"][lo:lo + k]), name
        lo += k


@pytest.mark.parametrize("cid", CONFIG_IDS)
def test_packed_entry_equals_planes_entry_bit_for_bit(cid):
    """lz_net_forward_packed_f16(pack(states)) == lz_net_forward_f16(planes) on the whole state set, all five outputs, and
    in values-only mode: both entries stage the same rows (0 / 1 are exact in fp16 and fp32), so there is no tolerance.
    The expected planes come from the reference / the oracle, not from a kernel of this project."""
    _need_gpu()
    net, _ = _net(cid)
    s = _state_set()
    n = s["packed"].shape[0]
    a = _launch(net, n, planes=s["planes"])
    b = _launch(net, n, packed=s["packed"])
    _written(a, n, cid)
    _same(b, a, n, (cid, "packed entry differs from the planes entry"))
    va = _launch(net, n, planes=s["planes"], heads=False, logits=False)
    vb = _launch(net, n, packed=s["packed"], heads=False, logits=False)
    assert list(va) == ["v"] and torch.equal(_bits(va["v"]), _bits(a["v"])), (cid, "values-only, planes entry")
    assert torch.equal(_bits(vb["v"]), _bits(a["v"])), (cid, "values-only, packed entry")


# ---- B. rows outside the call, the pass loop, the counted entry -------------------------------------------------------------
@pytest.mark.parametrize("cid", CONFIG_IDS)
def test_nothing_behind_the_last_row_is_written_and_every_grid_gives_the_same_rows(cid):
    """N = 5 S + 3 and N = S - 1 rows (S = samples per pass) into outputs of N + 2 S sentinel rows, planes and packed entry,
    on the default grid and on 1 and 3 workgroups (1: one workgroup runs six passes, the last one partial): rows at or
    beyond N keep the sentinel's bytes on all five outputs, rows below N are the default grid's bit for bit."""
    _need_gpu()
    net, S = _net(cid)
    for n in (5 * S + 3, S - 1):
        rows = n + 2 * S
        planes, packed = _rows(rows)
        ref = None
        for entry in ("planes", "packed"):
            for max_blocks in (0, 1, 3):
                what = (cid, n, entry, max_blocks)
                got = _launch(net, n, planes=planes if entry == "planes" else None,
                              packed=packed if entry == "packed" else None, rows=rows, max_blocks=max_blocks)
                _untouched(got, n, what)
                _written(got, n, what)
                if ref is None:
                    ref = got
                _same(got, ref, n, what)


@pytest.mark.parametrize("cid", CONFIG_IDS)
def test_counted_entry_writes_the_first_count_rows_only(cid):
    """lz_net_forward_packed_counted_f16 (the list-mode launch) with capacity 5 S + 3 and the count on the device: rows below
    min(count, capacity) equal the plain packed launch bit for bit, every other row keeps its sentinel -- for counts of 0,
    1, around one pass, the capacity, and 7 more than the capacity (clamped)."""
    _need_gpu()
    net, S = _net(cid)
    cap = 5 * S + 3
    rows = cap + 2 * S
    _, packed = _rows(rows)
    ref = _launch(net, cap, packed=packed)
    _written(ref, cap, cid)
    for cnt in sorted({0, 1, S - 1, S, S + 1, cap, cap + 7}):
        count = torch.tensor([cnt], dtype=torch.int64, device=DEV)
        for max_blocks in (0, 1):
            got = _launch(net, cap, packed=packed, rows=rows, count=count, max_blocks=max_blocks)
            live = min(cnt, cap)
            _same(got, ref, live, (cid, cnt, max_blocks))
            _untouched(got, live, (cid, cnt, max_blocks))
        assert int(count.item()) == cnt                            # the count is read, never written


@pytest.mark.parametrize("cid", CONFIG_IDS)
def test_values_only_on_the_packed_entry(cid):
    """The three policy pointers NULL on the packed entry: `value` (and the value logits, when asked for) equal the full
    forward bit for bit, rows behind the last one stay untouched; a partial last pass and several passes per workgroup."""
    _need_gpu()
    net, S = _net(cid)
    n = 5 * S + 3
    rows = n + 2 * S
    _, packed = _rows(rows)
    full = _launch(net, n, packed=packed)
    for max_blocks in (0, 1):
        only_v = _launch(net, n, packed=packed, rows=rows, heads=False, logits=False, max_blocks=max_blocks)
        assert list(only_v) == ["v"]
        _same(only_v, full, n, (cid, max_blocks, "value"))
        _untouched(only_v, n, (cid, max_blocks, "value"))
        with_logits = _launch(net, n, packed=packed, rows=rows, heads=False, max_blocks=max_blocks)
        assert sorted(with_logits) == ["v", "vl"]
        _same(with_logits, full, n, (cid, max_blocks, "value + logits"))
        _untouched(with_logits, n, (cid, max_blocks, "value + logits"))


# ---- C. depth limits against the module in float64 --------------------------------------------------------------------------
ARCHS = [(64, 0), (64, 1), (64, 47), (128, 0), (128, 47)]
N_DEPTH = 24


def _depth_case(channels, blocks):
    """(module on the device, planes, packed records of the same 24 positions, float64 reference on the CPU: three log-prob
    heads, value logits, value)."""
    key = ("depth", channels, blocks)
    if key not in _cache:
        from liuzhou_amd import _lib as L
        from liuzhou_amd.net import ChessNet, bucket_logits_to_scalar
        torch.manual_seed(11)
        m = perturb_bn(ChessNet(trunk_channels=channels, num_blocks=blocks).eval(), 100 + blocks)
        x = _planes(N_DEPTH, seed=47)
        # the same positions as packed records (the rows _planes draws)
        st_all = states(load("g1_rules.npz"), "s")
        idx = np.random.default_rng(47).integers(0, st_all["board"].shape[0], N_DEPTH)
        st = {f: np.ascontiguousarray(np.asarray(st_all[f])[idx]) for f in FIELDS}
        assert np.array_equal(x.cpu().numpy(), O.states_to_model_input(st))
        tensors = [t.contiguous() for t in to_gpu_batch(st, DEV).tensors()]
        packed = torch.zeros((N_DEPTH, 4), dtype=torch.int64, device=DEV)
        with torch.cuda.device(DEV):
            L.check(L.lib().lz_pack_states(C.byref(L.soa(tensors)), L.i64(N_DEPTH), L.ptr(packed), L.stream_ptr(DEV)), "pack_states")
        torch.cuda.synchronize()
        m64 = copy.deepcopy(m).double()
        with torch.inference_mode():
            r = m64(x.cpu().double())
            ref = (*r, bucket_logits_to_scalar(r[3]))
        _cache[key] = (m.to(DEV), x, packed, ref)
    return _cache[key]


def _depth_net(channels, blocks, precision):
    """The FusedNet of a depth case in one precision, packed once (both depth tests use it)."""
    key = ("depth net", channels, blocks, precision)
    if key not in _cache:
        from liuzhou_amd.net_hip import FusedNet
        _cache[key] = FusedNet(_depth_case(channels, blocks)[0], precision=precision)
    return _cache[key]


def _depth_outputs(net, x):
    lp1, lp2, lpm, vl = net(x)
    return tuple(t.double().cpu() for t in (lp1, lp2, lpm, vl, net.last_value))


@pytest.mark.parametrize("precision", ["fp32", "fp16x3", "fp16"])
@pytest.mark.parametrize("channels,blocks", ARCHS)
def test_depth_limits_against_the_float64_module(channels, blocks, precision):
    """0 and 1 residual blocks (the "no block" path: LzNetDesc.off_block0 has nothing to point at) and 47 (the descriptor's
    96 layer offsets filled to the last one) against the module in float64 on the host.
    fp32 / fp16x3: <= 1e-5 on the three log-prob heads, the value logits and the value (the bar of
    test_deeper_nets_than_15_blocks_run_the_fused_kernels; torch's own fp32 module is 3e-7 from float64 at 47 blocks).
    fp16 at 0 and 1 block: the 6-block bounds of tests/test_gpu_net.py (fewer roundings than at 6 blocks).
    fp16 at 47 blocks: no more than 4 x what torch.autocast(float16) of the same module on the same inputs loses against
    float64, + 1e-5, on probabilities and on the value (as test_fused_fp16_kernel_on_trained_scale_activations: two valid
    fp16 evaluations differ from each other about as much as from the exact result)."""
    _need_gpu()
    from liuzhou_amd.net import bucket_logits_to_scalar
    from liuzhou_amd.net_hip import MAX_BLOCKS, fused_supported
    m, x, _, ref = _depth_case(channels, blocks)
    assert fused_supported(m) and blocks <= MAX_BLOCKS == 47
    net = _depth_net(channels, blocks, precision)
    assert len(net.pack.layer_offsets) == 2 + 2 * blocks == net.desc.num_layers
    if blocks == 47:
        assert len(net.pack.layer_offsets) == 96 == len(net.desc.layer_offsets)
        assert [net.desc.layer_offsets[i] for i in range(96)] == [int(o) for o in net.pack.layer_offsets]
    got = _depth_outputs(net, x)
    for t in got:
        assert bool(torch.isfinite(t).all()), (precision, "inf / NaN")
    d_lp = max(float((got[k] - ref[k]).abs().max()) for k in range(3))
    d_prob = max(float((got[k].exp() - ref[k].exp()).abs().max()) for k in range(3))
    d_vl, d_v = float((got[3] - ref[3]).abs().max()), float((got[4] - ref[4]).abs().max())
    print(f"{channels} x {blocks} {precision} vs float64: max |dlog-prob| {d_lp:.2e}, |dprob| {d_prob:.2e}, "
          f"|dvalue logits| {d_vl:.2e}, |dvalue| {d_v:.2e}")
    if precision != "fp16":
        assert d_lp <= 1e-5 and d_vl <= 1e-5 and d_v <= 1e-5, (precision, d_lp, d_vl, d_v)
    elif blocks <= 1:
        assert d_prob < PROB_TOL and d_vl < VLOGIT_TOL and d_v < VALUE_TOL, (d_prob, d_vl, d_v)
    else:
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.float16):
            r16 = tuple(t.double().cpu() for t in m(x))
        a_prob = max(float((r16[k].exp() - ref[k].exp()).abs().max()) for k in range(3))
        a_v = float((bucket_logits_to_scalar(r16[3]) - ref[4]).abs().max())
        print(f"   autocast(float16) of the module vs float64: max |dprob| {a_prob:.2e}, |dvalue| {a_v:.2e}")
        # observed on MI355X, max error against float64 on the 24 positions (kernel | autocast(float16) of the module):
        #    64 x 47:  |dprob| 9.18e-06 | 2.43e-05    |dvalue| 3.98e-06 | 1.01e-05
        #   128 x 47:  |dprob| 8.36e-06 | 3.20e-05    |dvalue| 2.92e-06 | 1.30e-05
        # (the kernel loses 0.2 - 0.4 x what autocast loses, against the 4 x allowed)
        assert d_prob <= 4.0 * a_prob + 1e-5 and d_v <= 4.0 * a_v + 1e-5, (d_prob, a_prob, d_v, a_v)


@pytest.mark.parametrize("precision", ["fp16", "fp32", "fp16x3"])
@pytest.mark.parametrize("blocks", [0, 47])
def test_packed_entry_at_the_depth_limits(blocks, precision):
    """The packed entry of a 64-channel net without a block and with 47: bit-equal to the planes entry on all five outputs."""
    _need_gpu()
    _, x, packed, _ = _depth_case(64, blocks)
    net = _depth_net(64, blocks, precision)
    a = _launch(net, N_DEPTH, planes=x, rows=N_DEPTH + 16)
    b = _launch(net, N_DEPTH, packed=packed, rows=N_DEPTH + 16)
    _written(a, N_DEPTH, (blocks, precision))
    _same(b, a, N_DEPTH, (blocks, precision))
    _untouched(a, N_DEPTH, (blocks, precision, "planes"))
    _untouched(b, N_DEPTH, (blocks, precision, "packed"))
