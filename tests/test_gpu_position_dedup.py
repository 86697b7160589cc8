"""GPU: the position-dedup kernels (csrc/lz_dedup.hip) through the C ABI and through liuzhou_amd/position_dedup.py
against the numpy restatement (tests/position_dedup.py) and the host build, bit for bit; the trainer's merge step."""
import ctypes as C

import numpy as np
import pytest
import torch

from liuzhou_amd import _lib as L
from liuzhou_amd import position_dedup as D
from liuzhou_amd import symmetry as SY
from tests import position_dedup as PD
from tests.golden_utils import load, states, unpack_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20261019
FIVE = ("planes", "masks", "policy", "value", "soft")
STATS = D.STAT_KEYS + ("mode", "max_copies")
SENTINEL, PAD = 0xA5, 256
CASES = ((False, "exact"), (True, "symmetric"), (True, "exact"))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def grids():
    """(rows, keys, sym, not representable, group_of_row, order, group_begin, merged groups) of every case, computed once
    by the restatement and left unchanged."""
    out = {}
    for spread, mode in CASES:
        rows = PD.grid(SEED, spread)
        keys, sym, bad = PD.keys(rows["planes"], rows["masks"], mode == "symmetric")
        gor, order, begin = PD.group(keys)
        out[spread, mode] = (rows, keys, sym, bad, gor, order, begin,
                             PD.merge_groups(*(rows[f] for f in FIVE), sym, order, begin))
    return out


class _Guarded:
    """A device buffer of `nbytes` followed by sentinel bytes."""

    def __init__(self, nbytes: int) -> None:
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + PAD,), SENTINEL, dtype=torch.uint8, device=DEV)

    def ptr(self):
        return C.c_void_p(self.raw.data_ptr())

    def view(self, dtype, shape):
        return self.raw[:self.nbytes].view(dtype).view(shape).cpu().numpy()

    def intact(self) -> bool:
        return bool((self.raw[self.nbytes:] == SENTINEL).all())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return L.stream_ptr(torch.device(DEV))


def _device_keys(rows, symmetric, n=None):
    n = len(rows["value"]) if n is None else n
    pl, mk = _dev(rows["planes"].reshape(-1, 396)), _dev(rows["masks"])
    keys, sym, bad = _Guarded(n * 64), _Guarded(n), _Guarded(4)
    bad.raw[:4] = 0

    def launch():
        st = L.lib().lz_dedup_position_keys(L.ptr(pl), L.ptr(mk), n, 1 if symmetric else 0, keys.ptr(), sym.ptr(),
                                            bad.ptr(), _stream())
        torch.cuda.synchronize()
        return st
    return launch, keys, sym, bad


def _device_merge(rows, sym, order, begin):
    n, G = len(rows["value"]), len(begin) - 1
    ins = [_dev(rows["planes"].reshape(-1, 396)), _dev(rows["masks"]), _dev(rows["policy"]), _dev(rows["value"]),
           _dev(rows["soft"])]
    d_sym, d_order, d_begin = _dev(sym), _dev(order), _dev(begin)
    outs = [_Guarded(G * 1584), _Guarded(G * 220), _Guarded(G * 880), _Guarded(G * 4), _Guarded(G * 4), _Guarded(G * 4)]

    def launch():
        st = L.lib().lz_dedup_merge_groups(*[L.ptr(t) for t in ins], n, L.ptr(d_sym), L.ptr(d_order), L.ptr(d_begin), G,
                                           *[o.ptr() for o in outs], _stream())
        torch.cuda.synchronize()
        return st

    def read():
        return [outs[0].view(torch.float32, (G, 11, 36)), outs[1].view(torch.uint8, (G, 220)),
                outs[2].view(torch.float32, (G, 220)), outs[3].view(torch.float32, (G,)),
                outs[4].view(torch.float32, (G,)), outs[5].view(torch.int32, (G,))]
    return launch, read, outs


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- both kernels through the C ABI -------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread,mode", CASES)
def test_keys_kernel_matches_the_restatement_and_the_host_build(grids, spread, mode):
    _need_gpu()
    rows, keys, sym, bad = grids[spread, mode][:4]
    n = len(sym)
    assert n <= 4096
    launch, d_keys, d_sym, d_bad = _device_keys(rows, mode == "symmetric")
    assert launch() == 0
    got = d_keys.view(torch.int64, (n, 8)), d_sym.view(torch.int8, (n,)), d_bad.view(torch.int32, (1,))
    assert np.array_equal(got[0], keys) and np.array_equal(got[1], sym) and int(got[2][0]) == bad == 6
    assert d_keys.intact() and d_sym.intact() and d_bad.intact()
    hk, hs, hb = D.position_keys(torch.from_numpy(rows["planes"]), torch.from_numpy(rows["masks"]),
                                 symmetric=mode == "symmetric")
    assert np.array_equal(hk.numpy(), got[0]) and np.array_equal(hs.numpy(), got[1]) and int(hb) == 6
    assert launch() == 0                                         # again: the same keys, the counter adds
    assert np.array_equal(d_keys.view(torch.int64, (n, 8)), keys) and np.array_equal(d_sym.view(torch.int8, (n,)), sym)
    assert int(d_bad.view(torch.int32, (1,))[0]) == 12
    assert d_keys.intact() and d_sym.intact() and d_bad.intact()


@pytest.mark.parametrize("spread,mode", CASES)
def test_merge_kernel_matches_the_restatement_and_the_host_build(grids, spread, mode):
    _need_gpu()
    rows, keys, sym, bad, gor, order, begin, want = grids[spread, mode]
    if spread == (mode == "symmetric"):
        assert sorted(np.diff(begin).tolist())[-4:] == [255, 256, 257, 600]      # every chunk boundary
    launch, read, outs = _device_merge(rows, sym, order, begin)
    assert launch() == 0
    got = read()
    for name, g, w in zip(FIVE + ("count",), got, want):
        assert _same_bits(g, w), name
    assert all(o.intact() for o in outs)
    host, info = D.merge_duplicate_positions(*(torch.from_numpy(rows[f]) for f in FIVE), mode=mode)
    for name, g, h in zip(FIVE, got, host):
        assert _same_bits(g, h.numpy().reshape(g.shape)), name
    assert np.array_equal(info["count"].numpy(), got[5])
    assert launch() == 0                                         # again: nothing changes
    for g, a in zip(got, read()):
        assert _same_bits(g, a)
    assert all(o.intact() for o in outs)


def test_merge_kernel_zeroes_a_group_with_a_bad_entry_and_reads_nothing_outside(grids):
    _need_gpu()
    rows, keys, sym, bad, gor, order, begin, _ = grids[True, "symmetric"]
    n = len(sym)
    big = int(np.argmax(np.diff(begin)))
    broken, bad_sym, ranges = order.copy(), sym.copy(), begin.copy()
    broken[begin[big] + 555] = 1 << 40                           # far outside: it must not be followed
    small = int(np.flatnonzero(np.diff(begin) == 3)[0])
    broken[begin[small] + 1] = -1
    odd = int(np.flatnonzero(np.diff(begin) == 257)[0])
    bad_sym[order[begin[odd] + 256]] = 9                         # in the second chunk
    ranges[-1] = n + 1
    want = PD.merge_groups(*(rows[f] for f in FIVE), bad_sym, broken, ranges, check_members=False)
    assert int((want[5] == 0).sum()) == len({big, small, odd, len(begin) - 2})
    launch, read, outs = _device_merge(rows, bad_sym, broken, ranges)
    assert launch() == 0
    for name, g, w in zip(FIVE + ("count",), read(), want):
        assert _same_bits(g, w), name
    assert all(o.intact() for o in outs)


def test_nothing_to_do_and_bad_arguments():
    _need_gpu()
    H = L.lib()
    assert H.lz_dedup_position_keys(None, None, 0, 1, None, None, None, _stream()) == 0
    assert H.lz_dedup_merge_groups(*[None] * 5, 0, None, None, None, 0, *[None] * 6, _stream()) == 0
    assert H.lz_dedup_position_keys(None, None, 4, 1, None, None, None, _stream()) == -1
    assert H.lz_dedup_position_keys(None, None, -1, 0, None, None, None, _stream()) == -1
    assert H.lz_dedup_merge_groups(*[None] * 5, 5, None, None, None, 3, *[None] * 6, _stream()) == -1
    assert H.lz_dedup_merge_groups(*[None] * 5, 5, None, None, None, -3, *[None] * 6, _stream()) == -1
    for n in (0, 1):                                             # through the module
        rows = {k: v[:n] for k, v in PD.grid(SEED, False).items()}
        outs, info = D.merge_duplicate_positions(*(_dev(rows[f]) for f in FIVE), mode="symmetric")
        assert info["rows_in"] == info["rows_out"] == info["groups"] == n
        for f, o in zip(FIVE, outs):
            assert _same_bits(o.cpu().numpy(), rows[f])


# ---- the whole function ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,max_copies", [("symmetric", 1), ("exact", 3)])
def test_merge_duplicate_positions_on_the_tiled_trace_twice(mode, max_copies):
    _need_gpu()
    z = load("g8_selfplay.npz")
    perm = np.random.default_rng(SEED).permutation(328 * 12)
    rows = {"planes": np.tile(unpack_mask(z["state_tensors"], 396).astype(np.float32).reshape(-1, 11, 6, 6), (12, 1, 1, 1))[perm],
            "masks": np.tile(unpack_mask(z["legal_masks"], 220).astype(np.uint8), (12, 1))[perm],
            "policy": np.tile(z["policy_targets"].astype(np.float32), (12, 1))[perm],
            "value": np.tile(z["value_targets"].astype(np.float32), 12)[perm],
            "soft": np.tile(z["soft_value_targets"].astype(np.float32), 12)[perm]}
    want, winfo = PD.merge_duplicate_positions(*(rows[f] for f in FIVE), mode=mode, max_copies=max_copies)
    assert winfo["rows_in"] == 3936 and winfo["groups"] == 55 and winfo["largest_group"] > 256
    d = [_dev(rows[f]) for f in FIVE]
    d[1] = d[1].bool()                                           # the trainer's mask type
    runs = [D.merge_duplicate_positions(*d, mode=mode, max_copies=max_copies) for _ in range(2)]
    for outs, info in runs:
        assert {k: info[k] for k in STATS} == {k: winfo[k] for k in STATS}
        assert np.array_equal(info["group_of_row"].cpu().numpy(), winfo["group_of_row"])
        assert np.array_equal(info["count"].cpu().numpy(), winfo["count"]) and info["count"].dtype == torch.int32
        assert outs[1].dtype == torch.bool and outs[0].shape[1:] == (11, 6, 6)
        for name, o, w in zip(FIVE, outs, want):
            o = o.cpu().numpy()
            assert _same_bits(o.astype(np.uint8) if name == "masks" else o, w), (mode, name)
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---- the trainer --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unique_rows():
    """256 positions of the rules fixture, pairwise different even up to symmetry, with random targets."""
    from liuzhou_amd import v0_core
    z = load("g15_rules_large.npz")
    st = states(z, "s")
    t = [torch.from_numpy(np.ascontiguousarray(st[f])) for f in ("board", "marks_black", "marks_white", "phase", "current_player")]
    planes = v0_core.states_to_model_input(*t).numpy()
    masks = unpack_mask(z["legal_mask"], 220).astype(np.uint8)
    masks[:, 216] = 1                                            # never an empty mask (216 is fixed by every symmetry)
    keys, _, bad = PD.keys(planes, masks, True)
    assert bad == 0
    _, first = np.unique(keys, axis=0, return_index=True)
    pick = np.sort(first)[:256]
    assert len(pick) == 256
    rng = np.random.default_rng(SEED)
    planes, masks = planes[pick], masks[pick]
    policy = (rng.random((256, 220)) * masks).astype(np.float32)
    policy /= policy.sum(axis=1, keepdims=True, dtype=np.float32)
    return {"planes": planes, "masks": masks, "policy": policy, "value": rng.integers(-1, 2, 256).astype(np.float32),
            "soft": rng.uniform(-1, 1, 256).astype(np.float32)}


def _train(monkeypatch, rows, **kw):
    from liuzhou_amd import train_bridge as TB
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
    monkeypatch.setenv("LZ_TRAIN_MIOPEN", "immediate")
    seen = []
    step = TB._Stepper.step

    def spy(self, *batch):
        seen.append([t.detach().clone() for t in batch])
        return step(self, *batch)
    monkeypatch.setattr(TB._Stepper, "step", spy)
    model = ChessNet(**MODEL_CONFIGS["b6c64"])
    stable_resnet_init(model, 20260314)
    torch.manual_seed(5)
    batch = TensorSelfPlayBatch(_dev(rows["planes"]), _dev(rows["masks"]).bool(), _dev(rows["policy"]), _dev(rows["value"]),
                                _dev(rows["soft"]))
    _, metrics = TB.train_network_from_tensors(model, batch, batch_size=64, epochs=1, lr=1e-3, device=DEV, use_amp=False, **kw)
    torch.cuda.synchronize()
    return metrics, seen


def _row_bytes(five):
    cols = [np.ascontiguousarray(a).reshape(len(a), -1).view(np.uint8) for a in five]
    return sorted(b"".join(c[i].tobytes() for c in cols) for i in range(len(cols[0])))


def test_trainer_trains_on_each_position_once(monkeypatch, unique_rows):
    _need_gpu()
    x = unique_rows
    tripled = {f: np.concatenate([x[f]] * 3) for f in FIVE}
    metrics, seen = _train(monkeypatch, tripled, dedup_positions="exact")
    assert metrics["position_dedup"] == {"rows_in": 768, "rows_out": 256, "groups": 256, "merged_groups": 256,
                                         "merged_rows": 768, "largest_group": 3, "not_representable": 0, "mode": "exact",
                                         "max_copies": 1}
    assert metrics["num_samples"] == 768 and metrics["num_samples_after_filter"] == 768
    assert metrics["epoch_stats"][0]["samples"] == 256 and metrics["local_batch_count"] == 4 and len(seen) == 4
    got = [torch.cat([b[i] for b in seen]).cpu().numpy() for i in range(5)]
    want = [x["planes"], x["masks"].astype(bool), x["policy"], x["value"], x["soft"]]
    assert _row_bytes(got) == _row_bytes(want)                   # exactly the multiset of X's rows


def test_trainer_symmetric_merges_the_eight_images_and_off_adds_nothing(monkeypatch, unique_rows):
    _need_gpu()
    x = unique_rows
    parts = [x] + [dict(zip(("planes", "masks", "policy"), SY.np_transform_samples(x["planes"], x["masks"], x["policy"], k)),
                        value=x["value"], soft=x["soft"]) for k in range(8)]
    rows = {f: np.concatenate([p[f] for p in parts]) for f in FIVE}
    metrics, seen = _train(monkeypatch, rows, dedup_positions="symmetric", dedup_max_copies=2)
    assert metrics["position_dedup"] == {"rows_in": 2304, "rows_out": 512, "groups": 256, "merged_groups": 256,
                                         "merged_rows": 2304, "largest_group": 9, "not_representable": 0,
                                         "mode": "symmetric", "max_copies": 2}
    assert metrics["epoch_stats"][0]["samples"] == 512 and len(seen) == 8
    seen.clear()
    metrics, seen = _train(monkeypatch, x)
    assert "position_dedup" not in metrics and metrics["epoch_stats"][0]["samples"] == 256
    assert metrics["num_samples_after_filter"] == 256
