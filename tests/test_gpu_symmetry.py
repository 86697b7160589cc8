"""GPU: the board-symmetry kernels (csrc/lz_symmetry.hip) against the numpy restatement of liuzhou_amd/symmetry.py, and
the trainer's symmetry augmentation (train_bridge.py) against training on a dataset transformed beforehand."""
import numpy as np
import pytest
import torch

from liuzhou_amd import symmetry as S
from oracle import lz_oracle as O
from tests.golden_utils import FIELDS, load, states

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _random_rows(rng, n):
    planes = rng.standard_normal((n, 11, 6, 6)).astype(np.float32)
    masks = rng.random((n, 220)) < 0.3
    bits = rng.integers(0, 1 << 32, (n, 220), dtype=np.uint64).astype(np.uint32)
    exp = (bits >> 23) & 0xFF
    bits[exp == 0xFF] &= ~np.uint32(1 << 30)                    # arbitrary floats, NaN / inf payloads excepted
    return planes, masks, bits.view(np.float32)


@pytest.mark.parametrize("dtype", [torch.int8, torch.int32])
def test_device_gather_samples_match_numpy_on_100k_rows(dtype):
    _need_gpu()
    rng = np.random.default_rng(7)
    n = 100_000
    planes, masks, policy = _random_rows(rng, n)
    sym = rng.integers(0, 8, n)
    sym[:8] = np.arange(8)                                      # every id
    d = [torch.from_numpy(a).to(DEV) for a in (planes, masks, policy)]
    got = S.transform_samples(*d, torch.from_numpy(sym).to(dtype).to(DEV))
    torch.cuda.synchronize()
    wp, wm, wq = S.np_transform_samples(planes, masks, policy, sym)
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), wp.view(np.uint32))
    assert np.array_equal(got[1].cpu().numpy(), wm)
    assert np.array_equal(got[2].cpu().numpy().view(np.uint32), wq.view(np.uint32))
    m = 70_001
    idx = rng.integers(0, n, m)
    sym2 = rng.integers(0, 8, m)
    sym2[:8] = np.arange(8)
    got = S.transform_samples(*d, torch.from_numpy(sym2).to(dtype).to(DEV), torch.from_numpy(idx).to(DEV))
    sel = np.concatenate([np.arange(8), 8 + rng.choice(m - 8, 4000, replace=False)])
    wp, wm, wq = S.np_transform_samples(planes, masks, policy, sym2[sel], idx[sel])
    assert np.array_equal(got[0].cpu().numpy()[sel].view(np.uint32), wp.view(np.uint32))
    assert np.array_equal(got[1].cpu().numpy()[sel], wm)
    assert np.array_equal(got[2].cpu().numpy()[sel].view(np.uint32), wq.view(np.uint32))
    # the device and the host build agree on every row
    host = S.transform_samples(*(torch.from_numpy(a) for a in (planes, masks, policy)), torch.from_numpy(sym2).to(dtype),
                               torch.from_numpy(idx))
    for g, h in zip(got, host):
        assert torch.equal(g.cpu().view(torch.uint8), h.view(torch.uint8))


def test_device_transform_states_and_inverse_round_trip():
    _need_gpu()
    st = states(load("g16_garbage_large.npz"), "s")
    n = st["board"].shape[0]
    sym = np.random.default_rng(1).integers(0, 8, n)
    dst = {f: torch.from_numpy(np.asarray(st[f])).to(DEV) for f in FIELDS}
    got = S.transform_states(dst, torch.from_numpy(sym.astype(np.int32)).to(DEV))
    want = S.np_transform_states(st, sym)
    for f in FIELDS:
        assert np.array_equal(got[f].cpu().numpy(), np.asarray(want[f])), f
    inv = torch.tensor([S.inverse(int(k)) for k in sym], dtype=torch.int8, device=DEV)
    back = S.transform_states(got, inv)
    for f in FIELDS:
        assert torch.equal(back[f], dst[f]), f


def test_device_transform_packed_equals_transform_states_on_g15():
    _need_gpu()
    from liuzhou_amd import v0_core  # noqa: F401  (loads the library)
    from liuzhou_amd import _lib as L
    from tests.tree_parity import unpack_packed
    st = states(load("g15_rules_large.npz"), "s")
    n = st["board"].shape[0]
    ins = [torch.from_numpy(np.ascontiguousarray(np.asarray(st[f]))).to(DEV).to(dt).contiguous()
           for f, dt in zip(FIELDS, S._STATE_DTYPES)]
    packed = torch.empty((n, 4), dtype=torch.int64, device=DEV)
    import ctypes as C
    soa = L.soa(ins)
    L.check(L.lib().lz_pack_states(C.byref(soa), L.i64(n), L.ptr(packed), L.stream_ptr(DEV)), "pack_states")
    for k in range(8):
        got = S.transform_packed(packed, k).cpu().numpy()
        ts = S.transform_states(dict(zip(FIELDS, ins)), k)
        want_st = {f: ts[f].cpu().numpy() for f in FIELDS}
        un = unpack_packed(got)
        for f in FIELDS:
            assert np.array_equal(np.asarray(un[f]).reshape(np.asarray(want_st[f]).shape),
                                  np.asarray(want_st[f]).astype(np.asarray(un[f]).dtype)), (k, f)
        assert np.array_equal(got, S.np_transform_packed(packed.cpu().numpy(), k))
        assert np.array_equal(got, S.transform_packed(packed.cpu(), k).numpy())       # host build


# ---- trainer ---------------------------------------------------------------------------------------------------------
def _dataset(n=1536, seed=3):
    from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
    st = states(load("g15_rules_large.npz"), "s")
    rng = np.random.default_rng(seed)
    rows = rng.choice(st["board"].shape[0], n, replace=False)
    sub = {f: np.asarray(st[f])[rows] for f in FIELDS}
    mask, _ = O.encode_actions(sub)
    planes = O.states_to_model_input(sub)
    pol = rng.random((n, 220)).astype(np.float32) * mask
    pol = pol / np.maximum(pol.sum(1, keepdims=True), 1e-8)
    value = rng.integers(-1, 2, n).astype(np.float32)
    soft = (rng.random(n) * 2 - 1).astype(np.float32)
    return TensorSelfPlayBatch(*(torch.from_numpy(a).to(DEV) for a in (planes, mask, pol.astype(np.float32), value, soft)))


def _transformed(batch, k):
    from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
    p, m, q = S.transform_samples(batch.state_tensors, batch.legal_masks, batch.policy_targets, k)
    return TensorSelfPlayBatch(p, m, q, batch.value_targets, batch.soft_value_targets)


_INIT = {}


def _model():
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    if "sd" not in _INIT:
        m = ChessNet(**MODEL_CONFIGS["b6c64"])
        stable_resnet_init(m, 20260314)
        _INIT["sd"] = {k: v.clone() for k, v in m.state_dict().items()}
    m = ChessNet(**MODEL_CONFIGS["b6c64"])
    m.load_state_dict(_INIT["sd"])
    return m


def _train(batch, streaming, **kw):
    from liuzhou_amd.train_bridge import train_network_from_tensors, train_network_streaming
    torch.manual_seed(123)                                      # the shuffle
    model = _model()
    if streaming:
        bs = 256
        loader = [tuple(t[i:i + bs] for t in (batch.state_tensors, batch.legal_masks, batch.policy_targets,
                                              batch.value_targets, batch.soft_value_targets))
                  for i in range(0, batch.num_samples, bs)]
        model, m = train_network_streaming(model, loader, total_samples=batch.num_samples, batch_size=bs, epochs=2,
                                           lr=2e-3, device=DEV, **kw)
    else:
        model, m = train_network_from_tensors(model, batch, batch_size=256, epochs=2, lr=2e-3, device=DEV, **kw)
    torch.cuda.synchronize()
    return torch.cat([p.detach().float().flatten() for p in model.parameters()]).cpu(), m


def _diff(a, b):
    return float((a - b).abs().max())


@pytest.fixture
def deterministic_training(monkeypatch):
    """Fixed convolution kernels (no MIOpen search between runs) and MIOpen's deterministic algorithms."""
    monkeypatch.setenv("LZ_TRAIN_MIOPEN", "immediate")
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


@pytest.mark.parametrize("streaming", [False, True])
def test_trainer_symmetry_augmentation(streaming, deterministic_training):
    _need_gpu()
    data = _dataset()
    _train(data, streaming)                                     # warm-up: kernel selection, allocator
    w_off, m_off = _train(data, streaming)
    w_off2, _ = _train(data, streaming)
    noise = _diff(w_off, w_off2)                                # how closely two flag-off runs agree
    print(f"two flag-off runs differ by at most {noise:.3g}")
    assert noise < 1e-2, noise
    tol = 0.0 if noise == 0.0 else 4 * noise                    # bit-identical runs: bit-exact comparisons
    assert "symmetry_augment" not in m_off
    # the identity alone is the flag off
    w0, m0 = _train(data, streaming, symmetry_augment=True, symmetry_set=(0,))
    assert _diff(w0, w_off) <= tol
    assert m0["symmetry_augment"]["counts"][0] > 0 and sum(m0["symmetry_augment"]["counts"][1:]) == 0
    # one fixed element == the flag off on the dataset transformed beforehand
    for k in (1, 6):
        wk, _ = _train(data, streaming, symmetry_augment=True, symmetry_set=(k,))
        wt, _ = _train(_transformed(data, k), streaming)
        assert _diff(wk, wt) <= tol, k
        if tol == 0.0:
            assert _diff(wk, w_off) > 0.0                       # and it is a different training
    # the whole group: reproducible under one seed, every id drawn
    wa, ma = _train(data, streaming, symmetry_augment=True, symmetry_seed=9)
    wb, mb = _train(data, streaming, symmetry_augment=True, symmetry_seed=9)
    assert _diff(wa, wb) <= tol
    assert ma["symmetry_augment"]["counts"] == mb["symmetry_augment"]["counts"]
    assert all(c > 0 for c in ma["symmetry_augment"]["counts"])
    assert sum(ma["symmetry_augment"]["counts"]) == 2 * data.num_samples
    wc, mc = _train(data, streaming, symmetry_augment=True, symmetry_seed=10)
    assert mc["symmetry_augment"]["counts"] != ma["symmetry_augment"]["counts"]


def test_trainer_refuses_a_bad_symmetry_set():
    _need_gpu()
    data = _dataset(n=64)
    for bad in ((), (8,), (-1, 2)):
        with pytest.raises(ValueError):
            _train(data, False, symmetry_augment=True, symmetry_set=bad)
