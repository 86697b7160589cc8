"""GPU: per-row sample weights from the kernel up -- lz_policy_value_loss_weighted_fwd_bwd through
the C ABI against the unweighted entry (bit for bit at weights of one) and against the float64 restatement
(tests/row_weights_ref.py, anchored by tests/test_row_weights_cpu.py), `fused_policy_value_loss(row_weights=...)`, the
three consumers in the trainers (`row_weights`, `dedup_weighting="weight"`, `replay_age_decay`) and the staged loop.

Bounds: those of tests/test_gpu_train_kernels.py.  A row weight rw scales the gradients of its row exactly like
grad_scale, so a row's bound is `tolerance(name, B, grad_scale * rw)`; the factors of the wide classes are measured on the
float32 oracle, never on the kernel.  A row with weight 0 has the bound 0: its gradients are +-0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import row_weights_ref as R
from tests import train_loss_cases as K
from tests.test_gpu_train_kernels import (DEV, ERR_ARG, GUARD, LOSS_OUT, assert_bits, dv, host_sentinel, loss_inputs,
                                          run_loss, run_ref, sentinel)
from tests.train_loss_ref import BASE_TOL, POLICY_QUANTITIES, quantities, tolerance, wide_class_factors

pytestmark = pytest.mark.gpu
GRADS = ("g1", "g2", "g3", "gv")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from liuzhou_amd import _lib
    return _lib


# =========================================================================================================================
# lz_policy_value_loss_weighted_fwd_bwd
# =========================================================================================================================
def call_weighted(L, d_in, rw, B, setting, weight_sum, grad_scale, outs):
    """The argument order of include/liuzhou_hip.h: row_weight right after soft_value_target; `rw` may be None (NULL)."""
    ws = None if weight_sum is None else dv(np.array([weight_sum], np.float32))
    st = L.lib().lz_policy_value_loss_weighted_fwd_bwd(
        *(L.ptr(t) for t in d_in), L.ptr(rw), L.i64(B), C.c_float(setting[0]), C.c_float(setting[1]),
        C.c_float(setting[2]), L.ptr(ws), C.c_float(grad_scale), *(L.ptr(t) for t in outs),
        L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return st


def run_weighted(L, c, rw, setting, grad_scale=1.0):
    """-> the outputs of the B rows (numpy); the guard rows behind every output are checked here."""
    B = len(c["value"])
    assert rw.shape == (B,) and rw.dtype == np.float32
    ws = K.weight_sum_of(c["value"], setting[2])
    outs = [sentinel((B + GUARD, w)) for _, w in LOSS_OUT]
    L.check(call_weighted(L, loss_inputs(c), dv(rw), B, setting, ws, grad_scale, outs), "policy_value_loss_weighted_fwd_bwd")
    got = {}
    for (name, w), t in zip(LOSS_OUT, outs):
        a = t.cpu().numpy()
        assert_bits(a[B:], host_sentinel((GUARD, w)), f"{name} guard rows")
        got[name] = a[:B]
    return got


IDENTITY_CASES = [(K.EDGE_B, s) for s in range(len(K.SETTINGS))] + [(B, 1) for B in (1, 3, 4, 5, 257)]


@pytest.mark.parametrize("B, s", IDENTITY_CASES)
def test_weights_of_one_give_every_byte_of_the_unweighted_entry(L, B, s):
    """The edge batch under the three settings, and the tails and the crossing of the 4-wave workgroup."""
    c = K.edge_batch(B)
    setting = K.SETTINGS[s]
    plain = run_loss(L, c, setting, 3.0)
    one = run_weighted(L, c, np.ones(B, np.float32), setting, 3.0)
    for name, _ in LOSS_OUT:
        assert_bits(one[name], plain[name], f"B={B} {setting} {name}")


def assert_within_weighted(got, want, factors, c, rw, grad_scale, where):
    """Every entry: |got - want| <= factor(class of the row) * (atol(row) + rtol |want|), atol(row) that of grad_scale * rw
    for the gradients; the forward terms do not depend on rw."""
    B = len(c["value"])
    cls_p, cls_v = K.policy_class(c), K.value_class(c)
    g, w = quantities(got), quantities(want)
    for name in BASE_TOL:
        cls = cls_p if name in POLICY_QUANTITIES else cls_v
        f = np.array([factors[(name, str(k))] for k in cls])
        a, b = np.asarray(g[name], np.float64), np.asarray(w[name], np.float64)
        if name in GRADS:
            rows = [tolerance(name, B, grad_scale * float(r)) for r in rw]
        else:
            rows = [tolerance(name, B, grad_scale)] * B
        rtol = np.array([t[0] for t in rows]).reshape((-1,) + (1,) * (a.ndim - 1))
        atol = np.array([t[1] for t in rows]).reshape((-1,) + (1,) * (a.ndim - 1))
        bound = f.reshape(rtol.shape) * (atol + rtol * np.abs(b))
        diff = np.abs(a - b)
        assert np.isfinite(a).all(), f"{where} {name}: non-finite output"
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
        worst = np.unravel_index(np.argmax(ratio), ratio.shape)
        print(f"{where} {name:>3}: worst {ratio[worst]:.3f} x bound at {worst} (weight {rw[worst[0]]:g}, {cls[worst[0]]})")
        assert (diff <= bound).all(), (f"{where} {name}: {int((diff > bound).sum())} entries past the bound, worst at {worst}: "
                                       f"got {a[worst]!r}, want {b[worst]!r}, weight {rw[worst[0]]!r}, class {cls[worst[0]]}")


@pytest.fixture(scope="module")
def restated():
    """(case, weights, unweighted restatement, factors of the wide classes) by (B, grad_scale): computed once, left unchanged."""
    out = {}
    setting = K.SETTINGS[1]
    for B in (K.EDGE_B, 257):
        c = K.edge_batch(B)
        rw = R.cycle_weights(B)
        for gs in (1.0, 65536.0):
            plain = run_ref(c, setting, gs)
            factors, _ = wide_class_factors(c, K.policy_class(c), K.value_class(c), plain, setting, gs)
            want = R.ref_loss_weighted(c, rw, setting, K.weight_sum_of(c["value"], setting[2]), gs)
            out[B, gs] = (c, rw, want, factors)
    return out


@pytest.mark.parametrize("B", (K.EDGE_B, 257))
@pytest.mark.parametrize("grad_scale", (1.0, 65536.0))
def test_weighted_loss_equals_the_restatement(L, restated, B, grad_scale):
    c, rw, want, factors = restated[B, grad_scale]
    setting = K.SETTINGS[1]
    assert B >= len(R.WEIGHT_CYCLE) and np.array_equal(rw[:9], np.array(R.WEIGHT_CYCLE, np.float32))
    got = run_weighted(L, c, rw, setting, grad_scale)
    assert_bits(got["terms"][:, 1], want["terms"][:, 1].astype(np.float32), "weight column = float32(draw weight * rw)")
    assert_within_weighted(got, want, factors, c, rw, grad_scale, f"B={B} grad_scale={grad_scale:g}")
    # weight 0 and finite inputs: every gradient entry is +-0, and so is the weight column
    finite = np.all([np.isfinite(c[k]).reshape(B, -1).all(axis=1) for k in ("lp1", "lp2", "lpm", "vlogits", "target", "value",
                                                                            "soft")], axis=0)
    zero = (rw == 0) & finite
    assert zero.sum() >= B // len(R.WEIGHT_CYCLE) - 1 and zero.any()
    for name in GRADS:
        assert (got[name][zero] == 0).all(), name
    assert (got["terms"][zero, 1] == 0).all() and (got["terms"][rw != 0, 1] != 0).sum() > 0
    plain = run_loss(L, c, setting, grad_scale)
    for col in (0, 2, 3):                                     # kl, bucket CE and aux do not depend on the weight
        assert_bits(got["terms"][:, col], plain["terms"][:, col], f"terms column {col}")


def test_weighted_loss_is_bit_identical_on_a_second_run(L):
    c = K.edge_batch(257)
    rw = R.cycle_weights(257)
    a, b = run_weighted(L, c, rw, K.SETTINGS[1], 3.0), run_weighted(L, c, rw, K.SETTINGS[1], 3.0)
    for name, _ in LOSS_OUT:
        assert_bits(a[name], b[name], name)


def test_weighted_loss_refuses_bad_arguments_without_a_launch(L):
    c = K.edge_batch(4)
    d_in = loss_inputs(c)
    rw = dv(np.ones(4, np.float32))
    outs = [sentinel((4 + GUARD, w)) for _, w in LOSS_OUT]
    setting = K.SETTINGS[1]
    assert call_weighted(L, d_in, None, 4, setting, 4.0, 1.0, outs) == ERR_ARG          # NULL row_weight
    assert call_weighted(L, d_in, rw, -1, setting, 4.0, 1.0, outs) == ERR_ARG
    for i in range(len(d_in)):
        assert call_weighted(L, d_in[:i] + [None] + d_in[i + 1:], rw, 4, setting, 4.0, 1.0, outs) == ERR_ARG, K.INPUT_KEYS[i]
    for i in range(len(outs)):
        assert call_weighted(L, d_in, rw, 4, setting, 4.0, 1.0, outs[:i] + [None] + outs[i + 1:]) == ERR_ARG, LOSS_OUT[i][0]
    assert call_weighted(L, d_in, rw, 4, setting, None, 1.0, outs) == ERR_ARG
    assert call_weighted(L, d_in, rw, 0, setting, 4.0, 1.0, outs) == 0
    assert call_weighted(L, [None] * 8, None, 0, setting, None, 1.0, [None] * 5) == 0
    for (name, w), t in zip(LOSS_OUT, outs):
        assert_bits(t, host_sentinel((4 + GUARD, w)), name)


# =========================================================================================================================
# fused_policy_value_loss(row_weights=...)
# =========================================================================================================================
def _wrapper(c, setting, factor, B, rw=None):
    from liuzhou_amd.train_loss import fused_policy_value_loss
    heads = [dv(c[k]).reshape(B, 6, 6).requires_grad_(True) for k in ("lp1", "lp2", "lpm")]
    vl = dv(c["vlogits"]).half().requires_grad_(True)
    kw = {} if rw is None else {"row_weights": dv(rw)}
    loss, parts = fused_policy_value_loss(*heads, vl, dv(c["mask"] != 0), dv(c["target"]), dv(c["value"]), dv(c["soft"]),
                                          soft_label_alpha=setting[0], anti_draw_penalty=setting[1],
                                          policy_draw_weight=setting[2], **kw)
    (loss * factor).backward()
    assert all(h.grad.shape == (B, 6, 6) and h.grad.dtype == torch.float32 for h in heads)
    assert vl.grad.dtype == torch.float16 and vl.grad.shape == (B, 101)
    return [loss.detach().cpu().numpy(), *(parts[k].cpu().numpy() for k in ("wdl_aux_loss", "bucket_value_loss", "policy_loss")),
            *(h.grad.cpu().numpy() for h in heads), vl.grad.cpu().numpy()]


def test_wrapper_loss_parts_and_gradients_with_weights(L):
    """Weights as the trainers hand them over (the cycle, normalised to mean one), board-shaped heads, fp16 value logits
    and an upstream factor.  The fp16 value-logit gradient may be off by half an fp16 ulp on top of the kernel's bound."""
    c = dict(K.edge_batch(K.EDGE_B))
    c["vlogits"] = torch.from_numpy(c["vlogits"]).half().float().numpy()       # exactly representable in fp16
    setting, factor, B = K.SETTINGS[1], 3.0, K.EDGE_B
    rw = R.ref_normalise(R.cycle_weights(B))
    ws = K.weight_sum_of(c["value"], setting[2])
    want = R.ref_loss_weighted(c, rw, setting, ws, factor)
    factors, _ = wide_class_factors(c, K.policy_class(c), K.value_class(c), run_ref(c, setting, factor), setting, factor)
    assert max(factors.values()) == 1.0                       # hence the plain bounds on the batch sums below
    loss, aux, bucket, policy, g1, g2, g3, gv = _wrapper(c, setting, factor, B, rw)
    t, r64 = want["terms"], rw.astype(np.float64)
    pol = (t[:, 0] * t[:, 1]).sum() / (ws + 1e-8)             # the weight sum is that of the draw weights, without rw
    np.testing.assert_allclose(policy, pol, rtol=2e-5, atol=1e-5)
    np.testing.assert_allclose(bucket, (t[:, 2] * r64).sum() / B, rtol=2e-5, atol=1e-5)
    np.testing.assert_allclose(aux, (t[:, 3] * r64).sum() / B, rtol=2e-5, atol=1e-5)
    np.testing.assert_allclose(loss, pol + (t[:, 2] * r64).sum() / B, rtol=2e-5, atol=1e-5)
    for name, g, extra_r, extra_a in (("g1", g1, 0.0, 0.0), ("g2", g2, 0.0, 0.0), ("g3", g3, 0.0, 0.0),
                                      ("gv", gv, 2.0 ** -11, 2.0 ** -25)):
        a, b = g.reshape(B, -1).astype(np.float64), want[name]
        tol = [tolerance(name, B, factor * float(r)) for r in rw]
        bound = np.array([x[1] for x in tol])[:, None] + extra_a + (np.array([x[0] for x in tol])[:, None] + extra_r) * np.abs(b)
        assert (np.abs(a - b) <= bound).all(), name
        assert (a[rw == 0] == 0).all() and np.abs(a[rw != 0]).max() > 0


def test_wrapper_without_weights_returns_the_same_bits_and_bad_weights_raise(L):
    from liuzhou_amd.train_loss import fused_policy_value_loss
    c = dict(K.edge_batch(K.EDGE_B))
    setting, B = K.SETTINGS[1], K.EDGE_B
    a, b, ones = _wrapper(c, setting, 3.0, B), _wrapper(c, setting, 3.0, B, None), _wrapper(c, setting, 3.0, B, np.ones(B, np.float32))
    for x, y in zip(a, b):
        assert_bits(x, y, "row_weights=None twice")
    for x, y in zip(a[4:], ones[4:]):                         # the gradients with weights of one: the unweighted bits
        assert_bits(x, y, "weights of one")
    for x, y in zip(a[:4], ones[:4]):                         # the sums are formed in another order
        np.testing.assert_allclose(x, y, rtol=1e-6, atol=0)
    args = [dv(c[k]) for k in ("lp1", "lp2", "lpm", "vlogits")] + [dv(c["mask"] != 0), dv(c["target"]), dv(c["value"]), dv(c["soft"])]
    good = torch.ones(B, device=DEV)
    for bad, exc in ((good.double(), TypeError), (good.half(), TypeError), (np.ones(B, np.float32), TypeError),
                     (good[:-1], ValueError), (good.view(B, 1), ValueError), (torch.ones(()).to(DEV), ValueError),
                     (good.cpu(), ValueError)):
        with pytest.raises(exc, match="row_weights"):
            fused_policy_value_loss(*args, row_weights=bad)


# =========================================================================================================================
# the trainers
# =========================================================================================================================
FIVE = ("planes", "masks", "policy", "value", "soft")


@pytest.fixture
def deterministic_training(monkeypatch):
    """The recipe of tests/test_gpu_symmetry.py: fixed convolution kernels and MIOpen's deterministic algorithms."""
    monkeypatch.setenv("LZ_TRAIN_MIOPEN", "immediate")
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


@pytest.fixture(scope="module")
def unique_rows():
    """256 positions of the rules fixture, pairwise different even up to symmetry, with random targets whose soft values
    are pairwise different too (they identify a row in what the stepper is handed)."""
    from liuzhou_amd import v0_core
    from tests import position_dedup as PD
    from tests.golden_utils import load, states, unpack_mask
    z = load("g15_rules_large.npz")
    st = states(z, "s")
    t = [torch.from_numpy(np.ascontiguousarray(st[f])) for f in ("board", "marks_black", "marks_white", "phase", "current_player")]
    planes = v0_core.states_to_model_input(*t).numpy()
    masks = unpack_mask(z["legal_mask"], 220).astype(np.uint8)
    masks[:, 216] = 1
    keys, _, bad = PD.keys(planes, masks, True)
    assert bad == 0
    _, first = np.unique(keys, axis=0, return_index=True)
    pick = np.sort(first)[:256]
    assert len(pick) == 256
    rng = np.random.default_rng(20261020)
    planes, masks = planes[pick], masks[pick]
    policy = (rng.random((256, 220)) * masks).astype(np.float32)
    policy /= policy.sum(axis=1, keepdims=True, dtype=np.float32)
    soft = rng.uniform(-1, 1, 256).astype(np.float32)
    assert len(np.unique(soft)) == 256
    return {"planes": planes, "masks": masks, "policy": policy, "value": rng.integers(-1, 2, 256).astype(np.float32), "soft": soft}


def _take(rows, a, b):
    return {f: rows[f][a:b] for f in FIVE}


def _stack(*parts):
    return {f: np.concatenate([p[f] for p in parts]) for f in FIVE}


def _batch(rows):
    from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
    return TensorSelfPlayBatch(dv(rows["planes"]), dv(rows["masks"]).bool(), dv(rows["policy"]), dv(rows["value"]), dv(rows["soft"]))


def _spy(monkeypatch):
    from liuzhou_amd import train_bridge as TB
    seen = []
    step = TB._Stepper.step

    def spy(self, *batch, **kw):
        seen.append(([t.detach().clone() for t in batch], {k: v.detach().clone() for k, v in kw.items()}))
        return step(self, *batch, **kw)
    monkeypatch.setattr(TB._Stepper, "step", spy)
    return seen


def _model():
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    model = ChessNet(**MODEL_CONFIGS["b6c64"])
    stable_resnet_init(model, 20260314)
    return model


def _weights(model):
    torch.cuda.synchronize()
    return torch.cat([p.detach().float().flatten() for p in model.parameters()]).cpu()


def _train(rows, **kw):
    from liuzhou_amd.train_bridge import train_network_from_tensors
    torch.manual_seed(5)
    model, metrics = train_network_from_tensors(_model(), _batch(rows), batch_size=64, epochs=2, lr=2e-3, device=DEV, **kw)
    return _weights(model), metrics


def _seen_rows(seen, column=4):
    """The soft values (or another column) of the rows of every batch, and the weights it came with (None: none)."""
    return [(b[column].cpu().numpy(), kw["b_weights"].cpu().numpy() if "b_weights" in kw else None) for b, kw in seen]


def test_uniform_row_weights_train_to_the_same_bits_as_none(deterministic_training, monkeypatch, unique_rows, L):
    _train(unique_rows)                                           # warm-up: kernel selection, allocator
    w_none, m_none = _train(unique_rows)
    seen = _spy(monkeypatch)
    w_three, m_three = _train(unique_rows, row_weights=torch.full((256,), 3.0))
    assert torch.equal(w_none, w_three), float((w_none - w_three).abs().max())
    assert len(seen) == 8 and all(not b[5:] and bool((kw["b_weights"] == 1.0).all()) and kw["b_weights"].dtype == torch.float32
                                  and kw["b_weights"].shape == (64,) for b, kw in seen)
    assert set(m_three) - set(m_none) == {"row_weights"} and set(m_none) <= set(m_three)
    assert m_three["row_weights"] == {"source": "row_weights", "min": 3.0, "max": 3.0, "zero_weight_rows": 0}
    for a, b in zip(m_none["epoch_stats"], m_three["epoch_stats"]):
        assert set(b) - set(a) == {"row_weight_sum"} and set(a) <= set(b) and b["row_weight_sum"] == b["samples"] == a["samples"]
        assert a["avg_policy_loss"] == b["avg_policy_loss"] and abs(a["avg_loss"] - b["avg_loss"]) <= 1e-6 * abs(a["avg_loss"])


def test_mixed_row_weights_reach_the_stepper_with_their_rows(deterministic_training, monkeypatch, unique_rows, L):
    """Array weights, one row dropped by the non-finite filter: the weights are normalised over the 255 rows left and every
    batch carries the weights of exactly its rows."""
    rows = {f: unique_rows[f].copy() for f in FIVE}
    rows["value"][5] = np.nan
    raw = R.cycle_weights(256)
    raw[5] = 7.0                                                  # dropped with its row: must not enter the normalisation
    keep = np.arange(256) != 5
    want = R.ref_normalise(raw[keep])
    by_soft = dict(zip(rows["soft"][keep].tolist(), want.tolist()))
    seen = _spy(monkeypatch)
    _, m = _train(rows, row_weights=raw, use_amp=False)           # fp32: no step is skipped by the loss scaler
    assert m["filtered_non_finite_samples"] == 1 and m["num_samples_after_filter"] == 255 and len(seen) == 8
    assert m["row_weights"] == {"source": "row_weights", "min": 0.0, "max": 1e4,
                                "zero_weight_rows": int((raw[keep] == 0).sum())}
    for epoch in (seen[:4], seen[4:]):
        softs = np.concatenate([s for s, _ in _seen_rows(epoch)])
        assert sorted(softs.tolist()) == sorted(rows["soft"][keep].tolist())
        for s, w in _seen_rows(epoch):
            assert w.dtype == np.float32 and w.tolist() == [by_soft[x] for x in s.tolist()]
    for st in m["epoch_stats"]:
        assert abs(st["row_weight_sum"] - 255.0) < 1e-2 and st["samples"] == 255


def test_dedup_weight_on_three_copies_is_dedup_once(deterministic_training, monkeypatch, unique_rows, L):
    x = unique_rows
    tripled = _stack(x, x, x)
    _train(tripled, dedup_positions="exact")                      # warm-up
    w_once, m_once = _train(tripled, dedup_positions="exact", dedup_max_copies=1)
    seen = _spy(monkeypatch)
    w_weight, m_weight = _train(tripled, dedup_positions="exact", dedup_max_copies=3, dedup_weighting="weight")
    assert torch.equal(w_once, w_weight), float((w_once - w_weight).abs().max())
    assert len(seen) == 8
    for epoch in (seen[:4], seen[4:]):
        got = _seen_rows(epoch)
        assert sorted(np.concatenate([s for s, _ in got]).tolist()) == sorted(x["soft"].tolist())      # X's rows once each
        assert all(w is not None and (w == 1.0).all() for _, w in got)
    want = dict(m_once["position_dedup"], max_copies=3, weighting="weight")
    assert m_weight["position_dedup"] == want and want["rows_out"] == want["groups"] == 256
    assert "weighting" not in m_once["position_dedup"] and "row_weights" not in m_once
    assert m_weight["row_weights"] == {"source": "dedup_weighting", "min": 3.0, "max": 3.0, "zero_weight_rows": 0}


def test_dedup_weight_on_two_copies_and_singles(deterministic_training, monkeypatch, unique_rows, L):
    x, y = _take(unique_rows, 0, 192), _take(unique_rows, 192, 256)
    seen = _spy(monkeypatch)
    _, m = _train(_stack(x, x, y), dedup_positions="exact", dedup_max_copies=4, dedup_weighting="weight", use_amp=False)
    g, s = 256, 2 * 192 + 64
    d = m["position_dedup"]
    assert d["rows_in"] == 448 and d["rows_out"] == d["groups"] == g and d["weighting"] == "weight" and d["max_copies"] == 4
    assert m["epoch_stats"][0]["samples"] == g and m["row_weights"]["min"] == 1.0 and m["row_weights"]["max"] == 2.0
    two, one = np.float32(2.0 * (g / s)), np.float32(1.0 * (g / s))
    in_x = set(x["soft"].tolist())
    for soft, w in _seen_rows(seen):
        assert w.tolist() == [float(two) if v in in_x else float(one) for v in soft.tolist()]
    assert sorted(np.concatenate([sf for sf, _ in _seen_rows(seen[:4])]).tolist()) == sorted(unique_rows["soft"].tolist())
    # the cap: with M = 1 every group weighs 1
    seen.clear()
    _, m = _train(_stack(x, x, y), dedup_positions="exact", dedup_max_copies=1, dedup_weighting="weight")
    assert all((w == 1.0).all() for _, w in _seen_rows(seen)) and m["row_weights"]["max"] == 1.0


# ---- the replay window ---------------------------------------------------------------------------------------------------------
def _train_window(generations, **kw):
    from liuzhou_amd.replay_window import ReplayWindow
    from liuzhou_amd.train_bridge import train_network_from_window
    w = ReplayWindow(DEV, max_generations=len(generations), capacity_rows=sum(len(g["soft"]) for g in generations) + 5)
    w.add_generation(_batch(generations[0]), generation=3)          # off slot 0 from the second generation on
    for g in generations[1:]:
        w.add_generation(_batch(g))
    torch.manual_seed(5)
    model, m = train_network_from_window(_model(), w, batch_size=64, epochs=2, lr=2e-3, device=DEV, **kw)
    return _weights(model), m


def test_window_age_decay_weighs_rows_by_generation(deterministic_training, monkeypatch, unique_rows, L):
    old, new = _take(unique_rows, 0, 96), _take(unique_rows, 96, 256)
    _train_window([old, new], replay_budget_per_generation=96)      # warm-up
    w_plain, m_plain = _train_window([old, new], replay_budget_per_generation=96)
    seen = _spy(monkeypatch)
    w_one, m_one = _train_window([old, new], replay_budget_per_generation=96, replay_age_decay=1.0)
    assert torch.equal(w_plain, w_one) and m_plain["epoch_stats"] == m_one["epoch_stats"] and set(m_plain) == set(m_one)
    assert "row_weights" not in m_one and all(not kw and len(b) == 5 for b, kw in seen)
    assert all("row_weight_sum" not in st for st in m_one["epoch_stats"])
    seen.clear()
    w_half, m_half = _train_window([old, new], replay_budget_per_generation=96, replay_age_decay=0.5)
    assert set(m_half) - set(m_plain) == {"row_weights"} and m_half["replay_window"] == {**m_plain["replay_window"],
                                                                                        "select_sec": m_half["replay_window"]["select_sec"]}
    assert m_half["row_weights"] == {"source": "replay_age_decay", "min": 0.5, "max": 1.0, "zero_weight_rows": 0}
    c = 256 / (160 + 96 * 0.5)
    newer, older = float(np.float32(c)), float(np.float32(c / 2))
    in_new = set(new["soft"].tolist())
    total = 0.0
    for soft, w in _seen_rows(seen[:4]):
        assert w.tolist() == [newer if v in in_new else older for v in soft.tolist()]
        total += float(w.astype(np.float64).sum())
    assert abs(total / 256 - 1.0) <= 2.0 ** -23                     # mean one over the selection
    assert not torch.equal(w_plain, w_half)
    assert all(abs(st["row_weight_sum"] - 256.0) < 1e-3 for st in m_half["epoch_stats"] if st["samples"] == 256)
    assert all("row_weight_sum" in st for st in m_half["epoch_stats"])


# ---- the staged loop -----------------------------------------------------------------------------------------------------------
def test_staged_loop_reports_the_age_weights(L):
    from tests.test_gpu_replay_window import PARENT_ITERATION_KEYS, PARENT_KEYS, _staged_loop
    out = _staged_loop("--replay-generations", "2", "--replay-age-decay", "0.5")
    its = out["iterations"]
    assert set(out) == PARENT_KEYS and len(its) == 3
    for it in its:
        assert set(it) == PARENT_ITERATION_KEYS | {"replay", "row_weights"}
        assert it["row_weights"]["source"] == "replay_age_decay" and it["row_weights"]["max"] == 1.0
        assert it["row_weights"]["zero_weight_rows"] == 0 and it["avg_loss"] is not None
    assert its[0]["row_weights"]["min"] == 1.0                      # one generation in the window: every age is 0
    assert its[1]["row_weights"]["min"] == 0.5 and its[2]["row_weights"]["min"] == 0.5
    assert its[1]["replay"]["generations"] == [2, 1]


def test_staged_loop_default_prints_the_parent_keys(L):
    from tests.test_gpu_replay_window import PARENT_ITERATION_KEYS, PARENT_KEYS, _staged_loop
    out = _staged_loop()
    assert set(out) == PARENT_KEYS
    for it in out["iterations"]:
        assert set(it) == PARENT_ITERATION_KEYS
