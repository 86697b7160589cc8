"""GPU: the three entry points of csrc/lz_train.hip -- lz_policy_value_loss_fwd_bwd, lz_pack_trajectory_rows,
lz_unpack_trajectory_rows -- called through the C ABI with the inputs of tests/train_loss_cases.py and held to the
restatements tests/train_loss_ref.py (which tests/test_train_loss_ref_cpu.py anchors to the reference's golden values).

Every output is allocated with 8 rows more than the call covers and starts as a sentinel (a quiet NaN with a marked
payload, 0x7F bytes): the extra rows must come back untouched.  Bounds of the loss: the weight
column bit for bit; KL, bucket CE and WDL aux rtol 2e-5 / atol 1e-5; policy gradients rtol 1e-4 / atol 1e-6 * grad_scale;
gv rtol 1e-4 / atol 5e-5 * grad_scale / B.  For the wide classes (heads of log_softmax(25 * randn), value logits of
30 * randn or +-60000) the float32 oracle is measured against the float64 restatement on the same rows first, and where
it is further away than the bound, the class's bound is 4 x that distance -- never a figure taken from the kernel.
Every entry of every output is compared.  The codec is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import train_loss_cases as K
from tests.golden_utils import load
from tests.train_loss_ref import (BASE_TOL, POLICY_QUANTITIES, quantities, ref_loss, ref_pack, ref_representable,
                                  ref_unpack, tolerance, wide_class_factors)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = -1
ALL_SETTINGS = K.SETTINGS + K.EXTRA_SETTINGS
GUARD = K.GUARD_ROWS
LOSS_OUT = (("terms", 4), ("g1", 36), ("g2", 36), ("g3", 36), ("gv", 101))


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from liuzhou_amd import _lib
    return _lib


def dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sentinel(shape, dtype=torch.float32):
    if dtype == torch.float32:
        return torch.full(shape, K.SENT_F32, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full(shape, 0x7F, dtype=dtype, device=DEV)


def host_sentinel(shape, dtype=np.float32):
    if dtype == np.float32:
        return np.full(shape, K.SENT_F32, np.int32).view(np.float32)
    return np.full(shape, 0x7F, dtype)


def assert_bits(got, want, name):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, name
    a, b = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        e = int(bad[0]) // got.dtype.itemsize
        raise AssertionError(f"{name}: {bad.size} bytes differ, first at element {e}: got {got.reshape(-1)[e]!r}, "
                             f"want {want.reshape(-1)[e]!r}")


# =========================================================================================================================
# lz_policy_value_loss_fwd_bwd
# =========================================================================================================================
def loss_inputs(c):
    return [dv(c[k]) for k in K.INPUT_KEYS]


def call_loss(L, d_in, B, setting, weight_sum, grad_scale, outs):
    """The argument handling of liuzhou_amd/train_loss.py; any of d_in / outs / weight_sum may be None (a NULL pointer)."""
    ws = None if weight_sum is None else dv(np.array([weight_sum], np.float32))
    st = L.lib().lz_policy_value_loss_fwd_bwd(
        *(L.ptr(t) for t in d_in), L.i64(B), C.c_float(setting[0]), C.c_float(setting[1]), C.c_float(setting[2]),
        L.ptr(ws), C.c_float(grad_scale), *(L.ptr(t) for t in outs), L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return st


def run_loss(L, c, setting, grad_scale=1.0, weight_sum=None):
    """-> the outputs of the B rows (numpy); the guard rows are checked here."""
    B = len(c["value"])
    ws = K.weight_sum_of(c["value"], setting[2]) if weight_sum is None else weight_sum
    outs = [sentinel((B + GUARD, w)) for _, w in LOSS_OUT]
    L.check(call_loss(L, loss_inputs(c), B, setting, ws, grad_scale, outs), "policy_value_loss_fwd_bwd")
    got = {}
    for (name, w), t in zip(LOSS_OUT, outs):
        a = t.cpu().numpy()
        assert_bits(a[B:], host_sentinel((GUARD, w)), f"{name} guard rows")
        got[name] = a[:B]
    return got


def run_ref(c, setting, grad_scale=1.0, weight_sum=None):
    ws = K.weight_sum_of(c["value"], setting[2]) if weight_sum is None else weight_sum
    return ref_loss(*(c[k] for k in K.INPUT_KEYS), alpha=setting[0], anti_draw=setting[1], draw_weight=setting[2],
                    weight_sum=ws, grad_scale=grad_scale)


def assert_within(got, want, factors, c, grad_scale, where, B=None):
    """Every entry of every quantity: |got - want| <= factor(class of the row) * (atol + rtol |want|)."""
    B = len(c["value"]) if B is None else B
    cls_p, cls_v = K.policy_class(c), K.value_class(c)
    g, w = quantities(got), quantities(want)
    for name in BASE_TOL:
        rtol, atol = tolerance(name, B, grad_scale)
        cls = cls_p if name in POLICY_QUANTITIES else cls_v
        f = np.array([factors[(name, str(k))] for k in cls])
        a, b = np.asarray(g[name], np.float64), np.asarray(w[name], np.float64)
        f = f.reshape((-1,) + (1,) * (a.ndim - 1))
        ratio = np.abs(a - b) / (f * (atol + rtol * np.abs(b)))
        worst = np.unravel_index(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)), ratio.shape)
        print(f"{where} {name:>3}: worst {ratio[worst]:.3f} x bound at {worst} ({cls[worst[0]]})")
        assert np.isfinite(a).all(), f"{where} {name}: non-finite output"
        assert (ratio <= 1.0).all(), (f"{where} {name}: {int((ratio > 1).sum())} entries past the bound, worst at {worst}: got "
                                      f"{a[worst]!r}, want {b[worst]!r}, class {cls[worst[0]]}")


def check_against_ref(L, c, setting, grad_scale=1.0, where=""):
    got = run_loss(L, c, setting, grad_scale)
    want = run_ref(c, setting, grad_scale)
    assert_bits(got["terms"][:, 1], want["terms"][:, 1].astype(np.float32), f"{where} weight column")
    factors, _ = wide_class_factors(c, K.policy_class(c), K.value_class(c), want, setting, grad_scale)
    assert_within(got, want, factors, c, grad_scale, where)
    return got, want


@pytest.mark.parametrize("B", K.BATCH_SIZES)
def test_loss_equals_the_restatement_at_every_batch_size(L, B):
    """B < 4 leaves waves of the one workgroup idle; 5, 7, 9, 257 end inside a workgroup; four settings each."""
    c = K.edge_batch(B)
    for setting in ALL_SETTINGS:
        check_against_ref(L, c, setting, where=f"B={B} {setting}")


@pytest.mark.parametrize("grad_scale", K.GRAD_SCALES[1:])
def test_loss_gradients_carry_grad_scale(L, grad_scale):
    c = K.edge_batch(K.EDGE_B)
    got, _ = check_against_ref(L, c, K.SETTINGS[1], grad_scale, where=f"grad_scale={grad_scale:g}")
    one = run_loss(L, c, K.SETTINGS[1], 1.0)
    assert_bits(got["terms"], one["terms"], "terms do not depend on grad_scale")
    assert np.abs(got["g1"]).max() > 2 * np.abs(one["g1"]).max()


def test_loss_equals_the_reference_fixture_g21(L):
    """The reference's own functions on the edge batch (oracle/gen_golden.py::gen_loss_edges), three settings."""
    z = load("g21_loss_edges.npz")
    c = K.edge_batch(K.EDGE_B)
    for tag, setting in zip(K.SETTING_TAGS, K.SETTINGS):
        assert tuple(np.float32(setting)) == tuple(z[f"{tag}_params"])
        got = run_loss(L, c, setting)
        want = dict(terms=np.stack([z[f"{tag}_kl"], z[f"{tag}_weight"], z[f"{tag}_ce_value"], z[f"{tag}_wdl_aux"]], axis=1),
                    **{k: z[f"{tag}_{k}"] for k in ("g1", "g2", "g3", "gv")})
        assert_bits(got["terms"][:, 1], z[f"{tag}_weight"], f"g21/{tag} weight column")
        factors, _ = wide_class_factors(c, K.policy_class(c), K.value_class(c), run_ref(c, setting), setting, 1.0)
        assert_within(got, want, factors, c, 1.0, f"g21/{tag}")


def test_loss_is_bit_identical_on_a_second_run(L):
    c = K.edge_batch(257)
    a, b = run_loss(L, c, K.SETTINGS[1], 3.0), run_loss(L, c, K.SETTINGS[1], 3.0)
    for name, _ in LOSS_OUT:
        assert_bits(a[name], b[name], name)


def test_loss_with_weight_sum_zero_has_zero_policy_gradients_and_stays_finite(L):
    c = K.draws_only_batch()
    setting = (0.35, -0.15, 0.0)
    assert K.weight_sum_of(c["value"], setting[2]) == 0.0
    got, _ = check_against_ref(L, c, setting, 3.0, where="weight_sum=0")
    for name in ("g1", "g2", "g3"):
        assert (got[name] == 0).all(), name
    assert (got["terms"][:, 1] == 0).all()
    assert all(np.isfinite(got[name]).all() for name, _ in LOSS_OUT)


def test_loss_with_a_non_finite_log_sum_exp_takes_zero_for_it(L):
    """A +inf head cell on a legal action makes the log-sum-exp non-finite; masked_log_softmax (src/policy_batch.py:153-159)
    then subtracts 0: the finite legal entries keep their combined logit as log-probability, the +inf entry becomes -50.
    The reference's own gradient is NaN at the +inf cell (0 * NaN in the backward of logsumexp) and -target * weight at the
    finite ones; the kernel must give the latter and stay finite at the former.  Expected values in closed form, float64."""
    rng = np.random.default_rng(9)
    c = K.edge_batch(2, seed=9)
    acts = np.array([0, 5, 7, 183])
    tv = np.array([0.1, 0.2, 0.3, 0.4], np.float32)
    c["mask"][:] = 0
    c["target"][:] = 0
    c["mask"][:, acts] = 1
    c["target"][:, acts] = tv
    heads = torch.log_softmax(torch.from_numpy(rng.standard_normal((3, 2, 36)).astype(np.float32)), dim=2).numpy()
    c["lp1"], c["lp2"], c["lpm"] = heads[0].copy(), heads[1].copy(), heads[2].copy()
    c["lp1"][:, 0] = np.inf
    c["value"][:] = (1.0, -1.0)
    gs = 3.0
    got = run_loss(L, c, K.SETTINGS[0], gs, weight_sum=2.0)
    t64 = tv.astype(np.float64)
    ent = -(t64 * np.log(t64)).sum()
    for s in range(2):
        lp = np.array([-50.0, c["lp1"][s, 5], c["lp1"][s, 7], c["lpm"][s, 3]], np.float64)
        np.testing.assert_allclose(got["terms"][s, 0], -(t64 * lp).sum() - ent, rtol=2e-5, atol=1e-5)
        want1, want3 = np.zeros(36), np.zeros(36)
        want1[[5, 7]] = -t64[1:3] * gs / (2.0 + 1e-8)
        want3[3] = -t64[3] * gs / (2.0 + 1e-8)
        np.testing.assert_allclose(got["g1"][s], want1, rtol=1e-4, atol=1e-6 * gs)
        np.testing.assert_allclose(got["g3"][s], want3, rtol=1e-4, atol=1e-6 * gs)
        assert (got["g2"][s] == 0).all()
    assert all(np.isfinite(got[name]).all() for name, _ in LOSS_OUT)


def test_loss_refuses_bad_arguments_without_a_launch(L):
    c = K.edge_batch(4)
    d_in = loss_inputs(c)
    outs = [sentinel((4 + GUARD, w)) for _, w in LOSS_OUT]
    setting = K.SETTINGS[1]
    assert call_loss(L, d_in, -1, setting, 4.0, 1.0, outs) == ERR_ARG
    for i in range(len(d_in)):
        assert call_loss(L, d_in[:i] + [None] + d_in[i + 1:], 4, setting, 4.0, 1.0, outs) == ERR_ARG, K.INPUT_KEYS[i]
    for i in range(len(outs)):
        assert call_loss(L, d_in, 4, setting, 4.0, 1.0, outs[:i] + [None] + outs[i + 1:]) == ERR_ARG, LOSS_OUT[i][0]
    assert call_loss(L, d_in, 4, setting, None, 1.0, outs) == ERR_ARG
    assert call_loss(L, d_in, 0, setting, 4.0, 1.0, outs) == 0
    assert call_loss(L, [None] * 8, 0, setting, None, 1.0, [None] * 5) == 0
    for (name, w), t in zip(LOSS_OUT, outs):
        assert_bits(t, host_sentinel((4 + GUARD, w)), name)


def test_wrapper_board_shaped_heads_both_mask_types_half_value_logits_and_an_upstream_factor(L):
    """fused_policy_value_loss on one edge batch against ref_loss.  The value-logit gradient comes back in fp16: on top of
    the kernel's bound it may be off by half an fp16 ulp (2^-11 relative, 2^-25 absolute in the subnormal range)."""
    from liuzhou_amd.train_loss import fused_policy_value_loss
    c = dict(K.edge_batch(K.EDGE_B))
    c["vlogits"] = torch.from_numpy(c["vlogits"]).half().float().numpy()       # exactly representable in fp16
    setting, factor, B = K.SETTINGS[1], 3.0, K.EDGE_B
    want = run_ref(c, setting, factor)
    results = []
    for mask in (dv(c["mask"]), dv(c["mask"] != 0)):
        heads = [dv(c[k]).reshape(B, 6, 6).requires_grad_(True) for k in ("lp1", "lp2", "lpm")]
        vl = dv(c["vlogits"]).half().requires_grad_(True)
        loss, parts = fused_policy_value_loss(*heads, vl, mask, dv(c["target"]), dv(c["value"]), dv(c["soft"]),
                                              soft_label_alpha=setting[0], anti_draw_penalty=setting[1],
                                              policy_draw_weight=setting[2])
        (loss * factor).backward()
        assert all(h.grad.shape == (B, 6, 6) and h.grad.dtype == torch.float32 for h in heads)
        assert vl.grad.dtype == torch.float16
        results.append([loss.detach().cpu().numpy(),
                        *(parts[k].cpu().numpy() for k in ("wdl_aux_loss", "bucket_value_loss", "policy_loss")),
                        *(h.grad.cpu().numpy() for h in heads), vl.grad.cpu().numpy()])
    for a, b in zip(*results):                                # uint8 and bool masks: identical results
        assert_bits(a, b, "uint8 mask vs bool mask")
    loss, aux, bucket, policy, g1, g2, g3, gv = results[0]
    t = want["terms"]
    ws = K.weight_sum_of(c["value"], setting[2])
    factors, _ = wide_class_factors(c, K.policy_class(c), K.value_class(c), want, setting, factor)
    assert max(factors.values()) == 1.0                       # hence the plain bounds on the batch sums below
    np.testing.assert_allclose(policy, (t[:, 0] * t[:, 1]).sum() / (ws + 1e-8), rtol=2e-5, atol=1e-5)
    np.testing.assert_allclose(bucket, t[:, 2].mean(), rtol=2e-5, atol=1e-5)
    np.testing.assert_allclose(aux, t[:, 3].mean(), rtol=2e-5, atol=1e-5)
    np.testing.assert_allclose(loss, (t[:, 0] * t[:, 1]).sum() / (ws + 1e-8) + t[:, 2].mean(), rtol=2e-5, atol=1e-5)
    for name, g in (("g1", g1), ("g2", g2), ("g3", g3)):
        rtol, atol = tolerance(name, B, factor)
        np.testing.assert_allclose(g.reshape(B, 36), want[name], rtol=rtol, atol=atol, err_msg=name)
    rtol, atol = tolerance("gv", B, factor)
    np.testing.assert_allclose(gv.astype(np.float64), want["gv"], rtol=rtol + 2.0 ** -11, atol=atol + 2.0 ** -25)


# =========================================================================================================================
# lz_pack_trajectory_rows / lz_unpack_trajectory_rows
# =========================================================================================================================
UNPACK_OUT = ((396, torch.float32, np.float32), (220, torch.uint8, np.uint8), (220, torch.float32, np.float32),
              (None, torch.float32, np.float32), (None, torch.float32, np.float32))
UNPACK_NAMES = ("planes", "legal", "policy", "value", "soft")


def call_pack(L, d_rows, n, records, bad):
    st = L.lib().lz_pack_trajectory_rows(*(L.ptr(t) for t in d_rows), L.i64(n), L.ptr(records), L.ptr(bad),
                                         L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return st


def call_unpack(L, records, n, outs):
    st = L.lib().lz_unpack_trajectory_rows(L.ptr(records), L.i64(n), *(L.ptr(t) for t in outs),
                                           L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return st


def unpack_outputs(n):
    return [sentinel((n + GUARD,) if w is None else (n + GUARD, w), td) for w, td, _ in UNPACK_OUT]


def check_unpack(L, rec, where):
    n = rec.shape[0]
    outs = unpack_outputs(n)
    L.check(call_unpack(L, dv(rec), n, outs), "unpack_trajectory_rows")
    want = ref_unpack(rec)
    for name, t, w, (width, _, nd) in zip(UNPACK_NAMES, outs, want, UNPACK_OUT):
        got = t.cpu().numpy()
        assert_bits(got[:n], w.reshape(got[:n].shape), f"{where} {name}")
        assert_bits(got[n:], host_sentinel(got[n:].shape, nd), f"{where} {name} guard rows")


@pytest.mark.parametrize("n", K.CODEC_N)
def test_pack_equals_the_documented_layout_byte_for_byte(L, n):
    """All 360 bytes of every representable row (zero-filled policy slots and the pad included), the counter from a
    pre-set 7, the guard rows; once with the rows that are not representable in between, once without."""
    for defects in (True, False):
        rows, labels = K.codec_rows(n, seed=n, defects=defects)
        ok = ref_representable(rows)
        assert defects or ok.all()
        want, bad = ref_pack(rows)
        records = sentinel((n + GUARD, 360), torch.uint8)
        counter = dv(np.array([7], np.int32))
        d_rows = [dv(rows[0].reshape(n, 396)), dv(rows[1]), dv(rows[2]), dv(rows[3]), dv(rows[4])]
        L.check(call_pack(L, d_rows, n, records, counter), "pack_trajectory_rows")
        got = records.cpu().numpy()
        assert int(counter.item()) == 7 + bad, (labels, bad)
        assert_bits(got[:n][ok], want[ok], f"n={n} records")
        assert_bits(got[n:], host_sentinel((GUARD, 360), np.uint8), f"n={n} guard rows")
        if not defects:                                       # and back, on the device: the rows but for the -0.0 exception
            check_unpack(L, got[:n], f"n={n} unpack(pack)")


def test_pack_counts_each_defect_once(L):
    """One row per defect, each in a launch of its own among representable rows: the counter rises by exactly one."""
    rows, labels = K.codec_rows(20, seed=20)
    for r in np.flatnonzero(~np.isin(labels, ("ok", "minus_zero"))):
        keep = np.r_[0:3, r]
        sub = tuple(a[keep] for a in rows)
        counter = dv(np.array([7], np.int32))
        records = sentinel((4 + GUARD, 360), torch.uint8)
        d_rows = [dv(sub[0].reshape(4, 396)), dv(sub[1]), dv(sub[2]), dv(sub[3]), dv(sub[4])]
        L.check(call_pack(L, d_rows, 4, records, counter), "pack_trajectory_rows")
        assert int(counter.item()) == 8, labels[r]
        assert_bits(records[:3], ref_pack(tuple(a[:3] for a in rows))[0], labels[r])
        assert_bits(records[4:], host_sentinel((GUARD, 360), np.uint8), "guard rows")


@pytest.mark.parametrize("n", K.CODEC_N)
def test_unpack_of_random_records_equals_the_restatement(L, n):
    """Seeded random bytes (phase field, unowned bits, NaN payloads and all), at most 72 mask bits per record."""
    rec = K.random_records(n, seed=n)
    assert K.mask_bits_of(rec).max() <= 72
    check_unpack(L, rec, f"n={n} random records")


def test_unpack_of_overfull_records_gives_policy_zero_past_slot_71(L):
    """Records with 73 and 220 mask bits, each followed by at least three more records of the same buffer: a read past
    slot 71 would land in a neighbouring record (never outside the buffer) and show as wrong values."""
    rec, rows = K.overfull_records()
    nbits = K.mask_bits_of(rec)
    for row, count in rows.items():
        assert nbits[row] == count and len(rec) - 1 - row >= 3
    check_unpack(L, rec, "overfull records")


def test_codec_refuses_bad_arguments_without_a_launch(L):
    n = 4
    rows, _ = K.codec_rows(n, seed=4)
    d_rows = [dv(rows[0].reshape(n, 396)), dv(rows[1]), dv(rows[2]), dv(rows[3]), dv(rows[4])]
    records, counter = sentinel((n + GUARD, 360), torch.uint8), dv(np.array([7], np.int32))
    assert call_pack(L, d_rows, -1, records, counter) == ERR_ARG
    for i in range(5):
        assert call_pack(L, d_rows[:i] + [None] + d_rows[i + 1:], n, records, counter) == ERR_ARG, i
    assert call_pack(L, d_rows, n, None, counter) == ERR_ARG and call_pack(L, d_rows, n, records, None) == ERR_ARG
    assert call_pack(L, d_rows, 0, records, counter) == 0 and call_pack(L, [None] * 5, 0, None, None) == 0
    assert int(counter.item()) == 7
    assert_bits(records, host_sentinel((n + GUARD, 360), np.uint8), "records")
    rec = dv(K.random_records(n, seed=4))
    outs = unpack_outputs(n)
    assert call_unpack(L, rec, -1, outs) == ERR_ARG and call_unpack(L, None, n, outs) == ERR_ARG
    for i in range(5):
        assert call_unpack(L, rec, n, outs[:i] + [None] + outs[i + 1:]) == ERR_ARG, UNPACK_NAMES[i]
    assert call_unpack(L, rec, 0, outs) == 0 and call_unpack(L, None, 0, [None] * 5) == 0
    for name, t, (_, _, nd) in zip(UNPACK_NAMES, outs, UNPACK_OUT):
        assert_bits(t, host_sentinel(tuple(t.shape), nd), name)
