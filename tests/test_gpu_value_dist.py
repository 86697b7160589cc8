"""GPU: the distributional value target of merged positions from the kernels up --
lz_merge_value_distributions against the restatement (tests/value_dist_ref.py, anchored by tests/test_value_dist_cpu.py)
byte for byte, lz_policy_value_loss_dist_fwd_bwd through the C ABI against the entries without a table (byte for byte
where no table row is used, or where the row is the two-hot of identical members) and against the float64 restatement,
the linearity of the loss in its target through the kernels, and the two trainers end to end.

Bounds: those tests/test_gpu_train_kernels.py holds `terms[:, 2]` and `gv` to (tests/train_loss_ref.py::tolerance: bucket
CE rtol 2e-5 / atol 1e-5, gv rtol 1e-4 / atol 5e-5 * grad_scale * row weight / B) -- only the target changed.  The value
logits of these tests are 2 * randn, the base class of those bounds.

Case (d), the table path against the scalar path of the same rows at alpha 0.25, is printed by its test and recorded in
profiles/r23_value_dist.md."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import train_loss_cases as K
from tests import value_dist_ref as R
from tests.test_gpu_row_weights import (DEV, FIVE, _batch, _stack, _take, _weights,  # noqa: F401
                                        deterministic_training, unique_rows)
from tests.test_gpu_train_kernels import GUARD, LOSS_OUT, assert_bits, dv, host_sentinel, loss_inputs, run_loss, sentinel
from tests.test_gpu_row_weights import run_weighted
from tests.train_loss_ref import tolerance

pytestmark = pytest.mark.gpu
SEED = 20261022
F = np.float32
ERR_ARG, ERR_ALIGN = -1, -4
BATCHES = (1, 3, 4, 5, 9)                                          # around the four waves of a block
SENT_BITS = 0x7FC0BEEF


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from liuzhou_amd import _lib
    return _lib


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _table(rows):
    return torch.full((rows, R.BINS), SENT_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


# =========================================================================================================================
# lz_merge_value_distributions
# =========================================================================================================================
def gpu_merge(L, value_base, soft_base, stride, n, index, m, order, begin, rows, alpha, D, guard=2):
    """-> (status, table [D,101] numpy); `guard` sentinel rows behind the table are checked here."""
    dist = _table(D + guard)
    G = len(begin) - 1
    keep = [dv(index) if index is not None else None, dv(order), dv(begin), dv(rows)]
    st = L.lib().lz_merge_value_distributions(value_base, soft_base, L.i64(stride), L.i64(n), L.ptr(keep[0]), L.i64(m),
                                              L.ptr(keep[1]), L.ptr(keep[2]), L.i64(G), L.ptr(keep[3]), C.c_float(alpha),
                                              L.ptr(dist), L.i64(D), L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    out = dist.cpu().numpy()
    assert (out[D:].view(np.uint32) == SENT_BITS).all(), "guard rows behind the table"
    return st, out[:D]


def _skips(G):
    """dist_row: a permutation, with up to three groups skipped (-1, D, INT32_MIN) when there are enough groups."""
    rows = np.random.default_rng(SEED).permutation(G).astype(np.int32)
    D = G + 1
    if G >= 4:
        rows[1], rows[G - 2], rows[G - 1] = -1, D, R.INT32_MIN
    return rows, D


@pytest.mark.parametrize("alpha", R.ALPHAS)
@pytest.mark.parametrize("G", BATCHES)
def test_merge_kernel_is_byte_identical_to_the_restatement(L, G, alpha):
    c = R.build_case(SEED, G)
    v, s, order, begin = c["value"], c["soft"], c["order"], c["begin"]
    n = len(v)
    assert len(begin) - 1 == G and (G < 9 or 300 in c["sizes"])
    rows, D = _skips(G)
    blank = np.full((D, R.BINS), SENT_BITS, np.uint32).view(F)
    want = R.merge_ref(v, s, n, None, n, order, begin, rows, alpha, blank)
    dvv, dvs = dv(v), dv(s)
    st, got = gpu_merge(L, L.ptr(dvv), L.ptr(dvs), 4, n, None, n, order, begin, rows, alpha, D)
    assert st == 0 and _same(got, want)
    # the same members through a ring of records with guard records around them
    ring, slot = R.ring_of(v, s, guard=3, seed=SEED)
    d_ring = dv(ring)
    vb, sb = C.c_void_p(d_ring.data_ptr() + R.VALUE_OFF), C.c_void_p(d_ring.data_ptr() + R.SOFT_OFF)
    st, got = gpu_merge(L, vb, sb, R.REC, len(ring), slot, n, order, begin, rows, alpha, D)
    assert st == 0 and _same(got, want)
    # the host build gives the same bytes
    from liuzhou_amd import position_dedup as PD
    live = rows.copy()
    live[(rows < 0) | (rows >= D)] = -1
    host = PD.merge_value_distributions(torch.from_numpy(v), torch.from_numpy(s), 4, n, None, torch.from_numpy(order),
                                        torch.from_numpy(begin), torch.from_numpy(live), alpha, D).numpy()
    used = sorted(int(r) for r in live if r >= 0)
    assert _same(host[used], got[used])


def test_merge_kernel_zeroes_bad_groups_and_refuses_bad_arguments(L):
    c = R.build_case(SEED, 9)
    v, s, order, begin = c["value"], c["soft"], c["order"], c["begin"]
    n, G = len(v), 9
    rows = np.arange(G, dtype=np.int32)
    dvv, dvs = dv(v), dv(s)
    big = int(np.argmax(np.diff(begin)))
    _, good = gpu_merge(L, L.ptr(dvv), L.ptr(dvs), 4, n, None, n, order, begin, rows, 0.25, G)
    for where, bad_value in ((0, n), (70, -1), (299, 1 << 40)):      # in the first, second and last batch of 64 members
        broken = order.copy()
        broken[begin[big] + where] = bad_value
        st, got = gpu_merge(L, L.ptr(dvv), L.ptr(dvs), 4, n, None, n, broken, begin, rows, 0.25, G)
        assert st == 0 and not got[big].any() and _same(np.delete(got, big, 0), np.delete(good, big, 0))
    ring, slot = R.ring_of(v, s, guard=3, seed=SEED)
    d_ring = dv(ring)
    vb, sb = C.c_void_p(d_ring.data_ptr() + R.VALUE_OFF), C.c_void_p(d_ring.data_ptr() + R.SOFT_OFF)
    for far_value in (len(ring), -1):                                # a member's slot outside the ring
        far = slot.copy()
        far[order[begin[big] + 150]] = far_value
        st, got = gpu_merge(L, vb, sb, R.REC, len(ring), far, n, order, begin, rows, 0.25, G)
        assert st == 0 and not got[big].any() and _same(np.delete(got, big, 0), np.delete(good, big, 0))
    for b, e in ((5, 5), (7, 3), (-1, 2), (n, n + 1), (0, n + 1)):
        st, got = gpu_merge(L, L.ptr(dvv), L.ptr(dvs), 4, n, None, n, order, np.array([b, e], np.int64), np.zeros(1, np.int32), 0.0, 1)
        assert st == 0 and not got.any(), (b, e)
    # refusals: nothing is launched, the table keeps its sentinel
    M = L.lib().lz_merge_value_distributions
    d_order, d_begin, d_rows, dist = dv(order), dv(begin), dv(rows), _table(G)
    good_args = [L.ptr(dvv), L.ptr(dvs), 4, n, None, n, L.ptr(d_order), L.ptr(d_begin), G, L.ptr(d_rows), C.c_float(0.0),
                 L.ptr(dist), G]
    for i, value in ((3, -1), (5, -1), (8, -1), (12, -1), (2, 3), (2, 0)):
        args = list(good_args)
        args[i] = value
        assert M(*args, None) == ERR_ARG, i
    for i in (0, 1, 6, 7, 9, 11):
        args = list(good_args)
        args[i] = None
        assert M(*args, None) == ERR_ARG, i
    for i, by in ((0, 2), (6, 4), (7, 4), (9, 2), (11, 2)):
        args = list(good_args)
        args[i] = C.c_void_p(d_order.data_ptr() + by)
        assert M(*args, None) == ERR_ALIGN, i
    assert M(*good_args[:8], 0, None, good_args[10], None, G, None) == 0
    assert M(*good_args[:11], None, 0, None) == 0
    torch.cuda.synchronize()
    assert (dist.cpu().numpy().view(np.uint32) == SENT_BITS).all()


# =========================================================================================================================
# lz_policy_value_loss_dist_fwd_bwd
# =========================================================================================================================
def value_case(B, seed=SEED):
    """The edge batch with value logits of the base class (2 * randn) on every row."""
    c = dict(K.edge_batch(B))
    c["vlogits"] = (2.0 * np.random.default_rng(seed + B).standard_normal((B, R.BINS))).astype(F)
    return c


def run_dist(L, c, rw, setting, grad_scale, dist_row, table, D=None):
    """-> the outputs of the B rows (numpy) of the distributional entry; the guard rows behind every output are checked
    here.  `rw` None: a NULL row_weight; `table`: a device tensor or None."""
    B = len(c["value"])
    ws = dv(np.array([K.weight_sum_of(c["value"], setting[2])], F))
    outs = [sentinel((B + GUARD, w)) for _, w in LOSS_OUT]
    d_in, d_rw, d_row = loss_inputs(c), (None if rw is None else dv(rw)), dv(np.asarray(dist_row, np.int32))
    D = (0 if table is None else int(table.shape[0])) if D is None else D
    st = L.lib().lz_policy_value_loss_dist_fwd_bwd(
        *(L.ptr(t) for t in d_in), L.ptr(d_rw), L.i64(B), C.c_float(setting[0]), C.c_float(setting[1]), C.c_float(setting[2]),
        L.ptr(ws), C.c_float(grad_scale), *(L.ptr(t) for t in outs), L.stream_ptr(torch.device(DEV)), L.ptr(d_row), L.ptr(table),
        L.i64(D))
    torch.cuda.synchronize()
    L.check(st, "policy_value_loss_dist_fwd_bwd")
    got = {}
    for (name, w), t in zip(LOSS_OUT, outs):
        a = t.cpu().numpy()
        assert_bits(a[B:], host_sentinel((GUARD, w)), f"{name} guard rows")
        got[name] = a[:B]
    return got


def _weights_for(B):
    return np.array([(1.0, 0.5, 3.0, 2.0, 0.25)[i % 5] for i in range(B)], F)


@pytest.mark.parametrize("B", BATCHES)
def test_rows_without_a_table_row_give_every_byte_of_the_entries_without_a_table(L, B):
    """(a): dist_row of -1, D, D + 7 and INT32_MIN, over a table of NaNs that nothing may read."""
    c = K.edge_batch(B)
    D = 3
    table = _table(D + 2)                                            # quiet NaNs: a read would show in every output
    for setting in (K.SETTINGS[0], K.SETTINGS[1]):
        plain = run_loss(L, c, setting, 3.0)
        weighted = run_weighted(L, c, _weights_for(B), setting, 3.0)
        for fill in (-1, D, D + 7, R.INT32_MIN, "mixed"):
            row = np.array([(-1, D, D + 7, R.INT32_MIN)[i % 4] for i in range(B)] if fill == "mixed" else [fill] * B, np.int32)
            for rw, want in ((None, plain), (_weights_for(B), weighted)):
                got = run_dist(L, c, rw, setting, 3.0, row, table, D)
                for name, _ in LOSS_OUT:
                    assert_bits(got[name], want[name], f"B={B} {setting} dist_row={fill} weighted={rw is not None} {name}")
        got = run_dist(L, c, None, setting, 3.0, np.full(B, 0, np.int32), None, 0)      # D == 0: no table at all
        for name, _ in LOSS_OUT:
            assert_bits(got[name], plain[name], f"D=0 {name}")
    assert (table.cpu().numpy().view(np.uint32) == SENT_BITS).all()


def _identical_member_table(L, c, alpha, counts):
    """The table of B groups, group b = counts[b] copies of row b's (value, soft), built by the merge kernel."""
    B = len(c["value"])
    owner = np.repeat(np.arange(B), counts)
    order = np.arange(len(owner), dtype=np.int64)
    begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    v, s = dv(c["value"][owner]), dv(c["soft"][owner])
    st, table = gpu_merge(L, L.ptr(v), L.ptr(s), 4, len(owner), None, len(owner), order, begin, np.arange(B, dtype=np.int32), alpha, B)
    assert st == 0
    return table


@pytest.mark.parametrize("B", BATCHES)
def test_a_table_row_of_identical_members_is_the_scalar_path(L, B):
    """(b) at alpha 0 byte for byte; (d) at alpha 0.25 measured and held to the bounds of (c)."""
    c = value_case(B)
    counts = np.array([(1, 2, 3, 7, 300)[i % 5] for i in range(B)])
    gs = 3.0
    for alpha in (0.0, 0.25):
        setting = (alpha, 0.0, 1.0)
        table = _identical_member_table(L, c, alpha, counts)
        for b in range(B):                                           # the table row is the restatement's two-hot, exactly
            assert _same(table[b], R.two_hot_row(c["value"][b], c["soft"][b], alpha)), (alpha, b)
        d_table = torch.cat([dv(table), _table(2)])                  # sentinel rows behind the table
        for rw, scalar in ((None, run_loss(L, c, setting, gs)), (_weights_for(B), run_weighted(L, c, _weights_for(B), setting, gs))):
            got = run_dist(L, c, rw, setting, gs, np.arange(B, dtype=np.int32), d_table, B)
            ce_diff = float(np.abs(got["terms"][:, 2].astype(np.float64) - scalar["terms"][:, 2]).max())
            gv_diff = float(np.abs(got["gv"].astype(np.float64) - scalar["gv"]).max())
            print(f"B={B} alpha={alpha} weighted={rw is not None}: table path - scalar path: bucket CE {ce_diff:.3e}, gv {gv_diff:.3e}")
            for name in ("g1", "g2", "g3"):                          # policy: untouched
                assert_bits(got[name], scalar[name], name)
            for col in (0, 1, 3):
                assert_bits(got["terms"][:, col], scalar["terms"][:, col], f"terms column {col}")
            if alpha == 0.0:
                assert_bits(got["terms"], scalar["terms"], "terms")
                assert_bits(got["gv"], scalar["gv"], "gv")
            else:
                rt, at = tolerance("ce", B, gs)
                assert (np.abs(got["terms"][:, 2].astype(np.float64) - scalar["terms"][:, 2])
                        <= at + rt * np.abs(scalar["terms"][:, 2])).all()
                w = np.ones(B) if rw is None else rw.astype(np.float64)
                for b in range(B):
                    rt, at = tolerance("gv", B, gs * float(w[b]))
                    assert (np.abs(got["gv"][b].astype(np.float64) - scalar["gv"][b]) <= at + rt * np.abs(scalar["gv"][b])).all()
        assert (d_table[B:].cpu().numpy().view(np.uint32) == SENT_BITS).all()


@pytest.mark.parametrize("B", BATCHES)
def test_rows_with_real_mixtures_equal_the_float64_restatement(L, B):
    """(c), (e): every other row points at a table row mixed from 2..300 different members; the rows between take the
    scalar path in the same launch."""
    rng = np.random.default_rng(SEED + B)
    c = value_case(B)
    setting, gs = (0.25, 0.0, 1.0), 3.0
    D = (B + 1) // 2
    sizes = [(2, 3, 300, 5)[d % 4] for d in range(D)]
    n = sum(sizes)
    mv = rng.choice(np.array([-1, 0, 1], F), n).astype(F)
    ms = rng.uniform(-1.1, 1.1, n).astype(F)
    begin = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    order = rng.permutation(n).astype(np.int64)
    d_mv, d_ms = dv(mv), dv(ms)
    st, table = gpu_merge(L, L.ptr(d_mv), L.ptr(d_ms), 4, n, None, n, order, begin, np.arange(D, dtype=np.int32), setting[0], D)
    assert st == 0 and _same(table, R.merge_ref(mv, ms, n, None, n, order, begin, np.arange(D), setting[0], np.zeros((D, R.BINS), F)))
    dist_row = np.array([b // 2 if b % 2 == 0 else -1 for b in range(B)], np.int32)
    d_table = torch.cat([dv(table), _table(2)])
    for rw in (None, _weights_for(B)):
        scalar = run_loss(L, c, setting, gs) if rw is None else run_weighted(L, c, rw, setting, gs)
        got = run_dist(L, c, rw, setting, gs, dist_row, d_table, D)
        for name in ("g1", "g2", "g3"):
            assert_bits(got[name], scalar[name], name)
        for col in (0, 1, 3):
            assert_bits(got["terms"][:, col], scalar["terms"][:, col], f"terms column {col}")
        w = np.ones(B) if rw is None else rw.astype(np.float64)
        target = np.stack([table[dist_row[b]] if dist_row[b] >= 0 else R.two_hot_row(c["value"][b], c["soft"][b], setting[0])
                           for b in range(B)])
        ce, gv = R.ce_and_grad(c["vlogits"], target, gs / B * w)
        rt, at = tolerance("ce", B, gs)
        worst = float((np.abs(got["terms"][:, 2] - ce) / (at + rt * np.abs(ce))).max())
        print(f"B={B} weighted={rw is not None}: bucket CE worst {worst:.3f} x bound")
        assert worst <= 1.0
        for b in range(B):
            rt, at = tolerance("gv", B, gs * float(w[b]))
            ratio = float((np.abs(got["gv"][b] - gv[b]) / (at + rt * np.abs(gv[b]))).max())
            assert ratio <= 1.0, (b, ratio)
            if dist_row[b] < 0:                                      # the scalar rows of the same launch: the parent's bytes
                assert_bits(got["gv"][b], scalar["gv"][b], f"gv row {b}")
                assert_bits(got["terms"][b], scalar["terms"][b], f"terms row {b}")
        assert np.abs(got["gv"][0].astype(np.float64) - scalar["gv"][0]).max() > 1e-3 * gs / B * w[0]      # the target did change
    assert (d_table[D:].cpu().numpy().view(np.uint32) == SENT_BITS).all()


def test_dist_entry_refuses_bad_arguments_without_a_launch(L):
    c = K.edge_batch(4)
    d_in = loss_inputs(c)
    outs = [sentinel((4 + GUARD, w)) for _, w in LOSS_OUT]
    ws, row, table = dv(np.array([4.0], F)), dv(np.zeros(4, np.int32)), _table(2)
    fn = L.lib().lz_policy_value_loss_dist_fwd_bwd

    def call(d_in=d_in, rw=None, B=4, ws=ws, outs=outs, row=row, table=table, D=2):
        return fn(*(L.ptr(t) for t in d_in), L.ptr(rw), L.i64(B), C.c_float(0.0), C.c_float(0.0), C.c_float(1.0), L.ptr(ws),
                  C.c_float(1.0), *(L.ptr(t) for t in outs), L.stream_ptr(torch.device(DEV)), L.ptr(row), L.ptr(table), L.i64(D))
    assert call(row=None) == ERR_ARG and call(table=None) == ERR_ARG and call(D=-1) == ERR_ARG and call(B=-1) == ERR_ARG
    for i in range(len(d_in)):
        assert call(d_in=d_in[:i] + [None] + d_in[i + 1:]) == ERR_ARG, K.INPUT_KEYS[i]
    for i in range(len(outs)):
        assert call(outs=outs[:i] + [None] + outs[i + 1:]) == ERR_ARG, LOSS_OUT[i][0]
    assert call(ws=None) == ERR_ARG
    assert call(B=0) == 0 and call(d_in=[None] * 8, B=0, ws=None, outs=[None] * 5, row=None, table=None) == 0
    torch.cuda.synchronize()
    for (name, w), t in zip(LOSS_OUT, outs):
        assert_bits(t, host_sentinel((4 + GUARD, w)), name)


# =========================================================================================================================
# linearity through the kernels
# =========================================================================================================================
def test_linearity_on_the_device(L):
    """The CPU construction (tests/test_value_dist_cpu.py) through the kernels: the n unmerged rows through the entry
    without a table, one row per group through the distributional entry with weight count, B = groups and grad_scale =
    groups / n, its table from the merge kernel.  Each side within the gv bound of its float64 side; the float64 sides
    agree to 1e-12."""
    c = R.linearity_case(SEED, exact=True)
    owner, count = c["owner"], c["count"]
    n, G = len(owner), len(count)
    begin = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    d_v, d_s = dv(c["value"]), dv(c["soft"])
    st, table = gpu_merge(L, L.ptr(d_v), L.ptr(d_s), 4, n, None, n, np.arange(n, dtype=np.int64), begin, np.arange(G, dtype=np.int32),
                          c["alpha"], G)
    assert st == 0
    side_unmerged, side_merged = R.linearity_sides(c, table)
    assert np.abs(side_unmerged - side_merged).max() <= 1e-12
    setting = (c["alpha"], 0.0, 1.0)
    rows = dict(K.edge_batch(n))
    rows.update(vlogits=np.ascontiguousarray(c["logits"][owner]), value=c["value"], soft=c["soft"])
    got = run_loss(L, rows, setting, 1.0)
    summed = np.zeros((G, R.BINS))
    np.add.at(summed, owner, got["gv"].astype(np.float64))
    rt, at = tolerance("gv", n, 1.0)
    _, per_row = R.ce_and_grad(rows["vlogits"], np.stack([R.two_hot_row(v, s, c["alpha"]) for v, s in zip(c["value"], c["soft"])]),
                               1.0 / n)
    bound = np.zeros((G, R.BINS))
    np.add.at(bound, owner, at + rt * np.abs(per_row))               # the sum of the members' bounds
    assert (np.abs(summed - side_unmerged) <= bound).all()
    merged_rows = dict(K.edge_batch(G))
    mean_v = np.array([c["value"][owner == g].astype(np.float64).mean() for g in range(G)], F)
    merged_rows.update(vlogits=c["logits"], value=mean_v, soft=mean_v.copy())
    rw = count.astype(F)
    gs = G / n
    got = run_dist(L, merged_rows, rw, setting, gs, np.arange(G, dtype=np.int32), dv(table), G)
    for g in range(G):
        rt, at = tolerance("gv", G, float(np.float32(gs)) * float(rw[g]))
        assert (np.abs(got["gv"][g] - side_merged[g]) <= at + rt * np.abs(side_merged[g])).all(), g
    # the mean target on the (+1, -1) pair is far outside that bound: the defect, on the device
    mean_path = run_weighted(L, merged_rows, rw, setting, gs)
    assert np.abs(mean_path["gv"][0] - side_merged[0]).max() > 0.1 * count[0] / n


# =========================================================================================================================
# the trainers
# =========================================================================================================================
def _small_model():
    from liuzhou_amd.net import ChessNet, stable_resnet_init
    model = ChessNet(trunk_channels=16, num_blocks=2, policy_channels=8, value_channels=8, value_mlp_channels=16)
    stable_resnet_init(model, 20260314)
    with torch.no_grad():                                            # value logits of order one instead of 1e-3: the bucket
        for mod in model.modules():                                  # loss then depends on its target
            if isinstance(mod, torch.nn.Linear) and mod.out_features == R.BINS:
                mod.weight.mul_(300.0)
    return model


def _train_small(rows, **kw):
    from liuzhou_amd.train_bridge import train_network_from_tensors
    torch.manual_seed(5)
    kw.setdefault("soft_label_alpha", 0.0)
    model, metrics = train_network_from_tensors(_small_model(), _batch(rows), batch_size=32, epochs=1, lr=2e-3, device=DEV,
                                                use_amp=False, **kw)
    return _weights(model), metrics


def _train_window_small(generations, **kw):
    from liuzhou_amd.replay_window import ReplayWindow
    from liuzhou_amd.train_bridge import train_network_from_window
    w = ReplayWindow(DEV, max_generations=len(generations), capacity_rows=sum(len(g["soft"]) for g in generations) + 5)
    w.add_generation(_batch(generations[0]), generation=3)
    for g in generations[1:]:
        w.add_generation(_batch(g))
    torch.manual_seed(5)
    kw.setdefault("soft_label_alpha", 0.0)
    model, m = train_network_from_window(_small_model(), w, batch_size=32, epochs=1, lr=2e-3, device=DEV, use_amp=False, **kw)
    return _weights(model), m


def _spy_loss(monkeypatch):
    """Every call of the fused loss by the stepper: (value logits, value, soft, keyword arguments)."""
    from liuzhou_amd import train_bridge as TB
    seen = []
    real = TB.fused_policy_value_loss

    def spy(lp1, lp2, lpm, vlogits, masks, policy, values, soft, **kw):
        seen.append((vlogits.detach().float().cpu().numpy(), values.cpu().numpy(), soft.cpu().numpy(),
                     {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in kw.items()}))
        return real(lp1, lp2, lpm, vlogits, masks, policy, values, soft, **kw)
    monkeypatch.setattr(TB, "fused_policy_value_loss", spy)
    return seen


def _with_targets(rows, value, soft):
    out = {f: rows[f].copy() for f in FIVE}
    out["value"], out["soft"] = np.asarray(value, F), np.asarray(soft, F)
    return out


def test_tensor_trainer_without_duplicates_trains_to_the_bits_of_mean(deterministic_training, monkeypatch, unique_rows, L):
    rows = _take(unique_rows, 0, 64)
    _train_small(rows, dedup_positions="exact")                     # warm-up: kernel selection, allocator
    w_off, m_off = _train_small(rows)
    w_mean, m_mean = _train_small(rows, dedup_positions="exact")
    seen = _spy_loss(monkeypatch)
    w_dist, m_dist = _train_small(rows, dedup_positions="exact", dedup_value_target="distribution")
    assert torch.equal(w_mean, w_dist), float((w_mean - w_dist).abs().max())
    assert len(seen) == 2 and all((kw["value_dist_row"] == -1).all() and kw["value_dist"].shape == (0, 101) for *_, kw in seen)
    assert m_dist["position_dedup"] == dict(m_mean["position_dedup"], value_target="distribution")
    assert "value_target" not in m_mean["position_dedup"] and "position_dedup" not in m_off      # defaults: no new key
    assert set(m_dist) == set(m_mean) and m_dist["epoch_stats"][0]["avg_value_bucket_loss"] == m_mean["epoch_stats"][0]["avg_value_bucket_loss"]
    seen.clear()
    _train_small(rows, dedup_positions="exact")
    assert len(seen) == 2 and all("value_dist" not in kw and "value_dist_row" not in kw for *_, kw in seen)


def test_tensor_trainer_with_identical_duplicates_trains_to_the_bits_of_mean(deterministic_training, monkeypatch, unique_rows, L):
    x = _take(unique_rows, 0, 48)
    rows = _stack(x, _take(x, 0, 16))                                # 64 rows, 16 positions twice with the same targets
    seen = _spy_loss(monkeypatch)
    for kw in ({}, {"dedup_max_copies": 2, "dedup_weighting": "weight"}):
        w_mean, m_mean = _train_small(rows, dedup_positions="exact", **kw)
        seen.clear()
        w_dist, m_dist = _train_small(rows, dedup_positions="exact", dedup_value_target="distribution", **kw)
        assert torch.equal(w_mean, w_dist), float((w_mean - w_dist).abs().max())
        assert m_dist["position_dedup"]["merged_groups"] == 16 and m_dist["position_dedup"]["rows_out"] == 48
        used = np.concatenate([kw_["value_dist_row"] for *_, kw_ in seen])
        assert sorted(used[used >= 0].tolist()) == list(range(16)) and (used >= 0).sum() == 16 and len(used) == 48
        assert seen[0][3]["value_dist"].shape == (16, 101)


def test_tensor_trainer_with_a_won_and_lost_duplicate(deterministic_training, monkeypatch, unique_rows, L):
    """16 positions occur twice, won once and lost once: the weights differ from those of "mean", and the epoch's bucket
    loss is the restatement's -- the cross entropy of the model's own logits against halves on bins 0 and 100."""
    x = _take(unique_rows, 0, 48)
    first = _with_targets(x, np.where(np.arange(48) < 16, 1.0, x["value"]), np.where(np.arange(48) < 16, 1.0, x["soft"]))
    again = _with_targets(_take(x, 0, 16), -np.ones(16), -np.ones(16))
    rows = _stack(first, again)
    w_mean, m_mean = _train_small(rows, dedup_positions="exact")
    seen = _spy_loss(monkeypatch)
    w_dist, m_dist = _train_small(rows, dedup_positions="exact", dedup_value_target="distribution")
    assert not torch.equal(w_mean, w_dist)
    half = np.zeros(R.BINS, F)
    half[[0, 100]] = 0.5
    total, count = 0.0, 0
    for vlogits, values, soft, kw in seen:
        table, row = kw["value_dist"], kw["value_dist_row"]
        assert table.shape == (16, 101) and all(_same(t, half) for t in table)
        assert (values[row >= 0] == 0).all()                         # the merged rows keep the mean value: 0
        target = np.stack([table[d] if d >= 0 else R.two_hot_row(v, s, 0.0) for d, v, s in zip(row, values, soft)])
        ce, _ = R.ce_and_grad(vlogits, target, 1.0)
        total += float(ce.sum())
        count += len(ce)
    assert count == 48
    got, want = m_dist["epoch_stats"][0]["avg_value_bucket_loss"], total / count
    rt, at = tolerance("ce", 32, 1.0)
    print(f"avg_value_bucket_loss {got!r}, restatement {want!r}, mean target {m_mean['epoch_stats'][0]['avg_value_bucket_loss']!r}")
    assert abs(got - want) <= at + rt * abs(want)


def test_window_trainer_equals_the_tensor_trainer_on_the_concatenation(deterministic_training, unique_rows, L):
    """Section 30's equivalence, carried over: two generations merged record to record with the table computed from the
    ring, against the tensor trainer on the concatenation, newest first."""
    x = unique_rows
    rng = np.random.default_rng(SEED)

    def retarget(rows):
        n = len(rows["soft"])
        return _with_targets(rows, rng.choice(np.array([-1, 0, 1], F), n), rng.uniform(-1, 1, n))
    old = _stack(_take(x, 0, 24), retarget(_take(x, 0, 8)))         # 8 positions twice inside the old generation
    new = _stack(_take(x, 16, 40), retarget(_take(x, 20, 28)))      # 8 shared with the old one, 8 twice inside the new
    kw_t = {"dedup_positions": "exact", "dedup_max_copies": 4, "dedup_weighting": "weight"}
    kw_w = {"replay_budget_per_generation": 10 ** 6, "replay_merge_positions": "exact", "replay_merge_max_weight": 4}
    for alpha in (0.0, 0.25):
        w_tensor, m_tensor = _train_small(_stack(new, old), dedup_value_target="distribution", soft_label_alpha=alpha, **kw_t)
        w_window, m_window = _train_window_small([old, new], replay_merge_value_target="distribution", soft_label_alpha=alpha, **kw_w)
        assert torch.equal(w_tensor, w_window), (alpha, float((w_tensor - w_window).abs().max()))
        merge = m_window["replay_window"]["merge"]
        assert merge["value_target"] == "distribution" == m_tensor["position_dedup"]["value_target"]
        assert merge["rows_in"] == 64 and merge["groups"] == 40 == m_tensor["position_dedup"]["groups"]
        assert merge["merged_groups"] == m_tensor["position_dedup"]["merged_groups"] >= 16
        w_mean, m_mean = _train_window_small([old, new], soft_label_alpha=alpha, **kw_w)
        assert not torch.equal(w_mean, w_window) and "value_target" not in m_mean["replay_window"]["merge"]
