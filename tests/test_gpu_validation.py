"""GPU: the validation metrics -- lz_valid_row_metrics against the float64 restatement tests/valid_ref.py on the
hand-built rows of tests/valid_cases.py and against the loss kernel, lz_valid_reduce bit for bit against the exact
restatement, `validate_network` against its own parts, and the staged loop's --validate flag.

Bounds of the row kernel: the integer outputs and the 0/1 columns exactly (the inputs keep a margin between the two best
logits unless they tie exactly); the calibration bin is the rule applied in float32 to the kernel's own v_hat; the float
columns start from the loss kernel's bound (tests/train_loss_ref.py: rtol 2e-5 / atol 1e-5, for the wide class times the
factor measured between the float32 oracle and the float64 restatement -- never a figure from the kernel)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import valid_cases as VC
from tests import valid_ref as VR
from tests.train_loss_ref import BASE_TOL, ref_loss, wide_class_factors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8
SENT_F32 = 0x7FC0BEEF
POLICY_FLOAT = (VR.KL, VR.CE, VR.H_TARGET, VR.H_NET, VR.P_TOP)
VALUE_FLOAT = (VR.BUCKET_CE, VR.V_HAT, VR.SQ_ERR)
EXACT = (VR.TOP1, VR.DECISIVE, VR.POLICY_VALID)
REDUCE_B = (1, 63, 64, 65, 4097)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from liuzhou_amd import _lib
    return _lib


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_rows(L, c, alpha, B=None):
    """The C ABI with 8 guard rows behind both outputs -> rows f32[B,12], cls i32[B,4] (numpy)."""
    B = len(c["value"]) if B is None else B
    d = [dv(c[k]) for k in VC.INPUT_KEYS] + [dv(c["planes"])]
    rows = torch.full((B + GUARD, 12), SENT_F32, dtype=torch.int32, device=DEV).view(torch.float32)
    cls = torch.full((B + GUARD, 4), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    st = L.lib().lz_valid_row_metrics(*(L.ptr(t) for t in d), L.i64(B), C.c_float(alpha), L.ptr(rows), L.ptr(cls),
                                      L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert st == 0
    r, k = rows.cpu().numpy(), cls.cpu().numpy()
    assert (r[B:].view(np.int32) == SENT_F32).all() and (k[B:] == 0x7F7F7F7F).all(), "guard rows written"
    return r[:B], k[:B]


def _factors(c, alpha):
    B = len(c["value"])
    want = ref_loss(*(c[k] for k in VC.INPUT_KEYS), alpha=alpha, anti_draw=0.0, draw_weight=1.0, weight_sum=float(B))
    f, _ = wide_class_factors(c, VC.policy_class(c), VC.value_class(c), want, (alpha, 0.0, 1.0), 1.0)
    return f


# =========================================================================================================================
# lz_valid_row_metrics
# =========================================================================================================================
@pytest.mark.parametrize("B", VC.ROW_B)
def test_row_kernel_equals_the_restatement(L, B):
    """B = 1, 3, 4, 5: a last workgroup with one, three, four and one live waves; 257: every hand-built class."""
    c = VC.row_batch(B)
    for alpha in VC.ALPHAS:
        got, gcls = run_rows(L, c, alpha)
        want, wcls = VR.ref_rows(*(c[k] for k in VC.INPUT_KEYS), c["planes"], alpha=alpha)
        f = _factors(c, alpha)
        pf = np.array([f[("kl", str(k))] for k in VC.policy_class(c)])
        vf = np.array([f[("ce", str(k))] for k in VC.value_class(c)])
        rtol, atol = BASE_TOL["kl"]
        assert np.isfinite(got).all()
        for col in POLICY_FLOAT + VALUE_FLOAT:
            fac = pf if col in POLICY_FLOAT else vf
            ratio = np.abs(got[:, col].astype(np.float64) - want[:, col]) / (fac * (atol + rtol * np.abs(want[:, col])))
            i = int(np.argmax(ratio))
            print(f"B={B} alpha={alpha} col {col:2d}: worst {ratio[i]:.3f} x bound at row {i} ({c['kind'][i]})")
            assert (ratio <= 1.0).all(), (col, i, got[i, col], want[i, col], c["kind"][i])
        for col in EXACT:
            assert np.array_equal(got[:, col], want[:, col].astype(np.float32)), col
        sure = np.abs(want[:, VR.V_HAT]) > 1e-4                    # the sign of v_hat is beyond rounding
        assert np.array_equal(got[sure, VR.SIGN_OK], want[sure, VR.SIGN_OK].astype(np.float32))
        assert np.isin(got[:, VR.SIGN_OK], (0.0, 1.0)).all()
        assert np.array_equal(gcls[:, [0, 2, 3]], wcls[:, [0, 2, 3]])
        assert np.array_equal(gcls[:, 1], VR.calib_bin(got[:, VR.V_HAT]))      # the rule on the kernel's own v_hat
        u = (want[:, VR.V_HAT] + 1.0) * 5.0
        inside = np.abs(u - np.round(u)) > 1e-3                    # not at a bin edge
        assert np.array_equal(gcls[inside, 1], wcls[inside, 1])
        for i, tie in enumerate(c["tie"]):
            if tie is not None:
                assert gcls[i, 2] == min(tie)                       # the lowest index wins an exact tie
        # the public wrapper is the same call
        from liuzhou_amd.validation import row_metrics
        r2, k2 = row_metrics(*(dv(c[k]) for k in ("lp1", "lp2", "lpm", "vlogits", "planes")), dv(c["mask"]).bool(),
                             dv(c["target"]), dv(c["value"]), dv(c["soft"]), soft_label_alpha=alpha)
        assert r2.cpu().numpy().tobytes() == got.tobytes() and k2.cpu().numpy().tobytes() == gcls.tobytes()


def test_row_kernel_is_total_on_arbitrary_bits(L):
    """Every input filled with random bit patterns: outputs are defined, the integers stay in their ranges, nothing is
    written behind the batch (no index of the kernel depends on data)."""
    rng = np.random.default_rng(77)
    B = 67
    bits = lambda *s: rng.integers(0, 1 << 32, s, dtype=np.uint64).astype(np.uint32).view(np.float32)
    c = dict(lp1=bits(B, 36), lp2=bits(B, 36), lpm=bits(B, 36), vlogits=bits(B, 101),
             mask=rng.integers(0, 256, (B, 220)).astype(np.uint8) * (rng.random((B, 220)) < 0.5), target=bits(B, 220),
             value=bits(B), soft=bits(B), planes=bits(B, 11, 6, 6))
    c["mask"] = c["mask"].astype(np.uint8)
    got, cls = run_rows(L, c, 0.3)
    assert ((cls[:, 0] >= -1) & (cls[:, 0] <= 6)).all() and ((cls[:, 1] >= 0) & (cls[:, 1] <= 9)).all()
    assert ((cls[:, 2:] >= -1) & (cls[:, 2:] <= 219)).all()
    legal = c["mask"] != 0
    from tests.train_loss_ref import MOVE_DEST, MOVE_FROM, ON_BOARD
    with np.errstate(all="ignore"):                                  # the combined logits as the kernel adds them: float32
        moves = np.where(ON_BOARD[None, :], c["lp2"][:, MOVE_FROM] + c["lp1"][:, np.where(ON_BOARD, MOVE_DEST, 0)], -np.inf)
    comb = np.concatenate([c["lp1"], moves.astype(np.float32), c["lpm"], np.zeros((B, 4), np.float32)], axis=1)
    for i in range(B):
        assert cls[i, 2] == VR.argmax_legal(comb[i], legal[i])
    assert np.array_equal(cls[:, 0], VR.phase_of(c["planes"])) and np.array_equal(cls[:, 1], VR.calib_bin(got[:, VR.V_HAT]))
    for col in (VR.TOP1, VR.SIGN_OK, VR.DECISIVE, VR.POLICY_VALID):
        assert np.isin(got[:, col], (0.0, 1.0)).all()
    invalid = got[:, VR.POLICY_VALID] == 0
    assert not got[invalid, :6].any() and (cls[invalid, 3] == -1).all()


def test_row_kernel_argument_conventions(L):
    c = VC.row_batch(4)
    d = [dv(c[k]) for k in VC.INPUT_KEYS] + [dv(c["planes"])]
    rows, cls = torch.zeros((4, 12), device=DEV), torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    full = [L.ptr(t) for t in d] + [L.ptr(rows), L.ptr(cls)]
    ins, outs = full[:9], full[9:]
    assert L.lib().lz_valid_row_metrics(*[None] * 9, L.i64(0), C.c_float(0.0), None, None, None) == 0
    assert L.lib().lz_valid_row_metrics(*ins, L.i64(-1), C.c_float(0.0), *outs, None) == -1
    for k in range(11):
        p = list(full)
        p[k] = None
        assert L.lib().lz_valid_row_metrics(*p[:9], L.i64(4), C.c_float(0.0), *p[9:], None) == -1, k
    acc = torch.zeros((18, 14), dtype=torch.float64, device=DEV)
    assert L.lib().lz_valid_reduce(None, None, None, L.i64(0), None, None, None) == 0
    assert L.lib().lz_valid_reduce(L.ptr(rows), L.ptr(cls), None, L.i64(4), None, None, None) == -1
    assert L.lib().lz_valid_reduce(L.ptr(rows), L.ptr(cls), L.ptr(rows), L.i64(4), L.ptr(acc), None, None) == -1
    torch.cuda.synchronize()
    assert not acc.any() and not rows.any()


def test_means_equal_the_loss_kernel(L):
    from liuzhou_amd.train_loss import fused_policy_value_loss
    c = VC.row_batch(257)
    for alpha in VC.ALPHAS:
        got, _ = run_rows(L, c, alpha)
        _, parts = fused_policy_value_loss(dv(c["lp1"]), dv(c["lp2"]), dv(c["lpm"]), dv(c["vlogits"]), dv(c["mask"]).bool(),
                                           dv(c["target"]), dv(c["value"]), dv(c["soft"]), soft_label_alpha=alpha,
                                           anti_draw_penalty=0.0, policy_draw_weight=1.0)
        rtol, atol = BASE_TOL["kl"]
        for col, key in ((VR.KL, "policy_loss"), (VR.BUCKET_CE, "bucket_value_loss")):
            mine, theirs = float(got[:, col].astype(np.float64).mean()), float(parts[key])
            print(f"alpha={alpha} {key}: {mine!r} vs {theirs!r}")
            assert abs(mine - theirs) <= atol + rtol * abs(theirs), (key, mine, theirs)


# =========================================================================================================================
# lz_valid_reduce
# =========================================================================================================================
def _dev_reduce(L, batches, with_value=True):
    acc = torch.zeros((18, 14), dtype=torch.float64, device=DEV)
    zsum = torch.zeros(18, dtype=torch.float64, device=DEV)
    keep = []
    for rows, cls, value, _ in batches:                             # no host read between the calls
        t = (dv(rows), dv(cls), dv(value))
        keep.append(t)
        st = L.lib().lz_valid_reduce(L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]) if with_value else None, L.i64(len(rows)), L.ptr(acc),
                                     L.ptr(zsum) if with_value else None, L.stream_ptr(torch.device(DEV)))
        assert st == 0
    torch.cuda.synchronize()
    return acc.cpu().numpy(), zsum.cpu().numpy()


def _ref_reduce(batches, with_value=True):
    acc, zsum = np.zeros((18, 14)), np.zeros(18)
    for rows, cls, value, _ in batches:
        VR.ref_reduce(rows, cls, value if with_value else None, acc, zsum)
    return acc, zsum


@pytest.mark.parametrize("B", REDUCE_B)
def test_reduce_kernel_equals_the_restatement_bit_for_bit(L, B):
    for mode in ("mixed", "one_group", "all_skipped", ("bad", 7, np.nan), ("bad", 0, np.inf), ("bad", 11, -np.inf)):
        batch = VC.reduce_batch(B, 5, mode)
        got, want = _dev_reduce(L, [batch]), _ref_reduce([batch])
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (B, mode)
        if mode == "all_skipped":
            assert got[0][0, 13] == B and not got[0][:, :13].any()
        if mode == "one_group":
            assert got[0][0].tobytes() == got[0][4].tobytes() == got[0][12].tobytes() and got[0][0, 12] == B
    batch = VC.reduce_batch(B, 6)
    got, want = _dev_reduce(L, [batch], with_value=False), _ref_reduce([batch], with_value=False)
    assert got[0].tobytes() == want[0].tobytes() and not got[1].any()


def test_reduce_kernel_accumulates_on_the_stream(L):
    batches = [VC.reduce_batch(4097, 7), VC.reduce_batch(65, 8, ("bad", 8, np.nan)), VC.reduce_batch(1, 9)]
    got, want = _dev_reduce(L, batches), _ref_reduce(batches)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert got[0][0, 12] + got[0][0, 13] == 4097 + 65 + 1
    from liuzhou_amd.validation import MetricSums, summarize
    s = MetricSums(DEV)
    for rows, cls, value, _ in batches:
        s.add(dv(rows), dv(cls), dv(value))
    assert s.result() == summarize(want[0], want[1])
    s.reset()
    assert s.result()["rows"] == 0 and s.result()["ece"] is None
    for rows, cls, _, _ in batches:                                  # the two-argument form: the same sums, no z
        s.add(dv(rows), dv(cls))
    assert s.acc.cpu().numpy().tobytes() == want[0].tobytes() and not s.zsum.any()
    no_z = s.result()
    assert no_z == summarize(want[0], np.zeros(18)) and no_z["kl"] == summarize(want[0], want[1])["kl"] and no_z["mean_z"] == 0.0


def test_classify_kernel_equals_the_rules(L):
    """The device build of lz_valid_classify (the package itself calls the host build only)."""
    rows, _, _, planes = VC.reduce_batch(257, 11, ("bad", 7, np.nan))
    planes = planes.copy()
    planes[5, 10, 0, 0] = np.nan
    planes[6, 5, 0, 1] = 1.0
    d_rows, d_planes = dv(rows), dv(planes)
    out = torch.full((257 + GUARD, 2), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    st = L.lib().lz_valid_classify(L.ptr(d_planes), C.c_void_p(d_rows.data_ptr() + 4 * VR.V_HAT), L.i64(12), L.i64(257), L.ptr(out),
                                   L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert st == 0 and (got[257:] == 0x7F7F7F7F).all()
    assert np.array_equal(got[:257, 0], VR.phase_of(planes)) and np.array_equal(got[:257, 1], VR.calib_bin(rows[:, VR.V_HAT]))
    assert L.lib().lz_valid_classify(None, None, L.i64(1), L.i64(0), None, None) == 0
    assert L.lib().lz_valid_classify(None, None, L.i64(1), L.i64(3), None, None) == -1
    assert L.lib().lz_valid_classify(L.ptr(d_planes), L.ptr(d_rows), L.i64(0), L.i64(3), L.ptr(out), None) == -1


# =========================================================================================================================
# validate_network
# =========================================================================================================================
EXTRA_KEYS = ("filtered_non_finite_rows", "evaluator")


@pytest.fixture(scope="module")
def data(L):
    from tests.test_gpu_replay_window import _slice
    from tests.test_gpu_symmetry import _dataset
    return _slice(_dataset(), 0, 301)


@pytest.fixture()
def fixed_convolutions(monkeypatch):
    monkeypatch.setenv("LZ_TRAIN_MIOPEN", "immediate")
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _by_hand(forward, batch, bsz, alpha):
    from liuzhou_amd.validation import MetricSums, row_metrics
    s = MetricSums(DEV)
    n = batch.num_samples
    for a in range(0, n, bsz):
        sl = slice(a, min(a + bsz, n))
        planes = batch.state_tensors[sl].float().contiguous()
        lp1, lp2, lpm, vl = forward(planes)[:4]
        rows, cls = row_metrics(lp1, lp2, lpm, vl, planes, batch.legal_masks[sl], batch.policy_targets[sl],
                                batch.value_targets[sl], batch.soft_value_targets[sl], soft_label_alpha=alpha)
        s.add(rows, cls, batch.value_targets[sl])
    return s.result()


def _core(d):
    return {k: v for k, v in d.items() if k not in EXTRA_KEYS}


def test_validate_network_fused_is_its_parts(L, data):
    from liuzhou_amd.net_hip import FusedNet
    from liuzhou_amd.validation import validate_network
    from tests.test_gpu_symmetry import _model
    model = _model().to(DEV).eval()
    got = validate_network(model, data, batch_size=100, evaluator="fused", soft_label_alpha=0.3, device=DEV)
    want = _by_hand(FusedNet(model, DEV), data, 100, 0.3)           # 301 rows: the last batch has one row
    assert _core(got) == want
    assert got["rows"] == 301 and got["evaluator"] == "fused" and got["filtered_non_finite_rows"] == 0
    assert got["skipped_non_finite_rows"] == 0 and sum(c["count"] for c in got["calibration"]) == 301
    assert got["kl"] > 0 and 0 <= got["top1"] <= 1 and got["ece"] >= 0 and sum(g["rows"] for g in got["by_phase"].values()) <= 301
    # a FusedNet is taken as it is; a shape without a kernel is refused with the reason
    assert _core(validate_network(FusedNet(model, DEV), data, batch_size=100, evaluator="fused", soft_label_alpha=0.3,
                                  device=DEV)) == want
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import fused_unsupported_reason
    tiny = ChessNet(**MODEL_CONFIGS["tiny"]).to(DEV)
    with pytest.raises(RuntimeError) as exc:
        validate_network(tiny, data, evaluator="fused", device=DEV)
    assert fused_unsupported_reason(tiny) in str(exc.value)


def test_validate_network_module_is_its_parts_and_leaves_no_trace(L, data, fixed_convolutions):
    from liuzhou_amd.validation import validate_network
    from tests.test_gpu_replay_window import _slice
    from tests.test_gpu_symmetry import _model
    model = _model().to(DEV)
    model.train()                                                    # the flags must come back as they were, one by one:
    model.stem_bn.eval()                                             # a submodule the caller keeps in eval()
    model.policy_head.eval()
    flags = [m.training for m in model.modules()]
    assert True in flags and False in flags
    torch.manual_seed(99)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    cpu_rng, gpu_rng = torch.random.get_rng_state(), torch.cuda.get_rng_state(DEV)
    d300 = _slice(data, 0, 300)
    got = validate_network(model, d300, batch_size=100, evaluator="module", use_amp=False, soft_label_alpha=0.3, device=DEV)
    assert model.training is True and [m.training for m in model.modules()] == flags
    assert torch.equal(torch.random.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(DEV), gpu_rng)
    after = model.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert v.dtype == after[k].dtype and v.cpu().numpy().tobytes() == after[k].cpu().numpy().tobytes(), k
    model.eval()

    def forward(planes):
        with torch.no_grad(), torch.backends.miopen.flags(immediate=True):
            return model(planes)
    assert _core(got) == _by_hand(forward, d300, 100, 0.3)
    assert got["evaluator"] == "module" and got["rows"] == 300
    # autocast on, and a last batch of one row
    amp = validate_network(model, data, batch_size=100, evaluator="module", use_amp=True, soft_label_alpha=0.3, device=DEV)
    assert amp["rows"] == 301 and abs(amp["kl"] - got["kl"]) < 0.05 and model.training is False
    # a seeded subset without replacement
    a = validate_network(model, data, batch_size=64, use_amp=False, device=DEV, max_rows=120, seed=5)
    b = validate_network(model, data, batch_size=64, use_amp=False, device=DEV, max_rows=120, seed=5)
    c = validate_network(model, data, batch_size=64, use_amp=False, device=DEV, max_rows=120, seed=6)
    assert a == b and a["rows"] == 120 and c["rows"] == 120 and _core(a) != _core(c)
    assert torch.equal(torch.random.get_rng_state(), cpu_rng)


def test_validate_network_reads_a_wrapped_ring_and_records(L, data):
    from liuzhou_amd.replay_window import ReplayWindow
    from liuzhou_amd.trajectory_codec import pack_batch
    from liuzhou_amd.validation import validate_network
    from tests.test_gpu_replay_window import _slice
    from tests.test_gpu_symmetry import _model
    model = _model().to(DEV).eval()
    w = ReplayWindow(DEV, max_generations=2, capacity_rows=400)
    w.add_generation(_slice(data, 0, 250), generation=1)
    w.add_generation(data, generation=2)                             # 250 + 301 > 400: generation 1 leaves, 2 wraps the end
    (gid, first, count), = w.generations
    assert (gid, count) == (2, 301) and first + count > 400
    kw = dict(batch_size=128, evaluator="fused", soft_label_alpha=0.3, device=DEV)
    want = validate_network(model, data, **kw)
    assert validate_network(model, (w, [2]), **kw) == want
    assert validate_network(model, pack_batch(data), **kw) == want
    with pytest.raises(KeyError):
        validate_network(model, (w, [1]), **kw)
    # rows with a non-finite target are dropped by the trainer's filter and counted
    from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch
    v = data.value_targets.clone()
    v[[3, 200]] = float("nan")
    bad = TensorSelfPlayBatch(data.state_tensors, data.legal_masks, data.policy_targets, v, data.soft_value_targets)
    r = validate_network(model, bad, **kw)
    assert r["filtered_non_finite_rows"] == 2 and r["rows"] == 299 and r["skipped_non_finite_rows"] == 0


# =========================================================================================================================
# the staged loop
# =========================================================================================================================
_INITIAL = {}


def _initial_model():
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    model = ChessNet(**MODEL_CONFIGS["b6c64"])
    stable_resnet_init(model, 20260314)                              # the loop's own start
    return model.to(DEV).eval()


def _generation_one(games, plies):
    """Generation 1 of player rank 0 as the loop plays it (its seed, its arguments), and its validation by hand on the
    initial weights -- the weights the loop holds before its first training pass.  Played once per shape."""
    key = (games, plies)
    if key not in _INITIAL:
        from liuzhou_amd.distributed import worker_seed
        from liuzhou_amd.net_hip import FusedNet
        from liuzhou_amd.tree_engine import self_play_tree_gpu
        model = _initial_model()
        state = torch.random.get_rng_state()
        torch.manual_seed(worker_seed(1, 0))
        batch, _ = self_play_tree_gpu(FusedNet(model, DEV), num_games=games, mcts_simulations=8, temperature_init=1.0,
                                      temperature_final=0.1, temperature_threshold=10, exploration_weight=1.0, device=DEV,
                                      max_game_plies=plies, concurrent_games=games)
        torch.random.set_rng_state(state)
        _INITIAL[key] = (model, batch)
    return _INITIAL[key]


def _by_hand_generation_one(games, plies, batch_size):
    from liuzhou_amd.validation import validate_network
    model, batch = _generation_one(games, plies)
    want = validate_network(model, batch, batch_size=batch_size, evaluator="fused", soft_label_alpha=0.3, device=DEV)
    return json.loads(json.dumps(want)), batch.num_samples


def test_staged_loop_validates_before_it_trains_window(L):
    """Single process, a window of two generations (the rows are read from the ring), the fp16 kernels as evaluator
    (deterministic across processes): iteration 1's validation is validate_network by hand on the initial weights and
    generation 1's rows.  Later iterations run on trained weights, which a test cannot rebuild by hand."""
    from tests.test_gpu_replay_window import PARENT_ITERATION_KEYS, PARENT_KEYS, _staged_loop
    out = _staged_loop("--validate", "1", "--validate-evaluator", "fused", "--replay-generations", "2")
    its = out["iterations"]
    assert set(out) == PARENT_KEYS and len(its) == 3
    for it in its:
        assert set(it) == PARENT_ITERATION_KEYS | {"replay", "validation"}
        v = it["validation"]
        assert v["evaluator"] == "fused" and v["filtered_non_finite_rows"] == 0
        assert v["rows"] == it["positions"] - it["replay"]["filtered_non_finite_rows"] > 0
    assert its[0]["validation"] != its[1]["validation"]
    want, rows = _by_hand_generation_one(64, 40, 512)
    assert rows == its[0]["positions"] and want == its[0]["validation"]


def test_staged_loop_two_ranks_validate_the_tensors_before_training_and_off_adds_nothing(L):
    """The 2-rank gloo rehearsal (a player and a trainer on one GPU), no window: the trainer validates the gathered
    tensors inside train(), before train_network_from_tensors.  Iteration 1's validation equals the by-hand call on the
    initial weights and the player's generation 1 -- after the pass, or on another model, it would not.  The same run
    with --validate 0 has exactly the parent's keys."""
    from tests.test_gpu_distributed import _staged_loop as multi_rank_loop
    from tests.test_gpu_replay_window import PARENT_ITERATION_KEYS, PARENT_KEYS
    rows = 48 * 6
    out = multi_rank_loop(2, 0, iterations=2, games=48, plies=6, extra=("--validate", "1", "--validate-evaluator", "fused"))
    assert set(out) == PARENT_KEYS
    for it in out["iterations"]:
        assert set(it) == PARENT_ITERATION_KEYS | {"validation"}
        v = it["validation"]
        assert v["evaluator"] == "fused" and v["rows"] == rows == it["positions"] and v["kl"] > 0
        assert sum(c["count"] for c in v["calibration"]) == rows
    want, n = _by_hand_generation_one(48, 6, 128)
    assert n == rows and out["iterations"][0]["validation"] == want
    assert out["iterations"][1]["validation"] != want               # generation 2, on the weights trained on generation 1
    off = multi_rank_loop(2, 0, iterations=2, games=48, plies=6, extra=("--validate", "0"))
    assert set(off) == PARENT_KEYS and all(set(it) == PARENT_ITERATION_KEYS for it in off["iterations"])


def test_staged_loop_lag1_validates_the_lagged_generation(L):
    """Lag-1 schedule, 2 ranks: nothing is trained in iteration 1 (no validation yet); iteration 2 trains on generation 1
    with the weights still at their start, so its validation is the same by-hand dict; the tail trains on the last
    generation and carries its validation.  One run with the default (module) evaluator checks the key and the counts."""
    from tests.test_gpu_distributed import _staged_loop as multi_rank_loop
    from tests.test_gpu_replay_window import PARENT_ITERATION_KEYS
    rows = 48 * 6
    out = multi_rank_loop(2, 1, iterations=2, games=48, plies=6, extra=("--validate", "1", "--validate-evaluator", "fused"))
    its, tail = out["iterations"], out["tail"]
    assert out["overlap"] == 1 and all(set(it) == PARENT_ITERATION_KEYS | {"validation"} for it in its)
    assert its[0]["validation"] is None and its[0]["train_samples"] == 0
    want, n = _by_hand_generation_one(48, 6, 128)
    assert n == rows and its[1]["validation"] == want and its[1]["train_samples"] == rows
    assert tail["validation"]["rows"] == rows and tail["validation"]["evaluator"] == "fused" and tail["validation"] != want
    mod = multi_rank_loop(2, 1, iterations=1, games=48, plies=6, extra=("--validate", "1"))
    assert mod["iterations"][0]["validation"] is None
    assert mod["tail"]["validation"]["evaluator"] == "module" and mod["tail"]["validation"]["rows"] == rows


# =========================================================================================================================
# scripts/validate_checkpoint.py
# =========================================================================================================================
def test_validate_checkpoint_script_reads_a_manifest_and_a_checkpoint(L, tmp_path, capsys):
    import sys
    from liuzhou_amd import self_play_stage as S
    from liuzhou_amd.validation import validate_network
    from tests.stage_stub import random_batch
    from tests.test_gpu_symmetry import _model
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import validate_checkpoint as cli
    batch = random_batch(300, 4)
    manifest = str(tmp_path / "gen.pt")
    S.save_sharded(path=manifest, samples=batch, stats_payload={}, metadata={}, num_shards=3)
    model = _model()
    ckpt = str(tmp_path / "model.pt")
    torch.save({"iteration": 1, "model_state_dict": model.state_dict()}, ckpt)
    args = ["--load_checkpoint", ckpt, "--self_play_input", manifest, "--device", DEV, "--batch_size", "128", "--evaluator", "fused",
            "--soft_label_alpha", "0.3"]
    assert cli.main(args) == 0
    got = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    want = validate_network(model.to(DEV).eval(), batch, batch_size=128, evaluator="fused", soft_label_alpha=0.3, device=DEV)
    assert {k: got[k] for k in want} == json.loads(json.dumps(want))
    assert got["rows_in_input"] == 300 and got["rows"] == 300 and got["checkpoint"] == ckpt and got["self_play_input"] == manifest
    assert cli.main(args + ["--max_rows", "50", "--seed", "3"]) == 0
    assert json.loads(capsys.readouterr().out.splitlines()[-1])["rows"] == 50
