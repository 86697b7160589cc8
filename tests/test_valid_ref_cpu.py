"""CPU: the validation metrics -- the numpy restatement tests/valid_ref.py anchored to the loss restatement and to
liuzhou_amd.net, the host build of the reduction and the classification (libliuzhou_host.so, and a stand-alone program
built with -fsanitize=address,undefined and run as a child process) bit for bit against the restatement, the header
against the ctypes signatures, the result dict, and the staged loop's flags."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from liuzhou_amd import _lib as L
from tests import valid_cases as VC
from tests import valid_ref as VR
from tests.train_loss_ref import ref_loss, value_bins_fp32

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED = 20261020
BAD_VALUES = (np.nan, np.inf, -np.inf)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full():
    c = VC.row_batch(257)
    return c, {a: VR.ref_rows(*(c[k] for k in VC.INPUT_KEYS), c["planes"], alpha=a) for a in VC.ALPHAS}


@pytest.mark.parametrize("alpha", VC.ALPHAS)
def test_kl_and_bucket_ce_are_the_loss_restatements(full, alpha):
    c, want = full
    rows, _ = want[alpha]
    B = len(c["value"])
    r = ref_loss(*(c[k] for k in VC.INPUT_KEYS), alpha=alpha, anti_draw=0.0, draw_weight=1.0, weight_sum=float(B))
    valid = rows[:, VR.POLICY_VALID] == 1
    assert valid.sum() > 200 and (~valid).sum() >= 2
    np.testing.assert_allclose(rows[valid, VR.KL], r["terms"][valid, 0], rtol=1e-12, atol=1e-12)
    assert not rows[~valid, :6].any()
    np.testing.assert_allclose(rows[:, VR.BUCKET_CE], r["terms"][:, 2], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(rows[valid, VR.CE] - rows[valid, VR.H_TARGET], rows[valid, VR.KL], rtol=0, atol=1e-12)


def test_v_hat_and_the_two_hot_target_are_the_networks_own(full):
    from liuzhou_amd.net import bucket_logits_to_scalar, scalar_to_bucket_twohot
    c, want = full
    rows, _ = want[0.3]
    v = bucket_logits_to_scalar(torch.from_numpy(c["vlogits"]).double()).numpy()
    np.testing.assert_allclose(rows[:, VR.V_HAT], v, rtol=0, atol=1e-7)          # linspace centres are float32
    for alpha in VC.ALPHAS:
        _, mixed, _, _, _ = value_bins_fp32(c["value"], c["soft"], alpha, 0.0)
        assert np.array_equal(VR.twohot(c["value"], c["soft"], alpha).astype(np.float32),
                              scalar_to_bucket_twohot(mixed).numpy())
    z = c["value"].astype(np.float64)
    np.testing.assert_allclose(rows[:, VR.SQ_ERR], (rows[:, VR.V_HAT] - z) ** 2, rtol=0, atol=0)
    assert np.array_equal(rows[:, VR.DECISIVE], (np.abs(z) >= 1e-8).astype(np.float64))


def test_hand_built_rows_have_the_expected_classes(full):
    c, want = full
    rows, cls = want[0.0]
    kind = list(c["kind"])
    i = kind.index("none")
    assert cls[i, 2] == -1 and cls[i, 3] == -1 and rows[i, VR.POLICY_VALID] == 0 and not rows[i, :6].any()
    i = kind.index("zero_target")
    assert cls[i, 2] >= 0 and cls[i, 3] == -1 and rows[i, VR.POLICY_VALID] == 0
    for name in ("tie_pp", "tie_ps"):
        i = kind.index(name)
        assert cls[i, 2] == min(c["tie"][i]) and c["mask"][i][list(c["tie"][i])].all()
    i = kind.index("tie_target")
    legal = np.flatnonzero(c["mask"][i])
    assert cls[i, 3] == legal[1] and c["target"][i][legal[1]] == c["target"][i][legal[-1]] == c["target"][i].max()
    i = kind.index("all_neginf")
    assert cls[i, 2] == np.flatnonzero(c["mask"][i])[0] and rows[i, VR.H_NET] == 0 and rows[i, VR.P_TOP] == 0
    i = kind.index("last219")
    assert cls[i, 3] == 219
    i = kind.index("single")
    assert rows[i, VR.TOP1] == 1 and abs(rows[i, VR.P_TOP] - 1) < 1e-12 and abs(rows[i, VR.H_NET]) < 1e-12
    for k in range(10):
        i = kind.index(f"v{k}")
        assert cls[i, 1] == k and abs(rows[i, VR.V_HAT] - (-0.9 + 0.2 * k)) < 0.05
    assert np.array_equal(cls[:, 0], np.arange(257) % 8 - 1)
    assert set(cls[:, 0]) == set(range(-1, 7)) and set(cls[:, 1]) == set(range(10))
    valid = rows[:, VR.POLICY_VALID] == 1
    assert (rows[valid, VR.P_TOP] >= 0).all() and (rows[valid, VR.P_TOP] <= 1 + 1e-12).all()
    assert (rows[:, VR.H_NET] >= -1e-12).all() and (rows[:, VR.H_NET] <= np.log(72) + 1e-9).all()


def test_calibration_bin_and_phase_rules_at_their_edges():
    v = np.array([-1.0, -0.75, np.nextafter(np.float32(-0.75), np.float32(-1)), -0.5, 0.0, -0.0, 0.25, 0.75, 0.8, 1.0, 1.5,
                  -1.5, np.inf, -np.inf, np.nan, 3e38, -3e38, -0.8, 0.2], np.float32)
    # the rule is taken in float32: -0.8f + 1 = 0.19999999, times 5 is below 1
    want = [0, 1, 1, 2, 5, 5, 6, 8, 9, 9, 9, 0, 9, 0, 0, 9, 0, 0, 6]
    got = VR.calib_bin(v)
    assert got.tolist() == want
    finite = np.isfinite(v) & (np.abs(v) < 10)
    rule = np.minimum(9, np.maximum(0, np.floor((v[finite] + np.float32(1)) * np.float32(5)).astype(np.int64)))
    assert got[finite].tolist() == rule.tolist()
    planes = np.zeros((4, 11, 6, 6), np.float32)
    planes[1, 6] = 1
    planes[1, 9] = 1                                            # two phase planes: the lowest
    planes[2, 10, 0, 0] = np.nan                                # NaN is not zero
    planes[3, 5, 0, 1] = 1                                      # not cell 0
    assert VR.phase_of(planes).tolist() == [-1, 2, 6, -1]


# ---- the host build -----------------------------------------------------------------------------------------------------------
def _reduce_modes():
    modes = ["mixed", "one_group", "all_skipped"]
    modes += [("bad", col, BAD_VALUES[col % 3]) for col in range(12)]
    return modes


def _host_reduce(H, batches, with_value=True):
    acc, zsum = np.zeros((18, 14)), np.zeros(18)
    for rows, cls, value, _ in batches:
        st = H.lz_valid_reduce(_p(rows), _p(cls), _p(value) if with_value else None, len(rows), _p(acc),
                               _p(zsum) if with_value else None, None)
        assert st == 0
    return acc, zsum


def _ref_reduce(batches, with_value=True):
    acc, zsum = np.zeros((18, 14)), np.zeros(18)
    for rows, cls, value, _ in batches:
        VR.ref_reduce(rows, cls, value if with_value else None, acc, zsum)
    return acc, zsum


@pytest.mark.parametrize("B", VC.REDUCE_B)
def test_host_reduction_equals_the_restatement_bit_for_bit(B):
    H = L.host_lib()
    for mode in _reduce_modes():
        batch = VC.reduce_batch(B, SEED, mode)
        got, want = _host_reduce(H, [batch]), _ref_reduce([batch])
        assert _bits(got[0], want[0]) and _bits(got[1], want[1]), (B, mode)
        rows, cls = batch[0], batch[1]
        counted = np.isfinite(rows).all(axis=1)
        assert got[0][0, 12] == counted.sum() and got[0][0, 13] == B - counted.sum()
        assert got[0][1:8, 12].sum() == (counted & (cls[:, 0] >= 0)).sum()      # phase -1: group 0 and its bin only
        assert got[0][8:, 12].sum() == counted.sum() and got[0][8:, 13].sum() == B - counted.sum()
        if mode == "all_skipped":
            assert not got[0][:, :13].any() and not got[1].any()
        if mode == "one_group":
            assert _bits(got[0][0], got[0][4]) and _bits(got[0][0], got[0][12]) and got[0][[1, 2, 3, 5, 6, 7]].sum() == 0
    no_z = _host_reduce(H, [VC.reduce_batch(B, SEED)], with_value=False)
    assert _bits(no_z[0], _ref_reduce([VC.reduce_batch(B, SEED)])[0]) and not no_z[1].any()


def test_host_reduction_accumulates_three_batches():
    H = L.host_lib()
    batches = [VC.reduce_batch(130, SEED), VC.reduce_batch(65, SEED + 1, ("bad", 7, np.nan)), VC.reduce_batch(1, SEED + 2)]
    got, want = _host_reduce(H, batches), _ref_reduce(batches)
    assert _bits(got[0], want[0]) and _bits(got[1], want[1])
    assert got[0][0, 12] + got[0][0, 13] == 196
    one = _ref_reduce([tuple(np.concatenate([b[k] for b in batches]) for k in range(4))])
    assert not _bits(one[0], want[0])                             # the association is per call, not per row
    np.testing.assert_allclose(one[0], want[0], rtol=1e-12, atol=1e-9)


def test_host_classification_equals_the_restatement():
    H = L.host_lib()
    rows, cls, _, planes = VC.reduce_batch(130, SEED, ("bad", 7, np.nan))
    planes = planes.copy()
    planes[5, 10, 0, 0] = np.nan
    out = np.full((130, 2), -7, np.int32)
    assert H.lz_valid_classify(_p(planes), _p(rows[:, 7:]), 12, 130, _p(out), None) == 0
    assert np.array_equal(out[:, 0], VR.phase_of(planes)) and np.array_equal(out[:, 1], VR.calib_bin(rows[:, 7]))
    v = np.ascontiguousarray(rows[:, 7])
    assert H.lz_valid_classify(_p(planes), _p(v), 1, 130, _p(out), None) == 0
    assert np.array_equal(out[:, 1], cls[:, 1])


def test_abi_conventions_and_signatures():
    H = L.host_lib()
    assert H.lz_valid_reduce(None, None, None, 0, None, None, None) == 0
    assert H.lz_valid_reduce(None, None, None, 4, None, None, None) == -1
    assert H.lz_valid_reduce(None, None, None, -1, None, None, None) == -1
    rows, cls, value, planes = VC.reduce_batch(4, SEED)
    acc, zsum = np.zeros((18, 14)), np.zeros(18)
    assert H.lz_valid_reduce(_p(rows), _p(cls), _p(value), 4, _p(acc), None, None) == -1      # value and zsum: both or neither
    assert H.lz_valid_reduce(_p(rows), _p(cls), None, 4, _p(acc), _p(zsum), None) == -1
    assert not acc.any()
    assert H.lz_valid_classify(None, None, 1, 0, None, None) == 0
    assert H.lz_valid_classify(None, None, 1, 3, None, None) == -1
    assert H.lz_valid_classify(_p(planes), _p(rows), 0, 4, _p(np.zeros((4, 2), np.int32)), None) == -1
    # header against ctypes: scalars by exact width, every pointer a void pointer
    want = {"lz_valid_row_metrics": [C.c_void_p] * 9 + ["i64", "f32"] + [C.c_void_p] * 3,
            "lz_valid_reduce": [C.c_void_p] * 3 + ["i64"] + [C.c_void_p] * 3,
            "lz_valid_classify": [C.c_void_p] * 2 + ["i64", "i64"] + [C.c_void_p] * 2}
    for name, sig in want.items():
        restype, argtypes = L.DECLS[name]
        assert restype is C.c_int and len(argtypes) == len(sig), name
        for got, w in zip(argtypes, sig):
            if w is C.c_void_p:
                assert got is C.c_void_p, name
            else:
                assert issubclass(got, C.c_int64 if w == "i64" else C.c_float), name
    assert "lz_valid_reduce" in L.HOST_SYMBOLS and "lz_valid_classify" in L.HOST_SYMBOLS
    assert "lz_valid_row_metrics" in L.SYMBOLS and "lz_valid_row_metrics" not in L.HOST_SYMBOLS      # HIP only
    for name in ("lz_valid_reduce", "lz_valid_classify"):
        assert getattr(H, name).argtypes == L.DECLS[name][1]
    from liuzhou_amd.build import HOST_SOURCES, SOURCES
    assert "lz_valid.hip" in SOURCES and any(s.endswith("lz_valid_host.cpp") for s in HOST_SOURCES)


def test_sanitizer_build_of_the_host_code_agrees(tmp_path):
    """Host code only, in a program of its own: nothing is loaded into this interpreter."""
    exe = str(tmp_path / "valid_host_check")
    # the sanitizer runtimes are linked into the program itself: it starts whatever else the environment preloads
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(HERE, "valid_host_check.cpp"),
                           os.path.join(ROOT, "liuzhou_amd", "csrc", "lz_valid_host.cpp")])
    batches = [VC.reduce_batch(B, SEED, m) for B, m in
               ((1, "mixed"), (63, ("bad", 3, np.inf)), (64, "all_skipped"), (65, "one_group"), (130, ("bad", 7, np.nan)))]
    rng = np.random.default_rng(SEED)
    args = []
    for k in range(12):
        x = rng.standard_normal(220).astype(np.float32)
        legal = (rng.random(220) < 0.2).astype(np.uint8)
        if k == 0:
            legal[:] = 0
        if k == 1:
            x[:] = np.nan
        if k == 2:
            x[legal != 0] = -np.inf
        if k == 3:
            idx = np.flatnonzero(legal)
            x[idx[2]] = x[idx[-1]] = 9.0
        args.append((x, legal))
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("<q", len(batches)))
        for rows, cls, value, planes in batches:
            f.write(struct.pack("<qq", len(rows), 1))
            for a in (rows, cls, value, planes):
                f.write(np.ascontiguousarray(a).tobytes())
        f.write(struct.pack("<q", len(args)))
        for x, legal in args:
            f.write(x.tobytes() + legal.tobytes())
    run = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    raw = open(tmp_path / "out.bin", "rb").read()
    acc, zsum = np.frombuffer(raw, np.float64, 252).reshape(18, 14), np.frombuffer(raw, np.float64, 18, 252 * 8)
    want = _ref_reduce(batches)
    assert _bits(acc, want[0]) and _bits(zsum, want[1])
    off = 270 * 8
    for rows, cls, value, planes in batches:
        pb = np.frombuffer(raw, np.int32, 2 * len(rows), off).reshape(-1, 2)
        off += pb.nbytes
        assert np.array_equal(pb[:, 0], VR.phase_of(planes)) and np.array_equal(pb[:, 1], VR.calib_bin(rows[:, 7]))
    got = np.frombuffer(raw, np.int32, len(args), off)
    assert got.tolist() == [VR.argmax_legal(x, legal) for x, legal in args]
    assert got[0] == -1 and got[3] == np.flatnonzero(args[3][1])[2]


# ---- the result dict ------------------------------------------------------------------------------------------------------------
def test_summarize_divides_by_the_documented_counts():
    from liuzhou_amd import validation as V
    acc, zsum = np.zeros((18, 14)), np.zeros(18)
    acc[0] = [6, 8, 2, 3, 2, 1.5, 10, 1.0, 4, 3, 4, 2, 5, 1]             # 5 rows, 2 with a policy, 4 decisive, 1 skipped
    zsum[0] = 2.0
    acc[1 + 2] = acc[0]
    zsum[3] = 2.0
    acc[8 + 5], zsum[13] = [0] * 7 + [0.3, 0, 0, 0, 0, 3, 0], 1.5         # bin 5: mean v_hat 0.1, mean z 0.5
    acc[8 + 9], zsum[17] = [0] * 7 + [1.8, 0, 0, 0, 0, 2, 1], 2.0         # bin 9: 0.9 / 1.0
    r = V.summarize(acc, zsum)
    assert (r["rows"], r["skipped_non_finite_rows"], r["policy_rows"], r["decisive_rows"]) == (5, 1, 2, 4)
    assert (r["kl"], r["ce"], r["top1"], r["p_top"]) == (3.0, 4.0, 1.0, 0.75)
    assert (r["bucket_ce"], r["v_hat"], r["sq_err"], r["sign_ok"], r["mean_z"]) == (2.0, 0.2, 0.8, 0.75, 0.4)
    assert r["by_phase"]["2"]["kl"] == 3.0 and r["by_phase"]["0"]["rows"] == 0 and r["by_phase"]["0"]["kl"] is None
    assert len(r["calibration"]) == 10 and r["calibration"][5]["count"] == 3 and r["calibration"][0]["mean_z"] is None
    assert abs(r["ece"] - (3 / 5 * 0.4 + 2 / 5 * 0.1)) < 1e-12
    empty = V.summarize(np.zeros((18, 14)), np.zeros(18))
    assert empty["rows"] == 0 and empty["ece"] is None and empty["kl"] is None
    assert V.ROW_COLUMNS[VR.V_HAT] == "v_hat" and len(V.ROW_COLUMNS) == VR.ROW_COLS


def test_refusals_on_the_cpu():
    from liuzhou_amd import validation as V
    from tests.stage_stub import random_batch
    x = torch.zeros(2, 36)
    with pytest.raises(RuntimeError, match="HIP device"):
        V.row_metrics(x, x, x, torch.zeros(2, 101), torch.zeros(2, 11, 6, 6), torch.zeros(2, 220, dtype=torch.bool),
                      torch.zeros(2, 220), torch.zeros(2), torch.zeros(2))
    with pytest.raises(RuntimeError, match="HIP device"):
        V.validate_network(None, random_batch(4, 1), device="cpu")
    for kw in ({"evaluator": "eager"}, {"batch_size": 0}, {"max_rows": -1}, {"batch_size": 2.5}):
        with pytest.raises(ValueError):
            V.validate_network(None, random_batch(4, 1), **kw)


# ---- the loop's command line ---------------------------------------------------------------------------------------------------
def _loop_cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import staged_loop as cli
    return cli


def test_staged_loop_flags_parse_and_refuse_before_anything_runs():
    cli = _loop_cli()
    a = cli.parse_args([])
    assert a.validate == 0 and a.validate_evaluator is None
    a = cli.parse_args(["--validate", "1"])
    assert a.validate == 1 and a.validate_evaluator is None
    a = cli.parse_args(["--validate", "1", "--validate-evaluator", "fused", "--replay-generations", "3", "--overlap", "1"])
    assert a.validate == 1 and a.validate_evaluator == "fused"
    for bad in (["--validate", "2"], ["--validate-evaluator", "module"], ["--validate", "0", "--validate-evaluator", "fused"],
                ["--validate", "1", "--validate-evaluator", "eager"],
                ["--validate", "1", "--replay-generations", "2", "--dedup-positions", "exact"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    # parse_args needs no process group: every rank refuses before any collective
    text = open(os.path.join(ROOT, "scripts", "staged_loop.py")).read()
    assert text.index("args = parse_args(argv)") < text.index("init_process_group")
    assert text.count("liuzhou_amd.validation") == 1 and "from liuzhou_amd.validation import validate_network" in \
        text[text.index("def validate("):text.index("def train_window(")]       # imported only inside the call


def test_log_entry_gains_a_key_only_when_on():
    cli = _loop_cli()
    base = {"iteration": 1, "positions": 10, "net_check": None}
    assert cli.iteration_entry(base) == base
    assert cli.iteration_entry(base, validation={"kl": 1.0}, validate_on=False) == base
    assert list(cli.iteration_entry(base, replay={"x": 1}, window_on=True)) == list(base) + ["replay"]
    on = cli.iteration_entry(base, validation={"kl": 1.0}, validate_on=True)
    assert list(on) == list(base) + ["validation"] and on["validation"] == {"kl": 1.0}
    both = cli.iteration_entry(base, replay=None, window_on=True, validation=None, validate_on=True)
    assert list(both) == list(base) + ["replay", "validation"]


def test_validate_checkpoint_flags_parse():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import validate_checkpoint as cli
    a = cli.parse(["--self_play_input", "x.json"])
    assert (a.load_checkpoint, a.model, a.device, a.batch_size, a.evaluator, a.use_amp, a.soft_label_alpha, a.max_rows, a.seed) == \
        (None, "b10c128", "cuda:0", 4096, "module", 1, 0.0, 0, 0)
    a = cli.parse(["--self_play_input", "x", "--load_checkpoint", "c.pt", "--evaluator", "fused", "--use_amp", "0", "--max_rows", "9"])
    assert a.load_checkpoint == "c.pt" and a.evaluator == "fused" and a.use_amp == 0 and a.max_rows == 9
    for bad in ([], ["--self_play_input", "x", "--evaluator", "eager"], ["--self_play_input", "x", "--use_amp", "2"],
                ["--self_play_input", "x", "--model", "tiny"]):
        with pytest.raises(SystemExit):
            cli.parse(bad)
    with pytest.raises(FileNotFoundError):                           # the reader's own refusal, before any device work
        cli.main(["--self_play_input", os.path.join(ROOT, "no_such_payload.pt"), "--device", "cpu"])
