"""CPU: per-row sample weights -- the float64 restatement of the weighted loss anchored on repeated
rows, the normalisation rule, the age weights of a replay window from hand-built generation tables, the weights of
merged groups through the host build, every refusal of the trainers (all raised before any device work) and the three
command-line flags."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from liuzhou_amd import position_dedup as D
from liuzhou_amd import replay_window as RW
from liuzhou_amd import row_weights as W
from tests import row_weights_ref as R
from tests import train_loss_cases as K
from tests.train_loss_ref import ref_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement, anchored on repeated rows ------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (K.EDGE_B, 1, 4, 5, 257))
def test_integer_weights_equal_repeated_rows(B):
    """ref_loss on the batch with row i repeated k_i times, same weight_sum: the policy gradients of the copies sum to the
    weighted restatement's row; the value gradients (divided by the repeated batch's row count) after sum(k) / B."""
    c = K.edge_batch(B)
    counts = np.array([(1, 2, 3, 5)[i % 4] for i in np.random.default_rng(B).permutation(B)])
    rep, owner = R.repeat_rows(c, counts)
    total = int(counts.sum())
    assert len(owner) == total and (B == 1 or total > B)
    for setting in (K.SETTINGS if B == K.EDGE_B else K.SETTINGS[1:2]):
        ws = K.weight_sum_of(c["value"], setting[2])
        gs = 3.0
        want = R.ref_loss_weighted(c, counts.astype(np.float32), setting, ws, gs)
        got = ref_loss(*(rep[k] for k in K.INPUT_KEYS), alpha=setting[0], anti_draw=setting[1], draw_weight=setting[2],
                       weight_sum=ws, grad_scale=gs)
        for name, factor in (("g1", 1.0), ("g2", 1.0), ("g3", 1.0), ("gv", total / B)):
            summed = np.zeros_like(want[name])
            np.add.at(summed, owner, got[name])
            np.testing.assert_allclose(summed * factor, want[name], rtol=1e-12, atol=0, err_msg=f"{name} {setting}")
        first = np.concatenate([[0], np.cumsum(counts)[:-1]])
        for col in (0, 2, 3):                             # kl, bucket CE and aux do not depend on the weight
            assert np.array_equal(got["terms"][first, col], want["terms"][:, col])
        plain = ref_loss(*(c[k] for k in K.INPUT_KEYS), alpha=setting[0], anti_draw=setting[1], draw_weight=setting[2],
                         weight_sum=ws, grad_scale=gs)
        assert np.array_equal(want["terms"][:, 1], (plain["terms"][:, 1].astype(np.float32) *
                                                    counts.astype(np.float32)).astype(np.float64))


def test_weights_of_one_are_the_unweighted_restatement():
    c = K.edge_batch(9)
    setting = K.SETTINGS[1]
    ws = K.weight_sum_of(c["value"], setting[2])
    a = R.ref_loss_weighted(c, np.ones(9, np.float32), setting, ws)
    b = ref_loss(*(c[k] for k in K.INPUT_KEYS), alpha=setting[0], anti_draw=setting[1], draw_weight=setting[2], weight_sum=ws)
    for name in ("terms", "g1", "g2", "g3", "gv"):
        assert np.array_equal(a[name], b[name]), name


# ---- normalisation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", (3.0, 0.1))
@pytest.mark.parametrize("n", (1, 7, 512, 100003))
def test_uniform_weights_become_exactly_one(value, n):
    w, info = W.normalise_row_weights(torch.full((n,), value, dtype=torch.float32))
    assert w.dtype == torch.float32 and w.shape == (n,) and bool((w == 1.0).all())
    assert info == {"source": "row_weights", "min": float(np.float32(value)), "max": float(np.float32(value)),
                    "zero_weight_rows": 0}
    assert np.array_equal(R.ref_normalise(np.full(n, value, np.float32)), np.ones(n, np.float32))


def test_normalised_weights_have_mean_one_and_keep_their_zeros():
    rng = np.random.default_rng(11)
    raw = (rng.random(1000) * 5).astype(np.float32)
    raw[::7] = 0.0
    for src in (torch.from_numpy(raw), torch.from_numpy(raw.astype(np.float64)), torch.from_numpy(raw).half().float()):
        w, info = W.normalise_row_weights(src, source="x")
        assert w.dtype == torch.float32
        got = w.numpy()
        assert abs(float(got.astype(np.float64).mean()) - 1.0) <= 2.0 ** -23           # float32 rounding of each entry
        assert np.array_equal(got == 0, src.numpy() == 0) and info["zero_weight_rows"] == int((raw == 0).sum())
        assert info["source"] == "x" and info["min"] == 0.0 and info["max"] == float(src.max())
        np.testing.assert_allclose(got, R.ref_normalise(src.numpy()), rtol=2.0 ** -23, atol=0)
    ints, _ = W.normalise_row_weights(torch.tensor([1, 3, 0, 4]))                       # counts are welcome
    assert ints.tolist() == [0.5, 1.5, 0.0, 2.0]
    arr, _ = W.normalise_row_weights(np.array([2.0, 6.0]))
    assert arr.tolist() == [0.5, 1.5]


@pytest.mark.parametrize("bad", ([1.0, -0.5], [1.0, float("nan")], [float("inf"), 1.0], [1.0, -float("inf")], [0.0, 0.0],
                                 [-0.0], []))
def test_bad_weights_raise(bad):
    with pytest.raises(ValueError, match="row_weights"):
        W.normalise_row_weights(torch.tensor(bad, dtype=torch.float32))
    with pytest.raises(ValueError):
        R.ref_normalise(bad)


def test_weights_must_be_one_real_number_per_row():
    for bad in (torch.ones(2, 2), torch.ones(()), torch.ones(3, dtype=torch.bool)):
        with pytest.raises(ValueError):
            W.normalise_row_weights(bad)


# ---- age weights -------------------------------------------------------------------------------------------------------------
def _wrapped_table():
    """Three generations in a ring of 12: ids 1, 2, 3 with 4, 5 and 1 rows; generation 2 wraps the end of the ring."""
    t = RW.GenerationTable(3, 12)
    for count in (5, 4, 5, 1):
        t.add(count)
    assert t.entries == [(1, 5, 4), (2, 9, 5), (3, 2, 1)]
    return t


def _one_generation():
    t = RW.GenerationTable(3, 12)
    t.add(7, generation=4)
    return t


def _three_even():
    t = RW.GenerationTable(4, 64)
    for count in (10, 20, 6):
        t.add(count)
    return t


@pytest.mark.parametrize("make, budget", ((_wrapped_table, 3), (_wrapped_table, 0), (_wrapped_table, 100), (_one_generation, 0),
                                          (_one_generation, 5), (_three_even, 0), (_three_even, 4), (_three_even, 15)))
def test_ages_of_the_selected_slots(make, budget):
    t = make()
    plain = RW.select_slots(t, budget, 9, "cpu")
    slots, ages = RW.select_slots(t, budget, 9, "cpu", return_ages=True)
    assert torch.equal(plain, slots) and ages.dtype == torch.int64 and ages.shape == slots.shape
    want = R.ref_ages(t.entries, budget)
    assert ages.tolist() == [a for a, take in want for _ in range(take)]
    by_slot = {}
    for age, (gid, first, count) in enumerate(reversed(t.entries)):
        for r in range(count):
            by_slot[(first + r) % t.capacity_rows] = age
    assert [by_slot[int(s)] for s in slots] == ages.tolist()      # the age of the generation that owns the slot
    for decay in (0.5, 0.9, 1.0):
        raw = W.age_weights(ages, decay)
        assert raw.dtype == torch.float64
        np.testing.assert_allclose(raw.numpy(), R.ref_age_weights(t.entries, budget, decay), rtol=4e-16, atol=0)
        w, info = W.normalise_row_weights(raw, source="replay_age_decay")
        np.testing.assert_allclose(w.numpy(), R.ref_normalise(R.ref_age_weights(t.entries, budget, decay)), rtol=2.0 ** -23)
        assert info["max"] == 1.0 and info["min"] == decay ** max(a for a, _ in want) and info["zero_weight_rows"] == 0
        if decay == 1.0 or len(want) == 1:
            assert bool((w == 1.0).all())


def test_a_budget_of_zero_rows_leaves_the_newest_generation_alone():
    t = _wrapped_table()                                          # newest has 1 row, two older ones: 1 // 2 = 0 rows each
    slots, ages = RW.select_slots(t, 0, 0, "cpu", return_ages=True)
    assert slots.tolist() == [2] and ages.tolist() == [0]
    slots, ages = RW.select_slots(t, 3, 0, "cpu", return_ages=True)
    assert ages.tolist() == [0, 1, 1, 1, 2, 2, 2]
    assert set(slots[1:4].tolist()) <= {9, 10, 11, 0, 1} and set(slots[4:].tolist()) <= {5, 6, 7, 8}
    w, _ = W.normalise_row_weights(W.age_weights(ages, 0.5))
    c = 7 / (1 + 3 * 0.5 + 3 * 0.25)
    np.testing.assert_allclose(w.numpy(), [c] + [c / 2] * 3 + [c / 4] * 3, rtol=2.0 ** -23)
    empty = RW.select_slots(RW.GenerationTable(2, 8), 3, 0, "cpu", return_ages=True)
    assert empty[0].numel() == 0 and empty[1].numel() == 0 and empty[1].dtype == torch.int64


@pytest.mark.parametrize("bad", (0, 0.0, -0.5, 1.5, 2, float("nan"), float("inf"), True, False, None, "0.5"))
def test_bad_age_decay_is_refused(bad):
    from liuzhou_amd.train_bridge import train_network_from_window
    with pytest.raises(ValueError, match="replay_age_decay"):
        W.check_age_decay(bad)
    with pytest.raises(ValueError, match="replay_age_decay"):
        train_network_from_window(None, None, replay_age_decay=bad)
    assert W.check_age_decay(1) == 1.0 and W.check_age_decay(0.25) == 0.25


# ---- weights of merged groups (host build) -----------------------------------------------------------------------------------
def _distinct_rows(n, seed):
    """n rows with pairwise different positions (another cell of plane 0 each) and random targets, CPU tensors."""
    assert n <= 36
    rng = np.random.default_rng(seed)
    planes = np.zeros((n, 11, 6, 6), np.float32)
    planes[:, 4] = 1.0
    masks = np.zeros((n, 220), np.uint8)
    masks[:, 216] = 1
    for i in range(n):
        planes[i, 0, i // 6, i % 6] = 1.0
        masks[i, i] = 1
    policy = (rng.random((n, 220)) * masks).astype(np.float32)
    policy /= policy.sum(axis=1, keepdims=True, dtype=np.float32)
    return [torch.from_numpy(a) for a in (planes, masks, policy, rng.integers(-1, 2, n).astype(np.float32),
                                          rng.uniform(-1, 1, n).astype(np.float32))]


def _stack(*parts):
    return [torch.cat(cols) for cols in zip(*parts)]


def test_merged_groups_weigh_their_capped_count():
    x, y = _distinct_rows(36, 1), _distinct_rows(36, 2)
    x, y = [t[:20] for t in x], [t[20:33] for t in y]             # 20 + 13 different positions
    rows = _stack(x, x, y)
    outs, info = D.merge_duplicate_positions(*rows, mode="exact", max_copies=4, weighting="weight")
    assert info["groups"] == 33 and info["rows_out"] == 33 and info["rows_in"] == 53 and info["weighting"] == "weight"
    assert info["max_copies"] == 4 and outs[0].shape[0] == 33
    assert info["weights"].dtype == torch.float64 and info["weights"].tolist() == [2.0] * 20 + [1.0] * 13
    assert torch.equal(info["weights"], D.group_weights(info["count"], 4))
    assert D.stats_of(info)["weighting"] == "weight" and list(D.stats_of(info))[-1] == "weighting"
    copies, info_c = D.merge_duplicate_positions(*rows, mode="exact", max_copies=4)
    assert "weighting" not in info_c and "weights" not in info_c and "weighting" not in D.stats_of(info_c)
    assert info_c["rows_out"] == 53 and copies[0].shape[0] == 53
    once, info_1 = D.merge_duplicate_positions(*rows, mode="exact", max_copies=1)
    for a, b in zip(outs, once):                                  # the rows of "weight" are those of one copy each
        assert torch.equal(a.view(torch.uint8) if a.dtype != torch.bool else a, b.view(torch.uint8) if b.dtype != torch.bool else b)
    # max_copies caps the weight
    _, info = D.merge_duplicate_positions(*_stack(x, x, x, y), mode="exact", max_copies=2, weighting="weight")
    assert info["weights"].tolist() == [2.0] * 20 + [1.0] * 13 and info["largest_group"] == 3
    _, info = D.merge_duplicate_positions(*_stack(x, x, x, y), mode="exact", max_copies=1, weighting="weight")
    assert info["weights"].tolist() == [1.0] * 33
    _, info = D.merge_duplicate_positions(*_stack(x, x, x, y), mode="exact", max_copies=7, weighting="weight")
    assert info["weights"].tolist() == [3.0] * 20 + [1.0] * 13
    w, meta = W.normalise_row_weights(info["weights"], source="dedup_weighting")
    np.testing.assert_allclose(w.numpy(), np.array([3.0] * 20 + [1.0] * 13) * 33 / 73, rtol=2.0 ** -23)
    assert meta == {"source": "dedup_weighting", "min": 1.0, "max": 3.0, "zero_weight_rows": 0}
    assert D.group_weights(torch.tensor([1, 5, 2], dtype=torch.int32), 3).tolist() == [1.0, 3.0, 2.0]
    for bad in (0, True, 1.5):
        with pytest.raises(ValueError, match="dedup_max_copies"):
            D.group_weights(torch.tensor([1]), bad)


def test_dedup_weighting_is_validated_on_and_off():
    assert D.WEIGHTINGS == ("copies", "weight")
    assert D.weighting_on("copies") is False and D.weighting_on("copies", "exact", 3) is False
    assert D.weighting_on("weight", "exact", 1) is True and D.weighting_on("weight", "symmetric", 4) is True
    for mode in ("off", "exact"):
        for bad in ("weights", "", None, 1, "Weight", True):
            with pytest.raises(ValueError, match="dedup_weighting"):
                D.weighting_on(bad, mode, 2)
    with pytest.raises(ValueError, match="dedup_weighting='weight' needs dedup_positions"):
        D.weighting_on("weight", "off", 4)
    x = _distinct_rows(4, 3)
    with pytest.raises(ValueError, match="dedup_weighting"):
        D.merge_duplicate_positions(*x, mode="exact", weighting="mean")


# ---- the trainers' keywords: every refusal before any device work ----------------------------------------------------------
def test_tensor_trainer_refusals_come_before_any_device_work():
    from liuzhou_amd.train_bridge import train_network_from_tensors
    from tests.stage_stub import random_batch
    batch = random_batch(8, 1)
    for mode in ("off", "exact"):
        for bad in ("weights", None, 1, ""):
            with pytest.raises(ValueError, match="dedup_weighting"):
                train_network_from_tensors(None, batch, dedup_positions=mode, dedup_weighting=bad)
    with pytest.raises(ValueError, match="dedup_weighting='weight' needs dedup_positions"):
        train_network_from_tensors(None, batch, dedup_weighting="weight")
    with pytest.raises(ValueError, match="dedup_weighting='weight' needs dedup_positions"):
        train_network_from_tensors(None, batch, dedup_weighting="weight", dedup_max_copies=4)
    for kw in ({"policy_draw_weight": 0.5}, {"anti_draw_penalty": 0.1}):          # the existing refusals stay
        with pytest.raises(ValueError, match="drawn game"):
            train_network_from_tensors(None, batch, dedup_positions="exact", dedup_weighting="weight", **kw)
    with pytest.raises(ValueError, match="dedup_max_copies"):
        train_network_from_tensors(None, batch, dedup_positions="exact", dedup_weighting="weight", dedup_max_copies=0)
    ones = torch.ones(8)
    for mode in ("exact", "symmetric"):
        with pytest.raises(ValueError, match="row_weights cannot be combined with dedup_positions"):
            train_network_from_tensors(None, batch, dedup_positions=mode, row_weights=ones)
    for bad in (torch.ones(7), torch.ones(9), np.ones(3), torch.ones(8, 1), torch.ones(())):
        with pytest.raises(ValueError, match=r"one weight per sample, \[8\]"):
            train_network_from_tensors(None, batch, row_weights=bad)
    # what is valid gets as far as the device check: there is no CPU path
    for kw in ({"row_weights": ones}, {"row_weights": np.ones(8)}, {"dedup_positions": "exact", "dedup_weighting": "weight"},
               {"dedup_weighting": "copies"}):
        with pytest.raises(RuntimeError, match="HIP device"):
            train_network_from_tensors(None, batch, device="cpu", **kw)


def test_keywords_and_their_defaults():
    from liuzhou_amd import train_bridge as TB
    from liuzhou_amd.train_loss import fused_policy_value_loss
    from tests.stage_stub import random_batch
    # the two trainers take the row-weight keywords through `**weighting`: each knows its own and no other
    t = inspect.signature(TB.train_network_from_tensors).parameters
    w = inspect.signature(TB.train_network_from_window).parameters
    assert t["weighting"].kind == w["weighting"].kind == inspect.Parameter.VAR_KEYWORD
    batch = random_batch(4, 1)
    for kw in ({"dedup_weighting": "copies"}, {"row_weights": None}, {"dedup_weighting": "copies", "row_weights": None}):
        with pytest.raises(RuntimeError, match="HIP device"):                   # the defaults, spelled out: accepted
            TB.train_network_from_tensors(None, batch, device="cpu", **kw)
    for kw in ({"replay_age_decay": 0.5}, {"row_weight": None}, {"dedup_weights": "copies"}):
        with pytest.raises(TypeError, match=r"train_network_from_tensors\(\) got an unexpected keyword argument"):
            TB.train_network_from_tensors(None, batch, **kw)
    for kw in ({"row_weights": None}, {"dedup_weighting": "copies"}, {"replay_decay": 0.5}):
        with pytest.raises(TypeError, match=r"train_network_from_window\(\) got an unexpected keyword argument"):
            TB.train_network_from_window(None, None, **kw)

    class Empty:
        num_rows = 0
    for kw in ({}, {"replay_age_decay": 1.0}, {"replay_age_decay": 1}, {"replay_age_decay": 0.5}):
        assert TB.train_network_from_window(None, Empty(), **kw)[1] == {"epoch_stats": [], "num_samples": 0}
    s = inspect.signature(TB.train_network_streaming).parameters               # its batches carry no weights
    assert not [k for k in s if "weight" in k and k not in ("weight_decay", "policy_draw_weight")]
    assert "replay_age_decay" not in s and not [k for k in s.values() if k.kind == inspect.Parameter.VAR_KEYWORD]
    step = inspect.signature(TB._Stepper.step).parameters
    assert list(step) == ["self", "b_states", "b_masks", "b_policy", "b_values", "b_soft", "b_weights"]
    assert step["b_weights"].default is None
    f = inspect.signature(fused_policy_value_loss).parameters["row_weights"]
    assert f.default is None and f.kind == inspect.Parameter.KEYWORD_ONLY
    sel = inspect.signature(RW.select_slots).parameters["return_ages"]
    assert sel.default is False and inspect.signature(RW.ReplayWindow.select).parameters["return_ages"].default is False


def test_the_defaults_import_nothing_new():
    import subprocess
    code = ("import sys; from liuzhou_amd.train_bridge import train_network_from_tensors as t, train_network_from_window as w\n"
            "from liuzhou_amd.trajectory_buffer import TensorSelfPlayBatch as B\nimport torch\n"
            "e = B(torch.zeros(0, 11, 6, 6), torch.zeros(0, 220, dtype=torch.bool), torch.zeros(0, 220), torch.zeros(0), "
            "torch.zeros(0))\n"
            "class Win: num_rows = 0\n"
            "assert t(None, e)[1]['num_samples'] == 0 and w(None, Win())[1]['num_samples'] == 0\n"
            "assert w(None, Win(), replay_age_decay=1.0)[1]['num_samples'] == 0\n"
            "assert 'liuzhou_amd.row_weights' not in sys.modules and 'liuzhou_amd.position_dedup' not in sys.modules\n"
            "assert w(None, Win(), replay_age_decay=0.5)[1]['num_samples'] == 0\n"
            "assert 'liuzhou_amd.row_weights' in sys.modules\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr


def test_loss_wrapper_refuses_cpu_tensors_with_weights():
    from liuzhou_amd.train_loss import fused_policy_value_loss
    x = torch.zeros(2, 36)
    with pytest.raises(RuntimeError, match="HIP device"):
        fused_policy_value_loss(x, x, x, torch.zeros(2, 101), torch.zeros(2, 220, dtype=torch.bool), torch.zeros(2, 220),
                                torch.zeros(2), torch.zeros(2), row_weights=torch.ones(2))


# ---- command line ------------------------------------------------------------------------------------------------------------
def _cli(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    return __import__(name)


def test_train_stage_dedup_weighting_flag(monkeypatch, tmp_path, capsys):
    cli = _cli("train_stage")
    a = cli.parse(["--self_play_input", "x"])
    assert a.dedup_weighting == "copies"
    for spelling in ("--dedup_weighting", "--dedup-weighting"):
        a = cli.parse(["--self_play_input", "x", "--dedup_positions", "exact", spelling, "weight"])
        assert a.dedup_weighting == "weight" and a.ignored == []
    with pytest.raises(SystemExit):
        cli.parse(["--self_play_input", "x", "--dedup_weighting", "mean"])
    assert "invalid choice: 'mean' (choose from 'copies', 'weight')" in capsys.readouterr().err

    import liuzhou_amd.self_play_stage as S
    import liuzhou_amd.streaming as ST
    import liuzhou_amd.train_bridge as TB
    from tests.stage_stub import random_batch
    seen = {}

    def train(model, samples, **kw):
        seen.clear()
        seen.update(kw)
        return model, {"epoch_stats": [{"samples": 1}]}

    monkeypatch.setattr(TB, "train_network_from_tensors", train)
    monkeypatch.setattr(TB, "train_network_streaming", lambda model, loader, **kw: train(model, None, streaming=True, **kw))
    monkeypatch.setattr(S, "load_self_play_payload", lambda p, **kw: (random_batch(4, 1), {}))
    monkeypatch.setattr(S, "concat_batches", lambda batches: batches[0])
    monkeypatch.setattr(S, "resolve_shard_specs", lambda *a, **kw: ([], 4))
    monkeypatch.setattr(ST, "build_streaming_dataloader", lambda *a, **kw: [])
    base = ["--model", "b6c64", "--self_play_input", "x.pt", "--checkpoint_dir", str(tmp_path), "--device", "cpu"]
    assert cli.main(base) == 0 and "dedup_weighting" not in seen
    assert cli.main(base + ["--dedup_positions", "exact", "--dedup_max_copies", "4"]) == 0 and "dedup_weighting" not in seen
    assert cli.main(base + ["--dedup_positions", "exact", "--dedup_weighting", "copies"]) == 0 and "dedup_weighting" not in seen
    assert cli.main(base + ["--dedup_positions", "symmetric", "--dedup_max_copies", "4", "--dedup_weighting", "weight"]) == 0
    assert seen["dedup_weighting"] == "weight" and seen["dedup_positions"] == "symmetric" and seen["dedup_max_copies"] == 4
    with pytest.raises(SystemExit, match="--dedup_weighting weight needs --dedup_positions exact or symmetric"):
        cli.main(base + ["--dedup_weighting", "weight"])
    with pytest.raises(SystemExit, match="one batch at a time"):                  # the streaming trainer stays refused
        cli.main(base + ["--streaming_load", "1", "--dedup_positions", "exact", "--dedup_weighting", "weight"])


def test_staged_loop_flags(capsys):
    cli = _cli("staged_loop")
    a = cli.parse_args([])
    assert a.dedup_weighting == "copies" and a.replay_age_decay == 1.0
    a = cli.parse_args(["--dedup-positions", "exact", "--dedup-max-copies", "4", "--dedup-weighting", "weight"])
    assert a.dedup_weighting == "weight"
    a = cli.parse_args(["--replay-generations", "2", "--replay-age-decay", "0.5"])
    assert a.replay_age_decay == 0.5
    assert cli.parse_args(["--replay-age-decay", "1.0"]).replay_age_decay == 1.0      # the default needs no window
    for argv, text in ((["--dedup-weighting", "weight"], "--dedup-weighting weight needs --dedup-positions exact or symmetric"),
                       (["--dedup-weighting", "mean"], "invalid choice: 'mean' (choose from 'copies', 'weight')"),
                       (["--replay-generations", "2", "--replay-age-decay", "0"], "--replay-age-decay must be in (0, 1], got 0.0"),
                       (["--replay-generations", "2", "--replay-age-decay", "1.5"], "--replay-age-decay must be in (0, 1], got 1.5"),
                       (["--replay-generations", "2", "--replay-age-decay", "-0.5"], "--replay-age-decay must be in (0, 1]"),
                       (["--replay-generations", "2", "--replay-age-decay", "nan"], "--replay-age-decay must be in (0, 1], got nan"),
                       (["--replay-age-decay", "0.5"], "--replay-age-decay needs a window: --replay-generations > 1")):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
        assert text in capsys.readouterr().err, argv
    base = {"iteration": 1, "positions": 10}
    assert cli.iteration_entry(base, row_weights={"source": "x"}) == base
    on = cli.iteration_entry(base, replay={"r": 1}, window_on=True, row_weights={"source": "x"}, weights_on=True)
    assert list(on) == ["iteration", "positions", "replay", "row_weights"] and on["row_weights"] == {"source": "x"}
    text = open(os.path.join(ROOT, "scripts", "staged_loop.py")).read()
    assert '{"replay_age_decay": args.replay_age_decay}' in text and 'if args.replay_age_decay != 1.0 else {}' in text
    assert 'if args.dedup_weighting != "copies":' in text
