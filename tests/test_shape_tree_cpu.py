"""CPU: the checker of the PUCT-shape tests (tests/shape_tree.py), the inputs the GPU tests share with it, the table
function, and the validation that needs no device.

1. With the shape off the Python tree equals SolverTree and ForcedTree bit for bit (solver on / off, k = 0 / 2).
2. The shared 64 x 64 inputs are not vacuous: each setting changes the root visits of at least half the live roots, the
   FPU clamp and the table clamp both fire.
3. puct_shape.cpuct_table against its formula.
4. Every validation error; the ctypes mirror of LzTreeDesc against the header and the library."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from oracle import lz_oracle as O
from tests import forced_tree as FT
from tests import shape_tree as SH
from tests.solver_tree import SolverTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _states_list(states):
    return [O.state_from_batch(states, i) for i in range(np.asarray(states["board"]).shape[0])]


def _same_roots(a, b, tag):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.root_terminal() == y.root_terminal(), (tag, i)
        if x.root_terminal():
            continue
        p, q = x.root_children(), y.root_children()
        assert np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and np.array_equal(p[4], q[4]), (tag, i)
        assert np.array_equal(p[2].view(np.uint64), q[2].view(np.uint64)), (tag, i, "value sums differ")
        assert np.array_equal(p[3].view(np.uint32), q[3].view(np.uint32)), (tag, i, "priors differ")
        assert x.root_visits() == y.root_visits() and x.root_value_sum() == y.root_value_sum(), (tag, i)
        assert np.array_equal(x.prune_targets(), y.prune_targets()), (tag, i, "pruned targets differ")


# ---- 1. off is the tree below ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [False, True])
@pytest.mark.parametrize("k", [0.0, 2.0])
def test_shape_off_equals_the_trees_it_builds_on(solver, k):
    states, noise = FT.parity_inputs(True, num_games=24)
    css = _states_list(states)
    got = [SH.ShapedTree(cs, 1.0, solver=solver, forced_k=k) for cs in css]
    ref = [SolverTree(cs, 1.0, solver=solver, forced_k=k) for cs in css]
    assert not got[0].shape.on and got[0].table is None
    for _ in range(2):                                            # a second search on the kept trees
        FT.search_alone(got, 48, noise)
        FT.search_alone(ref, 48, noise)
        _same_roots(got, ref, (solver, k))
        assert [t.root_proven for t in got] == [t.root_proven for t in ref]
        assert [t.solver_count for t in got] == [t.solver_count for t in ref]
        assert [t.forced_count for t in got] == [t.forced_count for t in ref]
    if not solver:
        plain = [FT.ForcedTree(cs, 1.0, k) for cs in css]
        for _ in range(2):
            FT.search_alone(plain, 48, noise)
        _same_roots(got, plain, ("forced", k))


# ---- 2. the shared inputs are not vacuous -----------------------------------------------------------------------------------
_plain = {}


def _plain_vectors(with_noise):
    if with_noise not in _plain:
        states, noise = FT.parity_inputs(with_noise)
        trees = SH.make_trees(states, {})
        FT.search_alone(trees, FT.PARITY_SIMS, noise)
        _plain[with_noise] = SH.root_visit_vectors(trees)
    return _plain[with_noise]


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("name", sorted(SH.SETTINGS))
def test_each_setting_changes_at_least_half_the_live_roots(name, with_noise):
    """64 games x 64 simulations of forced_tree.parity_inputs (seed 11) under hash_evaluator: first-play urgency 0.2 / 0.1,
    the table with log 1.0 and base 8, and both, against the plain search.  (Observed with a prototype of this checker: 60
    to 62 of 64 roots changed; every root is live.)"""
    states, noise = FT.parity_inputs(with_noise)
    trees = SH.make_trees(states, SH.SETTINGS[name])
    FT.search_alone(trees, FT.PARITY_SIMS, noise)
    got, plain = SH.root_visit_vectors(trees), _plain_vectors(with_noise)
    live = [i for i, v in enumerate(plain) if v is not None]
    changed = sum(got[i] != plain[i] for i in live)
    print(f"{name}, noise={with_noise}: {changed} of {len(live)} live roots changed")
    assert 2 * len(live) >= len(plain)
    assert all(got[i] is not None and sum(got[i]) == FT.PARITY_SIMS for i in live)
    assert 2 * changed >= len(live)


def test_both_clamps_fire():
    """Reduction 1.5 sends f below -1 and a 16-entry table ends below the visit counts of a 64-simulation search."""
    states, noise = FT.parity_inputs(True)
    trees = SH.make_trees(states, SH.CLAMPS)
    FT.search_alone(trees, FT.PARITY_SIMS, noise)
    fpu, tab = sum(t.fpu_clamped for t in trees), sum(t.table_clamped for t in trees)
    print("levels with f clamped at -1:", fpu, "levels beyond the table:", tab)
    assert fpu > 0 and tab > 0
    assert len(trees[0].table) == 16


def test_fpu_zero_is_on_and_is_the_parent_value():
    states, _ = FT.parity_inputs(False, num_games=8)
    trees = SH.make_trees(states, dict(fpu_reduction=0.0))
    FT.search_alone(trees, 8)
    t = next(t for t in trees if not t.root_terminal())
    assert t.shape.fpu and not t.shape.table and t.shape.fpu_root_reduction == 0.0
    r = t.nodes[t.root]
    assert t.fpu_value(t.root) == max(r.value_sum / r.visit_count, -1.0)


# ---- 3. the table ---------------------------------------------------------------------------------------------------------
def test_cpuct_table_is_the_formula():
    from liuzhou_amd.puct_shape import CPUCT_TABLE_LEN, cpuct_table
    tab = cpuct_table(1.25, 0.5, 19652.0)
    assert len(tab) == CPUCT_TABLE_LEN == 65536
    for i in (0, 1, 2, 17, 800, 19651, 65535):
        assert tab[i] == 1.25 + 0.5 * math.log((i + 19652.0 + 1.0) / 19652.0)
    assert all(b > a for a, b in zip(tab[:1000], tab[1:1001]))
    assert cpuct_table(2.0, 0.0, 8.0, 4) == [2.0] * 4
    assert len(cpuct_table(1.0, 1.0, 8.0, 16)) == 16
    for bad in (dict(length=1), dict(cpuct_base=0.0), dict(cpuct_base=-1.0), dict(cpuct_base=float("nan"))):
        with pytest.raises(ValueError):
            cpuct_table(**{**dict(c_puct=1.0, cpuct_log=1.0, cpuct_base=8.0, length=4), **bad})


# ---- 4. validation ----------------------------------------------------------------------------------------------------------
def test_parameters_are_validated():
    from liuzhou_amd.puct_shape import parse_puct_shape as puct_shape_refusal
    off = puct_shape_refusal()
    assert not off.on and off.flags == 0 and off.kwargs() == {}
    assert not puct_shape_refusal(cpuct_base=8.0).on                # a base alone switches nothing on
    on = puct_shape_refusal(fpu_reduction=0.0)
    assert on.fpu and not on.table and on.flags == 1 and on.fpu_root_reduction == 0.0
    assert puct_shape_refusal(fpu_reduction=0.2).fpu_root_reduction == 0.2     # None = the same reduction at the root
    assert puct_shape_refusal(fpu_reduction=0.2, fpu_root_reduction=0.1).fpu_root_reduction == 0.1
    assert puct_shape_refusal(cpuct_log=1.0, cpuct_base=8.0).flags == 2
    for bad in (dict(fpu_reduction=-0.1), dict(fpu_reduction=float("inf")), dict(fpu_reduction=float("nan")),
                dict(fpu_reduction=0.2, fpu_root_reduction=-1.0), dict(fpu_reduction=0.2, fpu_root_reduction=float("nan")),
                dict(cpuct_log=-1.0), dict(cpuct_log=float("inf")), dict(cpuct_base=0.0), dict(cpuct_base=-3.0),
                dict(cpuct_base=float("nan")), dict(cpuct_log=1.0, cpuct_base=0.0),
                dict(fpu_root_reduction=0.1)):                    # a root reduction without first-play urgency
        with pytest.raises(ValueError):
            puct_shape_refusal(**bad)


def test_configurations_are_refused_with_a_reason(monkeypatch):
    from liuzhou_amd.search_rules import SearchRules, persistent_default

    def puct_shape_refusal(gumbel_considered=0, **kw):           # the shape's own rows of the table
        context = {k: kw.pop(k) for k in ("batch_k", "fused", "search_backend", "persistent") if k in kw}
        context.setdefault("persistent", persistent_default())
        why = SearchRules.parse(800, gumbel_considered=gumbel_considered, **kw).refusal(**context)
        if why is not None and why.startswith("first-play urgency"):
            raise ValueError(why)
    monkeypatch.delenv("LZ_TREE_PERSISTENT", raising=False)
    for shape in (dict(fpu_reduction=0.2), dict(cpuct_log=1.0)):
        with pytest.raises(ValueError, match="Gumbel"):
            puct_shape_refusal(gumbel_considered=8, **shape)
        with pytest.raises(ValueError, match="batch_k"):
            puct_shape_refusal(batch_k=2, **shape)
        with pytest.raises(ValueError, match="external evaluator"):
            puct_shape_refusal(fused=False, **shape)
        with pytest.raises(ValueError, match="root-PUCT"):
            puct_shape_refusal(search_backend="cuda_root", **shape)
        with pytest.raises(ValueError, match="persistent"):
            puct_shape_refusal(persistent=True, **shape)
    monkeypatch.setenv("LZ_TREE_PERSISTENT", "1")
    with pytest.raises(ValueError, match="persistent"):
        puct_shape_refusal(fpu_reduction=0.2)
    # off: none of these configurations is refused
    puct_shape_refusal(gumbel_considered=8, batch_k=2, fused=False, search_backend="cuda_root")


def test_engines_runner_worker_and_agents_refuse():
    from liuzhou_amd.eval_arena import make_agent
    from liuzhou_amd.self_play_stage import run_self_play_stage
    from liuzhou_amd.self_play_worker import run_self_play_worker
    from liuzhou_amd.tree_engine import PortableTreeMCTS, PriorEvaluator, self_play_tree_gpu
    with pytest.raises(ValueError, match="batch_k"):
        PortableTreeMCTS(object(), 4, 8, "cuda:0", batch_k=2, fpu_reduction=0.2)
    with pytest.raises(ValueError, match="external evaluator"):
        PortableTreeMCTS(PriorEvaluator(lambda p, s: None), 4, 8, "cuda:0", cpuct_log=1.0)
    with pytest.raises(ValueError, match="fpu_root_reduction"):
        PortableTreeMCTS(object(), 4, 8, "cuda:0", fpu_root_reduction=0.1)
    common = dict(num_games=2, mcts_simulations=8, temperature_init=1.0, temperature_final=0.1, temperature_threshold=4,
                  exploration_weight=1.0, device="cuda:0")
    with pytest.raises(ValueError, match="external evaluator"):
        self_play_tree_gpu(PriorEvaluator(lambda p, s: None), fpu_reduction=0.2, **common)
    with pytest.raises(ValueError, match="cpuct_base"):
        self_play_tree_gpu(PriorEvaluator(lambda p, s: None), cpuct_log=1.0, cpuct_base=0.0, **common)
    wk = dict(worker_idx=0, shard_device="cuda:0", shard_games=4, seed=1, model_state_path="none.pt", output_path="none",
              mcts_simulations=8, temperature_init=1.0, temperature_final=0.1, temperature_threshold=4,
              exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
              opening_random_moves=0, max_game_plies=8, concurrent_games_per_device=4)
    with pytest.raises(ValueError, match="root-PUCT"):
        run_self_play_worker(search_backend="cuda_root", fpu_reduction=0.2, **wk)
    with pytest.raises(ValueError, match="Gumbel"):
        run_self_play_worker(search_backend="tree", gumbel_considered=8, cpuct_log=1.0, **wk)
    with pytest.raises(ValueError, match="root-PUCT"):
        run_self_play_stage(model_state={}, num_games=4, output_path="none", devices=["cuda:0"], iteration_seed=1, mcts_simulations=8,
                            search_backend="cuda_root", cpuct_log=1.0)
    with pytest.raises(ValueError, match="tree backend"):
        make_agent(object(), "v1", "cuda:0", 8, 0.1, False, fpu_reduction=0.2)


def test_the_ctypes_mirror_follows_the_header():
    """Field names in the order of include/liuzhou_hip.h, the new fields last, and the size the library reports."""
    from liuzhou_amd import _lib as L
    from liuzhou_amd.tree_engine import LzTreeDesc
    text = open(os.path.join(ROOT, "include", "liuzhou_hip.h")).read()
    body = text[text.index("typedef struct LzTreeDesc {"):text.index("} LzTreeDesc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = body[body.index("{") + 1:]
    names = [re.findall(r"\w+", piece)[-1] for stmt in body.split(";") if stmt.strip() for piece in stmt.split(",")]
    mirror = [f[0] for f in LzTreeDesc._fields_]
    assert names == mirror
    assert mirror[-5:] == ["puct_shape", "cpuct_table_len", "fpu_reduction", "fpu_root_reduction", "cpuct_table"]
    types = dict(LzTreeDesc._fields_)
    assert types["puct_shape"] is C.c_int32 and types["cpuct_table_len"] is C.c_int32
    assert types["fpu_reduction"] is C.c_double and types["fpu_root_reduction"] is C.c_double
    assert types["cpuct_table"] is C.c_void_p
    assert LzTreeDesc.cpuct_table.offset + 8 == C.sizeof(LzTreeDesc)
    assert int(L.lib().lz_tree_desc_bytes()) == C.sizeof(LzTreeDesc)
