"""GPU: symmetric leaf evaluation in the tree search (`eval_symmetry`, csrc/lz_tree_dev.h): a fixed identity changes
nothing, a fixed element replays in the oracle with the evaluator modelled as net(sigma_k leaf) mapped back, "random"
is deterministic across launch forms and covers the group, and the paths without the hook refuse the option."""
import numpy as np
import pytest
import torch

from liuzhou_amd import symmetry as S
from oracle import lz_oracle as O
from tests.golden_utils import FIELDS, load, states as gstates
from tests.tree_parity import replay_part_in_oracle, root_edges, to_gpu_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_NET = {}


def _net():
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    if "net" not in _NET:
        torch.manual_seed(20260314)
        _NET["net"] = FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV))
    return _NET["net"]


def _states(n, seed):
    st = gstates(load("g1_rules.npz"), "s")
    idx = np.random.default_rng(seed).integers(0, st["board"].shape[0], n)
    return {f: np.ascontiguousarray(np.asarray(st[f])[idx]) for f in FIELDS}


def _mcts(n, sims, **kw):
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    args = dict(exploration_weight=1.0, add_dirichlet_noise=True, dirichlet_alpha=0.3, dirichlet_epsilon=0.25,
                sample_moves=True, reuse_tree=True, reuse_factor=4.0, seed=777)
    args.update(kw)
    return PortableTreeMCTS(_net(), n, sims, DEV, **args)


def _play(mcts, st, moves):
    """`moves` searches with subtree reuse; every move's outputs, root edges and (when traced) the trace."""
    B = st["board"].shape[0]
    cur = [O.state_from_batch(st, i) for i in range(B)]
    outs = []
    for _ in range(moves):
        out = mcts.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV),
                                temperatures=torch.ones((B,), dtype=torch.float32, device=DEV))
        torch.cuda.synchronize()
        chosen = out.chosen_action_indices.cpu().numpy()
        rec = {"policy": out.policy_dense.cpu().numpy(), "chosen": chosen,
               # root edge statistics (the node / pool indices of an edge depend on the order games take chunks)
               "edges": [tuple(e[f].tobytes() for f in ("W", "P", "n_info", "act")) for e in root_edges(mcts.engine)]}
        if getattr(mcts.engine, "trace", None) is not None:
            rec["trace"] = {k: v.cpu().numpy().copy() for k, v in mcts.engine.trace.items()}
        outs.append(rec)
        for i in range(B):
            if chosen[i] >= 0:
                cur[i] = O.apply_index(cur[i], int(chosen[i]))
    return outs


def test_fixed_identity_equals_none():
    _need_gpu()
    st = _states(32, 1)
    a = _play(_mcts(32, 32), st, 3)
    b = _play(_mcts(32, 32, eval_symmetry=0), st, 3)
    for x, y in zip(a, b):
        assert np.array_equal(x["policy"].view(np.uint32), y["policy"].view(np.uint32))
        assert np.array_equal(x["chosen"], y["chosen"])
        assert x["edges"] == y["edges"]


def _true_frame(trace, k):
    """The trace of a search under sigma_k mapped back: leaves sigma_k^-1(evaluated record), head rows read through
    the cell map -- what a search that evaluated the true leaves with net(sigma_k .) mapped back would have recorded."""
    inv = S.inverse(k)
    leaf = trace["trace_leaf"]
    n, B = leaf.shape[:2]
    true = S.transform_packed(torch.from_numpy(leaf.reshape(-1, 4)), inv).numpy().reshape(leaf.shape)
    cells = S.np_cell_perm(k)
    h = trace["trace_heads"].reshape(n, B, 3, 36)[..., cells].reshape(n, B, 108)
    kind = trace["trace_kind"]
    ev = kind == 1
    assert np.all(trace["trace_sym"][ev] == k)
    # the records the engine asked the network for are sigma_k of the true leaves
    again = S.transform_packed(torch.from_numpy(true.reshape(-1, 4)), k).numpy().reshape(leaf.shape)
    assert np.array_equal(again[ev], leaf[ev])
    return np.where(ev[..., None], true, leaf), np.where(ev[..., None], h, trace["trace_heads"])


@pytest.mark.parametrize("k,split,compact", [(1, True, False), (1, True, True), (1, False, False), (1, False, True),
                                             (4, True, False), (4, False, True), (6, True, True), (6, False, False)])
def test_fixed_element_replays_in_the_oracle(k, split, compact, monkeypatch):
    _need_gpu()
    if not split:
        monkeypatch.setenv("LZ_TREE_SPLIT", "0")
    B, sims, moves = 24, 24, 3
    st = _states(B, 10 + k)
    mcts = _mcts(B, sims, trace=True, eval_symmetry=k, compact_evals=compact)
    e = mcts.engine
    cur = [O.state_from_batch(st, i) for i in range(B)]
    trees = [O.OracleTree(cur[i], 1.0) for i in range(B)]
    evals = 0
    for mv in range(moves):
        out = mcts.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV),
                                temperatures=torch.ones((B,), dtype=torch.float32, device=DEV))
        torch.cuda.synchronize()
        tr = {n: t.cpu().numpy() for n, t in e.trace.items()}
        leaf, heads = _true_frame(tr, k)
        saved = {n: t.clone() for n, t in e.trace.items()}
        e.trace["trace_leaf"].copy_(torch.from_numpy(leaf))
        e.trace["trace_heads"].copy_(torch.from_numpy(heads))
        st_ = replay_part_in_oracle(mcts, trees, mv, 0.25)      # visit counts / W / priors bit-exact, root value 1e-6
        for n, t in saved.items():
            e.trace[n].copy_(t)
        evals += st_["evals"]
        chosen = out.chosen_action_indices.cpu().numpy()
        for i in range(B):
            if trees[i].root_terminal():
                trees[i] = O.OracleTree(cur[i], 1.0)
                continue
            cur[i] = O.apply_index(cur[i], int(chosen[i]))
            if not trees[i].advance(int(chosen[i])):
                trees[i] = O.OracleTree(cur[i], 1.0)
    assert evals > B * sims


def test_fixed_element_sharing_on_and_off_agree(monkeypatch):
    _need_gpu()
    st = _states(32, 3)
    a = _play(_mcts(32, 48, eval_symmetry=6), st, 3)
    monkeypatch.setenv("LZ_TREE_SHARE", "0")
    b = _play(_mcts(32, 48, eval_symmetry=6), st, 3)
    for x, y in zip(a, b):
        assert np.array_equal(x["policy"].view(np.uint32), y["policy"].view(np.uint32))
        assert np.array_equal(x["chosen"], y["chosen"])
        assert x["edges"] == y["edges"]


def _ids(rec):
    t = rec["trace"]
    return t["trace_sym"][t["trace_kind"] == 1]


def test_random_is_deterministic_across_launch_forms_and_covers_the_group():
    _need_gpu()
    st = _states(64, 4)
    base = _play(_mcts(64, 64, trace=True, eval_symmetry="random", compact_evals=False), st, 3)
    for kw in (dict(compact_evals=False), dict(compact_evals=True), dict(compact_evals=False, use_graph=False)):
        other = _play(_mcts(64, 64, trace=True, eval_symmetry="random", **kw), st, 3)
        for x, y in zip(base, other):
            assert np.array_equal(x["policy"].view(np.uint32), y["policy"].view(np.uint32)), kw
            assert np.array_equal(x["chosen"], y["chosen"]), kw
            assert x["edges"] == y["edges"], kw
            assert np.array_equal(_ids(x), _ids(y)), kw
    ids = np.concatenate([_ids(r) for r in base])
    assert ids.size >= 8_000
    frac = np.bincount(ids, minlength=8) / ids.size
    assert frac.shape == (8,) and np.all(frac >= 0.06) and np.all(frac <= 0.19), frac
    reseeded = _play(_mcts(64, 64, trace=True, eval_symmetry="random", seed=778), st, 1)
    a, b = _ids(base[0]), _ids(reseeded[0])
    n = min(a.size, b.size)
    assert not np.array_equal(a[:n], b[:n])


def test_refusals():
    _need_gpu()
    from liuzhou_amd.self_play_worker import run_self_play_worker
    from liuzhou_amd.tree_engine import parse_eval_symmetry
    with pytest.raises(ValueError, match="batch_k"):
        _mcts(8, 16, batch_k=4, eval_symmetry="random")
    with pytest.raises(ValueError, match="root-PUCT"):
        run_self_play_worker(worker_idx=0, shard_device=DEV, shard_games=2, seed=1, model_state_path="unused",
                             output_path="unused", mcts_simulations=8, temperature_init=1.0, temperature_final=0.1,
                             temperature_threshold=10, exploration_weight=1.0, dirichlet_alpha=0.3,
                             dirichlet_epsilon=0.25, soft_value_k=2.0, opening_random_moves=0, max_game_plies=8,
                             concurrent_games_per_device=2, search_backend="cuda_root", eval_symmetry="random")
    for bad in ("sometimes", 8, -1, True):
        with pytest.raises(ValueError):
            parse_eval_symmetry(bad)


def test_self_play_tree_gpu_end_to_end_with_random_symmetry():
    _need_gpu()
    from liuzhou_amd.tree_engine import self_play_tree_gpu
    batch, stats = self_play_tree_gpu(_net(), num_games=12, mcts_simulations=16, temperature_init=1.0,
                                      temperature_final=0.1, temperature_threshold=10, exploration_weight=1.0,
                                      device=DEV, max_game_plies=24, concurrent_games=12, seed=5,
                                      eval_symmetry="random")
    n = batch.num_samples
    assert n > 0
    assert tuple(batch.state_tensors.shape) == (n, 11, 6, 6)
    assert tuple(batch.legal_masks.shape) == (n, 220) and tuple(batch.policy_targets.shape) == (n, 220)
    assert batch.value_targets.numel() == n and batch.soft_value_targets.numel() == n
    pol, mask = batch.policy_targets.cpu(), batch.legal_masks.cpu().bool()
    assert float(pol[~mask].abs().max()) == 0.0
