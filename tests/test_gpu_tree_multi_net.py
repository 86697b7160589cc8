"""Tree search with one network per segment of slots (lz_tree_search_multi): every game's search must be bit-identical to
a single-network engine searching that game with its own network -- root visits, values, policies and picks -- in graph
and direct launches, with transposition sharing on and off, and through the split-phase path."""
import numpy as np
import pytest
import torch

from tests.golden_utils import load, states, FIELDS
from tests.tree_parity import to_gpu_batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G, SIMS, MOVES = 48, 24, 3


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _nets(config="b6c64", k=2):
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    out = []
    for i in range(k):
        m = ChessNet(**MODEL_CONFIGS[config]).eval()
        stable_resnet_init(m, 500 + 17 * i)
        out.append(FusedNet(m.to(DEV), DEV))
    return out


def _batch(n, seed):
    st_all = states(load("g1_rules.npz"), "s")
    idx = np.random.default_rng(seed).integers(0, st_all["board"].shape[0], n)
    return to_gpu_batch({f: np.ascontiguousarray(np.asarray(st_all[f])[idx]) for f in FIELDS}, DEV)


def _moves():
    """Per move: positions of the G games, which slots of each segment are active, plies (RNG keys)."""
    out = []
    for mv in range(MOVES):
        rng = np.random.default_rng(100 + mv)
        act = [torch.from_numpy(rng.random(G) < 0.7).to(DEV) for _ in range(2)]
        out.append((_batch(G, 40 + mv), act, torch.full((G,), mv, dtype=torch.int64, device=DEV)))
    return out


def _record(m, out, slots):
    e = m.engine
    return {"pick": out.chosen_action_indices[slots].clone(), "policy": out.policy_dense[slots].clone(),
            "value": out.root_value[slots].clone(), "visits": e.buf["root_visits"][slots].clone()}


def _single(net, moves, k, use_graph):
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    m = PortableTreeMCTS(net, G, SIMS, DEV, add_dirichlet_noise=True, sample_moves=True, seed=9, compact_evals=True,
                         use_graph=use_graph)
    temps = torch.ones(G, device=DEV)
    ids = torch.arange(G, dtype=torch.int64, device=DEV)
    res = []
    for batch, act, ply in moves:
        out = m.search_batch(batch, temperatures=temps, active=act[k], rng_game_ids=ids, rng_plies=ply)
        res.append(_record(m, out, act[k].nonzero().view(-1)))
    return res


def _joint(nets, moves, use_graph, multi_launch=True):
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    m = PortableTreeMCTS(nets, 2 * G, SIMS, DEV, add_dirichlet_noise=True, sample_moves=True, seed=9, use_graph=use_graph,
                         segment_games=G, multi_launch=multi_launch)
    assert m.fused_multi == multi_launch
    temps = torch.ones(2 * G, device=DEV)
    ids = torch.arange(G, dtype=torch.int64, device=DEV).repeat(2)
    both = torch.arange(2 * G, device=DEV) % G
    res = [[], []]
    for batch, act, ply in moves:
        out = m.search_batch(batch.select(both), temperatures=temps, active=torch.cat(act), rng_game_ids=ids,
                             rng_plies=ply.repeat(2))
        for k in range(2):
            res[k].append(_record(m, out, act[k].nonzero().view(-1) + k * G))
    return res, m


def _same(a, b):
    for x, y in zip(a, b):
        for key in x:
            assert torch.equal(x[key], y[key]), key


@pytest.mark.parametrize("share", ["1", "0"])
@pytest.mark.parametrize("use_graph", [True, False])
def test_two_segments_equal_two_single_network_engines(monkeypatch, share, use_graph):
    _need_gpu()
    monkeypatch.setenv("LZ_TREE_SHARE", share)
    nets = _nets()
    moves = _moves()
    joint, m = _joint(nets, moves, use_graph)
    for k in range(2):
        _same(joint[k], _single(nets[k], moves, k, use_graph))
    # one network launch per simulation, the lists padded per segment
    assert m.leaf_evals > 0 and m.engine.seg_off.abs().sum() > 0


def test_split_phase_path_builds_the_same_trees():
    _need_gpu()
    nets = _nets()
    moves = _moves()
    fused, _ = _joint(nets, moves, use_graph=False)
    split, _ = _joint(nets, moves, use_graph=False, multi_launch=False)
    for k in range(2):
        _same(fused[k], split[k])


def test_three_segments_wide_net():
    _need_gpu()
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    nets = _nets("b10c128", 3)
    g, sims = 16, 8
    batch = _batch(g, 77)
    m = PortableTreeMCTS(nets, 3 * g, sims, DEV, add_dirichlet_noise=False, sample_moves=False, segment_games=g)
    out = m.search_batch(batch.select(torch.arange(3 * g, device=DEV) % g), temperatures=torch.ones(3 * g, device=DEV))
    for k in range(3):
        s = PortableTreeMCTS(nets[k], g, sims, DEV, add_dirichlet_noise=False, sample_moves=False, compact_evals=True)
        ref = s.search_batch(batch, temperatures=torch.ones(g, device=DEV))
        assert torch.equal(out.chosen_action_indices[k * g:(k + 1) * g], ref.chosen_action_indices)
        assert torch.equal(out.policy_dense[k * g:(k + 1) * g], ref.policy_dense)


def test_refused_combinations():
    _need_gpu()
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    nets = _nets()
    with pytest.raises(ValueError):
        PortableTreeMCTS(nets, 2 * G, 8, DEV, segment_games=G, eval_symmetry="random")
    with pytest.raises(ValueError):
        PortableTreeMCTS(nets, 2 * G, 8, DEV, segment_games=G, batch_k=4)
    with pytest.raises(ValueError):
        PortableTreeMCTS(nets, 2 * G + 16, 8, DEV, segment_games=G)
    with pytest.raises(ValueError):
        PortableTreeMCTS(nets, 40, 8, DEV, segment_games=20)                 # not a multiple of 16
