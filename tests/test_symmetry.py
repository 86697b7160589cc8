"""Board symmetries (liuzhou_amd/symmetry.py, csrc/lz_symmetry.h) on the host: the group laws of the compiled tables,
the equivariance of the rules under every element (checked through the C oracle, so the action and direction tables are
checked against the rules themselves), and the host library's transforms against the numpy restatement."""
import numpy as np
import pytest
import torch

from liuzhou_amd import symmetry as S
from oracle import lz_oracle as O
from tests.golden_utils import FIELDS, load, states

KS = range(8)


def _permute_meta(meta, k):
    """metadata (kind, primary, secondary, extra) of an action, seen through sigma_k: cells mapped, the move direction
    mapped, the kind kept, -1 kept."""
    cell, dirs = S.np_cell_perm(k), S.np_dir_perm(k)
    out = meta.copy()
    kind = meta[..., 0]
    prim = meta[..., 1]
    out[..., 1] = np.where(prim >= 0, cell[np.clip(prim, 0, 35)], prim)
    move = kind == 2
    out[..., 2] = np.where(move, dirs[np.clip(meta[..., 2], 0, 3)], meta[..., 2])
    out[..., 3] = np.where(move & (meta[..., 3] >= 0), cell[np.clip(meta[..., 3], 0, 35)], meta[..., 3])
    return out


def test_tables_match_the_numpy_restatement():
    T = S.tables()
    for k in KS:
        assert np.array_equal(T["cells"][k], S.np_cell_perm(k))
        assert np.array_equal(T["directions"][k], S.np_dir_perm(k))
        assert np.array_equal(T["actions"][k], S.np_action_perm(k))
        assert np.array_equal(S.action_permutation(k).numpy(), S.np_action_perm(k))
        assert S.action_permutation(k).dtype == torch.int64 and S.action_permutation(k).shape == (220,)
        for b in KS:
            assert S.compose(k, b) == S.np_compose(k, b)


def test_group_laws():
    perms = {tuple(S.np_cell_perm(k)) for k in KS}
    assert len(perms) == 8                                      # 8 distinct cell permutations
    for a in KS:
        assert S.compose(a, S.inverse(a)) == 0 and S.compose(S.inverse(a), a) == 0
        assert S.compose(0, a) == a == S.compose(a, 0)
        for b in KS:
            c = S.compose(a, b)
            assert 0 <= c < 8                                   # closed
            assert np.array_equal(S.np_cell_perm(c), S.np_cell_perm(a)[S.np_cell_perm(b)])
            for d in KS:                                        # associative
                assert S.compose(S.compose(a, b), d) == S.compose(a, S.compose(b, d))
    for k in KS:                                                # every action table is a permutation fixing the aux indices
        P = S.np_action_perm(k)
        assert sorted(P.tolist()) == list(range(220))
        assert P[216:].tolist() == [216, 217, 218, 219]
    with pytest.raises(ValueError):
        S.inverse(8)


@pytest.mark.parametrize("fixture", ["g15_rules_large.npz", "g16_garbage_large.npz"])
def test_legal_mask_and_metadata_are_equivariant(fixture):
    st = states(load(fixture), "s")
    mask, meta = O.encode_actions(st)
    for k in KS:
        P = S.np_action_perm(k)
        ts = S.np_transform_states(st, k)
        m2, meta2 = O.encode_actions(ts)
        want = np.zeros_like(mask)
        want[:, P] = mask
        assert np.array_equal(m2, want), k                      # legal_mask(sigma s) == P_sigma legal_mask(s)
        want_meta = np.empty_like(meta)
        want_meta[:, P] = _permute_meta(meta, k)
        assert np.array_equal(meta2, want_meta), k


def test_transitions_are_equivariant_on_g15():
    st = states(load("g15_rules_large.npz"), "s")
    mask, meta = O.encode_actions(st)
    parents, actions = np.nonzero(mask)
    children = O.apply_moves(st, meta[parents, actions], parents.astype(np.int64), strict=True)
    for k in KS:
        P = S.np_action_perm(k)
        ts = S.np_transform_states(st, k)
        _, meta_t = O.encode_actions(ts)
        got = O.apply_moves(ts, meta_t[parents, P[actions]], parents.astype(np.int64), strict=True)
        want = S.np_transform_states(children, k)               # apply(sigma s, P a) == sigma apply(s, a)
        for f in FIELDS:
            assert np.array_equal(np.asarray(got[f]), np.asarray(want[f])), (k, f)


def _random_rows(rng, n):
    planes = rng.standard_normal((n, 11, 6, 6)).astype(np.float32)
    masks = rng.random((n, 220)) < 0.3
    policy = rng.standard_normal((n, 220)).astype(np.float32)
    policy.view(np.uint32)[:, ::7] ^= rng.integers(0, 1 << 22, (n, 32), dtype=np.uint32)   # arbitrary (finite) bit patterns
    policy[~np.isfinite(policy)] = 0.0
    return planes, masks, policy


@pytest.mark.parametrize("dtype", [torch.int8, torch.int32])
def test_host_gather_samples_match_numpy(dtype):
    rng = np.random.default_rng(11)
    n = 300
    planes, masks, policy = _random_rows(rng, n)
    sym = rng.integers(0, 8, n)
    got = S.transform_samples(torch.from_numpy(planes), torch.from_numpy(masks), torch.from_numpy(policy),
                              torch.from_numpy(sym).to(dtype))
    want = S.np_transform_samples(planes, masks, policy, sym)
    for g, w in zip(got, want):
        assert np.array_equal(g.numpy().view(np.uint8), w.view(np.uint8))
    idx = rng.integers(0, n, 517)
    sym2 = rng.integers(0, 8, 517)
    got = S.transform_samples(torch.from_numpy(planes), torch.from_numpy(masks), torch.from_numpy(policy),
                              torch.from_numpy(sym2).to(dtype), torch.from_numpy(idx))
    want = S.np_transform_samples(planes, masks, policy, sym2, idx)
    for g, w in zip(got, want):
        assert g.shape[0] == 517
        assert np.array_equal(g.numpy().view(np.uint8), w.view(np.uint8))
    # planes only
    p_only, m_none, q_none = S.transform_samples(torch.from_numpy(planes), None, None, 3)
    assert m_none is None and q_none is None
    assert np.array_equal(p_only.numpy(), S.np_transform_samples(planes, None, None, 3)[0])


def test_host_inverse_then_forward_is_identity():
    rng = np.random.default_rng(5)
    planes, masks, policy = (torch.from_numpy(a) for a in _random_rows(rng, 64))
    sym = torch.from_numpy(rng.integers(0, 8, 64).astype(np.int8))
    inv = torch.tensor([S.inverse(int(k)) for k in sym], dtype=torch.int8)
    once = S.transform_samples(planes, masks, policy, inv)
    back = S.transform_samples(*once, sym)
    for a, b in zip(back, (planes, masks, policy)):
        assert torch.equal(a.view(torch.uint8), b.contiguous().view(torch.uint8))


def test_host_transform_states_and_packed_match_numpy():
    st = states(load("g15_rules_large.npz"), "s")
    n = st["board"].shape[0]
    sym = np.random.default_rng(2).integers(0, 8, n)
    got = S.transform_states({f: torch.from_numpy(np.asarray(st[f])) for f in FIELDS}, torch.from_numpy(sym.astype(np.int32)))
    want = S.np_transform_states(st, sym)
    for f in FIELDS:
        assert np.array_equal(got[f].numpy(), np.asarray(want[f])), f
    inv = torch.tensor([S.inverse(int(k)) for k in sym], dtype=torch.int8)
    back = S.transform_states(got, inv)
    for f in FIELDS:
        assert np.array_equal(back[f].numpy(), np.asarray(st[f])), f
    rng = np.random.default_rng(3)
    packed = rng.integers(-(1 << 63), (1 << 63) - 1, (500, 4), dtype=np.int64)
    psym = rng.integers(0, 8, 500)
    got_p = S.transform_packed(torch.from_numpy(packed), torch.from_numpy(psym.astype(np.int8))).numpy()
    assert np.array_equal(got_p, S.np_transform_packed(packed, psym))
    assert np.array_equal(got_p[:, 0] & ~np.int64(0xFFFFFFFFF), packed[:, 0] & ~np.int64(0xFFFFFFFFF))


def test_invalid_ids_and_sets_are_refused():
    planes = torch.zeros(4, 11, 6, 6)
    with pytest.raises(ValueError):
        S.transform_samples(planes, None, None, 9)
    with pytest.raises(TypeError):
        S.transform_samples(planes, None, None, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        S.transform_samples(planes, torch.zeros(4, 220, dtype=torch.bool), None, 1)
