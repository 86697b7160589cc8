"""Several networks in one launch (lz_net_forward_packed_multi_f16): every row must be bit-identical to the single-network
kernel with that row's own network, padding behind a segment must stay untouched, and networks the launch cannot share
must be refused."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.golden_utils import load, states, FIELDS
from tests.tree_parity import to_gpu_batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _nets(config, k, **kw):
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.net_hip import FusedNet
    out = []
    for i in range(k):
        m = ChessNet(**MODEL_CONFIGS[config]).eval()
        stable_resnet_init(m, 1000 + i)
        out.append(FusedNet(m.to(DEV), DEV, **kw))
    return out


def _packed(n, seed):
    from liuzhou_amd import _lib as L
    st_all = states(load("g1_rules.npz"), "s")
    idx = np.random.default_rng(seed).integers(0, st_all["board"].shape[0], n)
    batch = to_gpu_batch({f: np.ascontiguousarray(np.asarray(st_all[f])[idx]) for f in FIELDS}, DEV)
    out = torch.zeros((n, 4), dtype=torch.int64, device=DEV)
    s = L.soa([t.contiguous() for t in batch.tensors()])
    with torch.cuda.device(DEV):
        L.check(L.lib().lz_pack_states(C.byref(s), L.i64(n), L.ptr(out), L.stream_ptr(DEV)), "pack_states")
    return out


def _layout(sizes):
    """Segment rows as lz_tree_search_multi lays them out: each segment from a 16-aligned base; seg_off[k + 1] = its end."""
    off, bases, cur = [0], [], 0
    for n in sizes:
        b = -(-cur // 16) * 16
        bases.append(b)
        cur = b + n
        off.append(cur)
    return off, bases


CASES = [[0, 1, 15], [16, 17], [1, 0], [300, 5, 0], [17, 250, 16]]


@pytest.mark.parametrize("config,kw", [("b6c64", {}), ("b6c64", {"half_workgroups": True}), ("b10c128", {})])
@pytest.mark.parametrize("sizes", CASES)
def test_every_row_equals_its_own_network(config, kw, sizes):
    _need_gpu()
    from liuzhou_amd.net_hip import forward_packed_multi
    nets = _nets(config, len(sizes), **kw)
    off, bases = _layout(sizes)
    cap = max(16, -(-off[-1] // 16) * 16 + 16)
    packed = _packed(cap, seed=sum(sizes) + len(sizes))
    seg = torch.tensor(off, dtype=torch.int64, device=DEV)
    lp1, lp2, lpm, val = forward_packed_multi(nets, packed, seg, cap)
    torch.cuda.synchronize()
    covered = torch.zeros(cap, dtype=torch.bool)
    for k, (b, n) in enumerate(zip(bases, sizes)):
        if n == 0:
            continue
        covered[b:b + n] = True
        r1, r2, rm, _, rv = nets[k].forward_packed(packed[b:b + n])
        for got, ref in ((lp1, r1), (lp2, r2), (lpm, rm), (val, rv)):
            assert torch.equal(got[b:b + n], ref), (k, b, n)
    # rows of no segment (padding behind a segment's live rows, the tail) are never written
    rest = (~covered).nonzero().view(-1).to(DEV)
    for t in (lp1, lp2, lpm, val):
        assert torch.count_nonzero(t.index_select(0, rest)) == 0


def test_one_network_equals_the_plain_launch():
    _need_gpu()
    from liuzhou_amd.net_hip import forward_packed_multi
    net, = _nets("b6c64", 1)
    packed = _packed(200, seed=3)
    lp1, lp2, lpm, val = forward_packed_multi([net], packed, torch.tensor([0, 200], dtype=torch.int64, device=DEV))
    r1, r2, rm, _, rv = net.forward_packed(packed)
    assert torch.equal(lp1, r1) and torch.equal(lp2, r2) and torch.equal(lpm, rm) and torch.equal(val, rv)


def _status(nets, n=32):
    from liuzhou_amd import _lib as L
    from liuzhou_amd.net_hip import DescArray
    packed = _packed(n, seed=1)
    seg = torch.tensor([0] + [n] * len(nets), dtype=torch.int64, device=DEV)
    outs = [torch.zeros((n, 36), device=DEV) for _ in range(3)] + [torch.zeros(n, device=DEV)]
    arr = DescArray(nets)
    with torch.cuda.device(DEV):
        rc = L.lib().lz_net_forward_packed_multi_f16(arr.arr, C.c_int32(len(arr)), L.ptr(packed), L.i64(n), L.ptr(seg),
                                                     L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), None, L.ptr(outs[3]),
                                                     L.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc


def test_networks_that_cannot_share_a_launch_are_refused():
    _need_gpu()
    from liuzhou_amd.net_hip import multi_compatible
    a, = _nets("b6c64", 1)
    b, = _nets("b10c128", 1)
    half, = _nets("b6c64", 1, half_workgroups=True)
    assert _status([a, b]) == -1 and not multi_compatible([a, b])            # LZ_ERR_ARG: another architecture
    assert _status([a, half]) == -1                                           # another kernel shape (flags bit 0)
    assert _status([a] * 9) == -1                                             # more than 8
    f32, = _nets("b6c64", 1, precision="fp32")
    x3, = _nets("b6c64", 1, precision="fp16x3")
    assert _status([a, f32]) == -2 and _status([x3]) == -2                    # LZ_ERR_UNSUPPORTED
    assert not multi_compatible([f32])
