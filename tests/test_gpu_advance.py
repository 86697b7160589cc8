"""GPU: lz_tree_advance (tree_advance_kernel of csrc/lz_engine.hip) on the hand-built arenas of tests/advance_cases.py,
written into the engine by tests/hand_arenas.py and held to the restatement and the verifier of tests/advance_ref.py
(DESIGN.md section 26).  Per launch: check_arena, upload, advance, read every buffer back, compare the WHOLE image with
`ref_advance` -- every byte the contract specifies, and every byte it leaves alone: chunk lists, records past n_nodes, the
0xA5 filler of the pool, the other games' chunks -- then `verify_advance`, which also checks the position index (its slots
follow the order of an atomic).  Fresh roots are compared with what lz_tree_begin leaves on a twin engine.

Everything here is integers and copied bits: there is no tolerance anywhere in this file.  No network and no search."""
import numpy as np
import pytest
import torch

from tests import advance_cases as K
from tests import advance_ref as R
from tests import hand_arenas as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ENGINES = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    _ENGINES.clear()


def engine_for(img, twin=False, solver=False):
    """One engine (and one twin) per engine shape and pool size: the launches of a shape reload it."""
    key = tuple(img[k] for k in H.SHAPE_KEYS) + (twin, solver)
    if key not in _ENGINES:
        _ENGINES[key] = H.ArenaEngine(img, DEV, solver=solver)
    return _ENGINES[key]


def launch_and_check(img, raw=False, counters=True, solver=False):
    """Upload, advance, read back; the whole image against the restatement, then the verifier.  Returns (got, want)."""
    assert H.check_arena(img, detached=[t == "fresh:no_child" for t in img.get("tags", [""] * img["B"])])
    want, counts = R.ref_advance(img)
    eng = engine_for(img, solver=solver)
    eng.load(img)
    if raw:
        rc, got_counts = eng.advance_raw(img, counters=counters)
        assert rc == 0
    else:
        got_counts = eng.advance(img)
    got = eng.read(img)
    print(f"dropped, pruned: device {got_counts}, restatement {counts}")
    assert got_counts == (counts if counters else (0, 0))
    bad = R.diff_images(want, got, img)
    assert bad == [], bad
    assert R.verify_advance(img, got)
    return got, want


LAUNCHES = [(s, i) for s in ("E1", "E2") for i in range(len(K.BUDGETS))] + [("E3", 0)]


@pytest.mark.parametrize("shape,i", LAUNCHES)
def test_advance_matches_the_restatement_on_hand_built_arenas(gpu, shape, i):
    name, img = K.launches(shape)[i]
    got, want = launch_and_check(img)
    # fresh roots: exactly what lz_tree_begin leaves for the same root states and active flags (twin engine)
    twin = engine_for(img, twin=True)
    twin.load(img)
    twin.engine.begin()
    began = twin.read(img)
    fresh = np.flatnonzero(got["leaf_kind"] != R.LEAF_REUSED_ROOT)
    assert len(fresh) == sum(i_["fresh"] for i_ in want["info"])
    for f in ("n_nodes", "n_edges", "n_chunks", "root_visits", "root_w", "root_init_value", "path_len", "root_terminal",
              "leaf_kind", "leaf_state", "leaf_value", "pos_index", "node_value"):
        a, b = np.ascontiguousarray(got[f][fresh]), np.ascontiguousarray(began[f][fresh])
        assert (a.view(np.uint8) == b.view(np.uint8)).all(), (name, f)
    a = np.ascontiguousarray(got["nodes"][fresh]).view(np.uint8).reshape(len(fresh), -1, 48)
    b = np.ascontiguousarray(began["nodes"][fresh]).view(np.uint8).reshape(len(fresh), -1, 48)
    assert (a[:, 0, :44] == b[:, 0, :44]).all() and (a[:, 1:] == b[:, 1:]).all(), name
    if len(fresh) == img["B"]:
        assert int(got["pool_stats"][2]) == int(began["pool_stats"][2])


def test_numpy_packer_matches_the_device_packer(gpu):
    from liuzhou_amd.tree_engine import TreeEngine
    from tests.tree_parity import to_gpu_batch
    st, packed, _ = H.fixture_rows()
    eng = TreeEngine(len(packed), 2, DEV, pool_chunks=len(packed))
    eng.set_roots(to_gpu_batch(st, DEV))
    torch.cuda.synchronize()
    assert np.array_equal(eng.buf["root_state"].cpu().numpy(), packed)


def test_three_advances_in_a_row_on_one_deep_tree(gpu):
    """Each advance starts from the image the device left (the second one cuts) and is compared with the restatement
    applied to that same image."""
    rng = np.random.default_rng(11)
    img = H.copy_image(K.chain_start())
    kept = []
    for step, next_sims in enumerate(K.CHAIN_NEXT_SIMS):
        img["next_sims"] = next_sims
        got, want = launch_and_check(img)
        kept.append([i_["kept"] for i_ in want["info"]])
        if step == 1:
            assert sum(i_["pruned"] for i_ in want["info"]) >= 1
        got.pop("info", None)
        img = H.next_move(got, rng)
        img["tags"] = [""] * img["B"]
    assert all(sum(k > 0 for k in ks) >= 3 for ks in kept), kept


def test_argument_error_changes_nothing(gpu):
    name, img = K.launches("E1")[1]
    eng = engine_for(img)
    eng.load(img)
    bad = H.copy_image(img)
    bad["next_sims"] = img["node_cap"]                              # next_sims + 1 > node_cap
    rc, counts = eng.advance_raw(bad)
    assert rc == -1 and counts == (0, 0)
    got = eng.read(img)
    for f in H.BUFFERS:
        assert (got[f].view(np.uint8) == img[f].view(np.uint8)).all(), f


def test_null_counters_and_null_played_action(gpu):
    name, img = K.launches("E1")[1]
    launch_and_check(img, raw=True, counters=False)                 # dropped and pruned both NULL
    every_fresh = H.copy_image(img)
    every_fresh["played"] = None                                    # played_action NULL: every game a fresh root
    every_fresh["reset"] = None
    got, want = launch_and_check(every_fresh, raw=True)
    assert all(i_["fresh"] for i_ in want["info"]) and (got["n_chunks"] == 0).all()
    assert int(got["pool_top"][0]) == img["pool_chunks"]


def test_solver_engine_gets_root_proven_zeroed(gpu):
    name, img = K.launches("E1")[2]
    eng = engine_for(img, solver=True)
    eng.engine.root_proven.fill_(3)
    launch_and_check(img, solver=True)
    assert eng.engine.root_proven.tolist() == [0] * img["B"]
