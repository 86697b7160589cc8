"""GPU: lz_tree_select and lz_tree_expand (tree_select / tree_expand of csrc/lz_tree_dev.h, the functions the fused
production step calls) on the hand-built launches of tests/step_cases.py, written into the engine by tests/hand_arenas.py
and held to the restatement of tests/step_ref.py.  Per step of a launch: check_step_arena, upload,
launch, read every buffer and side array back, compare the WHOLE image byte for byte -- other games, the 0xA5 filler,
records beyond n_nodes, path entries beyond path_len, chunk lists, counters.  The next step starts from the image the device
left.

No tolerance on the priors220 path.  The priors of a heads expansion are held to a float64 softmax under
step_ref.HEADS_TOL; every other field of such a record is exact.  No network and no search."""
import pytest
import torch

from tests import hand_arenas as H
from tests import step_cases as K
from tests import step_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ENGINES = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    _ENGINES.clear()


def engine_for(img):
    key = tuple(img[k] for k in H.SHAPE_KEYS)
    if key not in _ENGINES:
        _ENGINES[key] = H.ArenaEngine(img, DEV)
    return _ENGINES[key]


def run_launch(L):
    """Every step of a launch on the device, each compared with the restatement of the same input.  Returns the largest
    heads difference seen and the last image."""
    img, opts = L["img"], L["opts"]
    eng = engine_for(img)
    eng.set_options(opts)
    worst = 0.0
    for i, st in enumerate(L["steps"]):
        if st[0] == "hand":
            img = st[1](img)
            continue
        is_root = st[0] == "expand" and st[2]
        assert H.check_step_arena(img, "select" if st[0] == "select" else "root" if is_root else "expand")
        eng.load(img)
        eng.load_side(img)
        if st[0] == "select":
            eng.select()
        else:
            eng.expand(is_root, st[1])
        got = eng.read(img)
        got.update(eng.read_side(img))
        if st[0] == "select":
            want = R.ref_select(img, opts)
        else:
            want, soft = R.ref_expand(img, st[1], opts, is_root, taken=R.chunk_assignment(img, got))
            if soft:
                worst = max(worst, R.settle_heads(want, got, soft))
        bad = R.diff_step(want, got)
        if bad:
            print(L["name"], i, st[0], bad)
        assert bad == [], (L["name"], i, st[0], bad, [img["tags"][g] for g in range(img["B"])])
        img = got
    return worst, img


@pytest.mark.parametrize("name", K.NAMES)
def test_step_matches_the_restatement_on_hand_built_arenas(gpu, name):
    worst, _ = run_launch(K.launch(name))
    assert worst <= R.HEADS_TOL


@pytest.mark.parametrize("name", [n for n in K.NAMES if n in ("deep", "descent", "big_n", "expansion", "expansion_heads", "refusal")])
def test_single_precision_argmax_leaves_the_same_image(gpu, monkeypatch, name):
    """LZ_TREE_F32SEL=1: the image is the restatement's, which knows no single-precision path -- so it is the default run's."""
    L = K.launch(name)
    assert L["plain"]
    monkeypatch.setenv("LZ_TREE_F32SEL", "1")
    run_launch(L)
