"""Hand-built arenas for lz_tree_advance: the whole image of B games in one TreeEngine -- node records, edge runs, chunk
lists, the free-chunk stack, the root scalars and the position index -- written straight into the engine's buffers, the way
tests/hand_roots.py writes single roots for the read-out kernels.

The host half (`pack_states`, `make_tree`, `build_image`, `check_arena`, `next_move`) needs no GPU.  An image is a dict:
the engine's buffers by the names of `TreeEngine.buf` as numpy arrays, the launch arguments (`played`, `reset`,
`next_sims`) and the engine shape.  `check_arena` asserts everything a correct kernel relies on before anything is
uploaded, so a hand-made mistake cannot make a launch touch memory it does not own.  The device half (`ArenaEngine`)
uploads exactly the image, launches, and reads every buffer back as one image.

The second half of the file does the same for the tree step, lz_tree_select / lz_tree_expand:
`StepGame`, `build_step_image`, `check_step_arena`, and `ArenaEngine.select` / `expand`.

Record layouts: EDGE_DT / NODE_DT of tests/tree_parity.py (include/liuzhou_hip.h)."""
import numpy as np

from tests.golden_utils import FIELDS, load, states
from tests.readout_ref import game_status

EDGE_DT = np.dtype([("W", "<f8"), ("P", "<f4"), ("n_info", "<u4"), ("child", "<i4"), ("cbegin", "<i4"), ("act", "u1"),
                    ("cn", "u1"), ("pad", "V6")])                       # == tests/tree_parity.EDGE_DT (no torch import here)
NODE_DT = np.dtype([("state", "<i8", (4,)), ("edge_begin", "<i4"), ("nedges", "<i4"), ("parent", "<i4"), ("old_begin", "<i4")])
MAX_CHILDREN = 72
FILL = 0xA5
FULL = (1 << 36) - 1
INFO_TERMINAL = 2
WAVE = 64
PATH_CAP = 192
# the engine's buffers an image holds: name -> (dtype, shape as a function of the engine shape)
BUFFERS = {
    "root_state": ("<i8", lambda s: (s["B"], 4)), "nodes": (NODE_DT, lambda s: (s["B"], s["node_cap"])),
    "edges": (EDGE_DT, lambda s: (s["pool_chunks"] * s["chunk"],)),
    "n_nodes": ("<i4", lambda s: (s["B"],)), "n_edges": ("<i4", lambda s: (s["B"],)),
    "root_visits": ("<i4", lambda s: (s["B"],)), "root_w": ("<f8", lambda s: (s["B"],)),
    "root_init_value": ("<f4", lambda s: (s["B"],)), "path": ("<i4", lambda s: (s["B"] * s["path_cap"],)),
    "path_len": ("<i4", lambda s: (s["B"],)), "leaf_kind": ("<i4", lambda s: (s["B"],)),
    "leaf_state": ("<i8", lambda s: (s["B"], 4)), "leaf_value": ("<f4", lambda s: (s["B"],)),
    "root_terminal": ("u1", lambda s: (s["B"],)), "active": ("u1", lambda s: (s["B"],)),
    "leaf_edge": ("<i4", lambda s: (s["B"],)), "leaf_parent": ("<i4", lambda s: (s["B"],)),
    "chunk_list": ("<i4", lambda s: (s["B"], s["chunk_cap"])), "n_chunks": ("<i4", lambda s: (s["B"],)),
    "free_chunks": ("<i4", lambda s: (s["pool_chunks"],)), "pool_top": ("<i4", lambda s: (1,)),
    "pool_stats": ("<i4", lambda s: (3,)), "pos_index": ("<i4", lambda s: (s["B"], s["pos_slots"])),
    "node_value": ("<f4", lambda s: (s["B"], s["node_cap"])), "leaf_src": ("<i4", lambda s: (s["B"],)),
}
SHAPE_KEYS = ("B", "node_cap", "chunk", "chunk_cap", "pool_chunks", "pos_slots", "path_cap")


# ---- states -----------------------------------------------------------------------------------------------------------
def pack_states(st):
    """State dict of numpy arrays -> int64[B, 4] packed records: the inverse of tests/tree_parity.unpack_packed
    (csrc/lz_rules.h pack)."""
    board = np.asarray(st["board"]).astype(np.int64)
    B = board.shape[0]
    sh = np.arange(36, dtype=np.uint64)[None, :]
    bits = lambda m: (np.asarray(m).reshape(B, 36).astype(np.uint64) << sh).sum(1, dtype=np.uint64)
    f = lambda name, mask, shift: (np.asarray(st[name]).astype(np.int64).astype(np.uint64) & np.uint64(mask)) << np.uint64(shift)
    w0 = bits(board == 1) | f("move_count", 0xFF, 36) | f("moves_since_capture", 0x3F, 44) | f("phase", 7, 50) | \
        ((np.asarray(st["current_player"]).astype(np.int64) < 0).astype(np.uint64) << np.uint64(53)) | \
        f("forced_removals_done", 3, 54) | f("pending_marks_required", 3, 56) | f("pending_marks_remaining", 3, 58) | \
        f("pending_captures_required", 3, 60) | f("pending_captures_remaining", 3, 62)
    out = np.stack([w0, bits(board == -1), bits(st["marks_black"]), bits(st["marks_white"])], axis=1)
    return np.ascontiguousarray(out).view(np.int64)


def packed_status(w0, w1):
    """game_status (csrc/lz_rules.h) of a packed record, from its first two words as Python integers."""
    w0, w1 = int(w0) & (2 ** 64 - 1), int(w1) & (2 ** 64 - 1)
    return game_status((w0 >> 50) & 7, bin(w0 & FULL).count("1"), bin(w1 & FULL).count("1"), (w0 >> 36) & 0xFF, (w0 >> 44) & 0x3F)


_FIX = {}


def fixture_rows():
    """(state dict, packed int64[N, 4], status[N]) of the positions of tests/golden/g1_rules.npz."""
    if not _FIX:
        st = {k: np.asarray(v) for k, v in states(load("g1_rules.npz"), "s").items()}
        p = pack_states(st)
        _FIX["v"] = (st, p, np.array([packed_status(a, b) for a, b in p[:, :2]]))
    return _FIX["v"]


def node_states(rng, nn, game, open_only=True):
    """nn distinct packed states: the board words of fixture positions, made distinct by their mark words (w2 holds the
    node id, w3 the game and random bits) -- advance only hashes and compares node states."""
    _, p, status = fixture_rows()
    rows = np.flatnonzero(status == 0) if open_only else np.arange(len(p))
    s = p[rows[(game * 131 + np.arange(nn) * 7) % len(rows)]].copy()
    s[:, 2] = np.arange(nn, dtype=np.int64) | (rng.integers(0, 1 << 18, nn) << 18)
    s[:, 3] = (game & 0xFFF) | (rng.integers(0, 1 << 23, nn) << 12)
    return s


# ---- trees ------------------------------------------------------------------------------------------------------------
def members_by_word(rng, nn, c, counts):
    """Membership mask with counts[k] members in word (c // 64 + k), `c` itself counted in the first; members are ids > c."""
    m = np.zeros(nn, bool)
    m[c] = True
    for k, cnt in enumerate(counts):
        w = c // WAVE + k
        lo, hi = max(w * WAVE, c + 1), min((w + 1) * WAVE, nn)
        want = cnt - (1 if k == 0 else 0)
        assert 0 <= want <= max(hi - lo, 0), (k, cnt, lo, hi)
        if want:
            m[rng.choice(np.arange(lo, hi), want, replace=False)] = True
    return m


def make_tree(rng, nn, c, member, ne, mode="recent", window=6, force_parent=None):
    """Parents for nn nodes: node c hangs from the root, a member (ids > c) from an earlier member, every other node from
    the root or an earlier non-member; no node gets more children than its `ne` edges.  mode: 'chain' the latest node of
    the class with room, 'recent' one of the last `window` with room."""
    member = np.asarray(member, bool)
    assert member[c] and not member[:c].any() and 1 <= c < nn
    ne = np.asarray(ne, np.int64)
    room = np.maximum(ne, 0).copy()
    parent = np.full(nn, -1, np.int64)
    open_in, open_out = [], [0]                                  # nodes that may still have room (checked when drawn)
    room[0] -= 1                                                 # the played edge
    assert room[0] >= 0
    force_parent = force_parent or {}
    for i in range(1, nn):
        if i == c:
            parent[i] = 0
        else:
            lst = open_in if member[i] else open_out
            if i in force_parent:
                p = force_parent[i]
                assert member[p] == member[i] or (p == 0 and not member[i])
            else:
                while True:
                    assert lst, f"no parent with room for node {i}"
                    j = len(lst) - 1 - (0 if mode == "chain" else int(rng.integers(0, min(window, len(lst)))))
                    p = lst[j]
                    if room[p] > 0:
                        break
                    del lst[j]
            assert room[p] > 0, (i, p)
            parent[i] = p
            room[p] -= 1
        if room[i] > 0:
            (open_in if member[i] else open_out).append(i)
    return parent


def game(tag, nn, c, member, ne, rng, mode="recent", window=6, force_parent=None, **opts):
    """A game spec: the tree plus what `build_image` reads (see there)."""
    ne = np.asarray(ne, np.int64).copy()
    if isinstance(member, str):
        assert member == "all"
        member = np.arange(nn) >= c
    g = dict(tag=tag, nn=nn, c=c, ne=ne, member=np.asarray(member, bool),
             parent=make_tree(rng, nn, c, member, ne, mode, window, force_parent))
    g.update(opts)
    return g


# ---- the image --------------------------------------------------------------------------------------------------------
def engine_shape(B, node_cap, chunk, pool_chunks):
    from liuzhou_amd.tree_engine import chunk_cap_for, pos_slots_for
    return dict(B=B, node_cap=node_cap, chunk=chunk, chunk_cap=chunk_cap_for(node_cap, chunk), pool_chunks=pool_chunks,
                pos_slots=pos_slots_for(node_cap), path_cap=min(node_cap + 1, PATH_CAP))


def greedy_layout(ne, chunk):
    """Where the expand step's greedy rule puts the runs of nodes 0 .. nn-1: (chunk index in the game's list, offset) per
    node (-1 for a node without records), the chunks used and the final cursor."""
    ci, off = -1, chunk
    where = np.full((len(ne), 2), -1, np.int64)
    for i, n in enumerate(ne):
        n = int(n)
        if n <= 0:
            continue
        if off + n > chunk:
            ci, off = ci + 1, 0
        where[i] = (ci, off)
        off += n
    return where, ci + 1, off


def blank_image(shape, fill=FILL):
    img = {k: int(shape[k]) for k in SHAPE_KEYS}
    for name, (dt, shp) in BUFFERS.items():
        a = np.full(int(np.prod(shp(img))) * np.dtype(dt).itemsize, fill, np.uint8)
        img[name] = a.view(dt).reshape(shp(img))
    return img


def copy_image(img):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in img.items()}


def build_image(games, node_cap, chunk, next_sims, seed, spare_chunks=5):
    """The image of `games` (specs of `game`) in one engine.  Per spec, beyond the tree: `played_slot` (index of the played
    edge in the root's run), `played_n_info`, `played_W`, `twins` [(a, b)]: node b gets node a's state, `list_order`
    ('rand' / 'asc' / 'desc'), `fresh`: None or the reason the game must come out as a fresh root."""
    rng = np.random.default_rng(seed)
    B = len(games)
    lay = [greedy_layout(g["ne"], chunk) for g in games]
    need = sum(l[1] for l in lay)
    shape = engine_shape(B, node_cap, chunk, need + spare_chunks)
    img = blank_image(shape)
    img["active"][:] = 1
    img["root_terminal"][:] = 0
    img["played"] = np.zeros(B, np.int32)
    img["reset"] = np.zeros(B, np.uint8)
    img["next_sims"] = int(next_sims)
    img["tags"] = [g["tag"] for g in games]
    img["expect"] = [g.get("expect") for g in games]
    perm = rng.permutation(shape["pool_chunks"]).astype(np.int32)
    taken = 0
    edges = img["edges"]
    for gi, g in enumerate(games):
        nn, c, ne, parent = g["nn"], g["c"], g["ne"], g["parent"]
        where, nch, off = lay[gi]
        ids = perm[taken:taken + nch].copy()
        taken += nch
        order = g.get("list_order", "rand")
        if order != "rand":
            ids.sort()
            ids = ids[::-1].copy() if order == "desc" else ids
        img["chunk_list"][gi, :nch] = ids
        img["n_chunks"][gi] = nch
        begin = np.where(where[:, 0] >= 0, ids[np.maximum(where[:, 0], 0)].astype(np.int64) * chunk + where[:, 1], 0) \
            if nch else np.zeros(nn, np.int64)
        img["n_nodes"][gi] = nn
        img["n_edges"][gi] = int(ids[nch - 1]) * chunk + off if nch else 0
        rec = np.zeros(nn, NODE_DT)
        st = node_states(rng, nn, gi)
        for a, b in g.get("twins", ()):
            st[b] = st[a]
        rec["state"], rec["edge_begin"], rec["nedges"], rec["parent"] = st, begin, ne, parent
        rec["old_begin"] = rng.integers(0, 1 << 20, nn)
        img["nodes"][gi, :nn] = rec
        img["node_value"][gi, :nn] = rng.uniform(-1, 1, nn).astype(np.float32)
        # edge runs: random logical fields, distinct actions inside a run
        cnt = np.maximum(ne, 0)
        tot = int(cnt.sum())
        owner = np.repeat(np.arange(nn), cnt)
        k_in = np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        pos = begin[owner] + k_in
        run = np.zeros(tot, EDGE_DT)
        run["W"] = rng.normal(0, 3, tot)
        run["W"][rng.random(tot) < 0.05] = -0.0
        run["P"] = rng.random(tot, np.float32)
        info = rng.choice(np.array([0, 1, 4, 5, 8, 9, 16, 17, 24, 25], np.uint32), tot)
        run["n_info"] = rng.integers(0, 1 << 12, tot).astype(np.uint32) | (info << 24)
        run["child"] = -1
        run["cbegin"] = rng.integers(0, 1 << 16, tot)              # of an edge without a child: garbage, copied as it is
        run["cn"] = rng.integers(0, 73, tot)
        act_base = rng.integers(0, 220, nn)
        run["act"] = (act_base[owner] + k_in * 3) % 220                # 3 and 220 are coprime: distinct for k < 220
        run.view(np.uint8).reshape(tot, 32)[:, 26:] = rng.integers(0, 256, (tot, 6), dtype=np.uint8)
        # child links: the children of a node take random slots of its run; the played child takes `played_slot`
        start = np.cumsum(cnt) - cnt
        kids = [[] for _ in range(nn)]
        for i in range(1, nn):
            kids[parent[i]].append(i)
        pslot = g.get("played_slot")
        for p_, ch in enumerate(kids):
            if not ch:
                continue
            n_ = int(cnt[p_])
            if p_ == 0 and pslot is not None:
                rest = [s for s in rng.permutation(n_).tolist() if s != pslot][:len(ch) - 1]
                slots = {c: pslot}
                for s, k in zip(rest, [k for k in ch if k != c]):
                    slots[k] = s
            else:
                slots = dict(zip(ch, rng.choice(n_, len(ch), replace=False).tolist()))
            for k, s in slots.items():
                e = start[p_] + s
                run["child"][e], run["cbegin"][e], run["cn"][e] = k, begin[k] if ne[k] > 0 else 0, max(int(ne[k]), 0)
        # terminal bits only on edges without a child (the expand step never hangs a node from a terminal edge)
        term = (run["child"] < 0) & (rng.random(tot) < 0.2)
        run["n_info"][term] |= np.uint32(INFO_TERMINAL << 24)
        pe = int(np.flatnonzero((owner == 0) & (run["child"] == c))[0]) if cnt[0] > 0 else -1
        if pe >= 0:
            if "played_n_info" in g:
                run["n_info"][pe] = g["played_n_info"]
            if "played_W" in g:
                run["W"][pe] = g["played_W"]
        img["root_state"][gi] = st[c]
        img["played"][gi] = int(run["act"][pe]) if pe >= 0 else 0
        img["root_visits"][gi] = int(rng.integers(1, 1 << 20))
        img["root_w"][gi] = float(rng.normal(0, 50))
        fresh = g.get("fresh")
        if fresh == "reset":
            img["reset"][gi] = 1
        elif fresh == "played_negative":
            img["played"][gi] = -1
        elif fresh == "played_absent":
            used = set(run["act"][owner == 0].tolist())
            img["played"][gi] = next(a for a in range(220) if a not in used)
        elif fresh == "no_child":                                  # the played edge never got a node: node c hangs elsewhere
            assert g.get("c_detached")
        elif fresh == "terminal_bit":
            run["n_info"][pe] |= np.uint32(INFO_TERMINAL << 24)
        elif fresh == "state_w3":
            img["root_state"][gi, 3] ^= 1 << 35
        elif fresh == "root_terminal":
            img["root_terminal"][gi] = 1
        elif fresh == "inactive":
            img["active"][gi] = 0
        elif fresh == "root_over":                                 # the host moved to a finished position
            st[c, 0] = (int(st[c, 0]) & ~(0xFF << 36)) | (200 << 36)     # move_count past the limit: a draw (no fixture row is over)
            assert packed_status(st[c, 0], st[c, 1]) == 2
            img["nodes"]["state"][gi, c] = st[c]
            img["root_state"][gi] = st[c]
            img["reset"][gi] = 1
        else:
            assert fresh is None or fresh.startswith("root_ne"), fresh
        if g.get("c_detached"):                                    # "child = -1": the played edge loses its link
            run["child"][pe] = -1
        if g.get("duplicate_action"):                              # a later root edge repeats the played action: the first counts
            other = int(np.flatnonzero(owner == 0)[-1])
            if other != pe and other > pe:
                run["act"][other] = run["act"][pe]
        edges[pos] = run
    img["free_chunks"][:shape["pool_chunks"] - taken] = perm[taken:]
    img["pool_top"][0] = shape["pool_chunks"] - taken
    img["pool_stats"][:] = (0, shape["pool_chunks"], pending_count(img))
    img["pos_index"][:] = 7                                         # stale entries: advance clears every table
    check_arena(img, detached=[bool(g.get("c_detached")) for g in games])
    return img


def pending_count(img):
    """Games whose root is a fresh root that has not expanded yet (lz_tree_dev.h root_pending)."""
    return int(((img["n_nodes"] == 1) & (img["nodes"][:, 0]["nedges"] < 0) & (img["root_terminal"] == 0)).sum())


def run_indices(begin, cnt):
    """Concatenated pool indices of the runs (begin[i], cnt[i]) and the owner of each record."""
    cnt = np.maximum(np.asarray(cnt, np.int64), 0)
    owner = np.repeat(np.arange(len(cnt)), cnt)
    k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return np.asarray(begin, np.int64)[owner] + k, owner


def check_arena(img, detached=None):
    """Everything a correct lz_tree_advance relies on, asserted on the image alone (see the module docstring)."""
    B, cap, chunk, pool = img["B"], img["node_cap"], img["chunk"], img["pool_chunks"]
    assert chunk >= 128 and chunk & (chunk - 1) == 0 and img["pos_slots"] & (img["pos_slots"] - 1) == 0
    assert img["chunk_cap"] * (chunk - (MAX_CHILDREN - 1)) >= cap * MAX_CHILDREN           # lz_tree_advance's own condition
    for name, (dt, shp) in BUFFERS.items():
        assert img[name].dtype == np.dtype(dt) and img[name].shape == shp(img), name
    assert all(img[k] is None or img[k].shape == (B,) for k in ("played", "reset")) and 0 <= img["next_sims"]
    top = int(img["pool_top"][0])
    assert 0 <= top <= pool
    owned = [img["chunk_list"][g, :int(img["n_chunks"][g])] for g in range(B)]
    assert all(0 <= int(img["n_chunks"][g]) <= img["chunk_cap"] for g in range(B))
    every = np.concatenate(owned + [img["free_chunks"][:top]]).astype(np.int64)
    assert len(every) <= pool and (every >= 0).all() and (every < pool).all(), "chunk id outside the pool"
    assert len(np.unique(every)) == len(every), "a chunk is owned twice"
    assert top + sum(len(o) for o in owned) <= pool                  # room on the stack for every release
    assert int(img["pool_stats"][2]) == pending_count(img)
    for g in range(B):
        nn = int(img["n_nodes"][g])
        assert 1 <= nn <= cap, (g, nn)
        nd = img["nodes"][g, :nn]
        ne, parent, begin = nd["nedges"].astype(np.int64), nd["parent"].astype(np.int64), nd["edge_begin"].astype(np.int64)
        assert parent[0] == -1 and (parent[1:] >= 0).all() and (parent[1:] < np.arange(1, nn)).all(), (g, "parent order")
        assert (ne >= -1).all() and (ne <= MAX_CHILDREN).all(), (g, "nedges")
        # the greedy layout along the game's own chunk list, and its cursor
        where, nch, off = greedy_layout(ne, chunk)
        assert nch == len(owned[g]), (g, "n_chunks is not what the greedy rule uses", nch, len(owned[g]))
        has = ne > 0
        want = owned[g][np.maximum(where[:, 0], 0)].astype(np.int64) * chunk + where[:, 1] if nch else begin
        assert (begin[has] == want[has]).all(), (g, "run not where the greedy rule puts it")
        assert (begin[has] // chunk == (begin[has] + ne[has] - 1) // chunk).all(), (g, "run straddles a chunk")
        assert int(img["n_edges"][g]) == (int(owned[g][-1]) * chunk + off if nch else 0), (g, "n_edges")
        idx, owner = run_indices(begin, ne)
        run = img["edges"][idx]
        ch = run["child"].astype(np.int64)
        k = ch >= 0
        assert ((ch[k] >= 1) & (ch[k] < nn)).all(), (g, "child id")
        assert (parent[ch[k]] == owner[k]).all(), (g, "parent link does not point back")
        assert (run["cn"][k] == np.maximum(ne[ch[k]], 0)).all(), (g, "cn")
        kk = k.copy()
        kk[k] = ne[ch[k]] > 0
        assert (run["cbegin"][kk] == begin[ch[kk]]).all(), (g, "cbegin")
        seen = np.bincount(ch[k], minlength=nn)
        lost = np.flatnonzero(seen[1:] != 1) + 1
        if detached is not None and detached[g]:
            assert len(lost) == 1 and seen[lost[0]] == 0
        else:
            assert len(lost) == 0, (g, "node without exactly one incoming edge", lost[:5])
        # The restatement's packing never runs past the chunk list: it packs a subsequence of these runs by the same greedy
        # rule, which is never ahead of packing all of them (induction over the runs: the cursor of the subsequence is at
        # or before the cursor of the whole), and the whole uses exactly the nch chunks asserted above.  A kept game has a
        # root run, so nch >= 1 covers the cursor's start in chunk 0; ref_advance asserts it once more while it packs.
        assert nch >= 1 or ne[0] <= 0
    return True


def next_move(img, rng):
    """A next launch on the image a launch left: per game the action of a root edge with a child (the one whose child id is
    smallest), the child's state as the state the host moved to; games without one get played = -1."""
    out = copy_image(img)
    for g in range(img["B"]):
        nd = img["nodes"][g, 0]
        ne, e0 = int(nd["nedges"]), int(nd["edge_begin"])
        out["played"][g] = -1
        if ne > 0 and int(img["n_nodes"][g]) > 1:
            run = img["edges"][e0:e0 + ne]
            ok = np.flatnonzero((run["child"] > 0) & ((run["n_info"] >> 24) & INFO_TERMINAL == 0))
            if len(ok):
                k = ok[int(rng.integers(0, len(ok)))]
                out["played"][g] = int(run["act"][k])
                out["root_state"][g] = img["nodes"][g, int(run["child"][k])]["state"]
    out["reset"] = np.zeros(img["B"], np.uint8)
    return out


# ---- the device half --------------------------------------------------------------------------------------------------
class ArenaEngine:
    """A TreeEngine of the image's shape; `load` uploads exactly an image, `read` reads every buffer back as one."""

    def __init__(self, img, device, solver=False):
        from liuzhou_amd.tree_engine import TreeEngine
        eng = TreeEngine(img["B"], img["node_cap"] - 2, device, edge_chunk=img["chunk"], pool_chunks=img["pool_chunks"])
        assert (eng.node_cap, eng.chunk_cap, eng.path_cap) == (img["node_cap"], img["chunk_cap"], img["path_cap"])
        assert int(eng.desc.pos_slots) == img["pos_slots"]
        self.engine, self.dev, self.shape = eng, device, {k: img[k] for k in SHAPE_KEYS}
        if solver:
            eng.set_solver(True)

    def load(self, img):
        import torch
        assert all(img[k] == v for k, v in self.shape.items())
        for name in BUFFERS:
            t = self.engine.buf[name]
            a = np.ascontiguousarray(img[name])
            assert a.nbytes == t.numel() * t.element_size(), name
            t.view(torch.uint8).view(-1).copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)).to(self.dev))
        self.engine.reuse_dropped.zero_()
        torch.cuda.synchronize()

    def read(self, like):
        import torch
        torch.cuda.synchronize()
        out = {k: v for k, v in like.items() if k not in BUFFERS}
        for name, (dt, shp) in BUFFERS.items():
            raw = self.engine.buf[name].view(torch.uint8).view(-1).cpu().numpy()
            out[name] = raw.view(dt).reshape(shp(like)).copy()
        return out

    def advance(self, img):
        """Launch on what is loaded with the image's launch arguments (TreeEngine.advance); returns (dropped, pruned)."""
        import torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.engine.advance(up(img["played"]), up(img["reset"]), next_sims=img["next_sims"])
        torch.cuda.synchronize()
        return tuple(int(v) for v in self.engine.reuse_dropped.tolist())

    def advance_raw(self, img, counters=True):
        """The same launch through the C ABI, for what TreeEngine.advance cannot say: `played` / `reset` of None go down
        as NULL, and so do both counters with counters=False.  Returns (status, (dropped, pruned))."""
        import ctypes as C
        import torch
        from liuzhou_amd import _lib as L
        eng = self.engine
        keep = [None if img[k] is None else torch.from_numpy(np.ascontiguousarray(img[k])).to(self.dev) for k in ("played", "reset")]
        cnt = eng.reuse_dropped
        with torch.cuda.device(self.dev):
            rc = L.lib().lz_tree_advance(C.byref(eng.desc), L.ptr(keep[0]), L.ptr(keep[1]), L.i64(img["next_sims"]),
                                         L.ptr(cnt[0:1]) if counters else None, L.ptr(cnt[1:2]) if counters else None,
                                         L.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return int(rc), tuple(int(v) for v in cnt.tolist())

    def select(self):
        import torch
        self.engine.select()
        torch.cuda.synchronize()

    def expand(self, is_root, rows):
        """rows: values float32[B], either priors220 float32[B, 220] or heads (three float32[B, 36]), noise float32[B, 72] or
        None, epsilon."""
        import torch
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.dev)
        heads = None if rows.get("heads") is None else tuple(up(h) for h in rows["heads"])
        self.engine.expand(is_root=is_root, values=up(rows["values"]), heads=heads, priors220=up(rows.get("priors220")),
                           noise=up(rows.get("noise")), epsilon=float(rows.get("epsilon", 0.25)))
        torch.cuda.synchronize()

    def set_options(self, opts):
        """The search options of a launch (tests/step_ref.py `options`) on the engine: c_puct, forced playouts, the solver,
        the PUCT shape."""
        eng = self.engine
        eng.desc.exploration_weight = float(opts["c_puct"])
        eng.set_forced_playouts(float(opts["forced_k"]))
        eng.set_solver(bool(opts["solver"]))
        log, base, length = opts["cpuct"] or (0.0, 1.0, 2)
        eng.set_puct_shape(opts["fpu"], opts["fpu_root"], cpuct_log=log, cpuct_base=base, table_len=length)
        # every side array the step can write is there to be loaded and compared
        assert all(getattr(eng, k, None) is not None for k in ("forced_count", "share_count", "eval_count"))
        assert not opts["solver"] or (eng.root_proven is not None and eng.solver_count is not None)
        self.solver = bool(opts["solver"])

    def load_side(self, img):
        import torch
        for name in SIDE:
            t = getattr(self.engine, name, None)
            assert t is not None or (name in SIDE_SOLVER and not self.solver), name
            if t is not None:
                t.copy_(torch.from_numpy(np.ascontiguousarray(img[name])).to(self.dev))
        torch.cuda.synchronize()

    def read_side(self, like):
        """The side arrays as they stand.  Only root_proven and solver_count may be missing, and only while the solver is
        off (the engine allocates them when it is first switched on): they then come back as they were loaded, since the
        descriptor holds no pointer through which a kernel could write them."""
        out = {}
        for name in SIDE:
            t = getattr(self.engine, name, None)
            assert t is not None or (name in SIDE_SOLVER and not self.solver), name
            out[name] = like[name].copy() if t is None else t.cpu().numpy().astype(np.int32)
        return out


# =======================================================================================================================
# The tree STEP (lz_tree_select / lz_tree_expand): real skeletons with hand statistics.
# Node states are real positions, a node's run holds exactly the oracle's legal actions of its state in ascending order, a
# child's state is the oracle's successor; W, P, N, the proven bits and node_value are chosen per case.  Runs that no legal
# position can have (65 to 72 edges, or ballast of a chosen length) are SYNTHETIC: every edge of such a run is terminal or
# leads to a node with a real state, so no descent can end on it as an expandable leaf and no action of it is ever applied.
# =======================================================================================================================
M64 = (1 << 64) - 1
INFO_WHITE, INFO_PROVEN, INFO_DECIDED = 1, 16, 18
LEAF_INACTIVE, LEAF_EXPAND, LEAF_TERMINAL, LEAF_REUSED_ROOT, LEAF_SHARED = 0, 1, 2, 3, 4
PATH_FLIP = 0x80000000
# the counters and side arrays the step writes that are not engine buffers: name -> attribute of TreeEngine
SIDE = ("root_proven", "solver_count", "forced_count", "share_count", "eval_count")
SIDE_SOLVER = ("root_proven", "solver_count")                          # exist once the solver has been switched on
SIDE_PRESET = {"root_proven": 0, "solver_count": 1000, "forced_count": 2000, "share_count": 3000, "eval_count": 4000}


def cs_from_packed(p):
    """Packed record (4 words) -> oracle CState (csrc/lz_rules.h unpack)."""
    from oracle import lz_oracle as O
    w = [int(v) & M64 for v in p]
    cs = O.CState()
    for i in range(36):
        cs.board[i] = 1 if (w[0] >> i) & 1 else (-1 if (w[1] >> i) & 1 else 0)
        cs.mb[i], cs.mw[i] = (w[2] >> i) & 1, (w[3] >> i) & 1
    w0 = w[0]
    cs.move_count, cs.msc, cs.phase = (w0 >> 36) & 0xFF, (w0 >> 44) & 0x3F, (w0 >> 50) & 7
    cs.player = -1 if (w0 >> 53) & 1 else 1
    cs.forced, cs.pm_req, cs.pm_rem, cs.pc_req, cs.pc_rem = ((w0 >> s) & 3 for s in (54, 56, 58, 60, 62))
    return cs


def packed_from_cs(cs):
    """Oracle CState -> packed record int64[4] (csrc/lz_rules.h pack)."""
    w = [0, 0, 0, 0]
    for i in range(36):
        w[0] |= (1 << i) if cs.board[i] == 1 else 0
        w[1] |= (1 << i) if cs.board[i] == -1 else 0
        w[2] |= (1 << i) if cs.mb[i] else 0
        w[3] |= (1 << i) if cs.mw[i] else 0
    w[0] |= (cs.move_count & 0xFF) << 36 | (cs.msc & 0x3F) << 44 | (cs.phase & 7) << 50 | (1 << 53 if cs.player < 0 else 0)
    w[0] |= (cs.forced & 3) << 54 | (cs.pm_req & 3) << 56 | (cs.pm_rem & 3) << 58 | (cs.pc_req & 3) << 60 | (cs.pc_rem & 3) << 62
    return np.array(w, np.uint64).view(np.int64)


def edge_info_for(succ):
    """Info byte the expand step gives the edge to `succ`: the white bit, and the terminal mark with the value for succ's
    mover when the game is over there."""
    from oracle import lz_oracle as O
    info = INFO_WHITE if succ.player < 0 else 0
    st = O.game_status(succ)
    if st != 0:
        tv = (1 if st == succ.player else -1) if st in (1, -1) else 0
        info |= INFO_TERMINAL | ((tv + 1) << 2)
    return info


def playout(seed, start=None, plies=400):
    """A line of real positions: seeded uniform random play with the oracle from `start` (the initial position) until the
    game is over or a position has no legal move.  Returns (states, actions); len(states) == len(actions) + 1."""
    from oracle import lz_oracle as O
    rng = np.random.default_rng(seed)
    c = start if start is not None else O.state_from_batch(O.initial_states(1), 0)
    line, acts = [c], []
    while O.game_status(c) == 0 and len(acts) < plies:
        la = O.legal_indices_py(c)
        if not la:
            break
        a = la[int(rng.integers(len(la)))]
        c = O.apply_index(c, a)
        line.append(c)
        acts.append(a)
    return line, acts


class StepGame:
    """One game of a step image: nodes in expansion order, each with its run.  `real` runs come from the oracle, `synthetic`
    ones are written by hand under the rule above."""

    def __init__(self, tag, root, fresh=False, **scalars):
        self.tag, self.nodes, self.fresh = tag, [], fresh
        self.scalars = dict(root_visits=3, root_w=0.0, root_init_value=0.0, active=1, root_terminal=0)
        self.scalars.update(scalars)
        self.root = root
        self.index_skip = set()
        if not fresh:
            self._add(root, -1, None)

    def _add(self, cs, parent, acts, synthetic=False):
        from oracle import lz_oracle as O
        if acts is None:
            acts = O.legal_indices_py(cs)
            succ = [O.apply_index(cs, a) for a in acts]
            info = [edge_info_for(s) for s in succ]
        else:
            succ, info = [None] * len(acts), [0] * len(acts)
        n = len(acts)
        assert n > 0, "a node in the arena has a run"
        self.nodes.append(dict(cs=cs, parent=parent, act=np.array(acts, np.uint8), succ=succ, synthetic=synthetic,
                               W=np.zeros(n), P=np.full(n, np.float32(1.0) / np.float32(n), np.float32),
                               N=np.zeros(n, np.int64), info=np.array(info, np.uint8), child=np.full(n, -1, np.int64),
                               value=np.float32(0.0)))
        return len(self.nodes) - 1

    def slot_of(self, node, action):
        return int(np.flatnonzero(self.nodes[node]["act"] == action)[0])

    def child(self, node, slot, value=0.0):
        """Hang the real successor of (node, slot) as a new node; returns its id."""
        nd = self.nodes[node]
        assert not nd["synthetic"] and nd["child"][slot] < 0 and not nd["info"][slot] & INFO_TERMINAL
        i = self._add(nd["succ"][slot], node, None)
        nd["child"][slot] = i
        self.nodes[i]["value"] = np.float32(value)
        return i

    def synthetic(self, node, slot, n, terminal_values, white=None):
        """Hang a node with a synthetic run of n edges under the real edge (node, slot): its state is the real successor,
        its edges carry distinct action bytes and are all terminal (value terminal_values[k % len]); `attach` then gives
        chosen edges a child with a real state."""
        nd = self.nodes[node]
        cs = nd["succ"][slot]
        i = self._add(cs, node, [(7 + 3 * k) % 220 for k in range(n)], synthetic=True)
        nd["child"][slot] = i
        me = self.nodes[i]
        for k in range(n):
            tv = terminal_values[k % len(terminal_values)]
            w = (k % 2 == 0) if white is None else white
            me["info"][k] = (INFO_WHITE if w else 0) | INFO_TERMINAL | ((tv + 1) << 2)
        return i

    def attach(self, node, slot, cs, value=0.0):
        """Give edge (node, slot) of a synthetic run a child node with the real state `cs` (and its real run)."""
        nd = self.nodes[node]
        assert nd["synthetic"]
        i = self._add(cs, node, None)
        nd["child"][slot] = i
        nd["info"][slot] = INFO_WHITE if cs.player < 0 else 0
        self.nodes[i]["value"] = np.float32(value)
        return i

    def set(self, node, slot, **kw):
        for k, v in kw.items():
            self.nodes[node][k][slot] = v

    def steer(self, node, slot, q=0.9, n=3):
        """Statistics that make (node, slot) the clear PUCT choice: n visits with mean q for the node's mover."""
        nd = self.nodes[node]
        same = (-1 if nd["info"][slot] & INFO_WHITE else 1) == nd["cs"].player
        nd["N"][slot], nd["W"][slot] = n, (q if same else -q) * n

    def line(self, acts, q=0.9, n=3, values=None):
        """Hang the chain of `acts` below the root and steer every level along it; returns [(node, slot)] per level.  The
        last edge gets no node."""
        node, out = 0, []
        for j, a in enumerate(acts):
            s = self.slot_of(node, a)
            self.steer(node, s, q, n)
            out.append((node, s))
            if j + 1 < len(acts):
                node = self.child(node, s, value=0.0 if values is None else values[j])
        return out


def build_step_image(games, node_cap, chunk, seed, spare_chunks=6, stale_index=True):
    """The image of StepGames in one engine: layout, chunk lists, 0xA5 filler and stale tables as in `build_image`; the
    position index holds every non-root node with a real state that the game does not ask to leave out (`index_skip`)."""
    from tests.advance_ref import pos_hash
    rng = np.random.default_rng(seed)
    B = len(games)
    nes = [np.array([len(n["act"]) for n in g.nodes], np.int64) if g.nodes else np.array([-1]) for g in games]
    lay = [greedy_layout(ne, chunk) for ne in nes]
    shape = engine_shape(B, node_cap, chunk, sum(l[1] for l in lay) + spare_chunks)
    img = blank_image(shape)
    img["played"], img["reset"], img["next_sims"] = np.zeros(B, np.int32), np.zeros(B, np.uint8), 0
    img["tags"] = [g.tag for g in games]
    perm = rng.permutation(shape["pool_chunks"]).astype(np.int32)
    taken = 0
    img["pos_index"][:] = -1
    img["path_len"][:] = 0
    img["leaf_kind"][:] = LEAF_INACTIVE
    for gi, g in enumerate(games):
        ne = nes[gi]
        where, nch, off = lay[gi]
        ids = perm[taken:taken + nch].copy()
        taken += nch
        img["chunk_list"][gi, :nch], img["n_chunks"][gi] = ids, nch
        for k in ("root_visits", "root_w", "root_init_value", "active", "root_terminal"):
            img[k][gi] = g.scalars[k]
        img["root_state"][gi] = packed_from_cs(g.root)
        if g.fresh:                                                   # what lz_tree_begin leaves
            rec = np.zeros(1, NODE_DT)
            rec["state"], rec["nedges"], rec["parent"] = img["root_state"][gi], -1, -1
            img["nodes"][gi, :1] = rec
            img["nodes"][gi, 0]["old_begin"] = 0x5A5A5A5A
            img["n_nodes"][gi], img["n_edges"][gi] = 1, 0
            dead = img["root_terminal"][gi] != 0
            img["leaf_kind"][gi] = LEAF_INACTIVE if dead else LEAF_EXPAND
            img["leaf_state"][gi], img["leaf_value"][gi] = img["root_state"][gi], 0.0
            continue
        nn = len(g.nodes)
        begin = ids[where[:, 0]].astype(np.int64) * chunk + where[:, 1]
        img["n_nodes"][gi], img["n_edges"][gi] = nn, int(ids[nch - 1]) * chunk + off
        rec = np.zeros(nn, NODE_DT)
        rec["state"] = np.stack([packed_from_cs(n["cs"]) for n in g.nodes])
        rec["edge_begin"], rec["nedges"] = begin, ne
        rec["parent"] = [n["parent"] for n in g.nodes]
        rec["old_begin"] = rng.integers(0, 1 << 20, nn)
        img["nodes"][gi, :nn] = rec
        img["node_value"][gi, :nn] = [n["value"] for n in g.nodes]
        for i, n in enumerate(g.nodes):
            k = len(n["act"])
            run = np.zeros(k, EDGE_DT)
            run["W"], run["P"], run["act"], run["child"] = n["W"], n["P"], n["act"], n["child"]
            run["n_info"] = n["N"].astype(np.uint32) | (n["info"].astype(np.uint32) << 24)
            has = n["child"] >= 0
            ch = np.maximum(n["child"], 0)
            run["cbegin"] = np.where(has, begin[ch], 0)               # as the expand step leaves an edge without a child
            run["cn"] = np.where(has, ne[ch], 0)
            img["edges"][begin[i]:begin[i] + k] = run
        tab, mask = img["pos_index"][gi], shape["pos_slots"] - 1
        for i in range(1, nn):
            if g.nodes[i]["synthetic"] or i in g.index_skip:
                continue
            h = pos_hash(rec["state"][i])
            for p in range(WAVE):
                if tab[(h + p) & mask] == -1:
                    tab[(h + p) & mask] = i
                    break
    img["free_chunks"][:shape["pool_chunks"] - taken] = perm[taken:]
    img["pool_top"][0] = shape["pool_chunks"] - taken
    img["pool_stats"][:] = (0, shape["pool_chunks"], pending_count(img))
    for name in SIDE:
        img[name] = np.full(B, SIDE_PRESET[name], np.int32)
    return img


def longest_chain(img, g):
    """Edges on the longest root-to-leaf chain of game g (a descent writes one path entry per edge)."""
    nn = int(img["n_nodes"][g])
    depth = np.zeros(nn, np.int64)
    par = img["nodes"][g, :nn]["parent"]
    for i in range(1, nn):
        depth[i] = depth[par[i]] + 1
    return int(depth.max()) + 1 if int(img["nodes"][g, 0]["nedges"]) > 0 else 0


def check_step_arena(img, step="select"):
    """Everything a correct launch of `step` ('select': lz_tree_select, 'expand' / 'root': lz_tree_expand below the root /
    at it) relies on, asserted before any upload: everything `check_arena` asserts, plus the step's own needs (module
    comment above)."""
    assert step in ("select", "expand", "root")
    is_root = step == "root"
    from oracle import lz_oracle as O
    from tests.advance_ref import pos_hash
    assert check_arena(img)
    B, cap, chunk = img["B"], img["node_cap"], img["chunk"]
    for name in SIDE:
        assert img[name].dtype == np.int32 and img[name].shape == (B,), name
    takers = 0
    for g in range(B):
        nn = int(img["n_nodes"][g])
        nd = img["nodes"][g, :nn]
        kind = int(img["leaf_kind"][g])
        assert kind in (LEAF_INACTIVE, LEAF_EXPAND, LEAF_TERMINAL, LEAF_REUSED_ROOT, LEAF_SHARED), (g, "leaf_kind")
        if img["root_terminal"][g]:
            continue
        if int(nd["nedges"][0]) < 0:                                  # a fresh root: it expands from leaf_state
            assert nn == 1 and (img["leaf_state"][g] == img["root_state"][g]).all(), (g, "fresh root")
            assert kind == LEAF_EXPAND and step == "root", (g, "a fresh root meets another step than the root step")
            assert packed_status(*img["leaf_state"][g][:2]) == 0
            takers += 1
            continue
        assert nn + 1 <= cap, (g, "no room for the node of an expansion")
        assert longest_chain(img, g) < img["path_cap"] - 1, (g, "a chain reaches path_cap")
        takers += 1
        for i in range(nn):
            ne, e0 = int(nd["nedges"][i]), int(nd["edge_begin"][i])
            if ne <= 0:
                assert i == 0, (g, i, "a node below the root without a run")
                continue
            run = img["edges"][e0:e0 + ne]
            cs = cs_from_packed(nd["state"][i])
            info = (run["n_info"] >> 24).astype(np.int64)
            legal = O.legal_indices_py(cs) if O.game_status(cs) == 0 else []
            real = run["act"].tolist() == legal
            assert len(set(run["act"].tolist())) == ne, (g, i, "action bytes repeat inside a run")
            assert ((run["n_info"] & 0xFFFFFF) <= (1 << 24) - 2).all(), (g, i, "a visit count that one more visit overflows")
            for k in range(ne):
                ch = int(run["child"][k])
                term = bool(info[k] & INFO_TERMINAL)
                assert not (term and ch >= 0), (g, i, k, "a node hangs from a terminal edge")
                if real:
                    succ = O.apply_index(cs, int(run["act"][k]))
                    assert bool(info[k] & INFO_WHITE) == (succ.player < 0), (g, i, k, "player bit")
                    if O.game_status(succ) != 0:
                        assert info[k] & 0xF == edge_info_for(succ) & 0xF, (g, i, k, "terminal bits of a finished child")
                    if ch >= 0:
                        assert (nd["state"][ch] == packed_from_cs(succ)).all(), (g, i, k, "child state is not the successor")
                else:                                                  # synthetic: never an expandable leaf
                    assert term or ch >= 0, (g, i, k, "an edge of a synthetic run could be expanded")
                    if ch >= 0:
                        c2 = cs_from_packed(nd["state"][ch])
                        assert O.game_status(c2) == 0 and bool(info[k] & INFO_WHITE) == (c2.player < 0), (g, i, k, "synthetic child")
        # the position index names nodes that hold the state of their slot's window
        mask = img["pos_slots"] - 1
        tab = img["pos_index"][g]
        for s in ([] if g in img.get("hand_index", ()) else np.flatnonzero((tab >= 1) & (tab < nn))):
            h = pos_hash(nd["state"][int(tab[s])])
            assert ((int(s) - h) & mask) < WAVE, (g, int(s), "index entry outside the window of its state")
        assert ((tab == -1) | ((tab >= 1) & (tab < nn))).all(), (g, "index entry outside [1, n_nodes)")
        if kind == LEAF_SHARED:                                        # preset by hand: the source holds the leaf's state
            src = int(img["leaf_src"][g])
            assert 1 <= src < nn and (nd["state"][src] == img["leaf_state"][g]).all(), (g, "leaf_src")
            assert nd["nedges"][src] == len(O.legal_indices_py(cs_from_packed(img["leaf_state"][g]))), (g, "source run")
        if kind in (LEAF_EXPAND, LEAF_TERMINAL, LEAF_SHARED) and step == "expand":
            plen, le = int(img["path_len"][g]), int(img["leaf_edge"][g])
            assert 1 <= plen < img["path_cap"], (g, "path_len")
            p = img["path"][g * img["path_cap"]:g * img["path_cap"] + plen].astype(np.int64) & 0x7FFFFFFF
            owned = set((img["chunk_list"][g, :int(img["n_chunks"][g])]).tolist())
            assert all(int(e) // chunk in owned for e in p) and int(p[-1]) == le, (g, "path entry outside the game's chunks")
    # the pool: either room for every game that may take a chunk, or none for any (the order of the takes is not
    # specified, so a launch in which some takes succeed and others are refused has no single expected image)
    free = int(img["pool_top"][0]) - (0 if is_root else int(img["pool_stats"][2]))
    assert step == "select" or free >= takers or free <= 0, ("pool", free, takers)
    return True
