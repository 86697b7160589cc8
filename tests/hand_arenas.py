"""Hand-built arenas for lz_tree_advance: the whole image of B games in one TreeEngine -- node records, edge runs, chunk
lists, the free-chunk stack, the root scalars and the position index -- written straight into the engine's buffers, the way
tests/hand_roots.py writes single roots for the read-out kernels.

The host half (`pack_states`, `make_tree`, `build_image`, `check_arena`, `next_move`) needs no GPU.  An image is a dict:
the engine's buffers by the names of `TreeEngine.buf` as numpy arrays, the launch arguments (`played`, `reset`,
`next_sims`) and the engine shape.  `check_arena` asserts everything a correct kernel relies on before anything is
uploaded, so a hand-made mistake cannot make a launch touch memory it does not own.  The device half (`ArenaEngine`)
uploads exactly the image, launches, and reads every buffer back as one image.

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
