"""Numpy restatement of policy surprise weighting (liuzhou_amd/policy_surprise.py, csrc/lz_surprise.h): the surprise of a
row, the weights of a finished game, the systematic resampling and the in-place two-pass copy.  Plain sequential double
arithmetic; the kernels and the host build of the header are checked against it."""
import numpy as np

from oracle import rng_oracle

PURPOSE, INDEX = 3, 1022                                   # lz_rng.h: the index layout of purpose 3
LENGTHS = (1, 2, 63, 64, 65, 128, 129, 200, 512)
PATTERNS = ("gamma", "zero", "onehot", "uniform")
ALPHAS = (0.25, 0.5, 1.0)
NEAR = 1e-9                                                # a game may be left out of an equality check only inside this


def game_u(seed: int, game: int) -> np.float32:
    """The game's resampling offset: u01 of one Philox draw (purpose 3, ply 0, index 1022)."""
    return np.float32(rng_oracle.u01(rng_oracle.draw(int(seed), int(game), 0, PURPOSE, INDEX, 0)[:, 0])[0])


def surprise(legal, pi, p) -> float:
    """max(0, sum over legal actions with pi > 0 of pi (log pi - log max(p, 1e-30))) in double."""
    legal = np.asarray(legal).astype(bool)
    pi, p = np.asarray(pi, np.float32).astype(np.float64), np.asarray(p, np.float32).astype(np.float64)
    on = legal & (pi > 0.0)
    if not on.any():
        return 0.0
    s = float(np.sum(pi[on] * (np.log(pi[on]) - np.log(np.maximum(p[on], 1e-30)))))
    return max(0.0, s)


def pattern(name: str, n: int, rng) -> np.ndarray:
    """float32[n] surprises of one of the test patterns."""
    if name == "gamma":
        return rng.gamma(0.3, 1.0, n).astype(np.float32)
    if name == "zero":
        return np.zeros(n, np.float32)
    if name == "onehot":
        s = np.zeros(n, np.float32)
        s[int(rng.integers(0, n))] = np.float32(rng.uniform(0.1, 3.0))
        return s
    if name == "uniform":
        return np.full(n, np.float32(rng.uniform(0.1, 3.0)), np.float32)
    raise ValueError(name)


def weights(s, alpha: float) -> np.ndarray:
    s = np.asarray(s, np.float32).astype(np.float64)
    n = len(s)
    S = 0.0
    for x in s:                                            # the header's sequential sum
        S += float(x)
    if not S > 1e-12 * n:
        return np.ones(n, np.float64)
    return (1.0 - alpha) + alpha * n * s / S


def cumulative(s, alpha: float) -> np.ndarray:
    """C_0..C_N (C_0 = 0, C_N = N exactly), the running sum taken sequentially in double."""
    w = weights(s, alpha)
    n = len(w)
    C = np.zeros(n + 1, np.float64)
    for j in range(n):
        C[j + 1] = C[j] + w[j]
    C[n] = float(n)
    return C


def counts(s, alpha: float, u) -> np.ndarray:
    b = np.floor(cumulative(s, alpha) + float(u)).astype(np.int64)
    return b[1:] - b[:-1]


def plan(s, alpha: float, u) -> np.ndarray:
    """src int32[N]: output slot k takes source row src[k]."""
    c = counts(s, alpha, u)
    return np.repeat(np.arange(len(c), dtype=np.int32), c)


def near_integer(s, alpha: float, u, tol: float = NEAR) -> bool:
    """One of the C_j + u lies within `tol` of an integer: another summation order may round it to the other side."""
    x = cumulative(s, alpha)[1:-1] + float(u)              # C_N + u = N + u is exact and never near (u is k / 2^24)
    return bool(len(x)) and bool((np.abs(x - np.rint(x)) < tol).any())


def rows_dropped(src) -> int:
    return int(len(src) - len(np.unique(src)))


def two_pass_inplace(rows: np.ndarray, src: np.ndarray) -> np.ndarray:
    """The kernel's order on a copy of `rows`: ascending over the slots with src[k] > k, then descending over those with
    src[k] < k, each slot reading its source where it lies at that moment."""
    out = rows.copy()
    n = len(src)
    for k in range(n):
        if src[k] > k:
            out[k] = out[src[k]]
    for k in range(n - 1, -1, -1):
        if src[k] < k:
            out[k] = out[src[k]]
    return out


def games(seed: int, lengths=LENGTHS, patterns=PATTERNS, alphas=ALPHAS):
    """The grid of test games: (n, pattern, alpha, s float32[n], game id), game ids 0, 1, ... in grid order."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        for pat in patterns:
            for a in alphas:
                out.append((n, pat, a, pattern(pat, n, rng), len(out)))
    return out
