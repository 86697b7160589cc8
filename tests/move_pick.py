"""Sequential numpy float64 restatement of the visit-offset / value-cutoff move pick (include/liuzhou_hip.h,
lz_tree_move_pick).  Checker of the tests: it does nothing else."""
import numpy as np


def applies(*, terminal, sample_moves, temperature, force_uniform, offset, cutoff):
    """Does the rule re-pick this game's move?"""
    return bool((offset > 0.0 or cutoff > 0.0) and sample_moves and not terminal and not force_uniform
                and np.float32(temperature) > np.float32(1e-6))


def child_q(W, N, white, root_player):
    """q_k as the finish forms it: double W / N in the root mover's frame (white: the edge's info bit 0), 0 at N = 0."""
    q = np.zeros(len(N), dtype=np.float64)
    for k in range(len(N)):
        if N[k] > 0:
            mv = np.float64(W[k]) / np.float64(N[k])
            q[k] = mv if (-1 if white[k] else 1) == root_player else -mv
    return q


def pick(N, q, temperature, uniform, offset, cutoff):
    """One game the rule applies to.  Returns a dict: pick (edge index), kstar, eligible (bool array), weights, cum (C_k),
    total (S), target (u * S), cut_visits, cut_value."""
    N = np.asarray(N, dtype=np.int64)
    q = np.asarray(q, dtype=np.float64)
    ne = len(N)
    o, c = np.float64(offset), np.float64(cutoff)
    kstar = int(np.argmax(N))                                   # first of the maxima
    npr = N.astype(np.float64) - o
    eligible = np.zeros(ne, dtype=bool)
    weights = np.zeros(ne, dtype=np.float64)
    cut_visits = cut_value = 0
    for k in range(ne):
        if k == kstar:
            continue
        if N[k] > 0 and not npr[k] > 0.0:
            cut_visits += 1
        elif npr[k] > 0.0 and not (c == 0.0 or q[k] >= q[kstar] - c):
            cut_value += 1
    out = dict(kstar=kstar, cut_visits=cut_visits, cut_value=cut_value)
    if not npr[kstar] > 0.0:
        eligible[kstar] = True
        weights[kstar] = 1.0
        return dict(out, pick=kstar, eligible=eligible, weights=weights, cum=np.cumsum(weights), total=np.float64(1.0),
                    target=None)
    T = np.float64(max(np.float32(temperature), np.float32(1e-6)))
    for k in range(ne):
        if k == kstar:
            eligible[k], weights[k] = True, 1.0
        elif npr[k] > 0.0 and (c == 0.0 or q[k] >= q[kstar] - c):
            eligible[k] = True
            weights[k] = np.exp((np.log(npr[k]) - np.log(npr[kstar])) / T)
    cum = np.zeros(ne, dtype=np.float64)
    run = np.float64(0.0)
    for k in range(ne):
        run = run + weights[k]
        cum[k] = run
    target = np.float64(np.float32(uniform)) * run
    chosen = -1
    for k in range(ne):
        if eligible[k] and cum[k] > target:
            chosen = k
            break
    if chosen < 0:
        chosen = int(np.nonzero(eligible)[0][-1])
    return dict(out, pick=chosen, eligible=eligible, weights=weights, cum=cum, total=run, target=target)


def margin_ok(res, rel=1e-9):
    """Is u * S further than rel * S from every C_k?  (The device sums the weights by a wave scan, not sequentially.)"""
    if res["target"] is None:
        return True
    return bool(np.all(np.abs(res["target"] - res["cum"]) > rel * res["total"]))
