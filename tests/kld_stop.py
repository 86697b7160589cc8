"""Float64 numpy restatement of the KLD-gain early stopping rule (LzTreeDesc.kld_*): one check, and
the sequential replay of a search's checks from the root visits after 0, I, 2I, ... simulations."""
import numpy as np


def check(snapshot, visits, s, min_sims, theta):
    """One check behind launch `s` (> 0) of a game that takes part in it.  `snapshot`, `visits`: the root children's visit
    counts at the last check and now (equal lengths).  Returns (gain per simulation or None when no gain is formed,
    stop decision, new snapshot)."""
    o = np.asarray(snapshot, dtype=np.int64)
    n = np.asarray(visits, dtype=np.int64)
    O, N = int(o.sum()), int(n.sum())
    per = None
    if O > 0 and N > O:
        k = o > 0
        with np.errstate(divide="ignore"):
            terms = (o[k].astype(np.float64) / float(O)) * np.log((o[k].astype(np.float64) * float(N)) /
                                                                   (n[k].astype(np.float64) * float(O)))
        per = float(terms.sum()) / float(N - O)
    stop = per is not None and int(s) >= int(min_sims) and per < float(theta)
    return per, bool(stop), n.copy()


def replay(visits_at, sims, interval, min_sims, theta, budget=None):
    """The checks of one game's search of `sims` simulations: `visits_at[j]` = the root visits after j * interval
    simulations (j = 0: the snapshot).  Returns (the budget the search ends with, [(s, gain per simulation)] of the
    gains formed).  `budget`: the budget the search starts with (default `sims`)."""
    b = int(sims) if budget is None else int(budget)
    snap = np.asarray(visits_at[0], dtype=np.int64)
    gains = []
    j = 1
    while j * interval + 1 < sims:
        s = j * interval
        if b <= s + 1:
            break
        per, stop, snap = check(snap, visits_at[j], s, min_sims, theta)
        if per is not None:
            gains.append((s, per))
        if stop:
            b = s + 1
            break
        j += 1
    return b, gains
