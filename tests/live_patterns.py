"""Live-flag patterns shared by tests/test_live_gather_cpu.py and tests/test_gpu_net_gather.py."""
import numpy as np

SIZES = (1, 63, 64, 65, 511, 512, 513, 1025)
PATTERNS = ("none", "all", "first", "last", "alternating", "one_per_word", "random25", "random75", "random98")


def live_pattern(name: str, B: int) -> np.ndarray:
    """bool[B]: which slots are live."""
    live = np.zeros(B, dtype=bool)
    if name == "all":
        live[:] = True
    elif name == "first":
        live[0] = True
    elif name == "last":
        live[-1] = True
    elif name == "alternating":
        live[::2] = True
    elif name == "one_per_word":                       # one live game in every 64: a different bit in every mask word
        for w in range((B + 63) // 64):
            live[min(w * 64 + (w * 37 + 5) % 64, B - 1)] = True
    elif name.startswith("random"):
        pct = int(name[6:])
        live = np.random.default_rng(1000 * pct + B).random(B) < pct / 100.0
    elif name != "none":
        raise ValueError(name)
    return live
