"""PUCT shape of the tree search: first-play urgency and the visit-scaled exploration constant.

Host side only, no torch: the one function that builds the c(n) table -- the engine uploads its result, the test checker
indexes the same numbers -- and the validation the Python layers share."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional

CPUCT_TABLE_LEN = 65536          # entries of the uploaded table (512 KB); visit counts at or beyond it take the last entry
CPUCT_BASE_DEFAULT = 19652.0     # AlphaZero's c_base
SHAPE_FPU, SHAPE_TABLE = 1, 2    # LzTreeDesc.puct_shape bits


def cpuct_table(c_puct: float, cpuct_log: float, cpuct_base: float, length: int = CPUCT_TABLE_LEN) -> List[float]:
    """table[i] = c_puct + cpuct_log * ln((i + cpuct_base + 1) / cpuct_base), in float64: the exploration constant of a
    node with i visits.  The device never takes a logarithm (a library log one ulp off could flip an exact tie): it reads
    table[min(n, length - 1)]."""
    c_puct, cpuct_log, cpuct_base, length = float(c_puct), float(cpuct_log), float(cpuct_base), int(length)
    if length < 2:
        raise ValueError(f"the cpuct table needs at least 2 entries, got {length}")
    if not math.isfinite(cpuct_base) or cpuct_base <= 0.0:
        raise ValueError(f"cpuct_base must be a finite number > 0, got {cpuct_base}")
    return [c_puct + cpuct_log * math.log((i + cpuct_base + 1.0) / cpuct_base) for i in range(length)]


class PuctShape(NamedTuple):
    """Validated parameters.  `fpu` / `table`: which half is on; the reductions are 0.0 while `fpu` is off."""
    fpu: bool
    table: bool
    fpu_reduction: float
    fpu_root_reduction: float
    cpuct_log: float
    cpuct_base: float

    @property
    def on(self) -> bool:
        return self.fpu or self.table

    @property
    def flags(self) -> int:
        return (SHAPE_FPU if self.fpu else 0) | (SHAPE_TABLE if self.table else 0)

    def key(self):
        """What two searches must share to run as one (hashable; the same for every off state)."""
        return (self.fpu, self.table, self.fpu_reduction, self.fpu_root_reduction,
                self.cpuct_log if self.table else 0.0, self.cpuct_base if self.table else 0.0)

    def meta(self) -> dict:
        """The four values as the manifests record them."""
        return {"fpu_reduction": self.fpu_reduction if self.fpu else None,
                "fpu_root_reduction": self.fpu_root_reduction if self.fpu else None,
                "cpuct_log": self.cpuct_log, "cpuct_base": self.cpuct_base}

    def kwargs(self) -> dict:
        """The keyword arguments that switch this shape on in the layer below (empty while off)."""
        if not self.on:
            return {}
        return {**({"fpu_reduction": self.fpu_reduction, "fpu_root_reduction": self.fpu_root_reduction} if self.fpu else {}),
                **({"cpuct_log": self.cpuct_log, "cpuct_base": self.cpuct_base} if self.table else {})}


def parse_puct_shape(fpu_reduction: Optional[float] = None, fpu_root_reduction: Optional[float] = None,
                     cpuct_log: float = 0.0, cpuct_base: float = CPUCT_BASE_DEFAULT) -> PuctShape:
    """Validate the four parameters (ValueError: a negative or non-finite value, cpuct_base <= 0, fpu_root_reduction without
    fpu_reduction).  fpu_reduction None = first-play urgency off, 0.0 = on with no reduction; fpu_root_reduction None =
    fpu_reduction; cpuct_log 0 = the constant c_puct."""
    if fpu_reduction is None and fpu_root_reduction is not None:
        raise ValueError("fpu_root_reduction needs fpu_reduction (first-play urgency is off without it)")
    fpu = fpu_reduction is not None
    red = float(fpu_reduction) if fpu else 0.0
    root = float(fpu_root_reduction) if fpu_root_reduction is not None else red
    log, base = float(cpuct_log), float(cpuct_base)
    for name, v in (("fpu_reduction", red), ("fpu_root_reduction", root), ("cpuct_log", log)):
        if not math.isfinite(v) or v < 0.0:
            raise ValueError(f"{name} must be a finite number >= 0, got {v}")
    if not math.isfinite(base) or base <= 0.0:
        raise ValueError(f"cpuct_base must be a finite number > 0, got {base}")
    return PuctShape(fpu, log > 0.0, red, root, log, base)

