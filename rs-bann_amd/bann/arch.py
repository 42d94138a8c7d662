"""The architecture rules and the initialisation options of a new model.

  layer_widths   BlockNetCfg::add_branch (architectures.rs:93-122): one branch's layer widths from
                 its marker count and the width rules (bann_arch_layer_widths, host only)
  InitConfig     the BranchCfgBuilder options behind rs-bann train-new and simulate-y
                 (bann_init_cfg, include/bann.h)
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from ._lib import BannError, InitCfg, load_library

_HIDDEN = {"fixed": 0, "fraction": 1}
_SUMMARY = {"fixed": 0, "like_hidden": 1, "fraction": 2}


def layer_widths(m: int, depth: int, hidden: Tuple = ("fraction", 0.5), summary: Tuple = ("like_hidden",)) -> List[int]:
    """[hidden] * depth + [summary, 1] for a branch of m markers: the array add_branch takes.
    hidden: ("fixed", w) or ("fraction", f) = max(1, trunc(f32(m) * f)); summary: ("fixed", w),
    ("like_hidden",) or ("fraction", f) of the hidden width.  With depth 0 the hidden width is
    still formed and the summary width derives from it, as the reference does."""
    if hidden[0] not in _HIDDEN or summary[0] not in _SUMMARY:
        raise ValueError(f"unknown width rule: {hidden[0]!r} / {summary[0]!r}")
    hf = hidden[0] == "fixed"
    sf = summary[0] == "fixed"
    out = np.zeros(max(int(depth), 0) + 2, np.int32)
    lib = load_library()
    rc = lib.bann_arch_layer_widths(int(m), int(depth), _HIDDEN[hidden[0]], int(hidden[1]) if hf else 0,
                                    0.0 if hf else float(hidden[1]), _SUMMARY[summary[0]],
                                    int(summary[1]) if sf else 0,
                                    float(summary[1]) if summary[0] == "fraction" else 0.0,
                                    out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc < 0:
        raise BannError(rc, lib.bann_io_last_error().decode())
    return [int(v) for v in out[:rc]]


@dataclass
class InitConfig:
    """How BranchCfgBuilder draws the initial parameters.  variance: weights and biases ~ N(0, v);
    else gamma = (shape, scale): every layer ~ N(0, 1 / (shape * scale)); else weights ~ N(0, 1 / m_b)
    and biases 0.  num_effective (exactly that many markers keep their first-layer weights) takes
    precedence over proportion_effective.  fixed_precision: every precision is that value (base
    priors only)."""
    variance: Optional[float] = None
    gamma: Optional[Tuple[float, float]] = None
    num_effective: Optional[int] = None
    proportion_effective: Optional[float] = None
    fixed_precision: Optional[float] = None

    def to_c(self) -> InitCfg:
        mode = 1 if self.variance is not None else (2 if self.gamma is not None else 0)
        k, s = self.gamma if self.gamma is not None else (0.0, 0.0)
        return InitCfg(mode, self.variance or 0.0, k, s, -1 if self.num_effective is None else int(self.num_effective),
                       -1.0 if self.proportion_effective is None else float(self.proportion_effective),
                       int(self.fixed_precision is not None), self.fixed_precision or 0.0)
