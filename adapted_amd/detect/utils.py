"""The reference's detect helpers (adapted/detect/utils.py): range checks shared by its detect modules.  Host only."""
from __future__ import annotations

from typing import Optional, Tuple, Union

import numpy as np

LOCAL_RANGE_PCTLS = (85, 15)


def in_range(
    val: Union[float, np.ndarray],
    min: Union[Optional[float], float, np.ndarray],
    max: Union[Optional[float], float, np.ndarray],
) -> Union[bool, np.ndarray]:
    """min <= val <= max, None meaning no bound: a bool for a scalar, a bool array for an array (NaN never passes).  A float16 /
    float32 scalar compares in float64, as numpy 1.x (the reference's) does against Python floats."""
    min_ = -np.inf if min is None else min
    max_ = np.inf if max is None else max
    if np.ndim(val) == 0:
        if isinstance(val, (np.float16, np.float32)):
            val = float(val)
        return bool(min_ <= val <= max_)
    return np.asarray((min_ <= val) & (val <= max_))


def range_is_empty(range: Union[Tuple[Optional[float], Optional[float]], None]) -> bool:
    """True for no range, (-inf, inf) and (None, None)"""
    if range is None:
        return True
    return (range[0] == -np.inf and range[1] == np.inf) or (range[0] is None and range[1] is None)


__all__ = ["LOCAL_RANGE_PCTLS", "in_range", "range_is_empty"]
