"""The reference's pooling module ``adapted.detect.downscale`` on the HIP library: `efficient_average_pooling` and
`downscale_signal` with the same arguments, defaults and return types (the 2-D input is already a batch), and
`efficient_average_pooling_device` for rows that are resident on the device (adp_pool_mean: adapted_amd/csrc/sigstats_api.h).
There is no CPU path: without the HIP library every function raises ``HipLibraryError``.

Every block's mean is numpy's: the sum in numpy's order, divided by the pool size, in the input's type (float32 stays float32;
integers are widened to float64, numpy's own result type).  A ragged last block is filled with ZEROS, as in the reference: its
mean is pulled towards 0.  A pool size below 1 raises ValueError.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from ._rows import _engine, as_work


def _pool(pool_size) -> int:
    p = int(pool_size)
    if p < 1:
        raise ValueError("pool_size must be >= 1")
    return p


def efficient_average_pooling(data: np.ndarray, pool_size: int = 2) -> np.ndarray:
    if np.ndim(data) != 2:
        raise ValueError("Data must be a 2D array")
    x, p = as_work(data), _pool(pool_size)
    n, m = x.shape
    if n == 0 or m == 0:
        return np.zeros((n, -(-m // p)), dtype=x.dtype)
    return _engine().pool_mean(x, p)


def efficient_average_pooling_device(data: int, n: int, L: int, pool_size: int = 2, dtype=np.float32, out: Optional[int] = None,
                                     device=0):
    """`efficient_average_pooling` of a device-resident [n, L] array (a pointer) -> the pooled [n, ceil(L / pool_size)] array on
    the host, or None with ``out``, a device pointer it is written to"""
    dt = np.dtype(dtype)
    if dt not in (np.float32, np.float64):
        raise TypeError("device data must be float32 or float64")
    if int(n) < 1 or int(L) < 1:
        raise ValueError("n and L must be >= 1")
    return _engine(device).pool_mean(int(data), _pool(pool_size), n=int(n), L=int(L), f64=dt == np.float64, out_ptr=out)


def downscale_signal(signal: np.ndarray, factor: int = 2) -> np.ndarray:
    return efficient_average_pooling(signal, pool_size=factor)


__all__ = ["efficient_average_pooling", "downscale_signal", "efficient_average_pooling_device"]
