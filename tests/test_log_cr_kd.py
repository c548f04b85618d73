"""logcr_kd (adapted_amd/csrc/log_cr.h): the exponent k of a logarithm's argument as a float64 without the int -> float64
conversion -- k + 2^31 placed in the low mantissa word of 2^52, then one subtraction.  The host build of the header must return
the bits of (double)k for every exponent that log_cr_ok admits (k in [-1022, 1023]; the reduction around sqrt(2) moves it by one,
so -1024 .. 1024 are walked), for the ends of the int32 range, and for a spread of other int32 values."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adapted_amd", "csrc")


@pytest.fixture(scope="module")
def host_kd(tmp_path_factory):
    d = tmp_path_factory.mktemp("logcr_kd")
    src = d / "kd.cpp"
    src.write_text('#include "log_cr.h"\nextern "C" void kd_array(const int32_t *k, double *y, long n) '
                   "{ for (long i = 0; i < n; i++) y[i] = logcr_kd_host(k[i]); }\n"
                   'extern "C" void log_1ulp_array(const double *x, double *y, long n) '
                   "{ for (long i = 0; i < n; i++) y[i] = log_1ulp_host(x[i]); }\n"
                   'extern "C" void log_cr_array(const double *x, double *y, long n) '
                   "{ for (long i = 0; i < n; i++) y[i] = log_cr_host(x[i]); }\n")
    so = d / "libkd.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC, "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


def _kd(lib, k):
    k = np.ascontiguousarray(k, dtype=np.int32)
    y = np.empty(k.size, dtype=np.float64)
    lib.kd_array(k.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(k.size))
    return y


def test_kd_equals_the_conversion_for_every_exponent_in_range(host_kd):
    k = np.arange(-1024, 1025, dtype=np.int32)
    assert _kd(host_kd, k).tobytes() == k.astype(np.float64).tobytes()
    assert not np.signbit(_kd(host_kd, [0])[0])               # (double)0 is +0


def test_kd_equals_the_conversion_over_the_int32_range(host_kd):
    rng = np.random.default_rng(5)
    k = np.concatenate([np.array([-2 ** 31, -2 ** 31 + 1, -1, 0, 1, 2 ** 31 - 2, 2 ** 31 - 1], dtype=np.int64),
                        rng.integers(-2 ** 31, 2 ** 31, 100000), np.arange(-70000, 70000)]).astype(np.int32)
    assert _kd(host_kd, k).tobytes() == k.astype(np.float64).tobytes()


def test_the_logarithms_at_every_exponent(host_kd):
    """both logarithms at 2^k and next to sqrt(2) 2^k for every k of the domain against libm within their error bounds (1 ULP of
    log_1ulp_fast, 0.5001 + libm's 0.52 for log_cr_fast): a wrong kd would be off by about ln 2"""
    k = np.arange(-1022, 1024)
    x = np.concatenate([np.ldexp(1.0, k), np.ldexp(1.4142135623730951, k[:-1]), np.ldexp(1.414213562373095, k[:-1])])
    want = np.log(x)
    for fn, ulps in (("log_1ulp_array", 2.0), ("log_cr_array", 1.0)):
        y = np.empty_like(x)
        getattr(host_kd, fn)(x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(x.size))
        assert (np.abs(y - want) <= ulps * np.spacing(np.abs(want))).all(), fn
