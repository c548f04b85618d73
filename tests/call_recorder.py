"""A lib.Engine without a GPU: its ``lib`` attribute is a recorder, so every Python layer above the C ABI runs as it is and the
tests read what reached the library (tests/test_cnn_call_paths_cpu.py and the pipeline tests of the CNN options)."""
import numpy as np

# where n stands in the argument list of a detect call (behind the handle and the batch's pointers or arrays)
_N_AT = {"adp_detect_cnn": 3, "adp_detect_llr": 3, "adp_detect_cnn_i16": 5, "adp_detect_llr_i16": 5}


class RecorderLib:
    """every adp_* function returns 0 and leaves (name, arguments) in ``calls``.  bounds: what adp_detect_cnn* writes into a
    bounds array it is given (adapter end, poly(A) end), for the host-applied fallback's selection."""

    def __init__(self, bounds=None):
        self.calls, self.bounds = [], bounds

    def __getattr__(self, name):
        if not name.startswith("adp_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if self.bounds and name.startswith("adp_detect_cnn") and args[-1] is not None:
                args[-1][:, 0], args[-1][:, 1:] = self.bounds[0], self.bounds[1]
            return 0

        return fn


def recorder_engine(spc, m, bounds=None):
    from adapted_amd import lib

    eng = lib.Engine.__new__(lib.Engine)
    eng.lib, eng.m, eng.cfg, eng._h = RecorderLib(bounds), int(m), lib.make_cfg(spc), None
    return eng


def names(eng):
    return [name for name, _ in eng.lib.calls]


def detect_calls(eng):
    """the detect calls the library saw, each as a dict: fn, head (the batch: arrays or pointers), n, m, minibatch, flags, rows
    ("host" / the pointer) and bounds (None / (dtype, shape))"""
    out = []
    for name, a in eng.lib.calls:
        if name not in _N_AT:
            continue
        i = _N_AT[name]
        rows, last = a[i + 4], a[i + 5]
        assert a[0] is eng._h
        out.append(dict(fn=name, head=a[1:i], n=a[i], m=a[i + 1], minibatch=a[i + 2], flags=a[i + 3],
                        rows="host" if isinstance(rows, np.ndarray) else rows,
                        bounds=None if last is None else (last.dtype, last.shape)))
    return out


def head_kind(call):
    """"host": float32 [n, m] + int32 [n] arrays; "pointers": plain ints"""
    if all(isinstance(x, np.ndarray) for x in call["head"]):
        sig, lens = call["head"]
        assert sig.dtype == np.float32 and sig.shape == (call["n"], call["m"]) and lens.dtype == np.int32 and lens.shape == (call["n"],)
        return "host"
    assert all(type(x) is int for x in call["head"]), call["head"]
    return "pointers"
