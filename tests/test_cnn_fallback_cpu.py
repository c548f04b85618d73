"""The short-read fallback of the CNN operator inside adp_detect_cnn (ADP_CNN_FALLBACK): what can be checked without a GPU --
the flag's value in the header and in the binding, the untouched ABI surface, and the Python entry points' signatures (callers
pass their arguments by position; the new keyword comes last)."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_text():
    text = ""
    for name in ("adapted_hip.h", "adapted_hip_startmods.h"):
        with open(os.path.join(ROOT, "include", name)) as fh:
            text += re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S) + "\n"
    return text


def _flag_values(text):
    """the header's single-bit ADP_* flags (decimal or `1 << n`) -> {name: value}; ADP_SS_GRID_MIN is a size, the
    layouts / versions / limits are not flags of a `flags` argument"""
    not_flags = {"ADP_ABI_VERSION", "ADP_OK", "ADP_MB_OK", "ADP_MB_MAD_ZERO", "ADP_MB_EMPTY_TRACE", "ADP_MAX_CAND", "ADP_MAX_OPEN_PORES",
                 "ADP_LAYOUT_MINIBATCH", "ADP_LAYOUT_SINGLE_READ", "ADP_SS_GRID_MIN", "ADP_MVS_TO_EARLY_STOP"}
    out = {}
    for name, val in re.findall(r"^#define\s+(ADP_[A-Z0-9_]+)\s+\(?\s*(\d+\s*<<\s*\d+|\d+)\s*\)?\s*$", text, re.M):
        if name in not_flags:
            continue
        out[name] = eval(val)  # noqa: S307 -- digits and << only (the pattern above)
    return out


def test_header_defines_the_flag_with_a_bit_of_its_own():
    flags = _flag_values(_header_text())
    assert "ADP_CNN_FALLBACK" in flags and "ADP_IN_DEVICE" in flags and "ADP_SS_FORCE_WAVE" in flags
    v = flags["ADP_CNN_FALLBACK"]
    assert v > 0 and v & (v - 1) == 0
    others = {k: w for k, w in flags.items() if k != "ADP_CNN_FALLBACK"}
    assert all(w & (w - 1) == 0 for w in others.values()), others
    assert v not in others.values(), [k for k, w in others.items() if w == v]


def test_binding_carries_the_headers_value():
    from adapted_amd import lib

    assert lib.ADP_CNN_FALLBACK == _flag_values(_header_text())["ADP_CNN_FALLBACK"]
    assert "fallback" in inspect.signature(lib.Engine.detect_cnn_rows).parameters
    assert inspect.signature(lib.Engine.detect_cnn_rows).parameters["fallback"].default is False


def test_no_new_exported_function_and_the_same_abi_version():
    from adapted_amd import lib

    with open(os.path.join(ROOT, "include", "adapted_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    protos = re.findall(r"^(?:const\s+)?\w+\s*\**\s*(adp_\w+)\s*\([^)]*\)\s*;", text, re.M)
    assert len(protos) == len(set(protos)) == 62
    assert set(protos) == set(lib.PROTOTYPES)
    assert re.search(r"^#define\s+ADP_ABI_VERSION\s+3\s*$", text, re.M)


def test_entry_points_keep_their_positional_parameters():
    from adapted_amd.detect import cnn

    p = list(inspect.signature(cnn.detect_rows).parameters.values())
    assert [q.name for q in p] == ["eng", "sig", "lens", "model", "spc", "conv", "fallback"]
    assert p[5].default == "hip" and p[6].default == "device"
    p = list(inspect.signature(cnn.detect_rows_device).parameters.values())
    assert [q.name for q in p] == ["eng", "dsig", "dlen", "n", "lens_host", "model", "spc", "minibatch", "fallback"]
    assert p[7].default is None and p[8].default == "device"
    assert all(q.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for q in p)
