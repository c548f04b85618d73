"""adapted_amd/csrc/carve.h -- the pieces of the handle's carved buffers, shared by both translation units -- as a stand-alone host
program (tests/host/carve_check.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer: no HIP, no GPU, nothing loaded into
this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carve_pieces_under_sanitizers(tmp_path):
    cxx = next((c for c in (shutil.which(n) for n in ("c++", "g++", "clang++")) if c), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "carve_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "adapted_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "carve_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr and ("cannot find" in built.stderr or "unsupported" in built.stderr):
        pytest.skip("the compiler has no sanitizer runtime: " + built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "carve_check: ok", (run.returncode, run.stdout, run.stderr)


def test_both_translation_units_carve_through_the_one_header():
    """no second Carve, and no hand-written byte count beside a workspace piece in modules.hip"""
    import re

    src = {n: open(os.path.join(ROOT, "adapted_amd", "csrc", n)).read() for n in ("carve.h", "handle.h", "adapted_hip.hip", "modules.hip")}
    assert "struct Carve" in src["carve.h"] and "hip" not in src["carve.h"].split("#pragma once")[1].lower()
    assert all("struct Carve" not in src[n] for n in ("handle.h", "adapted_hip.hip", "modules.hip"))
    assert "carve_pieces(h->ws, 256" in src["handle.h"] and "carve_pieces(h->sub_ws, 16" in src["handle.h"]
    # every copy of modules.hip goes through h2d / d2h / stage_in / zero, which take their size from the piece
    body = src["modules.hip"].split("// a byte budget in MiB")[1]
    assert "hipMemcpy" not in body and "hipMemsetAsync" not in body
    for call in re.findall(r"\b(?:h2d|d2h|stage_in(?:<\w+>)?)\(h,[^;]*\)", body):
        assert "sizeof" not in call and not re.search(r"\*\s*(?:4|8|16|20|24|32|40)\b", call), call
