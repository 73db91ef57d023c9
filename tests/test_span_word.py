"""The packed span word of the emission (csrc/gsr_span_word.h) on the CPU: the header compiles as plain C++ with the
host compiler, and a stand-alone program (tests/span_word_check.cpp) round-trips it over rows 1-5, row lengths 0-16
and first rows / t0 at 0, 126, 127, 128 (and more): encodable inputs decode to the same spans, inputs past a limit
give "not encodable", all-empty rows decode to a kept count of 0.  Built with the address and undefined-behaviour
sanitizers where the host compiler links them (the program has its own main: no preloading)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "threestudio-3dgs_amd", "csrc")
CXX = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler in this image")
def test_span_word_round_trip(tmp_path):
    src = os.path.join(HERE, "span_word_check.cpp")
    base = [CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src]
    exe = tmp_path / "span_word_check"
    res = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)],
                         capture_output=True, text=True, timeout=300)
    if res.returncode != 0:  # (no sanitizer runtime for this compiler: the plain build still checks the values)
        res = subprocess.run(base + ["-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    tag, cases, enc = run.stdout.split()
    assert tag == "ok" and 0 < int(enc) < int(cases)
