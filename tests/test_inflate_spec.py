"""CPU: the decisions around the synchronous inflate's speculative first pass
(deflate.hpp_amd/csrc/inflate_plan.cpp: spec_knob, spec_wanted, spec_provision, spec_decide).

tests/cpp/inflate_spec_test.cpp is a stand-alone program that links inflate_plan.cpp alone (no
HIP, no GPU).  It runs twice: built plain, and built with AddressSanitizer + UBSan
(-fno-sanitize-recover: any report aborts) and run directly -- nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SRC = [os.path.join(CPP, "inflate_spec_test.cpp"), os.path.join(ROOT, "deflate.hpp_amd", "csrc", "inflate_plan.cpp")]


def _build(exe, flags):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = os.path.join(CPP, exe)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-o", out, *SRC], capture_output=True, text=True)
    if r.returncode != 0:
        if exe.endswith("_san") and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
            pytest.skip("g++ without the sanitizer runtimes: " + r.stderr[-200:])
        raise AssertionError(r.stderr)
    return out


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "[FAIL]" not in r.stderr and " 0 failed" in r.stdout, (r.stdout + r.stderr)[-3000:]
    return r


def test_spec_plain():
    _run(_build("inflate_spec_test", ["-O2"]))


def test_spec_under_asan_ubsan():
    exe = _build("inflate_spec_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                           "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = _run(exe, env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
