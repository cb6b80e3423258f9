"""CPU: the inflate planners (deflate.hpp_amd/csrc/inflate_plan.cpp: the pass plan, the path-4
chain walk, path 5's units, budgets, region units and chain walk) on hand-built records.

tests/cpp/plan_test.cpp is a stand-alone program that links inflate_plan.cpp alone (no HIP, no
GPU).  It runs twice: built plain, and built with AddressSanitizer + UBSan
(-fno-sanitize-recover: any report aborts) and run directly -- nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _make(target, exe):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-s", "-C", CPP, target], capture_output=True, text=True)
    if r.returncode != 0:
        if exe.endswith("_san") and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
            pytest.skip("g++ without the sanitizer runtimes: " + r.stderr[-200:])
        raise AssertionError(r.stderr)
    return os.path.join(CPP, exe)


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "[FAIL]" not in r.stderr and " 0 failed" in r.stdout, (r.stdout + r.stderr)[-3000:]
    return r


def test_plan_plain():
    _run(_make("plan", "plan_test"))


def test_plan_under_asan_ubsan():
    exe = _make("san", "plan_test_san")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = _run(exe, env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
