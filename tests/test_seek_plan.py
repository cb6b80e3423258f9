"""CPU: the host-side decisions of the seek index (deflate.hpp_amd/csrc/seek_plan.{h,cpp}) --
seek_select, which checkpoints of a decode become index entries, and seek_range_plan, which spans a
ranged read decodes.

tests/cpp/seek_plan_test.cpp is a stand-alone program (its own main, no HIP, no GPU) that this test
compiles itself with g++: once plain, once with AddressSanitizer + UBSan
(-fno-sanitize-recover=all: any report aborts).  Both binaries are run directly -- nothing is
preloaded.  seek_select is compared with a brute-force model on random candidate lists (a spacing
larger than the stream, candidates closer than the spacing, a zero-size tail); seek_range_plan with
a per-byte model of which entry yields which output byte (ranges inside one span, on exact span
edges, one byte on either side of an edge, the whole file, the last byte, len == 0) and on every
DMX_ERR_ARG case."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "seek_plan_test.cpp")


def _build(tmp_path, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", *extra, SRC, "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0:
        if extra and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
            pytest.skip("g++ without the sanitizer runtimes: " + r.stderr[-200:])
        raise AssertionError(r.stderr[-3000:])
    return exe


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "[FAIL]" not in r.stderr and " 0 failed" in r.stdout, (r.stdout + r.stderr)[-3000:]
    return r


def test_seek_plan_plain(tmp_path):
    _run(_build(tmp_path, "seek_plan_test", []))


def test_seek_plan_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "seek_plan_test_san",
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = _run(exe, env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
