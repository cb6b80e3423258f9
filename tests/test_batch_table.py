"""CPU: the steps that build a batch's tables from device-resident descriptor arrays
(deflate.hpp_amd/csrc/batch_table.h) -- the per-buffer segment count, the binary search of a table
slot's buffer, the segment entry, the capacity clip and the flags of the deflate side; the marks
and the longest-class-first counting sort of the inflate side -- which the kernels of
batch_table.hip call.

tests/cpp/batch_table_test.cpp is a stand-alone program (its own main, no HIP, no GPU) that this
test compiles itself with g++: once plain, once with AddressSanitizer + UBSan
(-fno-sanitize-recover=all: any report aborts).  Both binaries are run directly -- nothing is
preloaded.  The program runs the steps serially over all "threads" on exact-size heap arrays and
compares the table, bfirst, the segment count and the flags with the serial loop of
deflate_batch_locked."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "batch_table_test.cpp")


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


def test_batch_table_plain(tmp_path):
    _run(_build(tmp_path, "batch_table_test", []))


def test_batch_table_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "batch_table_test_san",
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = _run(exe, env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
