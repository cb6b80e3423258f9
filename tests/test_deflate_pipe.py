"""CPU: the chunk arithmetic of the deflate's chunk pipeline (deflate.hpp_amd/csrc/deflate_pipe.h),
which launch_deflate and deflate_device_locked share with this test: the chunks cover [0, nseg)
exactly once, a chunk is a multiple of the front kernel's grid, both 32 KiB halves of a 64 KiB
block fall into the block's chunk, the pipeline stays off below two grids' worth of segments, and
the DMX_DEFLATE_PIPE knob parses as documented.

tests/cpp/deflate_pipe_test.cpp is a stand-alone program (its own main, no HIP, no GPU) that this
test compiles itself with g++: once plain, once with AddressSanitizer + UBSan.  Both binaries are
run directly -- nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "deflate_pipe_test.cpp")


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


def test_deflate_pipe_plain(tmp_path):
    _run(_build(tmp_path, "deflate_pipe_test", []))


def test_deflate_pipe_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "deflate_pipe_test_san",
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = _run(exe, env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
