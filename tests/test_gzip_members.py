"""CPU: the plain C++ behind dmx_inflate_gzip_members -- gzip_head_len
(deflate.hpp_amd/csrc/container_parse.h), the header-only parse the candidate scan runs at every
offset, and gzm_walk with the cut rule (deflate.hpp_amd/csrc/gzip_members.{h,cpp}), the host's walk
over the records the device wrote.

tests/cpp/gzip_members_test.cpp is a stand-alone program (its own main, no HIP, no GPU) that this
test compiles itself with g++: once plain, once with AddressSanitizer + UBSan
(-fno-sanitize-recover=all: any report aborts).  Both binaries are run directly -- nothing is
preloaded.  gzip_head_len is compared with a serial parse on every flag byte, every truncation of a
header with all four optional fields and every single-byte change of its first 12 bytes; the walk
with a front-to-back model on files of stored-block members (1, 2 and 500 members, empty members,
zero and non-zero gaps, a nested .gz, false candidates, long members and the moving cut, truncation,
a start in mid-file)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "gzip_members_test.cpp")


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


def test_gzip_members_plain(tmp_path):
    _run(_build(tmp_path, "gzip_members_test", []))


def test_gzip_members_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "gzip_members_test_san",
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = _run(exe, env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
