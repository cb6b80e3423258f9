"""CPU: the parallel form of the ZIP directory walk (deflate.hpp_amd/csrc/zip_dir.h) -- the end
record search, the ZIP64 records, the base shift, the candidate predicate, the chain over central
records, the field decode with the ZIP64 extra, the local header and the layout that the kernels of
zip_dir.hip call.

tests/cpp/zip_dir_test.cpp is a stand-alone program (its own main, no HIP, no GPU) that this test
compiles itself with g++: once plain, once with AddressSanitizer + UBSan
(-fno-sanitize-recover=all: any report aborts).  Both binaries are run directly -- nothing is
preloaded.  The archives are written here with Python's zipfile (tests/zip_cases.py), each with the
table zipfile's ZipInfo states next to it; the program compares the steps, run serially over all
"threads" on exact-size heap copies, with that table and with its own serial walk, and then damages
the archives: every mutant must end in a status."""
import os
import shutil
import subprocess

import pytest

import zip_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "zip_dir_test.cpp")

CASES = [("empty", zc.empty), ("one", zc.one_entry), ("mixed", zc.mixed), ("descriptors", zc.data_descriptors),
         ("false_signatures", zc.false_signatures), ("prepended", zc.prepended), ("hand_zip64", zc.hand_zip64),
         ("names_3000", lambda: zc.many(3000, True)), ("many_65536", lambda: zc.many(65536))]


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


def _archives(tmp_path):
    args = []
    for name, make in CASES:
        data = make()
        (tmp_path / f"{name}.zip").write_bytes(data)
        (tmp_path / f"{name}.txt").write_text(zc.table_text(data))
        args += [str(tmp_path / f"{name}.zip"), str(tmp_path / f"{name}.txt")]
    return args


def _run(exe, args, env=None):
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "[FAIL]" not in r.stderr and " 0 failed" in r.stdout, (r.stdout + r.stderr)[-3000:]
    return r


def test_zip_cases_are_what_they_claim():
    """the archives hold what the C++ cases rely on"""
    import struct
    big = zc.many(65536)
    assert big[-22 - 20:-22 - 16] == b"PK\x06\x07" and big[-22 - 76:-22 - 72] == b"PK\x06\x06"  # natural ZIP64 records
    assert all(r[6] & 8 for r in zc.table(zc.data_descriptors()))
    pre = zc.prepended()
    assert struct.unpack("<I", pre[-6:-2])[0] + 1024 == pre.index(b"PK\x01\x02", 1024)  # the stated offset is short
    hz = zc.table(zc.hand_zip64())
    assert [r[4] for r in hz] == [8, 0] and hz[0][0] == 4
    assert zc.false_signatures().count(zc.SIG_CENTRAL) > 3 + 4


def test_zip_dir_plain(tmp_path):
    _run(_build(tmp_path, "zip_dir_test", []), _archives(tmp_path))


def test_zip_dir_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "zip_dir_test_san",
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = _run(exe, _archives(tmp_path), env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
