"""Entries for the ZIP writer's tests (tests/test_zip_write.py, tests/test_zip_write_abi.py on the
CPU, tests/test_gpu_zip_write.py): the member lists, the case files tests/cpp/zip_write_test.cpp
assembles, the program's build and what Python's zipfile must say about a written archive."""
import functools
import io
import os
import shutil
import struct
import subprocess
import tempfile
import zipfile
import zlib

import zip_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "zip_write_test.cpp")
DATE = (2024, 2, 29, 12, 34, 56)
DOSTIME = (DATE[0] - 1980) << 25 | DATE[1] << 21 | DATE[2] << 16 | DATE[3] << 11 | DATE[4] << 5 | DATE[5] // 2
DEFAULT_DATE = (1980, 1, 1, 0, 0, 0)  # dostime 0


def npy_bytes():
    import numpy as np
    buf = io.BytesIO()
    np.save(buf, np.arange(3000, dtype=np.float32).reshape(30, 100))
    return buf.getvalue()


def mixed():
    """(name, plain bytes, method, dostime): the shape of zip_cases.mixed, plus an .npy member"""
    m = [(b"text.txt", zc._text(70000, 1), 8, DOSTIME), (b"dir/", b"", 0, DOSTIME)]
    for n in (0, 1, 15, 16, 17, 4097):
        m.append((b"stored_%d.bin" % n, zc._rand(n, n), 0, 0))
    m.append((b"empty_deflated", b"", 8, DOSTIME))
    m.append((b"dir/random.bin", zc._rand(3000, 7), 8, 0))
    m.append((b"zeros", bytes(100000), 8, DOSTIME))
    m.append((b"array.npy", npy_bytes(), 8, DOSTIME))
    return m


def one():
    return [(b"hello.txt", zc._text(5000), 8, DOSTIME)]


def names_1_to_200():
    return [(bytes([97 + k % 26]) * (1 + k), zc._text(20 + k, k), 8 if k % 2 else 0, 0) for k in range(200)]


def non_ascii():
    return [("café/日本.txt".encode("utf-8"), zc._text(300, 3), 8, DOSTIME), (b"plain.txt", b"abc", 0, DOSTIME)]


def tiny(count):
    """the contents of zip_cases.many(count): every third entry deflated text, the others stored"""
    return [(b"%x" % k, b"%d\n" % k if k % 3 else zc._text(40 + k % 50, k), 0 if k % 3 else 8, 0) for k in range(count)]


CASES = {"empty": (lambda: [], b""), "one": (one, b""), "mixed": (mixed, b"an archive comment"),
         "names": (names_1_to_200, b""), "non_ascii": (non_ascii, b"")}


def raw_deflate(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def case_bytes(members, comment=b"", force64=False):
    """the case file zip_write_test.cpp reads; method 8 payloads are zlib's raw streams"""
    out = [b"ZWC1", struct.pack("<III", 1 if force64 else 0, len(members), len(comment)), comment]
    for name, data, method, dostime in members:
        payload = raw_deflate(data) if method == 8 else data
        out.append(struct.pack("<IHHIIQQ", len(name), method, 0, dostime, zlib.crc32(data), len(data), len(payload)))
        out.append(name)
        out.append(payload)
    return b"".join(out)


def build(out_dir, name, extra, skip):
    """compiles zip_write_test.cpp -> the program's path; skip(reason) where g++ or the sanitizer
    runtimes are missing"""
    if shutil.which("g++") is None:
        skip("no g++")
    exe = os.path.join(str(out_dir), name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", *extra, SRC, "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0:
        if extra and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
            skip("g++ without the sanitizer runtimes: " + r.stderr[-200:])
        raise AssertionError(r.stderr[-3000:])
    return exe


def run(exe, args, env=None):
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "[FAIL]" not in r.stderr and " 0 failed" in r.stdout, (r.stdout + r.stderr)[-3000:]
    return r


def all_cases():
    """(label, members, comment, force64) of every assembled case"""
    out = []
    for force64 in (False, True):
        for name, (make, comment) in CASES.items():
            out.append((name + ("_force64" if force64 else ""), make(), comment, force64))
    out.append(("tiny_65534", tiny(65534), b"", False))
    out.append(("tiny_65535", tiny(65535), b"", False))
    return out


def assemble_all(exe, out_dir, env=None):
    """runs the program over every case -> {label: (members, comment, force64, archive bytes)}"""
    args, cases = [], all_cases()
    for label, members, comment, force64 in cases:
        cp, zp = os.path.join(str(out_dir), label + ".case"), os.path.join(str(out_dir), label + ".zip")
        with open(cp, "wb") as f:
            f.write(case_bytes(members, comment, force64))
        args += [cp, zp]
    run(exe, args, env)
    got = {}
    for label, members, comment, force64 in cases:
        with open(os.path.join(str(out_dir), label + ".zip"), "rb") as f:
            got[label] = (members, comment, force64, f.read())
    return got


@functools.lru_cache(maxsize=None)
def assembled_plain():
    """the archives of the plain build, made once per session"""
    import pytest
    d = tempfile.mkdtemp(prefix="zip_write_")
    try:
        return assemble_all(build(d, "zip_write_test", [], pytest.skip), d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def check_with_zipfile(archive, members, comment=b"", read_all=True):
    """zipfile on a written archive: testzip, every stated field, every payload"""
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        assert z.testzip() is None
        infos = z.infolist()
        assert len(infos) == len(members)
        assert z.comment == comment
        for k, (zi, (name, data, method, dostime)) in enumerate(zip(infos, members)):
            utf8 = any(b > 127 for b in name)
            assert zi.orig_filename == name.decode("utf-8" if utf8 else "cp437"), k
            assert zi.flag_bits == (0x800 if utf8 else 0), k
            assert (zi.file_size, zi.CRC, zi.compress_type) == (len(data), zlib.crc32(data), method), k
            assert zi.date_time == (DATE if dostime else DEFAULT_DATE), k
            assert zi.is_dir() == name.endswith(b"/"), k
            assert zi.comment == b"" and (zi.extra == b"" or zi.extra[:2] == b"\x01\x00"), k
            if method == 0:
                assert zi.compress_size == len(data), k
            if read_all or k % 997 == 0 or k + 3 > len(members):
                assert z.read(zi) == data, k
        return infos
