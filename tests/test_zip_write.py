"""CPU: the ZIP writer's format and steps (deflate.hpp_amd/csrc/zip_write.h) -- the local headers,
the central records with the ZIP64 extra, the end records, the layout and the pack kernel's chunk
arithmetic that the kernels of zip_write.hip call.

tests/cpp/zip_write_test.cpp is a stand-alone program (its own main, no HIP, no GPU) that this test
compiles itself with g++: once plain, once with AddressSanitizer + UBSan
(-fno-sanitize-recover=all: any report aborts).  Both binaries are run directly -- nothing is
preloaded.  The entries are written here as case files (tests/zip_write_cases.py; deflated payloads
are zlib's raw streams); the program assembles each archive with zip_write.h alone, every step run
serially over all "threads" into an exact-size heap buffer, reads it back with zip_dir.h's steps
and writes it out; Python's zipfile then judges the file."""
import io
import os
import zipfile

import numpy as np
import pytest

import zip_write_cases as zw


def test_threshold_and_chunk_arithmetic(tmp_path):
    """record sizes, 0xFFFFFFFF fields, extra order and version needed around 2^32; the end records
    around 0xFFFF entries and 2^32 bytes; the chunks of the pack kernel on an exhaustive small grid"""
    r = zw.run(zw.build(tmp_path, "zip_write_test", [], pytest.skip), ["--arith"])
    assert int(r.stdout.split()[0]) > 10000


def check_archives(got):
    for label, (members, comment, force64, archive) in got.items():
        infos = zw.check_with_zipfile(archive, members, comment, read_all=len(members) < 1000)
        eocd = len(archive) - 22 - len(comment)
        assert archive[eocd:eocd + 4] == b"PK\x05\x06", label
        zip64 = archive[eocd - 20:eocd - 16] == b"PK\x06\x07"
        assert zip64 == (force64 or len(members) >= 65535), label
        if zip64:
            assert archive[eocd - 76:eocd - 72] == b"PK\x06\x06", label
        for zi in infos:  # version needed, as the local header states it
            h = zi.header_offset
            assert archive[h + 4:h + 6] == (b"\x2d\x00" if force64 else b"\x14\x00"), label
    assert got["empty"][3] == zw.zc.write_zip([]) and len(got["empty"][3]) == 22
    for label in ("mixed", "mixed_force64"):
        with zipfile.ZipFile(io.BytesIO(got[label][3])) as z:
            a = np.load(io.BytesIO(z.read("array.npy")))
        assert a.shape == (30, 100) and a[29, 99] == 2999.0


def test_assembled_archives_plain():
    check_archives(zw.assembled_plain())


def test_assembled_archives_under_asan_ubsan(tmp_path):
    exe = zw.build(tmp_path, "zip_write_test_san",
                   ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"], pytest.skip)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = zw.run(exe, ["--arith"], env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = zw.assemble_all(exe, tmp_path, env)
    plain = zw.assembled_plain()
    assert {k: v[3] for k, v in got.items()} == {k: v[3] for k, v in plain.items()}  # (judged there)


def test_cases_are_what_they_claim():
    names = [m[0] for m in zw.names_1_to_200()]
    assert sorted(len(n) for n in names) == list(range(1, 201)) and len(set(names)) == 200
    m = zw.mixed()
    assert sorted(len(d) for _, d, method, _ in m if method == 0 and d) == [1, 15, 16, 17, 4097]
    assert any(method == 8 and not d for _, d, method, _ in m) and any(n.endswith(b"/") for n, *_ in m)
    assert [len(d) for n, d, *_ in m if n in (b"text.txt", b"dir/random.bin", b"zeros")] == [70000, 3000, 100000]
    assert any(b > 127 for b in zw.non_ascii()[0][0])
    with zipfile.ZipFile(io.BytesIO(zw.zc.many(300))) as z:  # the tiny entries are zip_cases.many's
        assert [(zi.filename.encode(), z.read(zi), zi.compress_type) for zi in z.infolist()] == \
            [(n, d, method) for n, d, method, _ in zw.tiny(300)]
