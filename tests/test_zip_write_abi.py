"""CPU: the C-ABI of the ZIP writer (dmx_zip_bound, dmx_zip_write_device, dmx_zip_write), the layout
of dmx_zip_source and what dmx_zip_bound promises.  No GPU work is launched: a null context is
rejected before anything else is looked at, and the bound is host arithmetic."""
import ctypes
import os
import re
import subprocess

import dmx
import zip_write_cases as zw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dmx_zip_bound", "dmx_zip_write_device", "dmx_zip_write"]
FIELDS = ["data", "n", "name", "name_len", "method", "reserved", "dostime"]


def test_symbols_exported():
    lib = dmx.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in dmx.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "dmx.h")).read()
    assert re.search(r"#define DMX_ZIP_FORCE64 1u", hdr) and dmx.DMX_ZIP_FORCE64 == 1


def c_kind(param):
    """one C parameter -> the ctypes kind that must stand for it"""
    p = param.strip()
    if "*" in p:
        return "pointer"
    return {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "uint32_t": ctypes.c_uint32}[p.split()[0]]


def py_kind(t):
    return "pointer" if t is ctypes.c_void_p or t is ctypes.c_char_p or hasattr(t, "contents") else t


def test_prototypes_agree():
    """dmx.h's prototypes against the argtypes dmx.py declares: the count, and per parameter a
    pointer or the same integer type"""
    hdr = open(os.path.join(ROOT, "include", "dmx.h")).read()
    lib = dmx.lib()
    for name in NAMES:
        m = re.search(r"^(size_t|int) %s\((.*?)\);" % name, hdr, re.S | re.M)
        assert m, name
        params = [c_kind(p) for p in m.group(2).replace("\n", " ").split(",")]
        fn = getattr(lib, name)
        assert [py_kind(t) for t in fn.argtypes] == params, name
        assert (fn.restype is ctypes.c_size_t) == (m.group(1) == "size_t"), name


def test_source_layout(tmp_path):
    assert ctypes.sizeof(dmx.ZipSource) == 40
    mine = [getattr(dmx.ZipSource, f).offset for f in FIELDS]
    assert mine == [0, 8, 16, 24, 28, 30, 32]
    src = tmp_path / "source.c"
    prints = "".join(f'    printf("%zu\\n", offsetof(dmx_zip_source, {f}));\n' for f in FIELDS)
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <dmx.h>\n"
                   'int main(void) {\n    printf("%zu\\n", sizeof(dmx_zip_source));\n' + prints + "    return 0;\n}\n")
    exe = tmp_path / "source"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [40] + mine


def test_null_context_is_an_argument_error():
    lib = dmx.lib()
    n = ctypes.c_size_t(123)
    src = dmx.zip_sources([0], [0], [b"a"])
    buf = ctypes.create_string_buffer(64)
    assert lib.dmx_zip_write_device(None, src, 1, 2, 0, None, 0, None, 0, None, ctypes.byref(n), None) == dmx.DMX_ERR_ARG
    assert lib.dmx_zip_write(None, src, 1, 2, 0, None, 0, buf, 64, None, ctypes.byref(n)) == dmx.DMX_ERR_ARG
    assert n.value == 123 and buf.raw == bytes(64)  # nothing was looked at


SUM_SRC = r"""
#include <cstdio>
#include "../../deflate.hpp_amd/csrc/zip_write.h"
using namespace dmx;
// stdin: force64 comment_len count, then per entry "name_len usize payload_bound"
int main() {
    unsigned long long f64, cl, count, nl, us, pb, local = 0, central = 0;
    if (std::scanf("%llu %llu %llu", &f64, &cl, &count) != 3) return 2;
    for (unsigned long long k = 0; k < count; k++) {
        if (std::scanf("%llu %llu %llu", &nl, &us, &pb) != 3) return 2;
        central += zipw_central_bytes((uint32_t)nl, us, pb, local, f64 != 0);
        local += zipw_local_bytes((uint32_t)nl, us, pb, f64 != 0) + pb;
    }
    std::printf("%llu\n", (unsigned long long)(local + central + zipw_end_bytes(count, central, local, cl, f64 != 0)));
    return 0;
}
"""


def header_sum(exe, entries, comment_len, force64):
    text = f"{int(force64)} {comment_len} {len(entries)}\n" + "".join(f"{a} {b} {c}\n" for a, b, c in entries)
    return int(subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout)


def test_bound_is_the_sum_of_the_header_sizes(tmp_path):
    src = tmp_path / "sum.cpp"
    src.write_text(SUM_SRC.replace("../../deflate.hpp_amd", os.path.join(ROOT, "deflate.hpp_amd")))
    exe = str(tmp_path / "sum")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", exe], check=True)
    big = 1 << 32
    shapes = [[], [(1, 0, 0)], [(5, 70000, 8), (4, 0, 0), (200, 17, 0), (65535, 3, 8)],
              [(3, big - 2, 0), (3, 5, 8)], [(3, big - 1, 8), (9, 7, 0), (1, 1, 0)], [(2, 1 << 40, 0), (2, 1 << 40, 8)],
              [(1, 1, 0)] * 65534, [(1, 1, 0)] * 65535]
    for entries in shapes:
        for force64 in (False, True):
            for comment_len in (0, 77):
                sizes = [n for _, n, _ in entries]
                names = [b"n" * nl for nl, _, _ in entries]
                methods = [m for _, _, m in entries]
                got = dmx.zip_bound(sizes, names, methods, comment=b"c" * comment_len, force64=force64)
                want = header_sum(exe, [(nl, n, dmx.deflate_bound(n) if m == 8 else n) for nl, n, m in entries],
                                  comment_len, force64)
                assert got == want, (entries[:4], force64, comment_len)
    assert dmx.zip_bound([], []) == 22


def test_bound_covers_every_cpu_archive():
    for label, (members, comment, force64, archive) in zw.assembled_plain().items():
        bound = dmx.zip_bound([len(d) for _, d, _, _ in members], [n for n, *_ in members],
                              [m for _, _, m, _ in members], comment=comment, force64=force64)
        assert bound >= len(archive), label
        if not any(m == 8 for _, _, m, _ in members):
            assert bound == len(archive), label  # nothing to bound: the size itself
