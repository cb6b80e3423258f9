"""CPU: the batched entry points of include/dmx.h exist, reject a null context, and their
result struct has the header's layout.  No GPU work is launched here."""
import ctypes
import os
import subprocess

import dmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ["dmx_deflate_batch_device", "dmx_inflate_batch_device", "dmx_deflate_batch", "dmx_inflate_batch"]


def test_batch_symbols_exported():
    lib = dmx.lib()
    for s in BATCH:
        assert hasattr(lib, s), s
        assert s in dmx.EXPORTS


def test_batch_null_context_is_arg_error():
    lib = dmx.lib()
    one = (ctypes.c_void_p * 1)()
    n = (ctypes.c_size_t * 1)(0)
    res = (dmx.BatchResult * 1)()
    for count in (0, 1):
        assert lib.dmx_deflate_batch_device(None, one, n, count, 2, one, n, res, None) == dmx.DMX_ERR_ARG
        assert lib.dmx_inflate_batch_device(None, one, n, count, one, n, res, 0, None) == dmx.DMX_ERR_ARG
        assert lib.dmx_deflate_batch(None, one, n, count, 2, one, n, res) == dmx.DMX_ERR_ARG
        assert lib.dmx_inflate_batch(None, one, n, count, one, n, res, 0) == dmx.DMX_ERR_ARG


def test_batch_result_layout_matches_header(tmp_path):
    """dmx.BatchResult mirrors dmx_batch_result: 16 bytes, fields at 0, 8 and 12."""
    py = dmx.BatchResult
    fields = [f[0] for f in py._fields_]
    assert fields == ["bytes", "status", "path"]
    assert ctypes.sizeof(py) == 16
    assert [getattr(py, f).offset for f in fields] == [0, 8, 12]
    src = tmp_path / "layout.c"
    body = "".join(f'printf("{f} %zu\\n", offsetof(dmx_batch_result, {f}));' for f in fields)
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <dmx.h>\n"
                   f'int main(void){{{body} printf("sizeof %zu\\n", sizeof(dmx_batch_result)); return 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                        text=True).stdout.splitlines())
    for f in fields:
        assert int(got[f]) == getattr(py, f).offset, f
    assert int(got["sizeof"]) == ctypes.sizeof(py)


def test_batch_flag_values():
    hdr = open(os.path.join(ROOT, "include", "dmx.h")).read()
    assert "#define DMX_BATCH_NO_ROUTE 1u" in hdr
    assert dmx.DMX_BATCH_NO_ROUTE == 1 and dmx.BATCH_PATH == 6
