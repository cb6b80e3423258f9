"""CPU: the C-ABI of the ZIP calls (dmx_zip_index_device, dmx_zip_extract_device,
dmx_inflate_zip_device, dmx_zip_index, dmx_inflate_zip) and the layout of dmx_zip_entry.  No GPU work
is launched: a null context is rejected before anything else is looked at."""
import ctypes
import os
import subprocess

import dmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dmx_zip_index_device", "dmx_zip_extract_device", "dmx_inflate_zip_device", "dmx_zip_index",
         "dmx_inflate_zip"]
FIELDS = ["name_off", "data_off", "csize", "usize", "uoffset", "crc", "dostime", "name_len", "method", "gpflags",
          "reserved", "status", "path"]


def test_symbols_exported():
    lib = dmx.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in dmx.EXPORTS


def test_null_context_is_an_argument_error():
    lib = dmx.lib()
    n, m = ctypes.c_size_t(123), ctypes.c_size_t(5)
    plain = ctypes.c_uint64(7)
    ent = (dmx.ZipEntry * 2)()
    res = (dmx.BatchResult * 2)()
    buf = ctypes.create_string_buffer(64)
    assert lib.dmx_zip_index_device(None, None, 0, ent, 2, ctypes.byref(m), ctypes.byref(plain), None) == dmx.DMX_ERR_ARG
    assert lib.dmx_zip_extract_device(None, None, 0, ent, 2, None, 0, 0, None, 0, res, ctypes.byref(n),
                                      None) == dmx.DMX_ERR_ARG
    assert lib.dmx_inflate_zip_device(None, None, 0, 0, None, 0, ent, 2, ctypes.byref(m), ctypes.byref(n),
                                      None) == dmx.DMX_ERR_ARG
    assert lib.dmx_zip_index(None, buf, 64, ent, 2, ctypes.byref(m), ctypes.byref(plain)) == dmx.DMX_ERR_ARG
    assert lib.dmx_inflate_zip(None, buf, 64, 0, buf, 64, ent, 2, ctypes.byref(m), ctypes.byref(n)) == dmx.DMX_ERR_ARG
    # nothing was looked at: the outputs are as they were
    assert (n.value, m.value, plain.value) == (123, 5, 7)


def test_entry_layout(tmp_path):
    assert ctypes.sizeof(dmx.ZipEntry) == 64
    mine = [getattr(dmx.ZipEntry, f).offset for f in FIELDS]
    assert mine == [0, 8, 16, 24, 32, 40, 44, 48, 50, 52, 54, 56, 60]
    src = tmp_path / "entry.c"
    prints = "".join(f'    printf("%zu\\n", offsetof(dmx_zip_entry, {f}));\n' for f in FIELDS)
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <dmx.h>\n"
                   'int main(void) {\n    printf("%zu\\n", sizeof(dmx_zip_entry));\n' + prints + "    return 0;\n}\n")
    exe = tmp_path / "entry"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [64] + mine
