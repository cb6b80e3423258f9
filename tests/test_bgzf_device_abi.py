"""CPU: the C-ABI of the BGZF device calls (dmx_deflate_bgzf_device, dmx_bgzf_index_device,
dmx_inflate_bgzf_device, dmx_inflate_bgzf_range_device) and dmx.gzi_bytes.  No GPU work is launched:
a null context is rejected before anything else is looked at."""
import ctypes
import os
import struct
import subprocess

import numpy as np

import dmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dmx_deflate_bgzf_device", "dmx_bgzf_index_device", "dmx_inflate_bgzf_device",
         "dmx_inflate_bgzf_range_device"]


def test_symbols_exported():
    lib = dmx.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in dmx.EXPORTS


def test_null_context_is_an_argument_error():
    lib = dmx.lib()
    n = ctypes.c_size_t(123)
    m = ctypes.c_size_t(5)
    entry = (dmx.BgzfEntry * 2)()
    assert lib.dmx_deflate_bgzf_device(None, None, 0, 1, None, 0, ctypes.byref(n), None) == dmx.DMX_ERR_ARG
    assert lib.dmx_bgzf_index_device(None, None, 0, entry, 2, ctypes.byref(m), None, None) == dmx.DMX_ERR_ARG
    assert lib.dmx_inflate_bgzf_device(None, None, 0, 0, None, 0, ctypes.byref(n), None) == dmx.DMX_ERR_ARG
    assert lib.dmx_inflate_bgzf_range_device(None, None, 0, entry, 1, 0, 0, 0, None, None) == dmx.DMX_ERR_ARG


def test_entry_layout(tmp_path):
    assert ctypes.sizeof(dmx.BgzfEntry) == 16
    assert (dmx.BgzfEntry.coffset.offset, dmx.BgzfEntry.uoffset.offset) == (0, 8)
    src = tmp_path / "entry.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <dmx.h>\n"
                   'int main(void){printf("%zu %zu %zu\\n", sizeof(dmx_bgzf_entry), offsetof(dmx_bgzf_entry, coffset),'
                   " offsetof(dmx_bgzf_entry, uoffset)); return 0;}\n")
    exe = tmp_path / "entry"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [16, 0, 8]


def test_gzi_bytes_matches_a_hand_packed_example():
    # three members at 0, 1000 and 1500 of a 1528-byte file (the last one empty), 70000 plain bytes
    index = np.array([[0, 0], [1000, 65280], [1500, 70000], [1528, 70000]], dtype=np.uint64)
    want = (b"\x02\x00\x00\x00\x00\x00\x00\x00"
            b"\xe8\x03\x00\x00\x00\x00\x00\x00" b"\x00\xff\x00\x00\x00\x00\x00\x00"
            b"\xdc\x05\x00\x00\x00\x00\x00\x00" b"\x70\x11\x01\x00\x00\x00\x00\x00")
    assert dmx.gzi_bytes(index) == want
    assert struct.unpack("<Q", dmx.gzi_bytes(index)[:8])[0] == 2
    # one member: only the count; the empty file's index (the sentinel alone) as well
    assert dmx.gzi_bytes(np.array([[0, 0], [28, 0]], dtype=np.uint64)) == b"\x00" * 8
    assert dmx.gzi_bytes(np.array([[0, 0]], dtype=np.uint64)) == b"\x00" * 8
