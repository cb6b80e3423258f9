"""CPU: the C-ABI of the seek index (dmx_seek_windows_bound, dmx_inflate_index_device,
dmx_inflate_range_device) and the layout of dmx_seek_entry.  No GPU work is launched: a null
context is rejected before anything else is looked at."""
import ctypes
import os
import subprocess

import dmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dmx_seek_windows_bound", "dmx_inflate_index_device", "dmx_inflate_range_device"]


def test_symbols_exported():
    lib = dmx.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in dmx.EXPORTS


def test_null_context_is_an_argument_error():
    lib = dmx.lib()
    count, out_len = ctypes.c_size_t(7), ctypes.c_size_t(9)
    entries = (dmx.SeekEntry * 2)()
    assert lib.dmx_inflate_index_device(None, None, 0, None, 0, 262144, entries, 2, None, 0, ctypes.byref(count),
                                        ctypes.byref(out_len), None) == dmx.DMX_ERR_ARG
    assert lib.dmx_inflate_range_device(None, None, 0, entries, 1, None, 0, 0, None, None) == dmx.DMX_ERR_ARG


def test_entry_layout(tmp_path):
    E = dmx.SeekEntry
    assert ctypes.sizeof(E) == 24
    assert (E.bit.offset, E.uoffset.offset, E.window.offset, E.flags.offset) == (0, 8, 16, 20)
    src = tmp_path / "entry.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <dmx.h>\n"
                   'int main(void){printf("%zu %zu %zu %zu %zu %u %u\\n", sizeof(dmx_seek_entry),'
                   " offsetof(dmx_seek_entry, bit), offsetof(dmx_seek_entry, uoffset),"
                   " offsetof(dmx_seek_entry, window), offsetof(dmx_seek_entry, flags),"
                   " DMX_SEEK_WINDOW, DMX_SEEK_NOWINDOW); return 0;}\n")
    exe = tmp_path / "entry"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [24, 0, 8, 16, 20, dmx.DMX_SEEK_WINDOW, dmx.DMX_SEEK_NOWINDOW]
    assert (dmx.DMX_SEEK_WINDOW, dmx.DMX_SEEK_NOWINDOW) == (32768, 1)


def test_windows_bound():
    lib = dmx.lib()
    for cap, spacing in ((0, 32768), (1, 32768), (32767, 32768), (32768, 32768), (4 << 20, 262144),
                         ((4 << 20) + 1, 262144), (256 << 20, 65536), (1 << 20, 1 << 30), (12345678, 100000)):
        assert lib.dmx_seek_windows_bound(cap, spacing) == (cap // spacing + 2) * 32768, (cap, spacing)
        assert dmx.seek_windows_bound(cap, spacing) == (cap // spacing + 2) * 32768
    # a spacing the index call refuses has no bound
    assert lib.dmx_seek_windows_bound(1 << 20, 32767) == 0
    assert lib.dmx_seek_windows_bound(1 << 20, 0) == 0
    # 12.5 % of the plain size at the default spacing (plus the two slots of slack)
    assert dmx.seek_windows_bound(256 << 20) == (256 << 20) // 8 + 65536
