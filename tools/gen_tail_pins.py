"""Record tests/golden/tail_pins.json: length and SHA-256 of every level-2 stream of
tests/tail_pin_cases.py (plain, batch, dictionary batch, 64 KiB halves, path neighbours).

Run it on a GPU with the library whose output is to be pinned, selected with DMX_LIB (the commit
*before* a change that must keep the stream byte-identical: tools/ab_build.sh <parent> parent);
tests/test_gpu_tail_pins.py compares later builds against the file.
usage: DMX_LIB=ab/libdmx_parent.so python tools/gen_tail_pins.py [out.json]
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate.hpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dmx  # noqa: E402
import tail_pin_cases as cases  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "tail_pins.json")
    ctx32, ctx64 = dmx.Context(segment_bytes=32768), dmx.Context(segment_bytes=65536)
    pins = {"groups": {}}
    for group, made in cases.streams(ctx32, ctx64).items():
        g = pins["groups"][group] = {}
        for name, (stream, data, zd) in made.items():
            assert cases.inflate(stream, zd) == data, name
            g[name] = {"n": len(data), "input": hashlib.sha256(data).hexdigest(), "out": cases.digest(stream)}
    ctx32.close()
    ctx64.close()
    with open(out, "w") as f:
        json.dump(pins, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out, sum(len(g) for g in pins["groups"].values()), "streams")


if __name__ == "__main__":
    main()
