"""Record tests/golden/run_probe_pins.json: length and SHA-256 of every level-2 stream of
tests/run_probe_cases.py (plain, batch, dictionary batch, not-final, pipeline and 64 KiB calls,
and the carried-state stream).

Run it on a GPU with the library whose output is to be pinned, selected with DMX_LIB (the commit
*before* a change that must keep the stream byte-identical: tools/ab_build.sh <parent> parent);
tests/test_gpu_run_probe_pins.py compares later builds against the file.
usage: DMX_LIB=ab/libdmx_parent.so python tools/gen_run_probe_pins.py [out.json]
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate.hpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dmx  # noqa: E402
import run_probe_cases as cases  # noqa: E402


def contexts():
    """(32 KiB, 64 KiB, 32 KiB with the pipeline forced to chunks of two segments)"""
    old = os.environ.get("DMX_DEFLATE_PIPE")
    os.environ["DMX_DEFLATE_PIPE"] = "s2"
    try:
        pipe = dmx.Context(segment_bytes=32768)
    finally:
        if old is None:
            del os.environ["DMX_DEFLATE_PIPE"]
        else:
            os.environ["DMX_DEFLATE_PIPE"] = old
    return dmx.Context(segment_bytes=32768), dmx.Context(segment_bytes=65536), pipe


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "run_probe_pins.json")
    ctxs = contexts()
    pins = {"routes": {}}
    for route, made in cases.streams(*ctxs).items():
        r = pins["routes"][route] = {}
        for name, (stream, data, zd, final) in made.items():
            cases.check(stream, data, zd, final)
            r[name] = {"n": len(data), "input": hashlib.sha256(data).hexdigest()[:16], "out": cases.digest(stream)}
    for c in ctxs:
        c.close()
    with open(out, "w") as f:
        json.dump(pins, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out, sum(len(r) for r in pins["routes"].values()), "streams")


if __name__ == "__main__":
    main()
