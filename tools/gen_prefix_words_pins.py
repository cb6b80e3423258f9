"""Record tests/golden/prefix_words_pins.json: length and SHA-256 of every level-2 stream of
tests/prefix_words_cases.py (plain, batch, dictionary batch, not-final, pipeline and 64 KiB calls,
own dictionaries, and the carried-state stream).

Run it on a GPU with the library whose output is to be pinned, selected with DMX_LIB (the commit
*before* a change that must keep the stream byte-identical: tools/ab_build.sh <parent> parent);
tests/test_gpu_prefix_words_pins.py compares later builds against the file.
usage: DMX_LIB=ab/libdmx_parent.so python tools/gen_prefix_words_pins.py [out.json]
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate.hpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prefix_words_cases as cases  # noqa: E402
from gen_run_probe_pins import contexts  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "prefix_words_pins.json")
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
