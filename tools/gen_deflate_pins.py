"""Record tests/golden/deflate_pins.json: length and SHA-256 of ctx.compress() output for the
inputs of tests/deflate_pin_cases.py, per level and segment size.

Run it on a GPU with the build whose output is to be pinned (the commit *before* a change that
must keep the stream byte-identical); tests/test_gpu_deflate_pins.py compares later builds
against the file.  usage: python tools/gen_deflate_pins.py [out.json [cases_module]]

With a second argument another cases module of tests/ is recorded into out.json, e.g.
`tests/golden/parse_pins.json parse_pin_cases` for tests/test_gpu_parse_pins.py.  A module needs
SEGS, LEVELS and GROUPS; stale_lds() with STALE_SEG is recorded when it has one.
"""
import hashlib
import importlib
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate.hpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dmx  # noqa: E402

cases = importlib.import_module(sys.argv[2] if len(sys.argv) > 2 else "deflate_pin_cases")


def record(ctx, data, level):
    comp = ctx.compress(data, level)
    assert zlib.decompressobj(-15).decompress(comp) == data
    return [len(comp), hashlib.sha256(comp).hexdigest()]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "deflate_pins.json")
    ctxs = {seg: dmx.Context(segment_bytes=seg) for seg in cases.SEGS}
    pins = {"groups": {}}
    for group, make in cases.GROUPS.items():
        g = pins["groups"][group] = {}
        for name, data in make().items():
            e = g[name] = {"n": len(data), "input": hashlib.sha256(data).hexdigest(), "out": {}}
            for seg in cases.SEGS:
                for level in cases.LEVELS:
                    e["out"][f"L{level}_S{seg}"] = record(ctxs[seg], data, level)
    if hasattr(cases, "stale_lds"):
        data = cases.stale_lds()
        pins["stale_lds"] = {"n": len(data), "input": hashlib.sha256(data).hexdigest(),
                             "out": {f"L2_S{cases.STALE_SEG}": record(ctxs[cases.STALE_SEG], data, 2)}}
    for c in ctxs.values():
        c.close()
    with open(out, "w") as f:
        json.dump(pins, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out, sum(len(g) for g in pins["groups"].values()), "inputs")


if __name__ == "__main__":
    main()
