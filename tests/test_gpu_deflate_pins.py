"""GPU: byte-identity pin of our own deflate output.

tests/golden/deflate_pins.json holds the length and SHA-256 of ctx.compress() output, recorded
(tools/gen_deflate_pins.py) with the build before the front kernel ended its match rounds at
a terminal run.  Changes to the front kernel that only remove work must leave
every stream as it was, at levels 2 and 3 and at every segment size; every stream must also
decode to its input with zlib's raw inflate, an independent CPU check.  The inputs
(tests/deflate_pin_cases.py) are runs that reach the segment end, start late, stop 1..5 bytes
short of it or break in the middle, run-free corpora, and one long stream in which each
persistent workgroup alternates between run segments and run-free ones (stale LDS).
"""
import hashlib
import json
import os
import zlib

import pytest

import dmx
import deflate_pin_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = json.load(open(os.path.join(ROOT, "tests", "golden", "deflate_pins.json")))


@pytest.fixture(scope="module")
def ctxs():
    c = {seg: dmx.Context(segment_bytes=seg) for seg in cases.SEGS}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def inputs():
    """Every group's inputs, built once and checked against the recorded input hashes."""
    made = {}
    for group, make in cases.GROUPS.items():
        made[group] = make()
        pins = PINS["groups"][group]
        assert sorted(made[group]) == sorted(pins), group
        for name, data in made[group].items():
            assert len(data) == pins[name]["n"], name
            assert hashlib.sha256(data).hexdigest() == pins[name]["input"], name
    return made


def check(ctx, data, level, pin, what):
    comp = ctx.compress(data, level)
    z = zlib.decompressobj(-15)
    assert z.decompress(comp) == data and z.eof and not z.unused_data, f"{what}: does not decode to its input"
    assert [len(comp), hashlib.sha256(comp).hexdigest()] == pin, f"{what}: stream differs from the pinned one"


@pytest.mark.parametrize("group", list(cases.GROUPS))
@pytest.mark.parametrize("level", cases.LEVELS)
@pytest.mark.parametrize("seg", cases.SEGS)
def test_pinned_streams(ctxs, inputs, seg, level, group):
    key = f"L{level}_S{seg}"
    for name, data in inputs[group].items():
        check(ctxs[seg], data, level, PINS["groups"][group][name]["out"][key], f"{name} {key}")


def test_pinned_stale_lds(ctxs):
    pin = PINS["stale_lds"]
    data = cases.stale_lds()
    assert len(data) == pin["n"] and hashlib.sha256(data).hexdigest() == pin["input"]
    key = f"L2_S{cases.STALE_SEG}"
    check(ctxs[cases.STALE_SEG], data, 2, pin["out"][key], f"stale_lds {key}")
