"""GPU: byte-identity pin of the deflate output on the inputs of tests/parse_pin_cases.py.

tests/golden/parse_pins.json holds the length and SHA-256 of ctx.compress() output, recorded
(tools/gen_deflate_pins.py tests/golden/parse_pins.json parse_pin_cases) with the build before
the level-2 parse took match lengths from a proven terminal run and before its literal skip
looked several bitmap words ahead.  Both only remove work, so every stream stays as it was, at
levels 2 and 3 and at every segment size; every stream must also decode to its input with
zlib's raw inflate.  The mechanism is that of tests/test_gpu_deflate_pins.py.
"""
import hashlib
import json
import os
import zlib

import pytest

import dmx
import parse_pin_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = json.load(open(os.path.join(ROOT, "tests", "golden", "parse_pins.json")))


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
            assert len(data) == pins[name]["n"] <= 65536, name
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
