"""GPU: byte-identity pin of the level-2 streams of tests/run_probe_cases.py.

tests/golden/run_probe_pins.json holds the length and SHA-256 of every stream, recorded
(tools/gen_run_probe_pins.py) with the library of the commit before the front kernel's run test
moved in front of its round's table work ("Test first").  Which candidates a round
finds, and so which tokens a segment produces, must not depend on where in the round the test
runs: every stream equals its pin and decodes to its input with zlib's raw inflate.  The routes
cover the plain, batch, dictionary, not-final and pipeline kernels and the halves of 64 KiB
blocks; the carried-state streams alternate run, text and random segments inside the persistent
workgroups.
"""
import hashlib
import json
import os

import pytest

import dmx
import run_probe_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = json.load(open(os.path.join(ROOT, "tests", "golden", "run_probe_pins.json")))["routes"]


def _pipe_context():
    old = os.environ.get("DMX_DEFLATE_PIPE")
    os.environ["DMX_DEFLATE_PIPE"] = "s2"
    try:
        return dmx.Context(segment_bytes=32768)
    finally:
        if old is None:
            del os.environ["DMX_DEFLATE_PIPE"]
        else:
            os.environ["DMX_DEFLATE_PIPE"] = old


@pytest.fixture(scope="module")
def made():
    """Every stream, computed once."""
    ctxs = (dmx.Context(segment_bytes=32768), dmx.Context(segment_bytes=65536), _pipe_context())
    try:
        return cases.streams(*ctxs)
    finally:
        for c in ctxs:
            c.close()


def test_routes_are_the_pinned_ones(made):
    assert sorted(made) == sorted(PINS)
    routes = ("plain", "batch", "batch_dict", "not_final", "pipe", "halves")
    assert all(f"{g}/{r}" in PINS for g in cases.GROUPS for r in routes)


@pytest.mark.parametrize("route", sorted(PINS))
def test_pinned_streams(made, route):
    assert sorted(made[route]) == sorted(PINS[route]), route
    for name, (stream, data, zd, final) in made[route].items():
        pin = PINS[route][name]
        assert len(data) == pin["n"], name
        assert hashlib.sha256(data).hexdigest()[:16] == pin["input"], name
        cases.check(stream, data, zd, final)
        assert cases.digest(stream) == pin["out"], f"{route} {name}: stream differs from the pinned one"


def test_pipe_bundles_take_the_pipeline():
    """Five segments with chunks of two: three chunks; every input is in some bundle."""
    for make in cases.GROUPS.values():
        made = make()
        for k in (cases.PIPE_SEGMENTS, 2):
            b = cases.bundles(made, k)
            assert all(len(parts) == k for parts in b.values())
            assert all(len(made[p]) == cases.N for parts in b.values() for p in parts[:-1])
            assert {p for parts in b.values() for p in parts} == set(made)
