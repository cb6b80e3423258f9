"""GPU: byte-identity pin of the level-2 streams of tests/prefix_words_cases.py.

tests/golden/prefix_words_pins.json holds the length and SHA-256 of every stream, recorded
(tools/gen_prefix_words_pins.py) with the library of the commit before a run segment's literal
prefix was worded in closed form and before the proving round's exit lost its barrier (DESIGN 4.1,
"Prefix words in closed form").  Regrouping literals into words changes no token, so every stream
equals its pin and decodes to its input with zlib's raw inflate.  The inputs vary the prefix
length fm - D over 0 .. 4 (zeros-like), the bitmap-word edges 31 .. 33 and 95 .. 97, 251, the
thread count's 1023 .. 1025 and 3251 (more prefix words than threads), at full and ragged segment
lengths, behind dictionaries of 1, 33 and 4096 bytes; runs that are not terminal and run-free
segments keep the old grouping; the carried-state streams alternate five kinds of segment inside
the persistent workgroups.  The routes are the plain, batch, dictionary, not-final and pipeline
kernels and the halves of 64 KiB blocks.

A literal token exactly at fm needs no fingerprint collision and so no search: a match bit in the
last two positions of a parse chunk is clipped below three bytes (periods 256, 257, 514, 515; see
prefix_words_cases).  tests/test_prefix_words_model.py covers the rule on the CPU.
"""
import hashlib
import json
import os

import pytest

import dmx
import prefix_words_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = json.load(open(os.path.join(ROOT, "tests", "golden", "prefix_words_pins.json")))["routes"]


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


@pytest.mark.gpu
def test_routes_are_the_pinned_ones(made):
    assert sorted(made) == sorted(PINS)
    routes = ("plain", "batch", "batch_dict", "not_final", "pipe", "halves")
    assert all(f"{g}/{r}" in PINS for g in cases.GROUPS for r in routes)
    assert {"own_dict/batch_dict", "carried/plain", "carried/pipe", "carried/batch"} <= set(PINS)


@pytest.mark.gpu
@pytest.mark.parametrize("route", sorted(PINS))
def test_pinned_streams(made, route):
    assert sorted(made[route]) == sorted(PINS[route]), route
    for name, (stream, data, zd, final) in made[route].items():
        pin = PINS[route][name]
        assert len(data) == pin["n"], name
        assert hashlib.sha256(data).hexdigest()[:16] == pin["input"], name
        cases.check(stream, data, zd, final)
        assert cases.digest(stream) == pin["out"], f"{route} {name}: stream differs from the pinned one"


def _first_repeat(data):
    """The first position whose four bytes occurred before (the first match bit, collisions and
    evicted table entries apart); len(data) without one."""
    seen = set()
    for q in range(len(data) - 3):
        k = data[q:q + 4]
        if k in seen:
            return q
        seen.add(k)
    return len(data)


def test_inputs_have_the_intended_prefix_lengths():
    """(CPU) fm - D of the periodic inputs is their period; of the long head, head + period."""
    made = cases.prefix_lengths()
    for p in cases.PREFIXES:
        for n in cases.lengths(p):
            assert _first_repeat(made[f"p{p}_{n}"]) == p, (p, n)
    assert _first_repeat(cases.long_head()) == cases.LONG_HEAD + 251
    assert (cases.LONG_HEAD + 251 + 2) // 3 > 1024
    assert _first_repeat(made[f"p{cases.LONG_HEAD}_{cases.N}"]) == cases.LONG_HEAD
    for name, data in cases.literal_at_fm().items():
        head = 1000 if name.startswith("rnd") else 0
        p = int(next(x for x in name.split("_") if x.startswith("p"))[1:])
        assert _first_repeat(data) == head + p and (p % 258) in (256, 257), name
    for name, (zd, data) in cases.own_dicts().items():
        assert len(zd) + len(data) <= cases.N
        if "across" in name:
            # the image is periodic across the dictionary's end: the input's first byte has a match
            # wherever four bytes of the period lie before it; with a shorter dictionary, once they do
            p = int(name.rsplit("_p", 1)[1])
            assert _first_repeat(zd + data) <= max(len(zd), p)


def test_bundles_hold_every_input():
    for make in cases.GROUPS.values():
        made = make()
        for k in (cases.PIPE_SEGMENTS, 2):
            b = cases.bundles(made, k)
            assert all(len(parts) == k for parts in b.values())
            assert all(len(made[p]) == cases.N for parts in b.values() for p in parts[:-1])
            assert {p for parts in b.values() for p in parts} == set(made)
