"""GPU: byte-identity pin of the level-2 streams of tests/tail_pin_cases.py.

tests/golden/tail_pins.json holds the length and SHA-256 of every stream, recorded
(tools/gen_tail_pins.py) with the library of the commit before segments with a terminal run wrote
their token words per bitmap word ("Run-segment token writer").  The entropy stage
codes each token word on its own, so regrouping the literals into other words leaves every
stream as it was; every stream must also decode to its input with zlib's raw inflate.  The
groups cover the plain, batch and dictionary kernels and the halves of 64 KiB blocks.
"""
import hashlib
import json
import os

import pytest
import torch

import dmx
import tail_pin_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = json.load(open(os.path.join(ROOT, "tests", "golden", "tail_pins.json")))["groups"]
GROUPS = list(cases.GROUPS) + ["batch", "batch_dict", "halves", "neighbours"]


@pytest.fixture(scope="module")
def ctxs():
    c = {seg: dmx.Context(segment_bytes=seg) for seg in (32768, 65536)}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def made(ctxs):
    """Every stream, computed once."""
    return cases.streams(ctxs[32768], ctxs[65536])


@pytest.mark.parametrize("group", GROUPS)
def test_pinned_streams(made, group):
    assert sorted(made[group]) == sorted(PINS[group]), group
    for name, (stream, data, zd) in made[group].items():
        pin = PINS[group][name]
        assert len(data) == pin["n"] <= 65536, name
        assert hashlib.sha256(data).hexdigest() == pin["input"], name
        assert cases.inflate(stream, zd) == data, f"{group} {name}: does not decode to its input"
        assert cases.digest(stream) == pin["out"], f"{group} {name}: stream differs from the pinned one"


def test_path_neighbours(ctxs, made):
    """(2G + 1) segments, G the front kernel's grid: every workgroup takes a run segment, a
    run-free one and a run segment in turn, or the other way round.  The segments' streams
    concatenate bytewise, so the stream is put together from the pinned streams of group
    neighbours (test_pinned_streams), which are the same on every GPU: a segment that is not the
    last is what the two-segment prefix starting with it holds before its last segment."""
    G = torch.cuda.get_device_properties(0).multi_processor_count
    kinds = cases.neighbour_kinds(G, 2 * G + 1)
    assert kinds[:5] == [0, 1, 0, 1, 0] and kinds[G:G + 2] == [1, 0] and kinds[2 * G] == 0
    nb = made["neighbours"]
    seg = [nb["run"][1], nb["free"][1]]
    last = [nb["run"][0], nb["free"][0]]
    two = [nb["prefix"][0], nb["prefix_free_first"][0]]
    assert two[0].endswith(last[1]) and two[1].endswith(last[0])
    mid = [two[0][:-len(last[1])], two[1][:-len(last[0])]]
    data = b"".join(seg[k] for k in kinds)
    comp = ctxs[32768].compress(data, cases.LEVEL)
    assert cases.inflate(comp) == data
    assert comp.startswith(two[0][:-len(last[1])])  # the fixed prefix against its pin
    assert comp == b"".join(mid[k] for k in kinds[:-1]) + last[kinds[-1]]
