"""CPU: the seeded lenient / edge-case streams (tests/lenient_streams.py) are what they claim
to be, and the oracle is pinned to the compiled reference on them.

The GPU differential test (test_gpu_lenient.py) takes its expected bytes and errors from the
oracle at test time; this file checks, against the oracle alone, that the families reach the
rules they aim at, and that the oracle's outputs are the reference's: directly where the
reference build (oracle/_ref) is present, and through the digests make_golden.py --lenient
recorded from it (tests/golden/lenient_manifest.json) everywhere else.
"""
import json
import os

import pytest

import lenient_streams as LS
from oracle_bind import Reference

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAN = json.load(open(os.path.join(GOLD, "lenient_manifest.json")))
OVERREAD, DATA = -1, -2


def _errors(fam, code):
    return [c for c, (_, e) in zip(LS.cases(fam), LS.expected_all(fam)) if e == code]


@pytest.mark.parametrize("fam", LS.FAMILIES)
def test_generator_is_deterministic(fam):
    assert MAN["cases_per_family"] == LS.N_CASES
    assert LS.streams_digest(fam) == MAN["families"][fam]["streams_sha256"]


@pytest.mark.parametrize("fam", LS.FAMILIES)
def test_case_limits(fam):
    for c, (out, _) in zip(LS.cases(fam), LS.expected_all(fam)):
        assert len(c.stream) <= LS.MAX_STREAM
        assert out is None or len(out) <= LS.MAX_OUT


def test_interesting_block_starts_at_four_bit_offsets():
    assert {c.block[0] for c in LS.cases("prefix")} == {0, 1, 2, 3}  # bits 0, 10, 20, 30


@pytest.mark.parametrize("fam", [f for f in LS.FAMILIES if f != "truncated"])
def test_at_least_half_of_a_family_decodes(fam):
    ok = sum(e is None for _, e in LS.expected_all(fam))
    print(f"{fam}: {ok} of {LS.N_CASES} decode")
    assert 2 * ok >= LS.N_CASES


def test_families_yield_the_errors_they_name():
    # incomplete: the marked subset steps onto an unassigned prefix
    bad = [c for c in _errors("incomplete", DATA) if c.bad]
    assert len(bad) >= 8
    # fixedodd: a stored block one byte longer than the input left
    assert len([c for c in _errors("fixedodd", OVERREAD) if "toolong" in c.note]) >= 8
    # truncated: over-reads, and at least 8 of them end on real bits that lie on an unassigned
    # prefix (the lookup model: those bits followed by zeros hit at no length) -- the streams
    # on which "no code" and "out of input" compete
    over = _errors("truncated", OVERREAD)
    assert len(over) >= 8
    assert len([c for c in over if c.unassigned]) >= 8


def test_families_reach_the_rules_they_aim_at():
    ok = {f: [c for c, (_, e) in zip(LS.cases(f), LS.expected_all(f)) if e is None] for f in LS.FAMILIES}
    # symbols 286 / 287 get codes (HLIT 287, 288) and overshoot reaches the highest index a
    # repeat can write, 292 (see the module doc of lenient_streams: 300 is out of reach)
    assert max(c.max_sym for c in ok["prefix"]) == 287
    assert max(c.max_sym for c in ok["overshoot"]) == 292
    assert len([c for c in ok["overshoot"] if c.max_sym > 287]) >= 8
    # over-subscription: decodable cases of all three places, collisions among them
    assert len([c for c in ok["oversub"] if "precode" in c.note]) >= 8
    assert len([c for c in ok["oversub"] if "collision" in c.note]) >= 8
    # the header reader's refill: at least 10 % of longheader beyond 1938 bits of code lengths
    long_ = [c for c in LS.cases("longheader") if c.hdr_bits > LS.LONG_BITS]
    print(f"longheader: {len(long_)} of {LS.N_CASES} beyond {LS.LONG_BITS} bits")
    assert 10 * len(long_) >= LS.N_CASES
    # fixedodd's stored-block edges all occur in decodable cases
    for kind in ("len0", "len1", "nlen", "rest"):
        assert len([c for c in ok["fixedodd"] if kind in c.note.split()]) >= 8, kind
    # some cases copy from before their own output, most do not (the dictionary batch test
    # drops the ones that reach beyond a 1 KiB dictionary: under 10 %)
    for f in LS.FAMILIES:
        far = sum(c.far_by > 1024 for c in LS.cases(f))
        assert 10 * far < LS.N_CASES, f
    assert sum(c.far_by > 0 for c in LS.cases("prefix")) >= 8


def test_rfc_mode_results():
    """oracle.inflate(rfc=True) per case, as the rfc_strict GPU routes expect it: RFC 1951's
    single code-length sequence rejects the overshoot and most of the sixteen family; where the
    two readings agree on the code lengths (prefix) the results are equal."""
    assert LS.expected_all("prefix", rfc=True) == LS.expected_all("prefix")
    for fam in ("overshoot", "sixteen"):
        diff = sum(a != b for a, b in zip(LS.expected_all(fam, rfc=True), LS.expected_all(fam)))
        print(f"{fam}: RFC mode differs on {diff} of {LS.N_CASES}")
        assert diff >= LS.N_CASES // 2


@pytest.mark.parametrize("fam", LS.FAMILIES)
def test_oracle_gives_the_recorded_reference_results(fam):
    """The reference's results, recorded by make_golden.py --lenient, reach machines without the
    reference build this way: the oracle's outputs have the recorded digest."""
    outs = [out for out, _ in LS.expected_all(fam)]
    assert sum(o is not None for o in outs) == MAN["families"][fam]["decoded"]
    assert LS.records_digest(outs) == MAN["families"][fam]["reference_records_sha256"]


@pytest.mark.skipif(not Reference.available(), reason="oracle/_ref not built (no reference headers)")
@pytest.mark.parametrize("fam", LS.FAMILIES)
def test_oracle_equals_compiled_reference(fam):
    """Decodable cases only: on the oracle's error cases the reference is undefined (or reads
    past its buffer) and is not called."""
    ref = Reference()
    for c, (out, err) in zip(LS.cases(fam), LS.expected_all(fam)):
        if err is None:
            assert ref.decompress(c.stream) == out, (fam, c.note)
