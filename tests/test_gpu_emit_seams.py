"""GPU: the emission stage (deflate_kernels.hip: em_segment, em_build_codes) at the seams of its
own bookkeeping, bit for bit against the sequential model (tests/huff_model.py through the
checks of tests/test_gpu_deflate_entropy.py: zlib decodes the stream to the input, lengths, header
symbols, block type, bits and bytes equal the model's).

What the stage keeps between its passes, and where that can go wrong:
  * the first block of 256 token words stays in registers from the histogram to the packing pass:
    level-1 segments of exactly 255, 256 and 257 words (and the byte counts around them), the last
    of which is the first to read a second block from memory;
  * a 64-symbol chunk without a used symbol is passed over by the code build: a level-2 repeat
    segment and a zeros segment (one literal, one length, one distance symbol);
  * the ranking ballots run over the values a chunk holds: the histograms of
    tests/entropy_cases.py that reach the Kraft repair, the clamp and every arm of the run plan;
  * the staging window is cleared as far as the block reaches: a 32 KiB text segment, whose block
    is flushed several times, and blocks that end within a word of the flush threshold
    (256 staged words = 8192 bits), on either side of it.

Every input goes through the plain path at 16, 32 and 64 KiB segments, the level-2 streams also
through the chunk pipeline with chunks of one and of two segments (three full segments and a tail:
the last chunk is one segment either way, once alone and once behind a chunk of two), and every
segment through the batch kernels as a buffer of its own, two buffers per call.  The pipeline's
stream and the batch's buffers must be the plain 32 KiB path's bytes."""
import os

import numpy as np
import pytest

import dmx
import entropy_cases as EC
import huff_model as HM
from test_gpu_deflate_entropy import check_stream

pytestmark = pytest.mark.gpu

SEG = 32768
FLUSH_BITS = 32 * 256  # em_segment flushes the staging window once it holds 256 whole words

# the level-1 histograms of entropy_cases.py by what they reach (tests/test_huff_fit.py shows on the
# model that they do): the repair, the clamp, the arms of the run plan
FAMILIES = (["near-uniform 130", "near-uniform 200", "near-uniform 255", "uniform 130"] +
            ["geometric 0.5", "fibonacci 22", "one value at 99 %", "16 frequent + 240 rare"] +
            list(EC.ZERO_RUNS) + list(EC.EQUAL_RUNS))


def _context(knob, **kw):
    old = os.environ.get("DMX_DEFLATE_PIPE")
    os.environ["DMX_DEFLATE_PIPE"] = knob
    try:
        return dmx.Context(**kw)
    finally:
        if old is None:
            del os.environ["DMX_DEFLATE_PIPE"]
        else:
            os.environ["DMX_DEFLATE_PIPE"] = old


@pytest.fixture(scope="module")
def ctxs():
    c = {seg: _context("0", segment_bytes=seg) for seg in EC.SEGS}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def pipes():
    c = {knob: _context(knob) for knob in ("s1", "s2")}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def text():
    return dmx.corpus("text", 3 * SEG)


def _split(data, seg):
    return [data[o:o + seg] for o in range(0, len(data), seg)]


def _batch_pairs(ctx, parts, level):
    """every buffer through dmx_deflate_batch, two buffers per call"""
    out = []
    for i in range(0, len(parts), 2):
        out += ctx.compress_batch(parts[i:i + 2], level)
    return out


def check_paths(ctxs, pipes, data, level, what, decode):
    """The stream of `data` by every route; returns the parsed segments of the plain 32 KiB path."""
    parts = _split(data, SEG)
    comp = ctxs[SEG].compress(data, level)
    segs = check_stream(comp, parts, level, f"{what}, 32 KiB", decode)
    for seg in (16384, 65536):
        if len(data) <= 16384:  # one short segment: the same layout at every segment size
            assert ctxs[seg].compress(data, level) == comp, f"{what}, {seg}-byte segments"
        else:
            check_stream(ctxs[seg].compress(data, level), _split(data, seg), level, f"{what}, {seg}", decode)
    if level >= 2:
        for knob, p in pipes.items():
            assert p.compress(data, level) == comp, f"{what}: the pipeline's stream ({knob}) differs"
    singles = [ctxs[SEG].compress(p, level) for p in parts]
    for seg in (16384, SEG):
        if seg == SEG or max(len(p) for p in parts) <= 16384:
            assert _batch_pairs(ctxs[seg], parts, level) == singles, f"{what}: batch ({seg}) and single-stream bytes differ"
    if len(parts) > 1:  # a segment alone is a final block: checked against the model too
        for i, (p, s) in enumerate(zip(parts, singles)):
            check_stream(s, [p], level, f"{what}, segment {i} alone", decode)
    return segs


# ---- the first block in registers: 255, 256, 257 token words ----------------------------------------
@pytest.mark.parametrize("nbytes", [1017, 1020, 1021, 1023, 1024, 1025, 1028, 2048, 2049])
def test_level1_word_counts(ctxs, pipes, text, nbytes):
    assert (nbytes + 3) // 4 in (255, 256, 257, 512, 513)
    segs = check_paths(ctxs, pipes, text[100:100 + nbytes], 1, f"level 1, {nbytes} bytes", decode=False)
    assert segs[0].block.btype == 2


def test_level1_word_counts_in_one_batch(ctxs, text):
    """the same counts side by side in the waves of one workgroup (four segments each)"""
    parts = [text[7 * n:8 * n] for n in (1020, 1024, 1028, 1021, 1025, 3, 1024, 1019)]
    ctx = ctxs[SEG]
    assert ctx.compress_batch(parts, 1) == [ctx.compress(p, 1) for p in parts]


# ---- blocks that end at the flush threshold ---------------------------------------------------------
def _sixteen_values(n):
    return np.random.default_rng(41).integers(0x30, 0x40, n, dtype=np.uint8).tobytes()


def _bits(p):
    return HM.block(HM.byte_hist(p), [0] * 30, len(p), True).bits


def test_flush_threshold(ctxs, pipes):
    """Level 1 over sixteen equally frequent values: four bits a byte, so a byte more moves the
    block's end by four bits.  The model picks the lengths whose block (header, tokens, end of
    block) ends from a word below the threshold to a word above it."""
    lo = next(n for n in range(1800, 2200) if _bits(_sixteen_values(n)) >= FLUSH_BITS - 40)
    picked = []
    for n in range(lo, lo + 24):
        p = _sixteen_values(n)
        bits = _bits(p)
        if abs(bits - FLUSH_BITS) > 44:
            continue
        picked.append(bits)
        segs = check_paths(ctxs, pipes, p, 1, f"level 1, 16 values, {n} bytes ({bits} bits)", decode=False)
        assert segs[0].block.btype == 2 and segs[0].block.bits == bits
    assert min(picked) < FLUSH_BITS - 32 and max(picked) > FLUSH_BITS + 32 and len(picked) >= 16
    assert any(FLUSH_BITS - 12 <= b < FLUSH_BITS for b in picked) and any(FLUSH_BITS <= b < FLUSH_BITS + 12 for b in picked)


# ---- level 2: chunks without a used symbol, a block of many flushes ---------------------------------
@pytest.mark.parametrize("level", [2, 3])
def test_level2_segments(ctxs, pipes, text, level):
    parts = [dmx.corpus("repeat", SEG), bytes(SEG), text[:SEG], text[SEG + 500:SEG + 1521]]
    segs = check_paths(ctxs, pipes, b"".join(parts), level, f"level {level}, repeat + zeros + text + tail", decode=True)
    assert [g.block.btype for g in segs[:3]] == [2, 2, 2]
    rep, zer, txt = (g.block for g in segs[:3])
    # what the inputs are there for: 64-symbol chunks of the lit/len alphabet without a used
    # symbol (zeros: the literal 0, the end of block and the lengths only), one distance symbol,
    # and a block of several times the flush threshold
    assert not any(zer.lit_hist[64:256]) and sum(1 for f in zer.dist_hist if f) == 1
    assert rep.bits < FLUSH_BITS  # (a block that never flushes: cleared only as far as it reaches)
    assert txt.bits > 8 * FLUSH_BITS


# ---- the histograms that reach the repair, the clamp and every arm of the run plan ------------------
@pytest.mark.parametrize("first", range(0, len(FAMILIES), 3))
def test_level1_histograms(ctxs, pipes, first):
    names = FAMILIES[first:first + 3]
    parts = [EC.shuffled(EC.counts(EC.FAMILIES[nm], SEG), 977 + first + k) for k, nm in enumerate(names)]
    parts.append(EC.shuffled(EC.counts(EC.FAMILIES[names[0]], 1021), first))
    check_paths(ctxs, pipes, b"".join(parts), 1, f"level 1, {names}", decode=False)
