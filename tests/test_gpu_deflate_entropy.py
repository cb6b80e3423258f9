"""GPU: the deflate's entropy stage (deflate_kernels.hip: the histogram, em_build_codes, the
precode, the run-length header and the block-type compare of em_segment) against a sequential
model, symbol for symbol.

A round trip cannot see a code that is valid but not the documented one (a wrong rank gives a
short code to the wrong symbol: every decoder accepts it), nor a layout the lane decoder
declines (it is decoded again by the exact decoder: right bytes, lost speed).  So every emitted
segment is parsed bit by bit (tests/deflate_inspect.py) and compared with tests/huff_model.py,
which tests/test_huff_fit.py ties to the functions the kernels compile (csrc/huff_fit.h):

  (a) zlib decodes the stream to the input
  (b) the lit/len, distance and precode lengths equal the model's
  (c) so do HLIT, HDIST, HCLEN and the code-length symbols as written (16 / 17 / 18 and repeats)
  (d) so does the block type, and (e) the block's bits and the segment's bytes
  (f) the lane decoder's layout (inflate_lanes.hip), stated without the model: complete codes,
      lit/len <= 9, distance <= 6, precode <= 7 bits, codes for exactly the symbols that occur
      (two 1-bit codes where fewer than two occur), HLIT / HDIST end at the last coded symbol, no
      repeat across the HLIT / HDIST boundary, no 16 at the start of a sequence or behind a zero
  (g) the block is no larger than its tokens under the fixed code, nor than the stored form
  (h) the library's own inflate takes the stream on the lane path (stats().path == 4), with the
      heavy route off (heavy_bytes: every candidate goes to a lane, none to the workgroup decoder
      that the plan prefers for a stream of at most one candidate per CU), so that path 4 means
      the lane decoder itself accepted every segment.  The default context must give the bytes.
      (Measured with the default context on an MI355X: the level-1 streams whose lit/len code
      has one length for every byte value -- 3, 64, 128 or 130 equally frequent values, six used
      values -- leave path 4 and end on path 1 at 32 KiB segments: right bytes, slower route.)

Level 1 is Huffman-only: a segment's histogram is its byte histogram, so the level-1 inputs
(tests/entropy_cases.py) put chosen histograms in front of the code build -- tests/test_huff_fit.py
checks on the model that they reach the repair, the clamp and every arm of the header's run
plan -- and their tokens need not be decoded.  At levels 2 and 3 the parser decodes the tokens and
the model is fed with the histograms it finds."""
import os
import zlib

import pytest

import deflate_inspect as DI
import dmx
import entropy_cases as EC
import huff_model as HM

pytestmark = pytest.mark.gpu

PERM = DI.PERM


@pytest.fixture(scope="module")
def ctxs():
    c = {seg: dmx.Context(segment_bytes=seg) for seg in EC.SEGS}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def lanes():
    c = {seg: dmx.Context(segment_bytes=seg, heavy_bytes=1 << 30) for seg in (32768, 65536)}
    yield c
    for x in c.values():
        x.close()


def check_lane_path(ctx, lane_ctx, comp, data, what):
    """(h)"""
    assert ctx.decompress(comp) == data, what
    assert lane_ctx.decompress(comp) == data, what
    assert lane_ctx.stats().path == 4, f"{what}: inflate path {lane_ctx.stats().path}"


def _inflate(s):
    z = zlib.decompressobj(-15)
    out = z.decompress(s) + z.flush()
    assert z.eof and not z.unused_data
    return out


def _two_ones(lens, used):
    """The complete code of fewer than two used symbols: 1 bit for the highest used symbol (or
    symbol 0) and for symbol 0 (or 1)."""
    u = max(used) + 1 if used else 0
    want = [0] * len(lens)
    want[u - 1 if u else 0] = 1
    want[1 if u <= 1 else 0] = 1
    return list(lens) == want


def check_layout(g, nb, what):
    """(f) and (g): what the lane decoder takes and what the size compare promises, from the
    parsed segment alone."""
    b = g.block
    stored_bytes = 5 * (2 if nb > 65535 else 1) + nb + (0 if g.final else 5)
    assert g.end - g.start <= stored_bytes, f"{what}: larger than the stored form"
    if b.btype == 0:
        assert g.end - g.start == stored_bytes and sum(x.length for x in g.blocks) == nb, what
        return
    assert len(g.blocks) == 1, what
    assert b.bits <= DI.fixed_bits(b), f"{what}: larger than under the fixed code"
    if b.btype == 1:
        return
    lit, dist = b.litlens + [0] * (286 - b.hlit), b.distlens + [0] * (30 - b.hdist)
    assert max(lit) <= 9 and max(dist) <= 6 and max(b.prelens) <= 7, what
    assert DI.kraft(lit) == 32768 and DI.kraft(dist) == 32768 and DI.kraft(b.prelens) == 32768, f"{what}: incomplete code"
    for lens, hist in ((lit, b.lit_hist), (dist, b.dist_hist), (b.prelens, _pre_hist(b))):
        used = [s for s, f in enumerate(hist) if f]
        if len(used) >= 2:
            assert [s for s, l in enumerate(lens) if l] == used, f"{what}: codes and used symbols differ"
        else:
            assert _two_ones(lens, used), f"{what}: not the two 1-bit codes"
    assert b.hlit == max(257, max(s for s in range(286) if lit[s]) + 1), what
    assert b.hdist == max(s for s in range(30) if dist[s]) + 1, what
    assert b.hclen == max(4, max(i for i in range(19) if b.prelens[PERM[i]]) + 1), what
    pos, prev = 0, None
    for sym, rep in b.clsyms:
        if pos in (0, b.hlit):
            prev = None  # a sequence starts: nothing to repeat
        assert pos + rep <= b.hlit or pos >= b.hlit, f"{what}: a repeat straddles HLIT / HDIST"
        if sym == 16:
            assert prev not in (None, 0), f"{what}: a 16 with no non-zero length before it"
        else:
            prev = sym if sym < 16 else 0
        pos += rep
    assert pos == b.hlit + b.hdist, what


def _pre_hist(b):
    h = [0] * 19
    for sym, _ in b.clsyms:
        h[sym] += 1
    return h


def check_model(g, m, what):
    """(b) - (e): the parsed segment against the model's block."""
    b = g.block
    assert b.btype == m.btype, f"{what}: block type {b.btype}, the model says {m.btype}"
    assert g.end - g.start == m.nbytes, f"{what}: {g.end - g.start} bytes, the model says {m.nbytes}"
    if b.btype == 0:
        return
    assert b.bits == m.bits, f"{what}: {b.bits} bits, the model says {m.bits}"
    if b.btype == 1:
        return
    h = m.hdr
    assert (b.hlit, b.hdist, b.hclen) == (h.hlit, h.hdist, h.hclen), what
    assert b.litlens == m.litlens[:h.hlit], f"{what}: lit/len lengths differ from the model's"
    assert b.distlens == m.distlens[:h.hdist], f"{what}: distance lengths differ from the model's"
    assert b.prelens == h.prelens, f"{what}: precode lengths differ from the model's"
    assert b.clsyms == h.syms, f"{what}: code-length symbols differ from the model's"
    assert b.header_bits == 3 + h.bits, what


def check_stream(comp, parts, level, what, decode):
    """Checks (a) - (g) on a stream of the segments `parts`; returns the parsed segments."""
    data = b"".join(parts)
    assert _inflate(comp) == data, f"{what}: zlib does not decode the stream to the input"
    sizes = [len(p) for p in parts]
    if decode:
        out = bytearray()
        segs = DI.segments(comp, sizes, out=out)
        assert bytes(out) == data, what
    else:
        segs = DI.segments(comp, sizes, hists=[(HM.byte_hist(p), [0] * 30) for p in parts])
    assert sum(g.end - g.start for g in segs) == len(comp), what
    for i, (g, p) in enumerate(zip(segs, parts)):
        w = f"{what} segment {i}"
        assert g.final == (i + 1 == len(parts)), w
        check_layout(g, len(p), w)
        if g.block.btype == 0:
            if level > 1:
                continue  # (the tokens of a stored segment are not in the stream: no model input)
            lh, dh = HM.byte_hist(p), [0] * 30
        else:
            lh, dh = list(g.block.lit_hist), list(g.block.dist_hist)
            lh[256] -= 1
        if level == 1:
            assert sum(dh) == 0 and lh[:256] == HM.byte_hist(p)[:256], w
        check_model(g, HM.block(lh, dh, len(p), g.final), w)
    return segs


# ---- level 1: chosen histograms ---------------------------------------------------------------------
@pytest.mark.parametrize("seg", EC.SEGS)
def test_level1_families(ctxs, lanes, seg):
    ctx = ctxs[seg]
    types = set()
    for names, sizes, data in EC.level1_streams(seg):
        parts, o = [], 0
        for n in sizes:
            parts.append(data[o:o + n])
            o += n
        comp = ctx.compress(data, 1)
        what = f"level 1, {seg}-byte segments, {names}"
        segs = check_stream(comp, parts, 1, what, decode=False)
        types |= {g.block.btype for g in segs}
        for nm, g in zip(names, segs[:3]):
            if nm in ("uniform 256", "uniform 255"):
                assert g.block.btype == 0, what
            elif nm in ("uniform 1", "uniform 200", "near-uniform 255"):
                assert g.block.btype == 2, what
        if seg >= 32768:
            check_lane_path(ctx, lanes[seg], comp, data, what)
        if seg <= 32768:  # the batch kernels (16 and 32 KiB contexts), each segment a buffer of its own
            singles = [ctx.compress(p, 1) for p in parts]
            assert ctx.compress_batch(parts, 1) == singles, f"{what}: batch and single-stream bytes differ"
    assert {0, 2} <= types


# ---- the small-buffer sweep through the batch kernels -----------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    return EC.sweep_buffers(dmx.corpus("text", 1300))


@pytest.mark.parametrize("level", [1, 2])
def test_small_buffer_sweep(ctxs, sweep, level):
    outs = ctxs[32768].compress_batch([d for _, d in sweep], level)
    assert len(outs) == len(sweep) == 1800
    types = {a: set() for a in EC.SWEEP_ALPHABETS}
    for (alpha, d), comp in zip(sweep, outs):
        segs = check_stream(comp, [d], level, f"level {level}, {alpha}, {len(d)} bytes", decode=level > 1)
        types[alpha].add(segs[0].block.btype)
    if level == 1:  # what the model gives (test_huff_fit.py): stored needs byte values above 143
        assert types == {"two values": {1, 2}, "16 values geometric": {0, 1, 2}, "text": {1, 2}}


# ---- levels 2 and 3: the distance alphabet, mixed tokens ------------------------------------------
@pytest.fixture(scope="module")
def inputs23():
    return EC.level23_inputs(dmx.corpus("text", 32768), dmx.corpus("mixed", 32768, offset=49152))  # (across two of its 64 KiB pieces)


def _context(knob):
    old = os.environ.get("DMX_DEFLATE_PIPE")
    os.environ["DMX_DEFLATE_PIPE"] = knob
    try:
        return dmx.Context()
    finally:
        if old is None:
            del os.environ["DMX_DEFLATE_PIPE"]
        else:
            os.environ["DMX_DEFLATE_PIPE"] = old


@pytest.mark.parametrize("level", [2, 3])
def test_distance_alphabet(ctxs, lanes, inputs23, level):
    ctx = ctxs[32768]
    names, parts = list(inputs23), list(inputs23.values())
    data = b"".join(parts)
    comp = ctx.compress(data, level)
    what = f"level {level}, {names}"
    segs = check_stream(comp, parts, level, what, decode=True)
    by = dict(zip(names, segs))
    # what the inputs are there for
    for nm in ("zeros", "period 1"):
        assert [s for s, f in enumerate(by[nm].block.dist_hist) if f] == [0], nm
        assert by[nm].block.distlens == [1, 1], nm
    used = [s for s, f in enumerate(by["period 251"].block.dist_hist) if f]
    assert len(used) == 1 and used[0] < 29, ("period 251", used)
    assert [s for s, f in enumerate(by["period 25000"].block.dist_hist) if f] == [29]
    assert by["period 25000"].block.distlens == [1] + [0] * 28 + [1]  # 28 zeros between the two 1-bit codes
    b = by["30 distance symbols"].block
    assert sum(1 for f in b.dist_hist if f) >= 24 and sum(1 for l in b.distlens if l == 6) >= 4
    assert sum(1 for f in by["2 distance symbols"].block.dist_hist if f) == 2
    check_lane_path(ctx, lanes[32768], comp, data, what)
    # the same bytes by every route: the chunk pipeline against the single launch, and each
    # segment alone through the batch kernels against the single-stream call
    off, pipe = _context("0"), _context("s2")
    try:
        assert off.compress(data, level) == pipe.compress(data, level) == comp, "the pipeline's stream differs"
    finally:
        off.close()
        pipe.close()
    assert ctx.compress_batch(parts, level) == [ctx.compress(p, level) for p in parts]
