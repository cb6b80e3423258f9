"""CPU: tests/deflate_inspect.py, the bit-level DEFLATE reader of the entropy-stage tests, against
zlib.  On zlib's own raw streams (tests/streams.py: levels 1, 6 and 9, strategies default,
Z_FIXED, Z_HUFFMAN_ONLY and Z_RLE) the reader's decoded bytes equal zlib's, its blocks tile the
stream bit for bit, every dynamic block carries complete codes (zlib writes no others, but for a
distance code of a single 1-bit symbol), and a block's token bits follow from its histogram and
lengths -- which is how the reader skips the tokens of a block whose histogram the caller knows."""
import zlib

import pytest

import deflate_inspect as DI
import dmx
from streams import zlib_raw

STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman": zlib.Z_HUFFMAN_ONLY,
              "rle": zlib.Z_RLE}
N = 70000


@pytest.fixture(scope="module")
def inputs():
    d = {k: dmx.corpus(k, N) for k in ("text", "mixed", "zeros", "random", "repeat")}
    d["empty"], d["one"] = b"", b"x"
    return d


def _inflate(s):
    z = zlib.decompressobj(-15)
    out = z.decompress(s) + z.flush()
    assert z.eof and not z.unused_data
    return out


@pytest.mark.parametrize("strategy", list(STRATEGIES))
@pytest.mark.parametrize("level", [1, 6, 9])
def test_reader_agrees_with_zlib(inputs, level, strategy):
    for name, data in inputs.items():
        s = zlib_raw(data, level, 8, STRATEGIES[strategy])
        out = bytearray()
        bl = DI.blocks(s, out)
        assert bytes(out) == _inflate(s) == data, name
        # the blocks tile the stream: each starts where the one before ends, the last is the only
        # final one, and the stream is its end rounded up to a byte
        assert bl[0].start == 0 and all(a.end == b.start for a, b in zip(bl, bl[1:])), name
        assert [b.bfinal for b in bl] == [0] * (len(bl) - 1) + [1], name
        assert sum(b.bits for b in bl) == bl[-1].end and (bl[-1].end + 7) // 8 == len(s), name
        if strategy == "fixed":
            assert all(b.btype in (0, 1) for b in bl), name
        for b in bl:
            if b.btype == 0:
                continue
            assert b.bits == 3 + (b.header_bits - 3) + b.token_bits
            assert b.lit_hist[256] == 1
            if b.btype == 2:
                assert b.hlit == len(b.litlens) and b.hdist == len(b.distlens) and 4 <= b.hclen <= 19
                assert sum(rep for _, rep in b.clsyms) == b.hlit + b.hdist
                assert DI.kraft(b.litlens) == 32768 and DI.kraft(b.prelens) == 32768, name
                used = [l for l in b.distlens if l]
                assert DI.kraft(b.distlens) == 32768 or used in ([], [1]), name
            # the same block with its histogram given: the tokens are skipped, the end is the same
            q = DI.read_block(s, b.start, hist=(b.lit_hist, b.dist_hist))
            assert (q.end, q.token_bits, q.header_bits) == (b.end, b.token_bits, b.header_bits), name


def test_reader_rejects_a_wrong_histogram(inputs):
    s = zlib_raw(inputs["text"][:5000], 6, 8, zlib.Z_HUFFMAN_ONLY)
    b = DI.blocks(s)[0]
    h = list(b.lit_hist)
    h[ord("e")] -= 1
    with pytest.raises(DI.FormatError):
        DI.read_block(s, 0, hist=(h, b.dist_hist))


def test_segments_layout():
    """The libdmx layout, written here with zlib: a block per segment, the empty stored block
    behind each but the last (Z_FULL_FLUSH writes exactly that)."""
    parts = [dmx.corpus("text", 3000), dmx.corpus("random", 700), dmx.corpus("mixed", 1234)]
    z = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    s = b"".join(z.compress(p) + z.flush(zlib.Z_FULL_FLUSH) for p in parts[:-1]) + z.compress(parts[-1]) + z.flush()
    out = bytearray()
    segs = DI.segments(s, [len(p) for p in parts], out=out)
    assert bytes(out) == b"".join(parts)
    assert [g.final for g in segs] == [False, False, True]
    assert segs[0].start == 0 and segs[-1].end == len(s) and all(a.end == b.start for a, b in zip(segs, segs[1:]))
    with pytest.raises(DI.FormatError):
        DI.segments(s + b"\0", [len(p) for p in parts])
