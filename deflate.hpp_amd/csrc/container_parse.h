// container_parse.h -- zlib (RFC 1950), gzip (RFC 1952) and BGZF framing: the header parse, the
// header / trailer writers and the BGZF chain step.  Plain C++, no HIP: DMX_HD is empty under g++
// and __host__ __device__ under hipcc, so the code the frame kernels run (frame_batch.hip) is the
// code tests/test_container_parse.py checks on the CPU, sanitizers included.
//
// No function here reads a byte at or beyond in + n.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/dmx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DMX_HD __host__ __device__
#else
#define DMX_HD
#endif

namespace dmx {

constexpr uint32_t kBgzfBlock = 65280;  // input bytes per BGZF member (htslib's 0xff00)
constexpr uint32_t kBgzfEofBytes = 28;  // the empty member that ends a BGZF file

// One buffer's framing, as the parse found it; also the side record the framed batch calls keep
// per buffer on the device (ck: the checksum kernel's value).
struct FrameHead {
    uint64_t head;    // bytes before the raw stream (the raw stream is [head, n): like
                      // dmx_inflate_zlib / _gzip, the decoder is given the trailer too and stops
                      // at the final block)
    uint32_t want;    // the trailer's Adler-32 / CRC-32
    uint32_t isize;   // gzip: the trailer's ISIZE
    int32_t status;   // DMX_OK, DMX_ERR_OVERREAD or DMX_ERR_DATA
    uint32_t member;  // gzip: BSIZE + 1 of the BC subfield (the member's size), 0 = none
    uint32_t ck;      // Adler-32 / CRC-32 computed on the device
    uint32_t pad_;
};
static_assert(sizeof(FrameHead) == 32, "the side array is copied as 32-byte records");

DMX_HD inline uint32_t frame_head_bytes(uint32_t format) {
    return format == DMX_FRAME_ZLIB ? 2u : format == DMX_FRAME_GZIP ? 10u : format == DMX_FRAME_BGZF ? 18u : 0u;
}
DMX_HD inline uint32_t frame_tail_bytes(uint32_t format) {
    return format == DMX_FRAME_ZLIB ? 4u : (format == DMX_FRAME_GZIP || format == DMX_FRAME_BGZF) ? 8u : 0u;
}

DMX_HD inline uint32_t frame_le32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// Header checks of dmx_inflate_zlib / dmx_inflate_gzip, in their order:
//   zlib: n < 6 -> OVERREAD; CM != 8, CINFO > 7, FCHECK or FDICT -> DATA.
//   gzip: n < 18 -> OVERREAD; magic or CM -> DATA; FEXTRA, FNAME, FCOMMENT, FHCRC skipped; a
//         header that leaves fewer than 8 bytes for the trailer (XLEN past the end, an
//         unterminated name) -> OVERREAD.
//   BGZF: a gzip member that passes the above, then DATA unless its FEXTRA holds the BC subfield
//         (SI 66 67, SLEN 2) with BSIZE + 1 == n.
DMX_HD inline FrameHead parse_frame(uint32_t format, const uint8_t* in, uint64_t n) {
    FrameHead h{};
    if (format == DMX_FRAME_ZLIB) {
        if (n < 6) {
            h.status = DMX_ERR_OVERREAD;
            return h;
        }
        const uint32_t cmf = in[0], flg = in[1];
        if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (cmf * 256 + flg) % 31 != 0 || (flg & 0x20)) {
            h.status = DMX_ERR_DATA;  // (FDICT: preset dictionaries are not framed)
            return h;
        }
        h.head = 2;
        const uint8_t* t = in + n - 4;
        h.want = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | (uint32_t)t[3];
        return h;
    }
    if (n < 18) {
        h.status = DMX_ERR_OVERREAD;
        return h;
    }
    if (in[0] != 0x1F || in[1] != 0x8B || in[2] != 8) {
        h.status = DMX_ERR_DATA;
        return h;
    }
    const uint32_t flg = in[3];
    uint64_t head = 10;
    h.status = DMX_ERR_OVERREAD;  // until the header is known to leave room for the trailer
    if (flg & 4) {                // FEXTRA (bytes 10 and 11 exist: n >= 18)
        const uint64_t x0 = 12, x1 = x0 + ((uint32_t)in[10] | ((uint32_t)in[11] << 8));
        if (x1 + 8 > n) return h;
        for (uint64_t p = x0; p + 4 <= x1;) {  // subfields: SI1 SI2 SLEN data
            const uint32_t slen = (uint32_t)in[p + 2] | ((uint32_t)in[p + 3] << 8);
            if (in[p] == 66 && in[p + 1] == 67 && slen == 2 && p + 6 <= x1) {
                h.member = ((uint32_t)in[p + 4] | ((uint32_t)in[p + 5] << 8)) + 1;
                break;
            }
            p += 4 + (uint64_t)slen;
        }
        head = x1;
    }
    for (int z = 0; z < 2; z++) {  // FNAME, FCOMMENT: zero-terminated
        if (flg & (8u << z)) {
            while (head < n && in[head]) head++;
            head++;
            if (head + 8 > n) return h;
        }
    }
    if (flg & 2) head += 2;  // FHCRC
    if (head + 8 > n) return h;
    if (format == DMX_FRAME_BGZF && h.member != n) {
        h.status = DMX_ERR_DATA;
        return h;
    }
    h.status = DMX_OK;
    h.head = head;
    h.want = frame_le32(in + n - 8);
    h.isize = frame_le32(in + n - 4);
    return h;
}

// The gzip header alone, for a member whose end is not given (dmx_inflate_gzip_members): the
// checks and skips of parse_frame's gzip branch without the trailer reads.  in[0, avail) is what
// is left of the file; *head = the bytes before the raw stream.
//   DMX_ERR_DATA      in[0] != 1f, or avail >= 2 and in[1] != 8b, or avail >= 3 and in[2] != 8
//   DMX_ERR_OVERREAD  the header, or the header plus an 8-byte trailer, does not fit in avail
// No byte at or beyond in + avail is read.
DMX_HD inline int gzip_head_len(const uint8_t* in, uint64_t avail, uint64_t* head) {
    *head = 0;
    if (avail == 0) return DMX_ERR_OVERREAD;
    if (in[0] != 0x1F || (avail >= 2 && in[1] != 0x8B) || (avail >= 3 && in[2] != 8)) return DMX_ERR_DATA;
    if (avail < 18) return DMX_ERR_OVERREAD;
    const uint32_t flg = in[3];
    uint64_t h = 10;
    if (flg & 4) {  // FEXTRA (bytes 10 and 11 exist: avail >= 18)
        h = 12 + (uint64_t)((uint32_t)in[10] | ((uint32_t)in[11] << 8));
        if (h + 8 > avail) return DMX_ERR_OVERREAD;
    }
    for (int z = 0; z < 2; z++) {  // FNAME, FCOMMENT: zero-terminated
        if (flg & (8u << z)) {
            while (h < avail && in[h]) h++;
            h++;
            if (h + 8 > avail) return DMX_ERR_OVERREAD;
        }
    }
    if (flg & 2) h += 2;  // FHCRC
    if (h + 8 > avail) return DMX_ERR_OVERREAD;
    *head = h;
    return DMX_OK;
}

// The header dmx_deflate_zlib / dmx_deflate_gzip write for `level` (frame_head_bytes(format) bytes
// at out); BGZF: the gzip header with FEXTRA = the BC subfield, BSIZE = member - 1.
DMX_HD inline void frame_write_head(uint32_t format, int level, uint32_t member, uint8_t* out) {
    const int lv = (level < 0 || level > 3) ? 1 : level;
    if (format == DMX_FRAME_ZLIB) {
        const uint32_t flevel = lv <= 1 ? 0 : lv == 2 ? 1 : 3;  // RFC 1950 FLEVEL
        const uint32_t cmf = 0x78, flg0 = flevel << 6;
        out[0] = (uint8_t)cmf;
        out[1] = (uint8_t)(flg0 + (31 - (cmf * 256 + flg0) % 31) % 31);
        return;
    }
    out[0] = 0x1F;
    out[1] = 0x8B;
    out[2] = 8;
    out[3] = format == DMX_FRAME_BGZF ? 4 : 0;
    out[4] = out[5] = out[6] = out[7] = 0;  // MTIME
    out[8] = (uint8_t)(lv == 3 ? 2 : lv <= 1 ? 4 : 0);
    out[9] = 255;
    if (format == DMX_FRAME_BGZF) {
        const uint32_t bsize = member - 1;
        out[10] = 6;  // XLEN
        out[11] = 0;
        out[12] = 66;
        out[13] = 67;
        out[14] = 2;
        out[15] = 0;
        out[16] = (uint8_t)bsize;
        out[17] = (uint8_t)(bsize >> 8);
    }
}

// The trailer (frame_tail_bytes(format) bytes at out): ck = the plain bytes' Adler-32 / CRC-32
DMX_HD inline void frame_write_tail(uint32_t format, uint32_t ck, uint64_t n, uint8_t* out) {
    if (format == DMX_FRAME_ZLIB) {
        for (int b = 0; b < 4; b++) out[b] = (uint8_t)(ck >> (24 - 8 * b));
        return;
    }
    for (int b = 0; b < 4; b++) out[b] = (uint8_t)(ck >> (8 * b));
    for (int b = 0; b < 4; b++) out[4 + b] = (uint8_t)(n >> (8 * b));
}

// One step of the BGZF chain walk: the member that starts at `off` of a file of n bytes.
//   fewer than 18 bytes left, a header or a BSIZE that runs past n -> DMX_ERR_OVERREAD (a cut chain)
//   bad magic, no BC subfield, a BSIZE too small for the header and trailer -> DMX_ERR_DATA
struct BgzfMember {
    uint64_t off, size;  // the member is [off, off + size)
    uint32_t isize;      // its trailer's ISIZE
};
DMX_HD inline int bgzf_next(const uint8_t* in, uint64_t n, uint64_t off, BgzfMember* m) {
    if (off > n || n - off < 18) return DMX_ERR_OVERREAD;
    const FrameHead h = parse_frame(DMX_FRAME_GZIP, in + off, n - off);
    if (h.status != DMX_OK) return h.status;
    if (!h.member) return DMX_ERR_DATA;
    if (h.member > n - off) return DMX_ERR_OVERREAD;
    if (h.member < h.head + 8) return DMX_ERR_DATA;
    m->off = off;
    m->size = h.member;
    m->isize = frame_le32(in + off + h.member - 4);
    return DMX_OK;
}

}  // namespace dmx
