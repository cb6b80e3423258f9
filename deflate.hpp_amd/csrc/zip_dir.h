// zip_dir.h -- the directory of a ZIP archive (PKWARE APPNOTE 4.3, ZIP64 included), read in
// parallel: the steps the kernels of zip_dir.hip run, one call per "thread".  Plain C++, no HIP
// (DMX_HD as in container_parse.h): tests/cpp/zip_dir_test.cpp runs the same calls serially and
// compares with its own serial walk and with the table Python's zipfile states.
//
//   1. end record  the highest p in the last 65557 bytes where 50 4b 05 06 stands and the comment
//                  fits (zip_eocd_at); the ZIP64 locator and end record in front of it, the disk
//                  numbers, the base shift (zip_read_end)
//   2. candidates  every offset of the directory region where 50 4b 01 02 starts a record that
//                  lies inside the region, in offset order (zip_cd_candidate)
//   3. links, doubling, rank   bgzf_chain.h's generic steps over those candidates: a candidate's
//                  successor is the candidate at off + size, level k + 1 holds the 2^(k+1)-th
//                  successor, entry r is r hops behind candidate 0
//   4. chain       the walk from the region's first byte must end exactly at its end after as many
//                  records as the end record states (zip_chain_status); false signatures inside
//                  names, extras and comments are never counted, whatever chains they form
//   5. entry       the central record's fields with the ZIP64 extra 0x0001, the classification by
//                  flags and method, the local header (zip_entry)
//   6. layout      uoffset = the exclusive prefix sum of usize, as two 32-bit scans
//                  (zip_total)
// and, for the extraction, what becomes of an entry the caller hands back (zip_job).
//
// Every offset and length of the archive is untrusted: no function here reads a byte outside
// [in, in + n), and no sum of two archive values is formed before it is known not to wrap.
#pragma once
#include "bgzf_chain.h"  // BgzfCand and the generic chain steps (bgzf_link, bgzf_double, ...)

namespace dmx {

constexpr uint64_t kZipTailBytes = 22 + 65535;  // the end record and the longest archive comment
constexpr uint32_t kZipSigLocal = 0x04034B50u, kZipSigCentral = 0x02014B50u, kZipSigEnd = 0x06054B50u;
constexpr uint32_t kZipSigEnd64 = 0x06064B50u, kZipSigLoc64 = 0x07064B50u;
constexpr uint32_t kZip64Bytes = 56 + 20;  // the ZIP64 end record (no extensible data) and its locator

DMX_HD inline uint32_t zip_le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
DMX_HD inline uint64_t zip_le64(const uint8_t* p) { return (uint64_t)frame_le32(p) | ((uint64_t)frame_le32(p + 4) << 32); }

// What the end record says, and what the directory walk adds (entries, total, status)
struct ZipHead {
    uint64_t dir_off;   // the directory's first byte in the archive (base + the stated offset)
    uint64_t dir_size;  // its bytes: the directory is [dir_off, dir_off + dir_size)
    uint64_t count;     // the entries the end record states
    uint64_t base;      // bytes in front of the archive: every stated offset is shifted by it
    uint64_t total;     // the entries' plain bytes
    int32_t status;     // DMX_OK or DMX_ERR_DATA
    uint32_t zip64;     // the counts came from the ZIP64 end record
};
static_assert(sizeof(ZipHead) == 48, "the head is copied as one 48-byte record");

// ---- 1. the end record ----------------------------------------------------------------------
// the first position the search looks at
DMX_HD inline uint64_t zip_tail_start(uint64_t n) { return n > kZipTailBytes ? n - kZipTailBytes : 0; }

DMX_HD inline bool zip_eocd_at(const uint8_t* in, uint64_t n, uint64_t p) {
    if (p > n || n - p < 22) return false;
    if (frame_le32(in + p) != kZipSigEnd) return false;
    return zip_le16(in + p + 20) <= n - p - 22;
}

// The end record at p (zip_eocd_at holds).  Where the ZIP64 locator stands at p - 20 and the ZIP64
// end record directly in front of it, at p - 76, that record's count, size and offset are taken
// (Python's zipfile reads them there too).  DMX_ERR_DATA: a disk number other than 0, more than
// one disk, a directory that would begin in front of the archive's first byte.
DMX_HD inline int zip_read_end(const uint8_t* in, uint64_t n, uint64_t p, ZipHead* h) {
    (void)n;
    const uint8_t* const e = in + p;
    uint64_t count = zip_le16(e + 10), size = frame_le32(e + 12), off = frame_le32(e + 16);
    uint64_t end = p;  // where the directory ends
    bool z64 = false;
    if (p >= 20 && frame_le32(e - 20) == kZipSigLoc64) {
        if (frame_le32(e - 16) != 0 || frame_le32(e - 4) > 1) return DMX_ERR_DATA;  // the record's disk; disks
        if (p >= kZip64Bytes && frame_le32(e - kZip64Bytes) == kZipSigEnd64) {
            const uint8_t* const r = e - kZip64Bytes;
            if (frame_le32(r + 16) != 0 || frame_le32(r + 20) != 0) return DMX_ERR_DATA;  // this disk; the directory's
            count = zip_le64(r + 32);
            size = zip_le64(r + 40);
            off = zip_le64(r + 48);
            end = p - kZip64Bytes;
            z64 = true;
        }
    }
    if (!z64 && (zip_le16(e + 4) != 0 || zip_le16(e + 6) != 0)) return DMX_ERR_DATA;
    if (size > end || off > end - size) return DMX_ERR_DATA;  // (a negative base)
    h->dir_off = end - size;
    h->dir_size = size;
    h->count = count;
    h->base = end - size - off;
    h->zip64 = z64 ? 1u : 0u;
    return DMX_OK;
}

// ---- 2. central records -----------------------------------------------------------------------
// The candidate predicate: a record of the directory [d0, d1) starts at off.  d1 <= n.
DMX_HD inline bool zip_cd_candidate(const uint8_t* in, uint64_t d0, uint64_t d1, uint64_t off, BgzfCand* c) {
    if (off < d0 || off > d1 || d1 - off < 46) return false;
    const uint8_t* const r = in + off;
    if (frame_le32(r) != kZipSigCentral) return false;
    const uint64_t len = 46 + (uint64_t)zip_le16(r + 28) + zip_le16(r + 30) + zip_le16(r + 32);
    if (len > d1 - off) return false;
    c->off = off;
    c->size = (uint32_t)len;  // <= 46 + 3 * 65535
    c->isize = 0;
    return true;
}

// ---- 4. the chain -------------------------------------------------------------------------------
// J: the jump tables over the candidates, links made with bgzf_link(cands, ncand, i, d1).  *entries
// = the directory's records when the status is DMX_OK.  The end record's count is compared as it
// stands: 0xFFFF without a ZIP64 record is a count of 65535.
DMX_HD inline int zip_chain_status(const BgzfCand* cands, uint64_t ncand, const uint32_t* J, uint32_t levels,
                                   const ZipHead& h, uint64_t* entries) {
    *entries = 0;
    if (h.dir_size == 0) return h.count == 0 ? DMX_OK : DMX_ERR_DATA;
    if (ncand == 0 || cands[0].off != h.dir_off) return DMX_ERR_DATA;
    uint32_t last = 0;
    const uint64_t len = bgzf_chain_length(J, ncand, levels, &last);
    if (J[last] != kBgzfEnd || len != h.count) return DMX_ERR_DATA;
    *entries = len;
    return DMX_OK;
}

// ---- 5. one entry ---------------------------------------------------------------------------
// Flags and method: stored and deflate, not encrypted.  Bit 3 (data descriptor) needs nothing:
// sizes and CRC always come from the central directory.
DMX_HD inline int zip_classify(uint32_t gpflags, uint32_t method) {
    return ((gpflags & 1u) || (method != 0 && method != 8)) ? DMX_ERR_ARG : DMX_OK;
}

// The record c (a candidate of the directory) into e, all but uoffset.  The ZIP64 extra 0x0001
// supplies usize, csize and the local header's offset, in that order, for exactly the fields that
// read 0xFFFFFFFF; a subfield that overruns the extra, or a 0x0001 too short for them, is
// DMX_ERR_DATA (zipfile: "Corrupt extra field").  Then the local header at base + offset:
//   DMX_ERR_OVERREAD  the header, or data_off + csize, passes n
//   DMX_ERR_DATA      no 50 4b 03 04 there; a stored entry with csize != usize
// and DMX_ERR_ARG from zip_classify comes before both.  data_off is 0 where the local header did
// not give it.
DMX_HD inline void zip_entry(const uint8_t* in, uint64_t n, uint64_t base, const BgzfCand& c, ::dmx_zip_entry* e) {
    const uint8_t* const r = in + c.off;
    const uint32_t nl = zip_le16(r + 28), el = zip_le16(r + 30);
    uint64_t csize = frame_le32(r + 20), usize = frame_le32(r + 24), lho = frame_le32(r + 42);
    e->name_off = c.off + 46;
    e->crc = frame_le32(r + 16);
    e->dostime = zip_le16(r + 12) | (zip_le16(r + 14) << 16);
    e->name_len = (uint16_t)nl;
    e->method = (uint16_t)zip_le16(r + 10);
    e->gpflags = (uint16_t)zip_le16(r + 8);
    e->reserved = 0;
    e->uoffset = 0;
    e->path = 0;
    int st = DMX_OK;
    const uint8_t* x = r + 46 + nl;  // (inside the record: 46 + nl + el <= c.size)
    for (uint32_t left = el; left >= 4;) {
        const uint32_t id = zip_le16(x), sz = zip_le16(x + 2);
        if (sz + 4 > left) {
            st = DMX_ERR_DATA;
            break;
        }
        if (id == 1) {
            const uint32_t want = (usize == 0xFFFFFFFFull) + (csize == 0xFFFFFFFFull) + (lho == 0xFFFFFFFFull);
            if (8 * want > sz) {
                st = DMX_ERR_DATA;
                break;
            }
            const uint8_t* v = x + 4;
            if (usize == 0xFFFFFFFFull) usize = zip_le64(v), v += 8;
            if (csize == 0xFFFFFFFFull) csize = zip_le64(v), v += 8;
            if (lho == 0xFFFFFFFFull) lho = zip_le64(v);
        }
        x += 4 + sz;
        left -= 4 + sz;
    }
    e->csize = csize;
    e->usize = usize;
    e->data_off = 0;
    if (st == DMX_OK) st = zip_classify(e->gpflags, e->method);
    // the local header: its own name and extra lengths count, not the central record's
    int ls = DMX_OK;
    if (base > n || lho > n - base || n - (base + lho) < 30) {
        ls = DMX_ERR_OVERREAD;
    } else {
        const uint8_t* const l = in + base + lho;
        if (frame_le32(l) != kZipSigLocal) {
            ls = DMX_ERR_DATA;
        } else {
            const uint64_t d = base + lho + 30 + zip_le16(l + 26) + zip_le16(l + 28);
            if (d > n) {
                ls = DMX_ERR_OVERREAD;
            } else {
                e->data_off = d;
                if (csize > n - d) ls = DMX_ERR_OVERREAD;
                else if (e->method == 0 && csize != usize) ls = DMX_ERR_DATA;
            }
        }
    }
    e->status = st != DMX_OK ? st : ls;
}

// ---- 6. the layout ------------------------------------------------------------------------------
// The plain bytes from the totals of the two 32-bit scans (the low and the high halves of usize,
// fewer than 2^32 values each, so neither total wraps).  false: more than 2^63 bytes.
DMX_HD inline bool zip_total(uint64_t lo_total, uint64_t hi_total, uint64_t* total) {
    const uint64_t lim = 1ull << 63;
    if (hi_total > (1ull << 31)) return false;
    const uint64_t t = hi_total << 32;  // <= 2^63
    if (lo_total > lim - t) return false;
    *total = t + lo_total;
    return true;
}

// ---- extraction -------------------------------------------------------------------------------
// What the extraction does with an entry.  The entry comes from the caller and is untrusted again.
enum : uint32_t {
    ZIP_JOB_NONE = 0,     // nothing: *status says why
    ZIP_JOB_BATCH = 1,    // deflated, csize <= route_bytes: the batch decoder, one wavefront
    ZIP_JOB_COPY = 2,     // stored, csize <= route_bytes: the copy kernel
    ZIP_JOB_INFLATE = 3,  // deflated, above: the single-stream plan
    ZIP_JOB_MEMCPY = 4,   // stored, above: one device-to-device copy
};
DMX_HD inline uint32_t zip_job(const ::dmx_zip_entry& e, uint64_t n, uint64_t route_bytes, int* status) {
    int st = e.status;
    if (st == DMX_OK) st = zip_classify(e.gpflags, e.method);
    if (st == DMX_OK && (e.data_off > n || e.csize > n - e.data_off)) st = DMX_ERR_OVERREAD;
    if (st == DMX_OK && e.method == 0 && e.csize != e.usize) st = DMX_ERR_DATA;
    *status = st;
    if (st != DMX_OK) return ZIP_JOB_NONE;
    const bool big = e.csize > route_bytes;
    return e.method == 0 ? (big ? ZIP_JOB_MEMCPY : ZIP_JOB_COPY) : (big ? ZIP_JOB_INFLATE : ZIP_JOB_BATCH);
}

// The verdict on an entry that was decoded or copied: `status` and `bytes` as the decoder left
// them, ck the CRC-32 of the output (looked at only when verify).  A decoded size other than usize,
// or an output that did not fit its slot of usize bytes, is DMX_ERR_CHECKSUM with or without
// verification: the layout rests on usize (the BGZF ISIZE rule).
DMX_HD inline int zip_verdict(int status, uint64_t bytes, const ::dmx_zip_entry& e, bool verify, uint32_t ck) {
    if (status == DMX_ERR_CAPACITY || (status == DMX_OK && bytes != e.usize)) return DMX_ERR_CHECKSUM;
    if (status == DMX_OK && verify && ck != e.crc) return DMX_ERR_CHECKSUM;
    return status;
}

}  // namespace dmx
