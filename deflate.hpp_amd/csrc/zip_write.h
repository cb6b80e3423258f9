// zip_write.h -- writing a ZIP archive (PKWARE APPNOTE 4.3, ZIP64 included) in parallel: the records
// and the steps the kernels of zip_write.hip run, one call per "thread".  Plain C++, no HIP (DMX_HD
// as in container_parse.h): tests/cpp/zip_write_test.cpp runs the same calls serially, hands the
// archives to Python's zipfile and reads them back with zip_dir.h's own steps.
//
//   1. sizes    csize = the batch deflate's result (method 8) or the plain size (method 0); the
//               local record = header + name [+ ZIP64 extra] + csize bytes (zipw_csize,
//               zipw_local_bytes)
//   2. layout   local_off = the exclusive prefix sum of the local records, as two 32-bit scans;
//               the central record's bytes, which depend on local_off (zipw_central_bytes), and
//               their prefix sum; the directory starts where the local records end, the end
//               records behind it (zipw_layout)
//   3. pack     the payloads cut into chunks of kZipwChunk bytes whose interior starts are 16-byte
//               aligned in the destination: workgroup w finds its entry in the prefix sum of the
//               host's chunk bounds (zipw_find) and its byte range (zipw_chunk)
//   4. records  the local header, the central record, the written table's row (zipw_write_local,
//               zipw_write_central, zipw_row); the end records (zipw_write_end)
//
// Sizes and CRC are known before a header is written: flag bit 3 is never set and no data
// descriptor is written.  There is no entry comment and no extra other than 0x0001.
#pragma once
#include "zip_dir.h"

namespace dmx {

constexpr uint32_t kZipwDosTime = 0x00210000u;  // 1980-01-01 00:00:00, where the caller gives 0
// Payload bytes per pack workgroup (a multiple of 16): 16 stores of 16 bytes per lane of a
// 256-thread workgroup.  Measured (profiles/zip_write_probe.json): 64 entries of 16 MiB
// pack at the rate of a device-to-device copy of as many bytes; no other size was tried.
constexpr uint32_t kZipwChunk = 65536;
constexpr uint64_t kZipw32 = 0xFFFFFFFFull;

DMX_HD inline void zipw_le16(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
}
DMX_HD inline void zipw_le32(uint8_t* p, uint32_t v) {
    zipw_le16(p, v);
    zipw_le16(p + 2, v >> 16);
}
DMX_HD inline void zipw_le64(uint8_t* p, uint64_t v) {
    zipw_le32(p, (uint32_t)v);
    zipw_le32(p + 4, (uint32_t)(v >> 32));
}

// One entry as the records state it
struct ZipwEntry {
    const uint8_t* name;
    uint32_t name_len;  // 1..65535
    uint32_t method, gpflags, dostime, crc;
    uint64_t usize, csize;
};

// One entry as the host uploads it, beside desc[k] = {plain input, n, payload source, its bound}
struct ZipwSrc {
    uint64_t name_off;  // the name's first byte in the name blob
    uint64_t uoffset;   // the prefix sum of n: the written table's uoffset
    uint32_t dostime;   // as written (kZipwDosTime where the caller gave 0)
    uint32_t dres;      // method 8: the index of its batch deflate result
    uint16_t name_len, method, gpflags, pad_;
};
static_assert(sizeof(ZipwSrc) == 32, "the upload image is built from 8-byte words");

// What the pack launch leaves for the host
struct ZipwHead {
    uint64_t bytes;    // the archive's bytes (DMX_ERR_CAPACITY: the size needed)
    uint64_t cd_off;   // the central directory's first byte = the local records' bytes
    uint64_t cd_size;
    int32_t status;    // DMX_OK, DMX_ERR_CAPACITY or the first failing entry's status
    uint32_t pad_;
};
static_assert(sizeof(ZipwHead) == 32, "the head is copied as one 32-byte record");

// ---- arguments ----------------------------------------------------------------------------------
// (a name above 65535 bytes is rejected where name_len is still wider than 16 bits)
DMX_HD inline int zipw_check_source(uint32_t name_len, uint32_t method) {
    return (name_len == 0 || name_len > 65535 || (method != 0 && method != 8)) ? DMX_ERR_ARG : DMX_OK;
}

// bit 11 (UTF-8) iff the name holds a byte above 127
DMX_HD inline uint32_t zipw_flags(const uint8_t* name, uint32_t len) {
    for (uint32_t i = 0; i < len; i++)
        if (name[i] > 127) return 0x800u;
    return 0;
}

// external attributes: the DOS directory bit for a name that ends in '/'
DMX_HD inline uint32_t zipw_attr(const uint8_t* name, uint32_t len) { return len && name[len - 1] == '/' ? 0x10u : 0u; }

// ---- the records' sizes ---------------------------------------------------------------------------
// "big": the entry's sizes go to the ZIP64 extra and both 32-bit fields read 0xFFFFFFFF
DMX_HD inline bool zipw_big(uint64_t usize, uint64_t csize, bool force64) {
    return force64 || usize >= kZipw32 || csize >= kZipw32;
}
// the local header in front of the payload: 30 bytes, the name, the extra {0x0001, 16, usize, csize}
DMX_HD inline uint32_t zipw_local_bytes(uint32_t name_len, uint64_t usize, uint64_t csize, bool force64) {
    return 30 + name_len + (zipw_big(usize, csize, force64) ? 20u : 0u);
}
DMX_HD inline bool zipw_off64(uint64_t local_off, bool force64) { return force64 || local_off >= kZipw32; }
// the central record: 46 bytes, the name, the extra {0x0001, 8 * fields, [usize, csize,] [local_off]}
DMX_HD inline uint32_t zipw_central_bytes(uint32_t name_len, uint64_t usize, uint64_t csize, uint64_t local_off,
                                          bool force64) {
    const uint32_t fields = (zipw_big(usize, csize, force64) ? 2u : 0u) + (zipw_off64(local_off, force64) ? 1u : 0u);
    return 46 + name_len + (fields ? 4 + 8 * fields : 0u);
}
// the ZIP64 end record and its locator are written
DMX_HD inline bool zipw_end64(uint64_t count, uint64_t cd_size, uint64_t cd_off, bool force64) {
    return force64 || count >= 0xFFFFull || cd_size >= kZipw32 || cd_off >= kZipw32;
}
DMX_HD inline uint64_t zipw_end_bytes(uint64_t count, uint64_t cd_size, uint64_t cd_off, uint64_t comment_len,
                                      bool force64) {
    return (zipw_end64(count, cd_size, cd_off, force64) ? kZip64Bytes : 0u) + 22 + comment_len;
}

// ---- 1. sizes -----------------------------------------------------------------------------------
// res: the batch deflate's results over the method 8 entries.  The status is the deflate's for a
// deflated entry; a failed one has no payload.
DMX_HD inline int zipw_csize(const ZipwSrc& s, uint64_t n, const ::dmx_batch_result* res, uint64_t* csize) {
    if (s.method == 0) {
        *csize = n;
        return DMX_OK;
    }
    const int st = res[s.dres].status;
    *csize = st == DMX_OK ? res[s.dres].bytes : 0;
    return st;
}

// ---- 2. layout ------------------------------------------------------------------------------------
// local_total and cd_total: the totals of the scans (local_total from its two halves; the sum of
// real buffers' sizes does not wrap).  fail_key: the minimum of k << 32 | (uint32_t)status over the
// failing entries, all ones where there is none.
DMX_HD inline ZipwHead zipw_layout(uint64_t count, uint64_t local_total, uint64_t cd_total, uint64_t comment_len,
                                   bool force64, unsigned long long fail_key, uint64_t cap) {
    ZipwHead h;
    h.cd_off = local_total;
    h.cd_size = cd_total;
    h.bytes = local_total + cd_total + zipw_end_bytes(count, cd_total, local_total, comment_len, force64);
    h.status = fail_key != ~0ull ? (int)(uint32_t)fail_key : h.bytes > cap ? DMX_ERR_CAPACITY : DMX_OK;
    h.pad_ = 0;
    return h;
}

// ---- 3. the pack's chunks -------------------------------------------------------------------------
// The workgroups an entry of at most `bytes` payload bytes is given: its chunks at every
// destination alignment, one at least (workgroup 0 of an entry also writes its records).
DMX_HD inline uint64_t zipw_chunk_bound(uint64_t bytes, uint64_t chunk) { return (bytes + 15) / chunk + 1; }

// first[0 .. count]: the exclusive prefix sum of the entries' chunk bounds (each >= 1, so the sums
// rise strictly).  The entry workgroup w < first[count] belongs to: the last k with first[k] <= w.
DMX_HD inline uint64_t zipw_find(const uint64_t* first, uint64_t count, uint64_t w) {
    uint64_t lo = 0, hi = count;  // first[lo] <= w < first[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Chunk j of a payload of csize bytes whose first byte lands at an address that is `a` modulo 16:
// [*b0, *b1).  Chunk 0 is `a` bytes short, so that every later chunk starts 16-byte aligned in the
// destination; the chunks tile [0, csize).  false: the chunk starts at or beyond csize and owns
// nothing.
DMX_HD inline bool zipw_chunk(uint64_t csize, uint32_t a, uint64_t chunk, uint64_t j, uint64_t* b0, uint64_t* b1) {
    const uint64_t s = j ? j * chunk - a : 0, e = (j + 1) * chunk - a;
    if (s >= csize) return false;
    *b0 = s;
    *b1 = e < csize ? e : csize;
    return true;
}

// ---- 4. the records -------------------------------------------------------------------------------
// The local header at dst; returns its bytes (zipw_local_bytes).
DMX_HD inline uint32_t zipw_write_local(uint8_t* dst, const ZipwEntry& e, bool force64) {
    const bool big = zipw_big(e.usize, e.csize, force64);
    zipw_le32(dst, kZipSigLocal);
    zipw_le16(dst + 4, big ? 45 : 20);  // version needed
    zipw_le16(dst + 6, e.gpflags);
    zipw_le16(dst + 8, e.method);
    zipw_le32(dst + 10, e.dostime);
    zipw_le32(dst + 14, e.crc);
    zipw_le32(dst + 18, big ? 0xFFFFFFFFu : (uint32_t)e.csize);
    zipw_le32(dst + 22, big ? 0xFFFFFFFFu : (uint32_t)e.usize);
    zipw_le16(dst + 26, e.name_len);
    zipw_le16(dst + 28, big ? 20 : 0);
    uint8_t* p = dst + 30;
    for (uint32_t i = 0; i < e.name_len; i++) p[i] = e.name[i];
    p += e.name_len;
    if (big) {
        zipw_le16(p, 1);
        zipw_le16(p + 2, 16);
        zipw_le64(p + 4, e.usize);
        zipw_le64(p + 12, e.csize);
        p += 20;
    }
    return (uint32_t)(p - dst);
}

// The central record at dst; returns its bytes (zipw_central_bytes).  The extra holds usize and
// csize, then the local header's offset: the order zip_entry reads.
DMX_HD inline uint32_t zipw_write_central(uint8_t* dst, const ZipwEntry& e, uint64_t local_off, bool force64) {
    const bool big = zipw_big(e.usize, e.csize, force64), off64 = zipw_off64(local_off, force64);
    const uint32_t fields = (big ? 2u : 0u) + (off64 ? 1u : 0u);
    const uint32_t ver = fields ? 45 : 20;
    zipw_le32(dst, kZipSigCentral);
    zipw_le16(dst + 4, ver);  // made by: the specification's version, host system 0
    zipw_le16(dst + 6, ver);  // version needed
    zipw_le16(dst + 8, e.gpflags);
    zipw_le16(dst + 10, e.method);
    zipw_le32(dst + 12, e.dostime);
    zipw_le32(dst + 16, e.crc);
    zipw_le32(dst + 20, big ? 0xFFFFFFFFu : (uint32_t)e.csize);
    zipw_le32(dst + 24, big ? 0xFFFFFFFFu : (uint32_t)e.usize);
    zipw_le16(dst + 28, e.name_len);
    zipw_le16(dst + 30, fields ? 4 + 8 * fields : 0);
    zipw_le16(dst + 32, 0);  // no entry comment
    zipw_le16(dst + 34, 0);  // disk
    zipw_le16(dst + 36, 0);  // internal attributes
    zipw_le32(dst + 38, zipw_attr(e.name, e.name_len));
    zipw_le32(dst + 42, off64 ? 0xFFFFFFFFu : (uint32_t)local_off);
    uint8_t* p = dst + 46;
    for (uint32_t i = 0; i < e.name_len; i++) p[i] = e.name[i];
    p += e.name_len;
    if (fields) {
        zipw_le16(p, 1);
        zipw_le16(p + 2, 8 * fields);
        p += 4;
        if (big) {
            zipw_le64(p, e.usize);
            zipw_le64(p + 8, e.csize);
            p += 16;
        }
        if (off64) {
            zipw_le64(p, local_off);
            p += 8;
        }
    }
    return (uint32_t)(p - dst);
}

// The end records at dst = the archive's byte cd_off + cd_size: the ZIP64 end record and its
// locator where zipw_end64 holds -- the classic record then reads 0xFFFF, 0xFFFF, 0xFFFFFFFF and
// 0xFFFFFFFF -- and the 22-byte end record.  comment: its comment_len bytes follow (null: the
// caller writes them at the returned offset).  Returns the records' bytes without the comment.
DMX_HD inline uint32_t zipw_write_end(uint8_t* dst, uint64_t count, uint64_t cd_size, uint64_t cd_off,
                                      const uint8_t* comment, uint32_t comment_len, bool force64) {
    const bool z64 = zipw_end64(count, cd_size, cd_off, force64);
    uint8_t* p = dst;
    if (z64) {
        zipw_le32(p, kZipSigEnd64);
        zipw_le64(p + 4, 44);  // the record's bytes behind this field
        zipw_le16(p + 12, 45);
        zipw_le16(p + 14, 45);
        zipw_le32(p + 16, 0);  // this disk
        zipw_le32(p + 20, 0);  // the directory's disk
        zipw_le64(p + 24, count);
        zipw_le64(p + 32, count);
        zipw_le64(p + 40, cd_size);
        zipw_le64(p + 48, cd_off);
        p += 56;
        zipw_le32(p, kZipSigLoc64);
        zipw_le32(p + 4, 0);  // the ZIP64 end record's disk
        zipw_le64(p + 8, cd_off + cd_size);
        zipw_le32(p + 16, 1);  // disks
        p += 20;
    }
    zipw_le32(p, kZipSigEnd);
    zipw_le16(p + 4, 0);
    zipw_le16(p + 6, 0);
    zipw_le16(p + 8, z64 ? 0xFFFFu : (uint32_t)count);
    zipw_le16(p + 10, z64 ? 0xFFFFu : (uint32_t)count);
    zipw_le32(p + 12, z64 ? 0xFFFFFFFFu : (uint32_t)cd_size);
    zipw_le32(p + 16, z64 ? 0xFFFFFFFFu : (uint32_t)cd_off);
    zipw_le16(p + 20, comment_len);
    p += 22;
    if (comment)
        for (uint32_t i = 0; i < comment_len; i++) p[i] = comment[i];
    return (uint32_t)(p - dst);
}

// The written table's row: what zip_entry reads back from the archive.  central_off: the entry's
// central record in the archive.
DMX_HD inline void zipw_row(const ZipwEntry& e, uint64_t local_off, uint64_t central_off, uint64_t uoffset,
                            bool force64, ::dmx_zip_entry* r) {
    r->name_off = central_off + 46;
    r->data_off = local_off + zipw_local_bytes(e.name_len, e.usize, e.csize, force64);
    r->csize = e.csize;
    r->usize = e.usize;
    r->uoffset = uoffset;
    r->crc = e.crc;
    r->dostime = e.dostime;
    r->name_len = (uint16_t)e.name_len;
    r->method = (uint16_t)e.method;
    r->gpflags = (uint16_t)e.gpflags;
    r->reserved = 0;
    r->status = DMX_OK;
    r->path = 0;
}

}  // namespace dmx
