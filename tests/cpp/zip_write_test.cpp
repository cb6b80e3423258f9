// zip_write_test.cpp -- CPU test of deflate.hpp_amd/csrc/zip_write.h: the records and the steps
// that the kernels of zip_write.hip run when they write a ZIP archive.
//
// Stand-alone (no HIP, no GPU); tests/test_zip_write.py builds it plain and with AddressSanitizer +
// UBSan and runs both binaries directly:
//     zip_write_test <case> <archive> [<case> <archive> ...]   assemble each case file into an archive
//     zip_write_test --arith                                   threshold and chunk arithmetic alone
// <case>, little endian, written by the Python test:
//     "ZWC1", u32 flags (DMX_ZIP_FORCE64), u32 count, u32 comment_len, the comment, then per entry
//     u32 name_len, u16 method, u16 0, u32 dostime, u32 crc, u64 usize, u64 csize, the name, the
//     payload of csize bytes (method 8: a raw deflate stream made with zlib).
// Every step is run "for all threads" serially -- sizes, the two-halves scans, the central sizes,
// the layout, the pack's workgroups with a plain byte loop standing in for the shifted loads, the
// records -- into a heap buffer of exactly the archive's size at two alignments, so a write outside
// the archive is a sanitizer report.  The archive is then walked with zip_dir.h's own steps (end
// record, candidates, links, doubling, chain, zip_entry) and must give back the table the writer
// states, field for field.  Python's zipfile judges the file this program writes out.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../deflate.hpp_amd/csrc/zip_write.h"

using namespace dmx;
typedef std::vector<uint8_t> Bytes;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        g_checks++;                                        \
        if (!(cond)) {                                     \
            g_failed++;                                    \
            if (g_failed < 50) {                           \
                std::fprintf(stderr, "[FAIL] %s:%d %s -- ", __FILE__, __LINE__, #cond); \
                std::fprintf(stderr, __VA_ARGS__);         \
                std::fprintf(stderr, "\n");                \
            }                                              \
        }                                                  \
    } while (0)

typedef unsigned long long ull;

struct Case {
    bool force64 = false;
    Bytes comment, names;
    std::vector<ZipwSrc> src;
    std::vector<uint64_t> usize;
    std::vector<uint32_t> crc;
    std::vector<Bytes> payload;
    std::vector<dmx_batch_result> res;  // the batch deflate's results: the method 8 entries
};

static bool read_file(const char* path, Bytes* b) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) b->insert(b->end(), buf, buf + got);
    std::fclose(f);
    return true;
}

static bool parse_case(const Bytes& b, Case* c) {
    size_t p = 0;
    auto need = [&](size_t k) { return b.size() - p >= k; };
    if (!need(16) || std::memcmp(b.data(), "ZWC1", 4) != 0) return false;
    c->force64 = (frame_le32(b.data() + 4) & 1u) != 0;
    const uint32_t count = frame_le32(b.data() + 8), cl = frame_le32(b.data() + 12);
    p = 16;
    if (!need(cl)) return false;
    c->comment.assign(b.begin() + p, b.begin() + p + cl);
    p += cl;
    uint64_t uoff = 0;
    for (uint32_t k = 0; k < count; k++) {
        if (!need(32)) return false;
        const uint8_t* h = b.data() + p;
        const uint32_t nl = frame_le32(h), method = zip_le16(h + 4), dostime = frame_le32(h + 8);
        const uint64_t us = zip_le64(h + 16), cs = zip_le64(h + 24);
        p += 32;
        if (zipw_check_source(nl, method) != DMX_OK || !need(nl) || b.size() - p - nl < cs) return false;
        ZipwSrc s{};
        s.name_off = c->names.size();
        s.uoffset = uoff;
        s.dostime = dostime ? dostime : kZipwDosTime;
        s.dres = (uint32_t)c->res.size();
        s.name_len = (uint16_t)nl;
        s.method = (uint16_t)method;
        s.gpflags = (uint16_t)zipw_flags(b.data() + p, nl);
        c->names.insert(c->names.end(), b.begin() + p, b.begin() + p + nl);
        p += nl;
        c->payload.emplace_back(b.begin() + p, b.begin() + p + cs);
        p += cs;
        if (method == 8) c->res.push_back(dmx_batch_result{cs, DMX_OK, 0});
        c->src.push_back(s);
        c->usize.push_back(us);
        c->crc.push_back(frame_le32(h + 12));
        uoff += us;
    }
    return p == b.size();
}

// What the writer states
struct Written {
    ZipwHead h{};
    Bytes archive;
    std::vector<dmx_zip_entry> rows;
};

// the kernels' steps, every "thread" in turn; out sits `shift` bytes into its allocation
static Written assemble(const Case& c, size_t shift, uint64_t chunk, const char* what) {
    Written W;
    const uint64_t count = c.src.size();
    const bool f64 = c.force64;
    unsigned long long key = ~0ull;
    // k_zipw_sizes
    std::vector<uint64_t> csize(count), loff(count), coff(count);
    std::vector<uint32_t> lo(count), hi(count), cbytes(count);
    for (uint64_t k = 0; k < count; k++) {
        uint64_t cs;
        const int st = zipw_csize(c.src[k], c.usize[k], c.res.data(), &cs);
        if (st != DMX_OK) key = std::min<unsigned long long>(key, (k << 32) | (uint32_t)st);
        CHECK(cs == c.payload[k].size(), "%s: entry %llu csize", what, (ull)k);
        const uint64_t rec = zipw_local_bytes(c.src[k].name_len, c.usize[k], cs, f64) + cs;
        csize[k] = cs;
        lo[k] = (uint32_t)rec;
        hi[k] = (uint32_t)(rec >> 32);
    }
    // the two scans and k_zipw_central
    uint64_t slo = 0, shi = 0, scd = 0;
    for (uint64_t k = 0; k < count; k++) {
        loff[k] = slo + (shi << 32);
        slo += lo[k];
        shi += hi[k];
    }
    for (uint64_t k = 0; k < count; k++) cbytes[k] = zipw_central_bytes(c.src[k].name_len, c.usize[k], csize[k], loff[k], f64);
    for (uint64_t k = 0; k < count; k++) {
        coff[k] = scd;
        scd += cbytes[k];
    }
    const uint64_t local_total = slo + (shi << 32);
    const uint32_t cl = (uint32_t)c.comment.size();
    const ZipwHead need = zipw_layout(count, local_total, scd, cl, f64, key, ~0ull);
    CHECK(need.status == DMX_OK, "%s: status %d", what, need.status);
    if (need.bytes) {
        const ZipwHead shortcap = zipw_layout(count, local_total, scd, cl, f64, key, need.bytes - 1);
        CHECK(shortcap.status == DMX_ERR_CAPACITY && shortcap.bytes == need.bytes, "%s: one byte short", what);
    }
    const ZipwHead h = zipw_layout(count, local_total, scd, cl, f64, key, need.bytes);
    CHECK(h.status == DMX_OK && h.bytes == need.bytes, "%s: exact capacity", what);
    W.h = h;
    // the host's chunk bounds: a deflated entry's slot is larger than its stream
    std::vector<uint64_t> first(count + 1);
    uint64_t nchunks = 0;
    for (uint64_t k = 0; k < count; k++) {
        first[k] = nchunks;
        nchunks += zipw_chunk_bound(c.src[k].method == 8 ? csize[k] + 10 * ((c.usize[k] + 16383) / 16384) + 16 : csize[k], chunk);
    }
    first[count] = nchunks;
    std::unique_ptr<uint8_t[]> mem(new uint8_t[h.bytes + shift]);  // the archive ends where the allocation ends
    uint8_t* const out = mem.get() + shift;
    std::memset(mem.get(), 0xA5, h.bytes + shift);
    W.rows.resize(count);
    uint64_t written = 0;
    std::vector<uint64_t> next(count, 0);  // per entry: where its next chunk must start
    // k_zipw_pack, workgroups 0 .. nchunks
    for (uint64_t w = 0; w < nchunks; w++) {
        const uint64_t k = zipw_find(first.data(), count, w), j = w - first[k];
        CHECK(k < count && first[k] <= w && w < first[k + 1], "%s: workgroup %llu -> entry %llu", what, (ull)w, (ull)k);
        const ZipwSrc& s = c.src[k];
        uint8_t* const dst = out + loff[k] + zipw_local_bytes(s.name_len, c.usize[k], csize[k], f64);
        if (j == 0) {
            ZipwEntry e{c.names.data() + s.name_off, s.name_len, s.method, s.gpflags, s.dostime, c.crc[k], c.usize[k], csize[k]};
            const uint32_t lb = zipw_write_local(out + loff[k], e, f64);
            CHECK(lb == zipw_local_bytes(s.name_len, c.usize[k], csize[k], f64), "%s: local header %llu", what, (ull)k);
            const uint32_t cb = zipw_write_central(out + h.cd_off + coff[k], e, loff[k], f64);
            CHECK(cb == cbytes[k], "%s: central record %llu", what, (ull)k);
            zipw_row(e, loff[k], h.cd_off + coff[k], s.uoffset, f64, &W.rows[k]);
            written += lb + cb;
        }
        uint64_t b0 = 0, b1 = 0;
        if (!zipw_chunk(csize[k], (uint32_t)((uintptr_t)dst & 15), chunk, j, &b0, &b1)) {
            CHECK(next[k] == csize[k], "%s: entry %llu chunk %llu owns nothing before the payload is done", what, (ull)k, (ull)j);
            continue;
        }
        CHECK(b0 == next[k] && b1 > b0 && b1 <= csize[k], "%s: entry %llu chunk %llu [%llu, %llu)", what, (ull)k, (ull)j,
              (ull)b0, (ull)b1);
        CHECK(j == 0 || ((uintptr_t)(dst + b0) & 15) == 0, "%s: entry %llu chunk %llu starts unaligned", what, (ull)k, (ull)j);
        CHECK(b1 - b0 <= chunk, "%s: a chunk above the chunk size", what);
        for (uint64_t p = b0; p < b1; p++) dst[p] = c.payload[k][p];
        next[k] = b1;
        written += b1 - b0;
    }
    for (uint64_t k = 0; k < count; k++) CHECK(next[k] == csize[k], "%s: entry %llu payload not tiled", what, (ull)k);
    // the last workgroup
    uint8_t* const end = out + h.cd_off + h.cd_size;
    const uint32_t at = (uint32_t)zipw_end_bytes(count, h.cd_size, h.cd_off, 0, f64);
    const uint32_t eb = zipw_write_end(end, count, h.cd_size, h.cd_off, nullptr, cl, f64);
    CHECK(eb == at, "%s: end records", what);
    for (uint32_t i = 0; i < cl; i++) end[at + i] = c.comment[i];
    written += eb + cl;
    CHECK(written == h.bytes, "%s: %llu bytes written, the archive has %llu", what, (ull)written, (ull)h.bytes);
    W.archive.assign(out, out + h.bytes);
    return W;
}

// zip_dir.h's own steps over the written archive: the table they give back
static bool read_back(const Bytes& b, std::vector<dmx_zip_entry>* rows, const char* what) {
    const uint64_t n = b.size();
    std::unique_ptr<uint8_t[]> mem(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(mem.get(), b.data(), n);
    const uint8_t* in = mem.get();
    uint64_t best = 0;
    for (uint64_t p = zip_tail_start(n); p + 22 <= n; p++)
        if (in[p] == 0x50 && zip_eocd_at(in, n, p)) best = std::max(best, p + 1);
    CHECK(best != 0, "%s: no end record", what);
    if (!best) return false;
    ZipHead h{};
    const int st = zip_read_end(in, n, best - 1, &h);
    CHECK(st == DMX_OK && h.base == 0, "%s: end record status %d base %llu", what, st, (ull)h.base);
    if (st != DMX_OK) return false;
    rows->clear();
    if (!h.dir_size) return h.count == 0;
    const uint64_t d0 = h.dir_off, d1 = h.dir_off + h.dir_size;
    std::vector<BgzfCand> cands;
    for (uint64_t off = d0; off < d1; off++) {
        BgzfCand c;
        if (d1 - off >= 46 && frame_le32(in + off) == kZipSigCentral && zip_cd_candidate(in, d0, d1, off, &c)) cands.push_back(c);
    }
    const uint64_t nc = cands.size();
    CHECK(nc && h.count <= nc, "%s: %llu candidates for %llu entries", what, (ull)nc, (ull)h.count);
    if (!nc || h.count > nc) return false;
    const uint32_t levels = bgzf_levels(nc);
    std::vector<uint32_t> J((size_t)levels * nc, kBgzfNone);
    for (uint64_t i = 0; i < nc; i++) J[i] = bgzf_link(cands.data(), nc, i, d1);
    for (uint32_t k = 0; k + 1 < levels; k++)
        for (uint64_t i = 0; i < nc; i++) J[(size_t)(k + 1) * nc + i] = bgzf_double(J.data() + (size_t)k * nc, i);
    uint64_t entries = 0;
    const int cs = zip_chain_status(cands.data(), nc, J.data(), levels, h, &entries);
    CHECK(cs == DMX_OK, "%s: chain status %d", what, cs);
    if (cs != DMX_OK) return false;
    rows->resize(entries);
    uint64_t uoff = 0;
    for (uint64_t r = 0; r < entries; r++) {
        zip_entry(in, n, h.base, cands[bgzf_rank_lookup(J.data(), nc, levels, r)], &(*rows)[r]);
        (*rows)[r].uoffset = uoff;
        uoff += (*rows)[r].usize;
    }
    return true;
}

static bool same_entry(const dmx_zip_entry& a, const dmx_zip_entry& b) {
    return a.name_off == b.name_off && a.data_off == b.data_off && a.csize == b.csize && a.usize == b.usize &&
           a.uoffset == b.uoffset && a.crc == b.crc && a.dostime == b.dostime && a.name_len == b.name_len &&
           a.method == b.method && a.gpflags == b.gpflags && a.reserved == b.reserved && a.status == b.status &&
           a.path == b.path;
}

static void run_case(const char* case_path, const char* out_path) {
    Bytes raw;
    Case c;
    if (!read_file(case_path, &raw) || !parse_case(raw, &c)) {
        CHECK(false, "%s: not a case file", case_path);
        return;
    }
    const Written W = assemble(c, 0, kZipwChunk, case_path);
    // another alignment of the output and a small chunk size: the same archive
    for (const uint64_t chunk : {(uint64_t)kZipwChunk, (uint64_t)4096, (uint64_t)16})
        for (const size_t shift : {(size_t)9, (size_t)15}) {
            if (chunk == 16 && c.src.size() > 1000) continue;  // (the chunk grid has cases of its own)
            const Written V = assemble(c, shift, chunk, case_path);
            CHECK(V.archive == W.archive, "%s: shift %zu chunk %llu gives another archive", case_path, shift, (ull)chunk);
        }
    std::vector<dmx_zip_entry> rows;
    if (read_back(W.archive, &rows, case_path)) {
        CHECK(rows.size() == W.rows.size(), "%s: %zu entries read back, %zu written", case_path, rows.size(), W.rows.size());
        for (size_t r = 0; r < rows.size() && r < W.rows.size(); r++)
            CHECK(same_entry(rows[r], W.rows[r]), "%s: entry %zu reads back differently", case_path, r);
    }
    FILE* f = std::fopen(out_path, "wb");
    CHECK(f != nullptr, "%s: cannot write", out_path);
    if (f) {
        if (!W.archive.empty()) CHECK(std::fwrite(W.archive.data(), 1, W.archive.size(), f) == W.archive.size(), "short write");
        std::fclose(f);
    }
}

// ---- threshold arithmetic without big buffers ---------------------------------------------------
static void arith_records() {
    const uint64_t vals[] = {0xFFFFFFFEull, 0xFFFFFFFFull, 1ull << 32, 1ull << 40};
    const uint8_t name[] = {'b', 'i', 'g', '/', 'x'};
    for (const bool f64 : {false, true})
        for (const uint64_t us : vals)
            for (const uint64_t cs : vals)
                for (const uint64_t lo : vals) {
                    const bool big = f64 || us >= kZipw32 || cs >= kZipw32, off64 = f64 || lo >= kZipw32;
                    ZipwEntry e{name, 5, 8, 0, 0x5841u, 0x12345678u, us, cs};
                    uint8_t l[64];
                    std::memset(l, 0xA5, sizeof l);
                    const uint32_t lb = zipw_write_local(l, e, f64);
                    CHECK(lb == 30 + 5 + (big ? 20u : 0u) && lb == zipw_local_bytes(5, us, cs, f64), "local bytes");
                    CHECK(l[lb] == 0xA5, "local header overrun");
                    CHECK(frame_le32(l) == kZipSigLocal && zip_le16(l + 4) == (big ? 45u : 20u), "version needed");
                    CHECK(frame_le32(l + 18) == (big ? 0xFFFFFFFFu : (uint32_t)cs) &&
                              frame_le32(l + 22) == (big ? 0xFFFFFFFFu : (uint32_t)us), "local 32-bit sizes");
                    CHECK(zip_le16(l + 28) == (big ? 20u : 0u), "local extra length");
                    if (big)
                        CHECK(zip_le16(l + 35) == 1 && zip_le16(l + 37) == 16 && zip_le64(l + 39) == us &&
                                  zip_le64(l + 47) == cs, "local extra: usize, csize");
                    // the central record alone in an exact-size buffer that holds only the directory
                    const uint32_t want = 46 + 5 + ((big || off64) ? 4 + 8 * ((big ? 2u : 0u) + (off64 ? 1u : 0u)) : 0u);
                    CHECK(zipw_central_bytes(5, us, cs, lo, f64) == want, "central bytes");
                    std::unique_ptr<uint8_t[]> dir(new uint8_t[want]);
                    const uint32_t cb = zipw_write_central(dir.get(), e, lo, f64);
                    CHECK(cb == want, "central record length");
                    const uint8_t* r = dir.get();
                    CHECK(zip_le16(r + 6) == ((big || off64) ? 45u : 20u), "central version needed");
                    CHECK(frame_le32(r + 20) == (big ? 0xFFFFFFFFu : (uint32_t)cs) &&
                              frame_le32(r + 24) == (big ? 0xFFFFFFFFu : (uint32_t)us) &&
                              frame_le32(r + 42) == (off64 ? 0xFFFFFFFFu : (uint32_t)lo), "central 32-bit fields");
                    CHECK(frame_le32(r + 38) == 0u, "attributes of a file");
                    // decoded again with the reader's own step: a directory at offset 0 of a buffer of `want` bytes;
                    // the local header lies outside it, which is the entry's DMX_ERR_OVERREAD and nothing else
                    BgzfCand c;
                    CHECK(zip_cd_candidate(r, 0, want, 0, &c) && c.size == want, "the reader's candidate");
                    dmx_zip_entry d;
                    zip_entry(r, want, 0, c, &d);
                    CHECK(d.usize == us && d.csize == cs && d.crc == 0x12345678u && d.dostime == 0x5841u && d.method == 8 &&
                              d.gpflags == 0 && d.name_len == 5 && d.name_off == 46, "the reader's fields");
                    CHECK(d.status == DMX_ERR_OVERREAD, "status %d", d.status);
                    if (big || off64) {
                        const uint8_t* x = r + 51;
                        CHECK(zip_le16(x) == 1 && zip_le16(x + 2) == want - 55, "central extra header");
                        if (big) CHECK(zip_le64(x + 4) == us && zip_le64(x + 12) == cs, "extra order: usize, csize");
                        if (off64) CHECK(zip_le64(x + (big ? 20 : 4)) == lo, "extra order: the offset last");
                    }
                }
    // a directory entry's attributes, the UTF-8 flag
    const uint8_t dir[] = {'d', '/'}, utf[] = {'n', 0xC3, 0xA9};
    CHECK(zipw_attr(dir, 2) == 0x10 && zipw_attr(utf, 3) == 0, "attributes");
    CHECK(zipw_flags(dir, 2) == 0 && zipw_flags(utf, 3) == 0x800, "flags");
    CHECK(zipw_check_source(0, 8) == DMX_ERR_ARG && zipw_check_source(65536, 8) == DMX_ERR_ARG &&
              zipw_check_source(65535, 0) == DMX_OK && zipw_check_source(1, 8) == DMX_OK &&
              zipw_check_source(1, 12) == DMX_ERR_ARG && zipw_check_source(1, 1) == DMX_ERR_ARG, "source checks");
}

static void arith_end() {
    const uint64_t sizes[] = {0, 0xFFFFFFFEull, 0xFFFFFFFFull, 1ull << 32}, counts[] = {0, 0xFFFEull, 0xFFFFull, 0x10000ull, 1ull << 33};
    const uint8_t comment[] = {'h', 'i'};
    for (const bool f64 : {false, true})
        for (const uint64_t cnt : counts)
            for (const uint64_t sz : sizes)
                for (const uint64_t off : sizes)
                    for (const uint32_t cl : {0u, 2u}) {
                        const bool z64 = f64 || cnt >= 0xFFFF || sz >= kZipw32 || off >= kZipw32;
                        const uint64_t want = (z64 ? 76u : 0u) + 22 + cl;
                        CHECK(zipw_end_bytes(cnt, sz, off, cl, f64) == want, "end bytes");
                        std::unique_ptr<uint8_t[]> buf(new uint8_t[want]);
                        const uint32_t eb = zipw_write_end(buf.get(), cnt, sz, off, comment, cl, f64);
                        CHECK(eb + cl == want, "end records length");
                        const uint8_t* e = buf.get() + (z64 ? 76 : 0);
                        CHECK(frame_le32(e) == kZipSigEnd && zip_le16(e + 20) == cl, "end record");
                        CHECK(cl == 0 || (e[22] == 'h' && e[23] == 'i'), "comment");
                        if (z64) {
                            CHECK(zip_le16(e + 8) == 0xFFFF && zip_le16(e + 10) == 0xFFFF && frame_le32(e + 12) == 0xFFFFFFFFu &&
                                      frame_le32(e + 16) == 0xFFFFFFFFu, "classic record beside ZIP64");
                            const uint8_t* r = buf.get();
                            CHECK(frame_le32(r) == kZipSigEnd64 && zip_le64(r + 4) == 44 && zip_le64(r + 24) == cnt &&
                                      zip_le64(r + 32) == cnt && zip_le64(r + 40) == sz && zip_le64(r + 48) == off, "ZIP64 end record");
                            CHECK(frame_le32(r + 56) == kZipSigLoc64 && zip_le64(r + 64) == off + sz && frame_le32(r + 72) == 1, "locator");
                        } else {
                            CHECK(zip_le16(e + 8) == cnt && zip_le16(e + 10) == cnt && frame_le32(e + 12) == sz && frame_le32(e + 16) == off,
                                  "classic record");
                        }
                    }
    // the reader on end records that stand where they say (a directory of zero entries)
    for (const bool f64 : {false, true}) {
        uint8_t buf[kZip64Bytes + 22];
        const uint32_t eb = zipw_write_end(buf, 0, 0, 0, nullptr, 0, f64);
        ZipHead h{};
        CHECK(zip_eocd_at(buf, eb, eb - 22) && zip_read_end(buf, eb, eb - 22, &h) == DMX_OK && h.count == 0 && h.dir_size == 0 &&
                  h.base == 0 && h.zip64 == (f64 ? 1u : 0u), "empty archive read back");
    }
}

// For every (payload length, destination offset mod 16, chunk size): the chunks tile [0, csize)
// exactly once, interior starts are 16-byte aligned in the destination, workgroups past csize own
// nothing, and the host's bound covers them all.
static void arith_chunks() {
    for (const uint64_t chunk : {(uint64_t)16, (uint64_t)32, (uint64_t)64, (uint64_t)256}) {
        std::vector<uint64_t> lens;
        for (uint64_t len = 0; len <= 3 * chunk + 17; len++) lens.push_back(len);
        for (const uint64_t len : lens)
            for (uint32_t a = 0; a < 16; a++) {
                const uint64_t bound = zipw_chunk_bound(len, chunk);
                uint64_t next = 0, owned = 0;
                for (uint64_t j = 0; j < bound + 3; j++) {
                    uint64_t b0 = 0, b1 = 0;
                    if (!zipw_chunk(len, a, chunk, j, &b0, &b1)) {
                        CHECK(next == len, "len %llu a %u chunk %llu: workgroup %llu owns nothing too early", (ull)len, a, (ull)chunk, (ull)j);
                        continue;
                    }
                    CHECK(j < bound, "len %llu a %u chunk %llu: workgroup %llu beyond the bound %llu", (ull)len, a, (ull)chunk, (ull)j, (ull)bound);
                    CHECK(b0 == next && b1 > b0 && b1 <= len && b1 - b0 <= chunk, "len %llu a %u chunk %llu: [%llu, %llu)", (ull)len, a,
                          (ull)chunk, (ull)b0, (ull)b1);
                    CHECK(j == 0 || (a + b0) % 16 == 0, "len %llu a %u chunk %llu: chunk %llu starts at %llu", (ull)len, a, (ull)chunk, (ull)j, (ull)b0);
                    next = b1;
                    owned++;
                }
                CHECK(next == len && owned <= bound, "len %llu a %u chunk %llu: tiled to %llu", (ull)len, a, (ull)chunk, (ull)next);
            }
    }
    // the binary search over the prefix sums
    const uint64_t first[] = {0, 1, 2, 7, 8, 20};
    for (uint64_t w = 0; w < 20; w++) {
        const uint64_t k = zipw_find(first, 5, w);
        CHECK(k < 5 && first[k] <= w && w < first[k + 1], "workgroup %llu -> %llu", (ull)w, (ull)k);
    }
    const uint64_t one[] = {0, 3};
    CHECK(zipw_find(one, 1, 0) == 0 && zipw_find(one, 1, 2) == 0, "one entry");
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "--arith") {
        arith_records();
        arith_end();
        arith_chunks();
    } else if (argc >= 3 && argc % 2 == 1) {
        for (int i = 1; i + 1 < argc; i += 2) run_case(argv[i], argv[i + 1]);
    } else {
        std::fprintf(stderr, "usage: %s <case> <archive> [...] | --arith\n", argv[0]);
        return 2;
    }
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
