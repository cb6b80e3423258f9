// zip_dir_test.cpp -- CPU test of deflate.hpp_amd/csrc/zip_dir.h: the parallel form of the ZIP
// directory walk that the kernels of zip_dir.hip run.
//
// Stand-alone (no HIP, no GPU); tests/test_zip_dir.py builds it plain and with AddressSanitizer +
// UBSan, writes archives with Python's zipfile and runs both binaries directly:
//     zip_dir_test <archive> <table> [<archive> <table> ...]
//     zip_dir_test --walk <archive>     (the serial walk's time alone: the host alternative to the kernels)
// <table>: the entry count, then per entry "header_offset compress_size file_size CRC method
// data_offset flags" as zipfile's ZipInfo states them.  The steps (end record, candidates, links,
// doubling, chain, entries, layout) are run serially over all "threads" on a heap copy of exactly
// n bytes, so a read outside the archive is a sanitizer report; the result is compared with the
// table and with a serial walk of the directory.  Then the archives are damaged (truncations, a
// directory one byte short, a count off by one, records that overrun the directory, ZIP64 values
// near 2^64): every mutant must end in a status, and both walks must agree on it.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../deflate.hpp_amd/csrc/zip_dir.h"

using namespace dmx;
typedef std::vector<uint8_t> Bytes;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        g_checks++;                                        \
        if (!(cond)) {                                     \
            g_failed++;                                    \
            std::fprintf(stderr, "[FAIL] %s:%d %s -- ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);             \
            std::fprintf(stderr, "\n");                    \
        }                                                  \
    } while (0)

struct Table {
    int status = DMX_OK;
    ZipHead h{};
    uint64_t eocd = 0;
    std::vector<dmx_zip_entry> e;
    std::vector<uint64_t> rec;  // each entry's central record
    uint64_t total = 0;
};

// one record after another from the directory's first byte
static Table serial_walk(const uint8_t* in, uint64_t n) {
    Table t;
    t.status = DMX_ERR_DATA;
    if (n < 22) return t;
    uint64_t p = n - 22;
    for (;; p--) {  // from the end: the first hit is the highest
        if (zip_eocd_at(in, n, p)) break;
        if (p == zip_tail_start(n)) return t;
    }
    t.eocd = p;
    t.status = zip_read_end(in, n, p, &t.h);
    if (t.status != DMX_OK) return t;
    const uint64_t d1 = t.h.dir_off + t.h.dir_size;
    for (uint64_t off = t.h.dir_off; off < d1;) {
        BgzfCand c;
        if (!zip_cd_candidate(in, t.h.dir_off, d1, off, &c)) {
            t.status = DMX_ERR_DATA;
            return t;
        }
        dmx_zip_entry e;
        zip_entry(in, n, t.h.base, c, &e);
        e.uoffset = t.total;
        if (e.usize > (1ull << 63) - t.total) t.status = DMX_ERR_DATA;  // (the walk goes on: the count decides too)
        else t.total += e.usize;
        t.e.push_back(e);
        t.rec.push_back(off);
        off += c.size;
    }
    if (t.e.size() != t.h.count) t.status = DMX_ERR_DATA;
    return t;
}

// the kernels' steps, every "thread" in turn
static Table parallel_walk(const uint8_t* in, uint64_t n) {
    Table t;
    t.status = DMX_ERR_DATA;
    if (n < 22) return t;
    uint64_t best = 0;  // k_zip_tail: the highest valid position + 1
    for (uint64_t p = zip_tail_start(n); p + 22 <= n; p++)
        if (in[p] == 0x50 && zip_eocd_at(in, n, p)) best = std::max(best, p + 1);
    if (!best) return t;
    t.eocd = best - 1;
    t.status = zip_read_end(in, n, best - 1, &t.h);
    if (t.status != DMX_OK) return t;
    const ZipHead& h = t.h;
    if (!h.dir_size) {
        if (h.count) t.status = DMX_ERR_DATA;
        return t;
    }
    const uint64_t d0 = h.dir_off, d1 = h.dir_off + h.dir_size;
    std::vector<BgzfCand> cands;
    for (uint64_t off = d0; off < d1; off++) {  // (the kernels test the signature on staged bytes first)
        BgzfCand c;
        const bool magic = d1 - off >= 46 && frame_le32(in + off) == kZipSigCentral;
        const bool ok = zip_cd_candidate(in, d0, d1, off, &c);
        CHECK(!ok || magic, "offset %llu: a record the signature filter drops", (unsigned long long)off);
        if (magic && ok) cands.push_back(c);
    }
    const uint64_t nc = cands.size();
    if (!nc || h.count > nc) {  // (the host's check between the count and the chain)
        t.status = DMX_ERR_DATA;
        return t;
    }
    const uint32_t levels = bgzf_levels(nc);
    std::vector<uint32_t> J((size_t)levels * nc, kBgzfNone);
    for (uint64_t i = 0; i < nc; i++) J[i] = bgzf_link(cands.data(), nc, i, d1);
    for (uint32_t k = 0; k + 1 < levels; k++)
        for (uint64_t i = 0; i < nc; i++) J[(size_t)(k + 1) * nc + i] = bgzf_double(J.data() + (size_t)k * nc, i);
    uint64_t entries = 0;
    t.status = zip_chain_status(cands.data(), nc, J.data(), levels, h, &entries);
    if (t.status != DMX_OK) return t;
    t.e.resize(entries);
    std::vector<uint32_t> lo(entries), hi(entries);
    for (uint64_t r = 0; r < entries; r++) {
        const BgzfCand& c = cands[bgzf_rank_lookup(J.data(), nc, levels, r)];
        zip_entry(in, n, h.base, c, &t.e[r]);
        t.rec.push_back(c.off);
        lo[r] = (uint32_t)t.e[r].usize;
        hi[r] = (uint32_t)(t.e[r].usize >> 32);
    }
    uint64_t slo = 0, shi = 0;  // the two exclusive scans
    for (uint64_t r = 0; r < entries; r++) {
        t.e[r].uoffset = slo + (shi << 32);
        slo += lo[r];
        shi += hi[r];
    }
    if (!zip_total(slo, shi, &t.total)) t.status = DMX_ERR_DATA;
    return t;
}

static bool same_entry(const dmx_zip_entry& a, const dmx_zip_entry& b) {
    return a.name_off == b.name_off && a.data_off == b.data_off && a.csize == b.csize && a.usize == b.usize &&
           a.uoffset == b.uoffset && a.crc == b.crc && a.dostime == b.dostime && a.name_len == b.name_len &&
           a.method == b.method && a.gpflags == b.gpflags && a.status == b.status;
}

// both walks on an exact-size copy of b[0, n); they must agree
static Table compare(const Bytes& b, size_t n, const char* what, long tag = -1) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);  // exact size
    if (n) std::memcpy(p.get(), b.data(), n);
    const uint8_t* in = p.get();
    const Table s = serial_walk(in, n);
    Table t = parallel_walk(in, n);
    CHECK(t.status == s.status, "%s [%ld] n %zu: status %d, serial walk %d", what, tag, n, t.status, s.status);
    if (t.status != DMX_OK || s.status != DMX_OK) return t;
    CHECK(t.e.size() == s.e.size() && t.total == s.total && t.h.base == s.h.base && t.eocd == s.eocd,
          "%s [%ld] n %zu: %zu entries / %llu bytes, serial walk %zu / %llu", what, tag, n, t.e.size(),
          (unsigned long long)t.total, s.e.size(), (unsigned long long)s.total);
    if (t.e.size() != s.e.size()) return t;
    for (size_t r = 0; r < t.e.size(); r++)
        CHECK(same_entry(t.e[r], s.e[r]), "%s [%ld] n %zu: entry %zu differs", what, tag, n, r);
    return t;
}

static bool read_file(const char* path, Bytes* b) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) b->insert(b->end(), buf, buf + got);
    std::fclose(f);
    return true;
}

static void put16(Bytes& b, size_t at, uint32_t v) {
    b[at] = (uint8_t)v;
    b[at + 1] = (uint8_t)(v >> 8);
}
static void put64(Bytes& b, size_t at, uint64_t v) {
    for (int k = 0; k < 8; k++) b[at + k] = (uint8_t)(v >> (8 * k));
}

// the archive against what zipfile states
static void check_table(const Table& t, const char* table_path, const char* what) {
    FILE* f = std::fopen(table_path, "r");
    CHECK(f != nullptr, "%s: no table %s", what, table_path);
    if (!f) return;
    unsigned long long count = 0;
    CHECK(std::fscanf(f, "%llu", &count) == 1, "%s: table without a count", what);
    CHECK(t.status == DMX_OK, "%s: status %d", what, t.status);
    CHECK(t.e.size() == count, "%s: %zu entries, zipfile %llu", what, t.e.size(), count);
    uint64_t total = 0;
    for (size_t r = 0; r < t.e.size() && r < count; r++) {
        unsigned long long ho, cs, us, crc, method, doff, flags;
        if (std::fscanf(f, "%llu %llu %llu %llu %llu %llu %llu", &ho, &cs, &us, &crc, &method, &doff, &flags) != 7) {
            CHECK(false, "%s: table row %zu", what, r);
            break;
        }
        const dmx_zip_entry& e = t.e[r];
        const int want = zip_classify((uint32_t)flags, (uint32_t)method);
        CHECK(e.csize == cs && e.usize == us && e.crc == crc && e.method == method && e.gpflags == flags &&
                  e.data_off == doff && e.uoffset == total && e.status == want,
              "%s: entry %zu: csize %llu usize %llu crc %08x method %u flags %u data_off %llu uoffset %llu status %d",
              what, r, (unsigned long long)e.csize, (unsigned long long)e.usize, e.crc, e.method, e.gpflags,
              (unsigned long long)e.data_off, (unsigned long long)e.uoffset, e.status);
        total += us;
    }
    CHECK(t.total == total, "%s: plain bytes %llu, zipfile %llu", what, (unsigned long long)t.total,
          (unsigned long long)total);
    std::fclose(f);
}

// damaged copies of a good archive (t: its table)
static void mutants(const Bytes& good, const Table& t, const char* what) {
    const size_t n = good.size();
    // every single-byte truncation of the last 100 bytes
    for (size_t cut = 1; cut <= 100 && cut <= n; cut++) (void)compare(good, n - cut, "truncated", (long)cut);
    const ZipHead& h = t.h;
    const size_t eocd = (size_t)t.eocd;
    // a count off by one, both ways
    for (int d = -1; d <= 1; d += 2) {
        Bytes b = good;
        if (h.zip64) put64(b, eocd - kZip64Bytes + 32, h.count + d);
        else put16(b, eocd + 10, (uint32_t)(h.count + d));
        if (!h.zip64 && ((h.count == 0 && d < 0) || (h.count == 65535 && d > 0))) continue;  // (wraps to a valid count field)
        const Table m = compare(b, n, "count off by one", d);
        CHECK(m.status == DMX_ERR_DATA, "%s: count %+d: status %d", what, d, m.status);
    }
    if (!h.dir_size) return;
    {  // the directory one byte short: its last byte is gone, the end record still states the size
        Bytes b = good;
        b.erase(b.begin() + (size_t)(h.dir_off + h.dir_size - 1));
        const Table m = compare(b, n - 1, "directory one byte short");
        CHECK(m.status == DMX_ERR_DATA, "%s: short directory: status %d", what, m.status);
    }
    {  // ... and with the stated size one less, so that the region ends inside the last record
        Bytes b = good;
        if (h.zip64) put64(b, eocd - kZip64Bytes + 40, h.dir_size - 1);
        else {
            put16(b, eocd + 12, (uint32_t)(h.dir_size - 1));
            put16(b, eocd + 14, (uint32_t)((h.dir_size - 1) >> 16));
        }
        const Table m = compare(b, n, "stated size one short");
        CHECK(m.status == DMX_ERR_DATA, "%s: stated size one short: status %d", what, m.status);
    }
    // a length field that makes a record overrun the directory (the last record), or the chain
    // miss the next record (the first)
    for (int which = 0; which < 2; which++) {
        const size_t rec = (size_t)(which ? t.rec.front() : t.rec.back());
        for (int field = 28; field <= 32; field += 2) {
            Bytes b = good;
            put16(b, rec + field, zip_le16(&b[rec + field]) + 1);
            const Table m = compare(b, n, "record length + 1", field);
            CHECK(m.status == DMX_ERR_DATA, "%s: record %d field %d + 1: status %d", what, which, field, m.status);
            put16(b, rec + field, 0xFFFF);
            (void)compare(b, n, "record length ffff", field);
        }
    }
    // ZIP64 values near 2^64: in the end record, and in every 0x0001 extra
    const uint64_t wild[] = {~0ull, ~0ull - 1, ~0ull - 0xFFFF, 1ull << 63, (1ull << 63) + 1, (1ull << 63) - 1, 1ull << 32};
    if (h.zip64) {
        for (int field = 32; field <= 48; field += 8)
            for (const uint64_t v : wild) {
                Bytes b = good;
                put64(b, eocd - kZip64Bytes + field, v);
                const Table m = compare(b, n, "ZIP64 end record value", field);
                CHECK(m.status == DMX_ERR_DATA, "%s: ZIP64 end record field %d = %llx: status %d", what, field,
                      (unsigned long long)v, m.status);
            }
    }
    size_t patched = 0;
    for (size_t r = 0; r < t.rec.size() && patched < 8; r++) {
        const size_t rec = (size_t)t.rec[r];
        const uint32_t nl = zip_le16(&good[rec + 28]), el = zip_le16(&good[rec + 30]);
        for (size_t x = rec + 46 + nl, end = x + el; x + 4 <= end;) {
            const uint32_t id = zip_le16(&good[x]), sz = zip_le16(&good[x + 2]);
            if (x + 4 + sz > end) break;
            if (id == 1) {
                patched++;
                for (uint32_t at = 0; at + 8 <= sz; at += 8)
                    for (const uint64_t v : wild) {
                        Bytes b = good;
                        put64(b, x + 4 + at, v);
                        const Table m = compare(b, n, "ZIP64 extra value", (long)at);
                        // the archive stands or its total overflows; the entry never passes as good
                        CHECK(m.status == DMX_ERR_DATA || (m.e.size() == t.e.size() && m.e[r].status != DMX_OK) ||
                                  (m.e.size() == t.e.size() && m.e[r].method == 8 && m.e[r].usize == v),
                              "%s: entry %zu extra value %u = %llx: status %d", what, r, at, (unsigned long long)v,
                              m.status);
                    }
                Bytes b = good;  // the subfield too short for its values
                put16(b, x + 2, sz - 1);
                (void)compare(b, n, "ZIP64 extra short");
            }
            x += 4 + sz;
        }
    }
}

// the serial walk over an archive in memory, best of 20
static int time_walk(const char* path) {
    Bytes b;
    if (!read_file(path, &b)) return 2;
    double best = 1e30;
    size_t entries = 0;
    for (int rep = 0; rep < 20; rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        const Table t = serial_walk(b.data(), b.size());
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (t.status != DMX_OK) return 1;
        entries = t.e.size();
        best = std::min(best, ms);
    }
    std::printf("walk_ms %.4f entries %zu\n", best, entries);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "--walk")) return time_walk(argv[2]);
    if (argc < 3 || (argc - 1) % 2) {
        std::fprintf(stderr, "usage: zip_dir_test <archive> <table> [...]\n");
        return 2;
    }
    {  // no archive at all
        for (size_t n = 0; n < 22; n++) {
            const Bytes b(n, 0x50);
            const Table t = compare(b, n, "too short");
            CHECK(t.status == DMX_ERR_DATA, "n %zu: status %d", n, t.status);
        }
        const Bytes b(70000, 0);
        CHECK(compare(b, b.size(), "zeros").status == DMX_ERR_DATA, "zeros pass as an archive");
    }
    for (int a = 1; a + 1 < argc; a += 2) {
        Bytes b;
        if (!read_file(argv[a], &b)) {
            std::fprintf(stderr, "cannot read %s\n", argv[a]);
            return 2;
        }
        const Table t = compare(b, b.size(), argv[a]);
        check_table(t, argv[a + 1], argv[a]);
        if (t.status == DMX_OK) mutants(b, t, argv[a]);
    }
    {  // zip_total at its edges
        uint64_t tot = 0;
        CHECK(zip_total(0, 0, &tot) && tot == 0, "empty total");
        CHECK(zip_total(1ull << 63, 0, &tot) && tot == 1ull << 63, "2^63 is the most");
        CHECK(!zip_total((1ull << 63) + 1, 0, &tot), "2^63 + 1");
        CHECK(zip_total(0, 1ull << 31, &tot) && tot == 1ull << 63, "2^63 in the high halves");
        CHECK(!zip_total(1, 1ull << 31, &tot), "2^63 + 1 across the halves");
        CHECK(!zip_total(0, (1ull << 31) + 1, &tot), "the high halves alone");
        CHECK(zip_total(0xFFFFFFFFull, (1ull << 31) - 1, &tot) && tot == (1ull << 63) - 1, "2^63 - 1");
        CHECK(zip_total(1ull << 32, (1ull << 31) - 1, &tot) && tot == 1ull << 63, "the carry reaches 2^63");
        CHECK(!zip_total((1ull << 32) + 1, (1ull << 31) - 1, &tot), "the carry passes 2^63");
        CHECK(!zip_total(~0ull, (1ull << 31) - 1, &tot), "both near their ends");
    }
    std::printf("zip_dir_test: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
