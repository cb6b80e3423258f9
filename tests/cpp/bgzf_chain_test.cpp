// bgzf_chain_test.cpp -- CPU test of deflate.hpp_amd/csrc/bgzf_chain.h: the parallel form of the
// BGZF member-chain walk that the kernels of bgzf_chain.hip run.
//
// Stand-alone (no HIP, no GPU); tests/test_bgzf_chain.py builds it plain and with
// AddressSanitizer + UBSan and runs both directly.  The steps (candidates, links, doubling,
// length, rank, end of chain) are run serially over all "threads" on a heap copy of exactly n
// bytes, so a read at or beyond n is a sanitizer report; the member table and the status are
// compared with the serial walk `for (off = 0; off < n;) bgzf_next(...)` of dmx_inflate_bgzf.
// Also the plain C++ of the candidate scan's staging (cand_scan.h): which bytes of an aligned
// 16-byte line lie in the scanned region, for every misalignment and every short length.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../deflate.hpp_amd/csrc/bgzf_chain.h"
#include "../../deflate.hpp_amd/csrc/cand_scan.h"

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
    std::vector<BgzfCand> rows;
    std::vector<uint64_t> uoff;
    uint64_t total = 0;
    int status = DMX_OK;
};

// the host loop of dmx_inflate_bgzf
static Table serial_walk(const uint8_t* in, uint64_t n) {
    Table t;
    for (uint64_t off = 0; off < n;) {
        BgzfMember m;
        t.status = bgzf_next(in, n, off, &m);
        if (t.status != DMX_OK) break;
        t.rows.push_back(BgzfCand{m.off, (uint32_t)m.size, m.isize});
        t.uoff.push_back(t.total);
        t.total += m.isize;
        off += m.size;
    }
    return t;
}

// the kernels' steps, every "thread" in turn
static Table parallel_walk(const uint8_t* in, uint64_t n, uint64_t* ncand_out) {
    Table t;
    std::vector<BgzfCand> cands;
    for (uint64_t off = 0; off < n; off++) {  // (the kernels test bgzf_magic on staged bytes first)
        BgzfCand c;
        const bool magic = n - off >= 4 && bgzf_magic(frame_le32(in + off));
        const bool ok = bgzf_candidate(in, n, off, &c);
        CHECK(!ok || magic, "offset %llu: a member the magic filter drops", (unsigned long long)off);
        if (magic && ok) cands.push_back(c);
    }
    const uint64_t nc = cands.size();
    *ncand_out = nc;
    const uint32_t levels = bgzf_levels(nc);
    std::vector<uint32_t> J((size_t)levels * (nc ? nc : 1), kBgzfNone);
    for (uint64_t i = 0; i < nc; i++) J[i] = bgzf_link(cands.data(), nc, i, n);
    for (uint32_t k = 0; k + 1 < levels; k++)
        for (uint64_t i = 0; i < nc; i++) J[(size_t)(k + 1) * nc + i] = bgzf_double(J.data() + (size_t)k * nc, i);
    uint64_t members = 0;
    t.status = bgzf_chain_status(in, n, cands.data(), nc, J.data(), levels, &members);
    t.rows.resize(members);
    for (uint64_t r = 0; r < members; r++) t.rows[r] = cands[bgzf_rank_lookup(J.data(), nc, levels, r)];
    for (uint64_t r = 0; r < members; r++) {  // the exclusive scan of ISIZE
        t.uoff.push_back(t.total);
        t.total += t.rows[r].isize;
    }
    return t;
}

static uint64_t compare(const Bytes& b, size_t n, const char* what, long tag = -1) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);  // exact size
    if (n) std::memcpy(p.get(), b.data(), n);
    const uint8_t* in = p.get();
    const Table s = serial_walk(in, n);
    uint64_t nc = 0;
    const Table t = parallel_walk(in, n, &nc);
    CHECK(t.status == s.status, "%s [%ld] n %zu: status %d, serial walk %d", what, tag, n, t.status, s.status);
    CHECK(t.rows.size() == s.rows.size(), "%s [%ld] n %zu: %zu members, serial walk %zu", what, tag, n,
          t.rows.size(), s.rows.size());
    CHECK(t.total == s.total, "%s [%ld] n %zu: plain bytes differ", what, tag, n);
    if (t.rows.size() != s.rows.size()) return nc;
    for (size_t r = 0; r < t.rows.size(); r++)
        CHECK(t.rows[r].off == s.rows[r].off && t.rows[r].size == s.rows[r].size &&
                  t.rows[r].isize == s.rows[r].isize && t.uoff[r] == s.uoff[r],
              "%s [%ld] n %zu: member %zu differs", what, tag, n, r);
    return nc;
}

// ---- file builders: members with stored payloads (the chain never decodes them) -----------------
static void put16(Bytes& b, size_t at, uint32_t v) {
    b[at] = (uint8_t)v;
    b[at + 1] = (uint8_t)(v >> 8);
}

// one member around `plain` (<= 65535 bytes); extra: a subfield "XY" of 3 bytes before BC
static Bytes member(const Bytes& plain, bool extra = false) {
    Bytes m = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, (uint8_t)(extra ? 13 : 6), 0};
    if (extra) {
        const uint8_t x[7] = {'X', 'Y', 3, 0, 1, 2, 3};
        m.insert(m.end(), x, x + 7);
    }
    const uint8_t bc[6] = {66, 67, 2, 0, 0, 0};
    m.insert(m.end(), bc, bc + 6);
    const size_t bsize_at = m.size() - 2;
    const uint32_t len = (uint32_t)plain.size();
    const uint8_t st[5] = {1, (uint8_t)len, (uint8_t)(len >> 8), (uint8_t)~len, (uint8_t)(~len >> 8)};
    m.insert(m.end(), st, st + 5);
    m.insert(m.end(), plain.begin(), plain.end());
    for (int k = 0; k < 4; k++) m.push_back((uint8_t)(0xC0 + k));  // CRC-32: not looked at
    for (int k = 0; k < 4; k++) m.push_back((uint8_t)(len >> (8 * k)));
    put16(m, bsize_at, (uint32_t)m.size() - 1);
    return m;
}
static Bytes eof_member() { return member(Bytes()); }

static Bytes pattern(size_t n, uint32_t seed) {
    Bytes p(n);
    for (size_t i = 0; i < n; i++) {
        seed = seed * 1664525u + 1013904223u;
        p[i] = (uint8_t)(seed >> 24);
    }
    return p;
}
static void append(Bytes& f, const Bytes& m) { f.insert(f.end(), m.begin(), m.end()); }

// hostile (a): a BGZF file stored again -- the inner headers sit verbatim in the outer payloads
static Bytes stored_again(const Bytes& inner, size_t block) {
    Bytes f;
    for (size_t o = 0; o < inner.size(); o += block)
        append(f, member(Bytes(inner.begin() + o, inner.begin() + std::min(inner.size(), o + block))));
    append(f, eof_member());
    return f;
}

// hostile (b): one stored member whose payload is back-to-back fake 18-byte headers, then real
// members.  Fake k's BSIZE: k % 3 == 0 lands exactly on the next real member's start, k % 3 == 1
// points past n, k % 3 == 2 lands on a later fake header (a chain of false candidates).
static Bytes fake_headers(size_t payload) {
    const size_t nfake = payload / 18;
    Bytes pay(payload, 0);
    const Bytes tail1 = member(pattern(300, 5)), tail2 = member(pattern(40, 6)), tail3 = eof_member();
    const size_t pay_at = 18 + 5, next_real = pay_at + payload + 8;
    const size_t n = next_real + tail1.size() + tail2.size() + tail3.size();
    for (size_t k = 0; k < nfake; k++) {
        const uint8_t h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0};
        std::memcpy(&pay[18 * k], h, 16);
        const size_t at = pay_at + 18 * k;  // the fake header's file offset
        size_t size;
        if (k % 3 == 0) size = next_real - at;
        else if (k % 3 == 1) size = n - at + 1 + k % 7;
        else size = 18 * (2 + k % 5);
        if (size < 26 || size > 65536) size = 65536;
        put16(pay, 18 * k + 16, (uint32_t)size - 1);
    }
    Bytes f = member(pay);
    append(f, tail1);
    append(f, tail2);
    append(f, tail3);
    return f;
}

// cand_scan.h's ragged-end rule against its bytewise definition: the region is [lead, lead + len) of
// the aligned view; every line the staging can load (and one past), every byte of it
static void line_masks() {
    for (uint64_t lead = 0; lead < 16; lead++)
        for (uint64_t len = 0; len <= 48; len++) {
            const uint64_t vend = lead + len;
            for (uint64_t q = 0; q <= vend + 16; q += 16) {
                uint32_t m[4];
                scan_line_mask(q, lead, vend, m);
                bool all = true;
                for (uint64_t j = 0; j < 16; j++) {
                    const bool in = q + j >= lead && q + j < vend;
                    all = all && in;
                    const uint32_t got = (m[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                    CHECK(got == (in ? 0xFFu : 0u), "line mask: lead %llu len %llu line %llu byte %llu: %02x",
                          (unsigned long long)lead, (unsigned long long)len, (unsigned long long)q,
                          (unsigned long long)j, got);
                }
                CHECK(scan_line_inside(q, lead, vend) == all, "line inside: lead %llu len %llu line %llu",
                      (unsigned long long)lead, (unsigned long long)len, (unsigned long long)q);
            }
            // the tiles cover the view: the last one holds its last byte
            const uint8_t* const reg = reinterpret_cast<const uint8_t*>((uintptr_t)(4096 + lead));
            CHECK(scan_tiles(reg, len) == (len ? 1u : 0u), "tiles: lead %llu len %llu", (unsigned long long)lead,
                  (unsigned long long)len);
        }
    const uint8_t* const r5 = reinterpret_cast<const uint8_t*>((uintptr_t)(4096 + 5));
    CHECK(scan_tiles(r5, kScanTile - 5) == 1 && scan_tiles(r5, kScanTile - 4) == 2, "tiles: the edge");
}

int main() {
    line_masks();
    // three members: every truncation, every single-byte change of the first 64 bytes and of
    // each member's BSIZE / ISIZE bytes
    const Bytes m0 = member(pattern(200, 1)), m1 = member(pattern(77, 2)), m2 = member(pattern(130, 3));
    Bytes three = m0;
    append(three, m1);
    append(three, m2);
    for (size_t n = 0; n <= three.size(); n++) compare(three, n, "truncation");
    auto flips = [&](size_t at) {
        for (int v = 0; v < 256; v++) {
            if ((uint8_t)v == three[at]) continue;
            Bytes f = three;
            f[at] = (uint8_t)v;
            compare(f, f.size(), "byte change", (long)at);
        }
    };
    for (size_t at = 0; at < 64; at++) flips(at);
    const size_t starts[3] = {0, m0.size(), m0.size() + m1.size()}, sizes[3] = {m0.size(), m1.size(), m2.size()};
    for (int k = 0; k < 3; k++) {
        for (size_t b = 16; b < 18; b++)
            if (starts[k] + b >= 64) flips(starts[k] + b);
        for (size_t b = sizes[k] - 4; b < sizes[k]; b++) flips(starts[k] + b);
    }

    // an empty member in the middle; with and without the EOF member
    Bytes mid = m0;
    append(mid, eof_member());
    append(mid, m1);
    compare(mid, mid.size(), "empty member in the middle, no EOF");
    append(mid, eof_member());
    compare(mid, mid.size(), "empty member in the middle, EOF");
    compare(eof_member(), eof_member().size(), "EOF alone");
    compare(Bytes(), 0, "empty file");

    // FEXTRA with another subfield before BC
    Bytes ex = member(pattern(90, 7), true);
    append(ex, m1);
    append(ex, member(pattern(10, 8), true));
    append(ex, eof_member());
    compare(ex, ex.size(), "subfield before BC");
    for (size_t n = 0; n <= 60; n++) compare(ex, n, "subfield before BC, cut");

    // hostile candidates
    Bytes inner;
    for (uint32_t k = 0; k < 40; k++) append(inner, member(pattern(50 + 13 * k, 100 + k)));
    append(inner, eof_member());
    for (const size_t block : {(size_t)65280, (size_t)1000, (size_t)97}) {
        const Bytes a = stored_again(inner, block);
        const uint64_t nc = compare(a, a.size(), "stored again", (long)block);
        CHECK(nc > serial_walk(a.data(), a.size()).rows.size(), "stored again: no false candidates (%llu)",
              (unsigned long long)nc);
        compare(a, a.size() - 1, "stored again, cut", (long)block);
    }
    const Bytes b = fake_headers(65280);
    const uint64_t ncb = compare(b, b.size(), "fake headers");
    CHECK(ncb > 1000, "fake headers: only %llu candidates", (unsigned long long)ncb);
    CHECK(serial_walk(b.data(), b.size()).rows.size() == 4, "fake headers: the true chain has 4 members");
    compare(b, b.size() - 5, "fake headers, cut");
    const Bytes b2 = fake_headers(18 * 40 + 7);
    compare(b2, b2.size(), "fake headers, short");

    std::printf("bgzf_chain_test: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
