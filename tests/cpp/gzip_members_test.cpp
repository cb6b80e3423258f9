// gzip_members_test.cpp -- CPU test of the plain C++ behind dmx_inflate_gzip_members:
// gzip_head_len (deflate.hpp_amd/csrc/container_parse.h), the header-only parse the candidate scan
// runs at every offset, and gzm_walk with the cut rule (deflate.hpp_amd/csrc/gzip_members.{h,cpp}),
// the host's walk over the records the device wrote.
//
// Stand-alone (its own main, no HIP, no GPU); tests/test_gzip_members.py builds it plain and with
// AddressSanitizer + UBSan and runs both directly.  gzip_head_len is compared with a serial parse
// that reads through a bounds-checked accessor, on exact-size heap copies (a read at or beyond
// in + avail is a sanitizer report).  The walk runs on files built from stored-block members, so
// no decoder is needed: candidates and records are synthesised from the bytes by a stored-block
// reader with the device's window rule, and the outcome of the driver loop (walk, long members,
// moving cut, gap check) is compared with a serial model that reads the file front to back.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../deflate.hpp_amd/csrc/container_parse.h"
#include "../../deflate.hpp_amd/csrc/gzip_members.cpp"

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

// ---- gzip_head_len ---------------------------------------------------------------------------

// the serial parse: byte i of the r bytes left, or -1 behind them
struct Left {
    const Bytes& f;
    size_t p;
    int at(size_t i) const { return p + i < f.size() ? f[p + i] : -1; }
    size_t r() const { return f.size() - p; }
};
static int model_head(const Bytes& f, size_t p, uint64_t* head) {
    const Left L{f, p};
    *head = 0;
    if (L.at(0) != 0x1f) return L.at(0) < 0 ? DMX_ERR_OVERREAD : DMX_ERR_DATA;
    if (L.at(1) >= 0 && L.at(1) != 0x8b) return DMX_ERR_DATA;
    if (L.at(2) >= 0 && L.at(2) != 8) return DMX_ERR_DATA;
    if (L.r() < 10) return DMX_ERR_OVERREAD;
    const int flg = L.at(3);
    size_t h = 10;
    if (flg & 4) {
        if (L.r() < 12) return DMX_ERR_OVERREAD;
        h = 12 + (size_t)L.at(10) + 256 * (size_t)L.at(11);
        if (h > L.r()) return DMX_ERR_OVERREAD;
    }
    for (int bit = 8; bit <= 16; bit *= 2) {
        if (!(flg & bit)) continue;
        for (;;) {
            const int b = L.at(h++);
            if (b < 0) return DMX_ERR_OVERREAD;
            if (b == 0) break;
        }
    }
    if (flg & 2) h += 2;
    if (h + 8 > L.r()) return DMX_ERR_OVERREAD;
    *head = h;
    return DMX_OK;
}

// gzip_head_len on an exact-size heap copy of f[p, end)
static int real_head(const Bytes& f, size_t p, uint64_t* head) {
    const size_t r = f.size() - p;
    std::unique_ptr<uint8_t[]> heap(new uint8_t[r ? r : 1]);
    if (r) std::memcpy(heap.get(), f.data() + p, r);
    return gzip_head_len(heap.get(), r, head);
}

static Bytes header(int flg, const Bytes& extra, const std::string& name, const std::string& comment) {
    Bytes h = {0x1f, 0x8b, 8, (uint8_t)flg, 1, 2, 3, 4, 0, 3};
    if (flg & 4) {
        h.push_back((uint8_t)extra.size());
        h.push_back((uint8_t)(extra.size() >> 8));
        h.insert(h.end(), extra.begin(), extra.end());
    }
    if (flg & 8) {
        h.insert(h.end(), name.begin(), name.end());
        h.push_back(0);
    }
    if (flg & 16) {
        h.insert(h.end(), comment.begin(), comment.end());
        h.push_back(0);
    }
    if (flg & 2) {
        h.push_back(0xAB);
        h.push_back(0xCD);
    }
    return h;
}

static void test_head() {
    const Bytes extra = {'X', 'Y', 3, 0, 'a', 'b', 'c'};
    for (int flg = 0; flg < 256; flg++) {  // every flag combination (the reserved bits are ignored)
        Bytes f = header(flg, extra, "name.txt", "a comment");
        const size_t want = f.size();
        f.insert(f.end(), 8, 0x55);
        uint64_t h = 0, hm = 0;
        CHECK(real_head(f, 0, &h) == DMX_OK && h == want, "flags %02x: head %llu, built %zu", flg, (unsigned long long)h, want);
        CHECK(model_head(f, 0, &hm) == DMX_OK && hm == want, "flags %02x: the model disagrees with the construction", flg);
        f.pop_back();  // one byte short of the trailer
        CHECK(real_head(f, 0, &h) == DMX_ERR_OVERREAD, "flags %02x: 7 bytes behind the header", flg);
    }
    // every truncation of a header with FEXTRA, FNAME, FCOMMENT and FHCRC, and of its trailer
    Bytes full = header(0x1e, extra, "n", "comment");
    full.insert(full.end(), 12, 0x77);
    for (size_t len = 0; len <= full.size(); len++) {
        const Bytes f(full.begin(), full.begin() + len);
        uint64_t h = 0, hm = 0;
        const int st = real_head(f, 0, &h), sm = model_head(f, 0, &hm);
        CHECK(st == sm && h == hm, "truncated to %zu: %d head %llu, model %d head %llu", len, st, (unsigned long long)h, sm,
              (unsigned long long)hm);
        if (len < full.size() - 4) CHECK(st == DMX_ERR_OVERREAD, "truncated to %zu: status %d", len, st);
    }
    // every single-byte change of the first 12 bytes (FEXTRA set: bytes 10 and 11 are XLEN), at
    // several amounts of bytes left
    for (int flg : {0x04, 0x1e, 0x00, 0x08}) {
        Bytes base = header(flg, extra, "nm", "c");
        base.insert(base.end(), 40, 0x33);
        for (size_t at = 0; at < 12; at++)
            for (int v = 0; v < 256; v++)
                for (size_t keep : {base.size(), (size_t)30, (size_t)12, (size_t)3, (size_t)2, (size_t)1}) {
                    Bytes f(base.begin(), base.begin() + keep);
                    if (at < f.size()) f[at] = (uint8_t)v;
                    uint64_t h = 0, hm = 0;
                    const int st = real_head(f, 0, &h), sm = model_head(f, 0, &hm);
                    CHECK(st == sm && h == hm, "flags %02x byte %zu = %02x, %zu left: %d head %llu, model %d head %llu", flg, at,
                          v, keep, st, (unsigned long long)h, sm, (unsigned long long)hm);
                }
    }
    // an unterminated name that runs to the last byte; a header in mid-file
    Bytes f = header(8, {}, "abcdefghijklmnopqrstuvwxyz", "");
    f.pop_back();
    uint64_t h = 0;
    CHECK(real_head(f, 0, &h) == DMX_ERR_OVERREAD, "an unterminated name");
    Bytes g(5, 0);
    const Bytes hd = header(0, {}, "", "");
    g.insert(g.end(), hd.begin(), hd.end());
    g.insert(g.end(), 8, 1);
    CHECK(real_head(g, 5, &h) == DMX_OK && h == 10, "a header at offset 5");
    CHECK(real_head(g, 0, &h) == DMX_ERR_DATA, "zeros where a header is expected");
}

// ---- files of stored-block members ------------------------------------------------------------

// a raw DEFLATE stream of stored blocks (at most `block` bytes each) holding `plain`
static Bytes stored_stream(const Bytes& plain, size_t block = 65535) {
    Bytes s;
    size_t o = 0;
    do {
        const size_t len = plain.size() - o < block ? plain.size() - o : block;
        s.push_back(o + len == plain.size() ? 1 : 0);
        s.push_back((uint8_t)len);
        s.push_back((uint8_t)(len >> 8));
        s.push_back((uint8_t)~len);
        s.push_back((uint8_t)(~len >> 8));
        s.insert(s.end(), plain.begin() + o, plain.begin() + o + len);
        o += len;
    } while (o < plain.size());
    return s;
}
static Bytes member(const Bytes& plain, int flg = 0, size_t block = 65535) {
    Bytes m = header(flg, {'Q', 'Q', 1, 0, 9}, "file", "note");
    const Bytes s = stored_stream(plain, block);
    m.insert(m.end(), s.begin(), s.end());
    m.insert(m.end(), 4, 0xC5);  // (the CRC-32 is not looked at here)
    for (int b = 0; b < 4; b++) m.push_back((uint8_t)(plain.size() >> (8 * b)));
    return m;
}
static Bytes filler(size_t n, uint32_t seed) {  // bytes that hold neither 1f nor 00
    Bytes b(n);
    for (size_t i = 0; i < n; i++) {
        seed = seed * 1664525u + 1013904223u;
        b[i] = (uint8_t)(0x20 + (seed >> 24) % 0x5f);
    }
    return b;
}
static void append(Bytes& f, const Bytes& b) { f.insert(f.end(), b.begin(), b.end()); }

// The stored-block reader over f[s0, lim): DMX_OK with *end (just past the final block) and
// *plain, DMX_ERR_OVERREAD where a block runs past lim, DMX_ERR_DATA on another block type.
static int read_stored(const Bytes& f, uint64_t s0, uint64_t lim, uint64_t* end, uint64_t* plain) {
    uint64_t p = s0;
    *plain = 0;
    for (;;) {
        if (p + 5 > lim) return DMX_ERR_OVERREAD;
        if ((f[p] >> 1) & 3) return DMX_ERR_DATA;
        const uint64_t len = f[p + 1] | (f[p + 2] << 8);
        if (p + 5 + len > lim) return DMX_ERR_OVERREAD;
        *plain += len;
        const bool fin = f[p] & 1;
        p += 5 + len;
        if (fin) {
            *end = p;
            return DMX_OK;
        }
    }
}

// what the device hands the host: every offset whose header parses, each measured over a window
// of at most `limit` bytes
static void synthesise(const Bytes& f, uint64_t limit, std::vector<GzmCand>* cands, std::vector<GzmRec>* recs) {
    for (size_t p = 0; p + 18 <= f.size(); p++) {
        uint64_t head;
        if (f[p] != 0x1f || f[p + 1] != 0x8b || f[p + 2] != 8) continue;
        if (gzip_head_len(f.data() + p, f.size() - p, &head) != DMX_OK) continue;
        cands->push_back(GzmCand{p, head});
        const uint64_t s0 = p + head, avail = f.size() - s0, win = avail < limit ? avail : limit;
        GzmRec r{};
        r.status = read_stored(f, s0, s0 + win, &r.end, &r.plain);
        if (r.status != DMX_OK) r.end = r.plain = 0;
        r.cut = r.status == DMX_ERR_OVERREAD && win < avail;
        recs->push_back(r);
    }
}

struct Outcome {
    int status = DMX_OK;
    std::vector<GzmRow> rows;  // on an error: the members in front of it
    unsigned long_decodes = 0;
    bool operator==(const Outcome& o) const {
        if (status != o.status || rows.size() != o.rows.size()) return false;
        for (size_t k = 0; k < rows.size(); k++)
            if (rows[k].coff != o.rows[k].coff || rows[k].head != o.rows[k].head || rows[k].end != o.rows[k].end ||
                rows[k].plain != o.rows[k].plain)
                return false;
        return true;
    }
};

// the serial model: the file front to back, as gzip.decompress reads it
static Outcome model_file(const Bytes& f, uint64_t from = 0) {
    Outcome o;
    uint64_t p = from;
    const uint64_t n = f.size();
    if (p > n) {
        o.status = DMX_ERR_OVERREAD;
        return o;
    }
    while (p < n) {
        if (p != 0)
            while (p < n && f[p] == 0) p++;
        if (p == n) break;
        uint64_t head, end, plain;
        o.status = model_head(f, p, &head);
        if (o.status != DMX_OK) return o;
        o.status = read_stored(f, p + head, n, &end, &plain);
        if (o.status != DMX_OK) return o;
        if (end + 8 > n) {
            o.status = DMX_ERR_OVERREAD;
            return o;
        }
        o.rows.push_back(GzmRow{p, head, end, plain});
        p = end + 8;
    }
    return o;
}

// the host driver's loop over gzm_walk, the cut rule and the gap check, with the stored-block
// reader in place of the single-stream decode of a long member
static Outcome drive(const Bytes& f, uint64_t limit, uint64_t from = 0) {
    std::vector<GzmCand> cv;
    std::vector<GzmRec> rv;
    synthesise(f, limit, &cv, &rv);
    // exact-size heap copies: the walk must not read past ncand
    const uint64_t ncand = cv.size(), n = f.size();
    std::unique_ptr<GzmCand[]> cands(new GzmCand[ncand ? ncand : 1]);
    std::unique_ptr<GzmRec[]> recs(new GzmRec[ncand ? ncand : 1]);
    for (uint64_t i = 0; i < ncand; i++) cands[i] = cv[i], recs[i] = rv[i];
    Outcome o;
    std::vector<GzmGap> gaps;
    bool bad_start = false;
    for (;;) {
        const GzmWalk w = gzm_walk(cands.get(), recs.get(), ncand, n, from, &o.rows, &gaps);
        if (w.what == GZM_DONE) break;
        if (w.what == GZM_BAD_START) {
            bad_start = true;
            break;
        }
        if (w.what != GZM_LONG) {
            o.status = w.what;
            break;
        }
        const GzmCand lc = cands[w.k];
        GzmCut cut = gzm_first_cut(cands.get(), ncand, w.k, n, limit);
        uint64_t end = 0, plain = 0;
        int rc;
        for (;;) {
            CHECK(cut.end > lc.off + lc.head && cut.end <= n, "a cut at %llu", (unsigned long long)cut.end);
            rc = read_stored(f, lc.off + lc.head, cut.end, &end, &plain);
            o.long_decodes++;
            if (rc != DMX_ERR_OVERREAD || !gzm_next_cut(cands.get(), ncand, n, &cut)) break;
        }
        if (rc == DMX_OK && end + 8 > n) rc = DMX_ERR_OVERREAD;
        if (rc != DMX_OK) {
            o.status = rc;
            break;
        }
        o.rows.push_back(GzmRow{lc.off, lc.head, end, plain});
        from = end + 8;
    }
    uint64_t q = ~0ull;  // the gap check
    if (bad_start) q = 0;
    for (size_t g = 0; g < gaps.size() && q == ~0ull; g++) {
        CHECK(gaps[g].a < gaps[g].b && gaps[g].b <= n, "gap %zu is [%llu, %llu)", g, (unsigned long long)gaps[g].a,
              (unsigned long long)gaps[g].b);
        for (uint64_t p = gaps[g].a; p < gaps[g].b; p++)
            if (f[p]) {
                q = p;
                break;
            }
    }
    if (q != ~0ull) {
        while (!o.rows.empty() && o.rows.back().coff > q) o.rows.pop_back();
        uint64_t head;
        o.status = real_head(f, q, &head);
        CHECK(o.status != DMX_OK, "a header that parses at %llu was no candidate", (unsigned long long)q);
    }
    return o;
}

static void check_file(const Bytes& f, uint64_t limit, const char* what, int want_status, long want_members = -1,
                       uint64_t from = 0) {
    const Outcome m = model_file(f, from), d = drive(f, limit, from);
    CHECK(m.status == want_status, "%s: the model's status is %d, expected %d", what, m.status, want_status);
    if (want_members >= 0) CHECK((long)m.rows.size() == want_members, "%s: the model has %zu members", what, m.rows.size());
    CHECK(d == m, "%s (limit %llu): status %d with %zu members, model %d with %zu", what, (unsigned long long)limit, d.status,
          d.rows.size(), m.status, m.rows.size());
}

static void test_walk() {
    const uint64_t BIG = 1u << 20;
    const Bytes a = filler(300, 1), b = filler(70000, 2), e;
    {
        const Bytes f = member(a);
        check_file(f, BIG, "one member", DMX_OK, 1);
        check_file(Bytes(), BIG, "the empty file", DMX_OK, 0);
    }
    {
        Bytes f = member(a, 0x1e);
        append(f, member(b, 8));
        check_file(f, BIG, "two members", DMX_OK, 2);
        check_file(f, 1000, "two members, the second one long", DMX_OK, 2);
    }
    {
        Bytes f;
        for (int k = 0; k < 500; k++) append(f, member(filler(k % 7 == 3 ? 0 : 10 + k, k), k % 3 ? 0 : 8));
        check_file(f, BIG, "500 members, some empty", DMX_OK, 500);
        check_file(f, 300, "500 members, some of them long", DMX_OK, 500);
    }
    {
        Bytes f = member(e);
        append(f, member(e, 2));
        append(f, member(a));
        append(f, member(e));
        check_file(f, BIG, "empty members", DMX_OK, 4);
    }
    for (size_t gap : {(size_t)1, (size_t)7, (size_t)4096}) {
        Bytes f = member(a);
        f.insert(f.end(), gap, 0);
        append(f, member(b));
        f.insert(f.end(), gap, 0);
        append(f, member(e));
        check_file(f, BIG, "zero gaps between members", DMX_OK, 3);
        f.insert(f.end(), gap, 0);
        check_file(f, BIG, "zero gaps between members and at the end", DMX_OK, 3);
        check_file(f, 200, "zero gaps, long members", DMX_OK, 3);
        Bytes g = f;
        g[g.size() - 1] = 'x';
        check_file(g, BIG, "a non-zero byte ends the padding", DMX_ERR_DATA);
        g = f;
        g[member(a).size() + gap / 2] = 0x1f;  // a lone 1f in the first gap: the header does not fit or is bad
        check_file(g, BIG, "a non-zero byte in the first gap", model_file(g).status);
        CHECK(model_file(g).rows.size() == 1, "one member in front of the bad gap");
    }
    {
        Bytes f = member(a);
        append(f, {'x', 'y'});
        check_file(f, BIG, "garbage behind the last trailer", DMX_ERR_DATA);
        Bytes z(40, 0);
        append(z, member(a));
        check_file(z, BIG, "leading zeros", DMX_ERR_DATA, 0);
        check_file(Bytes(3, 0), BIG, "zeros alone", DMX_ERR_DATA, 0);
        check_file(filler(100, 5), BIG, "no candidate at all", DMX_ERR_DATA, 0);
    }
    {
        // a complete .gz and the bare magic inside a stored payload: a candidate with a good record
        // and one with an error, neither on the chain
        Bytes pay = filler(100, 7);
        append(pay, member(filler(50, 8)));
        append(pay, filler(30, 9));
        append(pay, {0x1f, 0x8b, 8, 0});
        append(pay, filler(60, 10));
        Bytes f = member(pay);
        append(f, member(a));
        append(f, member(e));
        std::vector<GzmCand> cv;
        std::vector<GzmRec> rv;
        synthesise(f, BIG, &cv, &rv);
        CHECK(cv.size() == 5, "nested: %zu candidates", cv.size());
        if (cv.size() == 5) {
            CHECK(rv[1].status == DMX_OK && rv[1].plain == 50, "the nested file's record is good");
            CHECK(rv[2].status != DMX_OK, "the bare magic's record is an error");
        }
        check_file(f, BIG, "a nested .gz and a bare magic in a payload", DMX_OK, 3);
        check_file(f, 120, "nested, the outer member long", DMX_OK, 3);
    }
    {
        // a false candidate on the chain's path: garbage that starts like a header where the next
        // member is expected -- its record is the status
        Bytes f = member(a);
        append(f, {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3, 0x07});  // block type 3
        append(f, filler(40, 11));
        check_file(f, BIG, "a candidate whose record is an error", DMX_ERR_DATA);
    }
    {
        // a long member, behind its limit a false candidate (a nested .gz) and then true ones: the
        // first cut is the false one, the decode runs off it, the cut moves on
        Bytes pay = filler(5000, 12);
        append(pay, member(filler(40, 13)));
        append(pay, filler(3000, 14));
        Bytes f = member(filler(20, 15));
        const size_t long_at = f.size();
        append(f, member(pay, 0, 1000));
        append(f, member(a));
        append(f, member(e));
        check_file(f, 2000, "a cut that moves past a false candidate", DMX_OK, 4);
        const Outcome d = drive(f, 2000);
        CHECK(d.long_decodes == 2, "the long member was decoded %u times", d.long_decodes);
        std::vector<GzmCand> cv;
        std::vector<GzmRec> rv;
        synthesise(f, 2000, &cv, &rv);
        const uint64_t k = gzm_cand_at(cv.data(), cv.size(), long_at);
        CHECK(k == 1 && rv[k].cut, "candidate %llu is the long member", (unsigned long long)k);
        GzmCut cut = gzm_first_cut(cv.data(), cv.size(), k, f.size(), 2000);
        CHECK(cut.idx == 2 && cut.end == cv[2].off && cv[2].off > long_at + 5000, "the first cut is the nested file");
        CHECK(gzm_next_cut(cv.data(), cv.size(), f.size(), &cut) && cut.idx == 3 && cut.end == cv[3].off, "the second cut");
        CHECK(gzm_next_cut(cv.data(), cv.size(), f.size(), &cut) && cut.idx == 4, "the third cut");
        CHECK(gzm_next_cut(cv.data(), cv.size(), f.size(), &cut) && cut.idx == cv.size() && cut.end == f.size(), "the file's end");
        CHECK(!gzm_next_cut(cv.data(), cv.size(), f.size(), &cut), "no cut behind the file's end");
        // the same with no false candidate: one decode
        Bytes g = member(filler(9000, 16), 0, 1000);
        append(g, member(a));
        CHECK(drive(g, 2000).long_decodes == 1, "a long member with no false candidate behind it is decoded once");
        check_file(g, 2000, "a long member, then a small one", DMX_OK, 2);
        // a long member that is truncated: every cut runs off, the last one is the file's end
        Bytes t(f.begin(), f.begin() + long_at + 7000);
        check_file(t, 2000, "a truncated long member", DMX_ERR_OVERREAD, 1);
    }
    {
        Bytes f = member(a);
        append(f, member(b));
        for (size_t cutoff : {f.size() - 1, f.size() - 8, f.size() - 9, f.size() - 30000, member(a).size() + 12,
                              member(a).size() + 2, member(a).size() + 1}) {
            const Bytes t(f.begin(), f.begin() + cutoff);
            check_file(t, BIG, "a truncated last member", DMX_ERR_OVERREAD, 1);
            check_file(t, 500, "a truncated last member, long", DMX_ERR_OVERREAD, 1);
        }
    }
    {
        // `from` in mid-file: behind the first member's trailer, inside padding, at n, past n
        Bytes f = member(a);
        const uint64_t second = f.size();
        f.insert(f.end(), 5, 0);
        append(f, member(b));
        append(f, member(e));
        check_file(f, BIG, "from the first trailer's end", DMX_OK, 2, second);
        check_file(f, BIG, "from inside the padding", DMX_OK, 2, second + 3);
        check_file(f, BIG, "from n", DMX_OK, 0, f.size());
        check_file(f, BIG, "from past n", DMX_ERR_OVERREAD, 0, f.size() + 1);
        check_file(f, BIG, "from inside a member", DMX_ERR_DATA, 0, second + 6);
    }
}

int main() {
    test_head();
    test_walk();
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
