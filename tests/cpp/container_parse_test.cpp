// container_parse_test.cpp -- CPU test of deflate.hpp_amd/csrc/container_parse.h: the zlib / gzip /
// BGZF header parse the frame kernels run, the header / trailer writers and the BGZF chain step.
//
// Stand-alone (no HIP, no GPU); tests/test_container_parse.py builds it plain and with
// AddressSanitizer + UBSan and runs both directly.  Every buffer handed to the parser is a heap
// copy of exactly n bytes, so a read at or beyond n is a sanitizer report.  Statuses are compared
// with ref_parse below, the checks of dmx_inflate_zlib / dmx_inflate_gzip written the plain way
// on a zero-padded copy.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../deflate.hpp_amd/csrc/container_parse.h"

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

// parse an exact-size heap copy
static FrameHead parse_exact(uint32_t format, const Bytes& b, size_t n) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    if (n) std::memcpy(p.get(), b.data(), n);
    return parse_frame(format, p.get(), n);
}

struct Ref {
    int status;
    uint64_t head;
    uint32_t member;
};
static Ref ref_parse(uint32_t format, const Bytes& b, size_t n) {
    Bytes in(b.begin(), b.begin() + n);
    in.resize(n + 16, 0);  // (bytes 10 and 11 are read once n >= 18; every other read is guarded by n)
    Ref r{DMX_OK, 0, 0};
    if (format == DMX_FRAME_ZLIB) {
        if (n < 6) return Ref{DMX_ERR_OVERREAD, 0, 0};
        const uint32_t cmf = in[0], flg = in[1];
        if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (cmf * 256 + flg) % 31 != 0) return Ref{DMX_ERR_DATA, 0, 0};
        if (flg & 0x20) return Ref{DMX_ERR_DATA, 0, 0};
        r.head = 2;
        return r;
    }
    if (n < 18) return Ref{DMX_ERR_OVERREAD, 0, 0};
    if (in[0] != 0x1F || in[1] != 0x8B || in[2] != 8) return Ref{DMX_ERR_DATA, 0, 0};
    const uint8_t flg = in[3];
    size_t head = 10;
    if (flg & 4) {
        const size_t xlen = in[10] | (in[11] << 8);
        if (12 + xlen + 8 <= n)
            for (size_t p = 12; p + 4 <= 12 + xlen;) {
                const size_t slen = in[p + 2] | (in[p + 3] << 8);
                if (in[p] == 'B' && in[p + 1] == 'C' && slen == 2 && p + 6 <= 12 + xlen) {
                    r.member = (uint32_t)(in[p + 4] | (in[p + 5] << 8)) + 1;
                    break;
                }
                p += 4 + slen;
            }
        head += 2 + xlen;
    }
    for (int z = 0; z < 2; z++) {
        if (flg & (8 << z)) {
            while (head < n && in[head]) head++;
            head++;
        }
    }
    if (flg & 2) head += 2;
    if (head + 8 > n) return Ref{DMX_ERR_OVERREAD, 0, 0};
    if (format == DMX_FRAME_BGZF && r.member != n) return Ref{DMX_ERR_DATA, 0, 0};
    r.head = head;
    return r;
}

static void compare(uint32_t format, const Bytes& b, size_t n, const char* what) {
    const FrameHead h = parse_exact(format, b, n);
    const Ref r = ref_parse(format, b, n);
    CHECK(h.status == r.status, "%s fmt %u n %zu: status %d, expected %d", what, format, n, h.status, r.status);
    if (h.status != DMX_OK || r.status != DMX_OK) return;
    CHECK(h.head == r.head, "%s fmt %u n %zu: head %llu, expected %llu", what, format, n, (unsigned long long)h.head,
          (unsigned long long)r.head);
    CHECK(h.head + frame_tail_bytes(format) <= n, "%s: head past the trailer", what);
    if (format != DMX_FRAME_ZLIB) {
        CHECK(h.member == r.member, "%s fmt %u n %zu: member %u, expected %u", what, format, n, h.member, r.member);
        CHECK(h.want == frame_le32(b.data() + n - 8) && h.isize == frame_le32(b.data() + n - 4), "%s: trailer", what);
    } else {
        const uint8_t* t = b.data() + n - 4;
        CHECK(h.want == (((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3]), "%s: trailer", what);
    }
}

static void put16(Bytes& b, uint32_t v) {
    b.push_back((uint8_t)v);
    b.push_back((uint8_t)(v >> 8));
}
static void put32(Bytes& b, uint32_t v) {
    put16(b, v & 0xFFFF);
    put16(b, v >> 16);
}

static Bytes payload(size_t n, uint32_t seed) {  // stands for a raw stream (never decoded here); no zero bytes
    Bytes p(n);
    for (size_t i = 0; i < n; i++) p[i] = (uint8_t)(1 + (seed + 7 * i) % 255);
    return p;
}

// gzip member with the optional fields of `flg` (4 FEXTRA, 8 FNAME, 16 FCOMMENT, 2 FHCRC)
static Bytes make_gzip(uint32_t flg, const Bytes& extra, const Bytes& raw, size_t* head_out = nullptr) {
    Bytes g = {0x1F, 0x8B, 8, (uint8_t)flg, 0, 0, 0, 0, 0, 255};
    if (flg & 4) {
        put16(g, (uint32_t)extra.size());
        g.insert(g.end(), extra.begin(), extra.end());
    }
    if (flg & 8) {
        const char* s = "name.txt";
        g.insert(g.end(), s, s + std::strlen(s) + 1);
    }
    if (flg & 16) {
        const char* s = "a comment";
        g.insert(g.end(), s, s + std::strlen(s) + 1);
    }
    if (flg & 2) put16(g, 0xBEEF);
    if (head_out) *head_out = g.size();
    g.insert(g.end(), raw.begin(), raw.end());
    put32(g, 0x12345678u);
    put32(g, 0x9ABCDEF0u);
    return g;
}

// BGZF member: FEXTRA = `before` (other subfields) + BC; bsize_delta falsifies BSIZE
static Bytes make_bgzf(const Bytes& before, const Bytes& raw, uint32_t isize, int bsize_delta = 0) {
    Bytes extra = before;
    extra.insert(extra.end(), {66, 67, 2, 0, 0, 0});
    Bytes g = make_gzip(4, extra, raw);
    const uint32_t bsize = (uint32_t)((int)g.size() - 1 + bsize_delta);
    g[12 + before.size() + 4] = (uint8_t)bsize;
    g[12 + before.size() + 5] = (uint8_t)(bsize >> 8);
    for (int b = 0; b < 4; b++) g[g.size() - 4 + b] = (uint8_t)(isize >> (8 * b));
    return g;
}

static void truncations_and_mutations(const Bytes& b, const char* what) {
    for (uint32_t format = 1; format <= 3; format++) {
        for (size_t n = 0; n <= b.size(); n++) compare(format, b, n, what);  // every truncation length
        for (size_t i = 0; i < 32 && i < b.size(); i++) {                    // every single-byte change
            Bytes m = b;
            for (int v = 0; v < 256; v++) {
                if (v == b[i]) continue;
                m[i] = (uint8_t)v;
                compare(format, m, m.size(), what);
            }
        }
    }
}

static void test_zlib() {
    for (int level = -1; level <= 4; level++) {
        Bytes z(2);
        frame_write_head(DMX_FRAME_ZLIB, level, 0, z.data());
        const Bytes raw = payload(40, level + 5);
        z.insert(z.end(), raw.begin(), raw.end());
        z.resize(z.size() + 4);
        frame_write_tail(DMX_FRAME_ZLIB, 0xA1B2C3D4u, 40, z.data() + z.size() - 4);
        const FrameHead h = parse_exact(DMX_FRAME_ZLIB, z, z.size());
        CHECK(h.status == DMX_OK && h.head == 2 && h.want == 0xA1B2C3D4u, "zlib level %d: %d", level, h.status);
        CHECK(z[0] == 0x78 && (z[0] * 256 + z[1]) % 31 == 0, "zlib header");
        const int lv = (level < 0 || level > 3) ? 1 : level;
        CHECK((z[1] >> 6) == (lv <= 1 ? 0 : lv == 2 ? 1 : 3), "FLEVEL of level %d", level);
        if (level == 2) {
            CHECK(z[1] == 0x5E, "78 5e");
            truncations_and_mutations(z, "zlib");
        }
    }
    // documented statuses
    Bytes z = {0x78, 0x9C, 1, 2, 3, 4, 5, 6};
    CHECK(parse_exact(DMX_FRAME_ZLIB, z, 8).status == DMX_OK, "78 9c");
    CHECK(parse_exact(DMX_FRAME_ZLIB, z, 5).status == DMX_ERR_OVERREAD, "n < 6");
    CHECK(parse_exact(DMX_FRAME_ZLIB, z, 0).status == DMX_ERR_OVERREAD, "n == 0");
    z[1] = 0x9D;
    CHECK(parse_exact(DMX_FRAME_ZLIB, z, 8).status == DMX_ERR_DATA, "FCHECK");
    z[0] = 0x78;
    z[1] = 0xBB;  // FDICT set, FCHECK right
    CHECK((0x78 * 256 + 0xBB) % 31 == 0 && parse_exact(DMX_FRAME_ZLIB, z, 8).status == DMX_ERR_DATA, "FDICT");
    z[0] = 0x79;
    z[1] = 0x9C;
    CHECK(parse_exact(DMX_FRAME_ZLIB, z, 8).status == DMX_ERR_DATA, "CM");
    z[0] = 0x88;
    z[1] = 0x1C;  // CINFO 8, FCHECK right
    CHECK((0x88 * 256 + 0x1C) % 31 == 0 && parse_exact(DMX_FRAME_ZLIB, z, 8).status == DMX_ERR_DATA, "CINFO");
}

static void test_gzip() {
    const Bytes raw = payload(30, 3);
    for (uint32_t k = 0; k < 16; k++) {  // every combination of the optional fields
        const uint32_t flg = ((k & 1) ? 4 : 0) | ((k & 2) ? 8 : 0) | ((k & 4) ? 16 : 0) | ((k & 8) ? 2 : 0);
        size_t head = 0;
        const Bytes g = make_gzip(flg, Bytes{'a', 'b', 3, 0, 1, 2, 3}, raw, &head);
        const FrameHead h = parse_exact(DMX_FRAME_GZIP, g, g.size());
        CHECK(h.status == DMX_OK && h.head == head && h.want == 0x12345678u && h.isize == 0x9ABCDEF0u && h.member == 0,
              "gzip flg %u: status %d head %llu (expected %zu)", flg, h.status, (unsigned long long)h.head, head);
        CHECK(parse_exact(DMX_FRAME_BGZF, g, g.size()).status == DMX_ERR_DATA, "gzip without BC as BGZF");
        truncations_and_mutations(g, "gzip");
    }
    // the writer's header is the one dmx_deflate_gzip writes
    Bytes g(10);
    frame_write_head(DMX_FRAME_GZIP, 2, 0, g.data());
    CHECK(g == (Bytes{0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 255}), "gzip header, level 2");
    frame_write_head(DMX_FRAME_GZIP, 3, 0, g.data());
    CHECK(g[8] == 2, "XFL level 3");
    frame_write_head(DMX_FRAME_GZIP, 0, 0, g.data());
    CHECK(g[8] == 4, "XFL level 0");
    g.resize(18);
    frame_write_tail(DMX_FRAME_GZIP, 0xCAFEF00Du, 0x100000005ull, g.data() + 10);
    const FrameHead h = parse_exact(DMX_FRAME_GZIP, g, 18);
    CHECK(h.status == DMX_OK && h.head == 10 && h.want == 0xCAFEF00Du && h.isize == 5, "gzip write / parse");
    CHECK(parse_exact(DMX_FRAME_GZIP, g, 17).status == DMX_ERR_OVERREAD, "n < 18");
    // an unterminated FNAME: the name runs to the end
    Bytes u = {0x1F, 0x8B, 8, 8, 0, 0, 0, 0, 0, 255};
    for (int i = 0; i < 40; i++) u.push_back('x');
    CHECK(parse_exact(DMX_FRAME_GZIP, u, u.size()).status == DMX_ERR_OVERREAD, "unterminated FNAME");
    u[3] = 16;
    CHECK(parse_exact(DMX_FRAME_GZIP, u, u.size()).status == DMX_ERR_OVERREAD, "unterminated FCOMMENT");
    // a name that ends inside the last 8 bytes leaves no room for the trailer
    u[3] = 8;
    u[u.size() - 5] = 0;
    CHECK(parse_exact(DMX_FRAME_GZIP, u, u.size()).status == DMX_ERR_OVERREAD, "FNAME ends in the trailer");
    u[u.size() - 5] = 'x';
    u[u.size() - 9] = 0;
    CHECK(parse_exact(DMX_FRAME_GZIP, u, u.size()).status == DMX_OK, "FNAME ends just before the trailer");
    // XLEN running past the end
    Bytes x = make_gzip(4, Bytes{'a', 'b', 1, 0, 9}, raw);
    x[10] = 0xFF;
    x[11] = 0xFF;
    CHECK(parse_exact(DMX_FRAME_GZIP, x, x.size()).status == DMX_ERR_OVERREAD, "XLEN past the end");
    put16(x, 0);
    x[10] = (uint8_t)(x.size() - 12 - 8 + 1);  // one byte too many for the trailer
    x[11] = 0;
    CHECK(parse_exact(DMX_FRAME_GZIP, x, x.size()).status == DMX_ERR_OVERREAD, "XLEN into the trailer");
    x[10]--;
    CHECK(parse_exact(DMX_FRAME_GZIP, x, x.size()).status == DMX_OK, "XLEN up to the trailer");
    // a subfield whose SLEN runs past XLEN hides nothing behind it
    Bytes e = make_gzip(4, Bytes{'a', 'b', 0xFF, 0xFF, 66, 67, 2, 0, 9, 9}, raw);
    CHECK(parse_exact(DMX_FRAME_GZIP, e, e.size()).member == 0, "SLEN past XLEN");
}

static void test_bgzf() {
    const Bytes raw = payload(25, 9);
    Bytes b = make_bgzf(Bytes{}, raw, 77);
    FrameHead h = parse_exact(DMX_FRAME_BGZF, b, b.size());
    CHECK(h.status == DMX_OK && h.head == 18 && h.member == b.size() && h.isize == 77, "BGZF: %d", h.status);
    CHECK(parse_exact(DMX_FRAME_GZIP, b, b.size()).status == DMX_OK, "BGZF member as gzip");
    truncations_and_mutations(b, "bgzf");
    // the writer's header
    Bytes w(18);
    frame_write_head(DMX_FRAME_BGZF, 2, 0x1234 + 1, w.data());
    CHECK(w == (Bytes{0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 0x34, 0x12}), "BGZF header");
    // the BC subfield behind another subfield
    Bytes c = make_bgzf(Bytes{'X', 'Y', 3, 0, 1, 2, 3}, raw, 5);
    h = parse_exact(DMX_FRAME_BGZF, c, c.size());
    CHECK(h.status == DMX_OK && h.head == 12 + 7 + 6 && h.member == c.size(), "BC second: %d", h.status);
    truncations_and_mutations(c, "bgzf, BC second");
    // BSIZE + 1 != n
    for (int d : {-1, 1, -20}) {
        Bytes f = make_bgzf(Bytes{}, raw, 5, d);
        CHECK(parse_exact(DMX_FRAME_BGZF, f, f.size()).status == DMX_ERR_DATA, "BSIZE off by %d", d);
        CHECK(parse_exact(DMX_FRAME_GZIP, f, f.size()).status == DMX_OK, "... is still a gzip member");
    }
    // a BC subfield with another SLEN is not BSIZE
    Bytes s = make_gzip(4, Bytes{66, 67, 3, 0, 1, 2, 3}, raw);
    CHECK(parse_exact(DMX_FRAME_BGZF, s, s.size()).status == DMX_ERR_DATA, "BC with SLEN 3");
}

static int walk(const Bytes& file, size_t n, std::vector<BgzfMember>* out) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    if (n) std::memcpy(p.get(), file.data(), n);
    out->clear();
    for (uint64_t off = 0; off < n;) {
        BgzfMember m;
        const int rc = bgzf_next(p.get(), n, off, &m);
        if (rc != DMX_OK) return rc;
        out->push_back(m);
        off += m.size;
    }
    return DMX_OK;
}

static void test_chain() {
    const Bytes eof = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                       0x02, 0,    0x1b, 0,    0x03, 0, 0, 0, 0, 0,    0,    0, 0,    0};
    std::vector<Bytes> ms = {make_bgzf(Bytes{}, payload(100, 1), 1000), make_bgzf(Bytes{'Z', 'Z', 1, 0, 5}, payload(7, 2), 0),
                             make_bgzf(Bytes{}, payload(60000, 3), 65280), eof};
    Bytes file;
    std::vector<size_t> starts;
    for (const Bytes& m : ms) {
        starts.push_back(file.size());
        file.insert(file.end(), m.begin(), m.end());
    }
    starts.push_back(file.size());
    std::vector<BgzfMember> got;
    CHECK(walk(file, file.size(), &got) == DMX_OK && got.size() == 4, "chain: %zu members", got.size());
    const uint32_t isz[4] = {1000, 0, 65280, 0};
    for (size_t i = 0; i < got.size() && i < 4; i++)
        CHECK(got[i].off == starts[i] && got[i].size == ms[i].size() && got[i].isize == isz[i], "member %zu", i);
    CHECK(walk(file, 0, &got) == DMX_OK && got.empty(), "empty file");
    // a cut chain: every length that is no member boundary
    for (size_t n = 1; n < file.size(); n++) {
        size_t whole = 0;
        while (starts[whole + 1] <= n) whole++;
        const int rc = walk(file, n, &got);
        if (n == starts[whole]) CHECK(rc == DMX_OK && got.size() == whole, "cut at a boundary, n %zu: %d", n, rc);
        else CHECK(rc == DMX_ERR_OVERREAD, "cut chain, n %zu: %d", n, rc);
    }
    // a plain gzip member, a bad magic, a BSIZE smaller than the header
    Bytes plain = make_gzip(8, Bytes{}, payload(50, 4));
    CHECK(walk(plain, plain.size(), &got) == DMX_ERR_DATA, "no BC subfield");
    Bytes bad = file;
    bad[starts[1]] = 0x1E;
    CHECK(walk(bad, bad.size(), &got) == DMX_ERR_DATA, "bad magic in member 1");
    for (uint32_t tiny : {0u, 16u, 24u}) {  // member sizes 1, 17, 25 < head 18 + trailer 8
        Bytes sm = file;
        sm[16] = (uint8_t)tiny;
        sm[17] = 0;
        CHECK(walk(sm, sm.size(), &got) == DMX_ERR_DATA, "BSIZE %u smaller than the header", tiny);
    }
    Bytes ok = file;  // 26 = header + trailer: an empty raw part is the parser's business no more
    ok[16] = 25;
    ok[17] = 0;
    std::unique_ptr<uint8_t[]> p(new uint8_t[ok.size()]);
    std::memcpy(p.get(), ok.data(), ok.size());
    BgzfMember m;
    CHECK(bgzf_next(p.get(), ok.size(), 0, &m) == DMX_OK && m.size == 26, "BSIZE 25");
    CHECK(bgzf_next(p.get(), ok.size(), ok.size() + 5, &m) == DMX_ERR_OVERREAD, "offset past the end");
}

int main() {
    test_zlib();
    test_gzip();
    test_bgzf();
    test_chain();
    CHECK(frame_head_bytes(1) == 2 && frame_head_bytes(2) == 10 && frame_head_bytes(3) == 18 && frame_head_bytes(0) == 0 &&
              frame_head_bytes(4) == 0, "head bytes");
    CHECK(frame_tail_bytes(1) == 4 && frame_tail_bytes(2) == 8 && frame_tail_bytes(3) == 8 && frame_tail_bytes(9) == 0,
          "tail bytes");
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
