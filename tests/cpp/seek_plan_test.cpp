// seek_plan_test.cpp -- CPU test of deflate.hpp_amd/csrc/seek_plan.{h,cpp}: the host-side
// decisions of the seek index (dmx_inflate_index_device, dmx_inflate_range_device).
//
// Stand-alone (its own main, no HIP, no GPU); tests/test_seek_plan.py builds it plain and with
// AddressSanitizer + UBSan and runs both directly.  seek_select is compared with a brute-force
// model (each kept entry found by a scan from the start of the list) on random candidate lists;
// seek_range_plan with a per-byte model of which entry yields which output byte.  The arrays are
// exact-size heap copies, so a read past the sentinel is a sanitizer report.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../deflate.hpp_amd/csrc/seek_plan.cpp"

using namespace dmx;

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

// ---- seek_select ---------------------------------------------------------------------------

// the kept candidates' indices: after an entry at plain offset `last`, the next one is the first
// later candidate at or beyond last + spacing -- found by a scan over the whole list each time
static std::vector<size_t> select_model(const std::vector<SeekCand>& c, uint64_t spacing) {
    std::vector<size_t> kept;
    uint64_t last = 0;
    size_t from = 0;
    for (;;) {
        size_t next = c.size();
        for (size_t i = 0; i < c.size(); i++)
            if (i >= from && c[i].uoffset >= last + spacing) {
                next = i;
                break;
            }
        if (next == c.size()) return kept;
        kept.push_back(next);
        last = c[next].uoffset;
        from = next + 1;
    }
}

static void check_select(const std::vector<SeekCand>& c, uint64_t spacing, const char* what) {
    // exact-size copy: seek_select must not read past ncand
    std::unique_ptr<SeekCand[]> heap(new SeekCand[c.size() ? c.size() : 1]);
    for (size_t i = 0; i < c.size(); i++) heap[i] = c[i];
    const std::vector<dmx_seek_entry> e = seek_select(heap.get(), c.size(), spacing);
    const std::vector<size_t> kept = select_model(c, spacing);
    CHECK(!e.empty(), "%s: no entry 0", what);
    if (e.empty()) return;
    CHECK(e[0].bit == 0 && e[0].uoffset == 0 && e[0].window == 0 && e[0].flags == DMX_SEEK_NOWINDOW, "%s: entry 0", what);
    CHECK(e.size() == kept.size() + 1, "%s: %zu entries, model %zu", what, e.size(), kept.size() + 1);
    for (size_t k = 1; k < e.size() && k <= kept.size(); k++) {
        const SeekCand& m = c[kept[k - 1]];
        CHECK(e[k].bit == m.bit && e[k].uoffset == m.uoffset, "%s: entry %zu is not candidate %zu", what, k, kept[k - 1]);
        CHECK(e[k].flags == (m.nowindow ? DMX_SEEK_NOWINDOW : 0u), "%s: entry %zu flags", what, k);
        CHECK(e[k].window == (m.nowindow ? 0u : DMX_SEEK_WINDOW), "%s: entry %zu window", what, k);
        CHECK(e[k].uoffset - e[k - 1].uoffset >= spacing, "%s: entry %zu closer than the spacing", what, k);
        CHECK(e[k].window == 0 || e[k].uoffset >= DMX_SEEK_WINDOW, "%s: entry %zu has no full window", what, k);
    }
}

static void test_select() {
    std::mt19937_64 rng(12345);
    check_select({}, 32768, "no candidates");
    check_select({{0, 0, false}}, 32768, "bit 0 alone");
    check_select({{0, 0, true}, {80, 10, true}, {800, 32767, true}}, 32768, "all closer than the spacing");
    check_select({{0, 0, false}, {800, 32768, false}}, 32768, "exactly the spacing");
    check_select({{0, 0, false}, {800, 40000, false}, {900, 90000, false}}, 1u << 30, "spacing larger than the stream");
    // a zero-size tail: the last candidate sits at the stream's last plain byte + 1, twice
    check_select({{0, 0, false}, {100, 32768, false}, {200, 65536, false}, {210, 65536, false}}, 32768, "zero-size tail");
    check_select({{0, 0, false}, {5, 0, false}, {9, 0, false}, {100, 70000, false}}, 32768, "empty blocks at the start");
    for (int it = 0; it < 3000; it++) {
        const uint64_t spacing = it % 3 == 0 ? 32768 : 32768 + rng() % 300000;
        const size_t nc = rng() % 60;
        std::vector<SeekCand> c;
        uint64_t bit = 0, u = 0;
        const uint64_t step = it % 5 == 0 ? 1000 : it % 5 == 1 ? 2 * spacing : spacing / 2 + 1;
        for (size_t i = 0; i < nc; i++) {
            c.push_back({bit, u, (rng() & 7) == 0});
            bit += 3 + rng() % (8 * step + 1);
            u += rng() % 4 == 0 ? 0 : rng() % (step + 1);  // (runs of equal uoffset: empty blocks)
            if (rng() % 16 == 0) u += spacing;             // exactly the spacing further
        }
        check_select(c, spacing, "random");
    }
}

// ---- seek_range_plan ------------------------------------------------------------------------

struct Index {
    std::vector<dmx_seek_entry> e;  // count + 1
    uint64_t n;                     // stream bytes
    uint64_t count() const { return e.size() - 1; }
    uint64_t total() const { return e.back().uoffset; }
};

static int plan(const Index& ix, uint64_t n, uint64_t u, uint64_t len, std::vector<SeekSpan>* spans) {
    std::unique_ptr<dmx_seek_entry[]> heap(new dmx_seek_entry[ix.e.size()]);
    for (size_t i = 0; i < ix.e.size(); i++) heap[i] = ix.e[i];
    return seek_range_plan(heap.get(), ix.count(), n, u, len, spans);
}

// per byte: output byte j is plain byte u + j, which the last entry starting at or before it yields
static void check_range(const Index& ix, uint64_t u, uint64_t len, const char* what) {
    std::vector<SeekSpan> spans;
    const int rc = plan(ix, ix.n, u, len, &spans);
    CHECK(rc == DMX_OK, "%s: (%llu, %llu) rc %d", what, (unsigned long long)u, (unsigned long long)len, rc);
    if (rc != DMX_OK) return;
    if (len == 0) {
        CHECK(spans.empty(), "%s: spans for an empty range", what);
        return;
    }
    std::vector<int64_t> owner(len, -1);   // span that writes output byte j
    std::vector<uint64_t> plainof(len, 0);  // the plain byte it writes there
    for (size_t s = 0; s < spans.size(); s++) {
        const SeekSpan& sp = spans[s];
        CHECK(sp.slot < ix.count(), "%s: span %zu slot %llu", what, s, (unsigned long long)sp.slot);
        if (sp.slot >= ix.count()) return;
        const dmx_seek_entry& en = ix.e[sp.slot];
        CHECK(sp.bit == en.bit, "%s: span %zu bit", what, s);
        CHECK(sp.window == ((en.flags & DMX_SEEK_NOWINDOW) ? 0u : DMX_SEEK_WINDOW), "%s: span %zu window", what, s);
        CHECK(sp.skip < sp.limit, "%s: span %zu writes nothing", what, s);
        CHECK(s == 0 || sp.skip == 0, "%s: span %zu skips", what, s);
        CHECK(en.uoffset + sp.limit <= ix.e[sp.slot + 1].uoffset, "%s: span %zu runs into the next entry", what, s);
        CHECK(s == 0 || sp.slot == spans[s - 1].slot + 1, "%s: span %zu out of order", what, s);
        for (uint64_t p = sp.skip; p < sp.limit; p++) {
            const uint64_t j = sp.out_off + (p - sp.skip);
            CHECK(j < len, "%s: span %zu writes past the range", what, s);
            if (j >= len) return;
            CHECK(owner[j] < 0, "%s: output byte %llu written twice", what, (unsigned long long)j);
            owner[j] = (int64_t)sp.slot;
            plainof[j] = en.uoffset + p;
        }
    }
    for (uint64_t j = 0; j < len; j++) {
        uint64_t k = 0;
        for (uint64_t i = 0; i < ix.count(); i++)
            if (ix.e[i].uoffset <= u + j) k = i;
        CHECK(owner[j] == (int64_t)k, "%s: (%llu, %llu) byte %llu from entry %lld, model %llu", what, (unsigned long long)u,
              (unsigned long long)len, (unsigned long long)j, (long long)owner[j], (unsigned long long)k);
        CHECK(plainof[j] == u + j, "%s: byte %llu is plain byte %llu", what, (unsigned long long)j,
              (unsigned long long)plainof[j]);
        if (owner[j] != (int64_t)k || plainof[j] != u + j) return;
    }
}

static Index random_index(std::mt19937_64& rng, bool zero_tail) {
    Index ix;
    const uint64_t count = 1 + rng() % 9;
    uint64_t bit = 0, u = 0;
    for (uint64_t k = 0; k < count; k++) {
        const bool nw = k == 0 || (rng() & 3) == 0;
        ix.e.push_back(dmx_seek_entry{bit, u, nw ? 0u : DMX_SEEK_WINDOW, nw ? DMX_SEEK_NOWINDOW : 0u});
        bit += 1 + rng() % 500;
        u += 1 + rng() % 40;
    }
    if (zero_tail) u = ix.e.back().uoffset;  // the sentinel equals the last entry
    ix.n = (bit + 7) / 8 + rng() % 3;
    ix.e.push_back(dmx_seek_entry{8 * ((bit + 7) / 8), u, 0, 0});
    return ix;
}

static void expect_arg(const Index& ix, uint64_t n, uint64_t u, uint64_t len, const char* what) {
    std::vector<SeekSpan> spans;
    const int rc = plan(ix, n, u, len, &spans);
    CHECK(rc == DMX_ERR_ARG, "%s: rc %d", what, rc);
    CHECK(spans.empty(), "%s: spans with an error", what);
}

static void test_range() {
    std::mt19937_64 rng(777);
    for (int it = 0; it < 400; it++) {
        const Index ix = random_index(rng, it % 7 == 0);
        const uint64_t total = ix.total();
        check_range(ix, 0, total, "the whole file");
        check_range(ix, 0, 0, "len 0 at the start");
        check_range(ix, total, 0, "len 0 at the end");
        if (total) {
            check_range(ix, total - 1, 1, "the last byte");
            check_range(ix, 0, 1, "the first byte");
        }
        for (uint64_t k = 0; k < ix.count(); k++) {
            const uint64_t a = ix.e[k].uoffset, b = ix.e[k + 1].uoffset;
            if (b > a) check_range(ix, a, b - a, "exactly one span");
            if (b - a >= 3) check_range(ix, a + 1, b - a - 2, "inside one span");
            if (a > 0 && a + 1 <= total) check_range(ix, a - 1, 2, "one byte on either side of an edge");
            if (a + 1 < total) check_range(ix, a + 1, 1, "one byte behind an edge");
            if (a > 0) check_range(ix, a - 1, 1, "one byte before an edge");
            if (a < total) check_range(ix, a, 1, "the byte on an edge");
        }
        for (int r = 0; r < 8 && total; r++) {
            const uint64_t u = rng() % total;
            check_range(ix, u, 1 + rng() % (total - u), "random");
        }
        // every DMX_ERR_ARG case
        expect_arg(ix, ix.n, total, 1, "one byte past the end");
        expect_arg(ix, ix.n, 0, total + 1, "longer than the file");
        expect_arg(ix, ix.n, total + 1, 0, "an empty range past the end");
        expect_arg(ix, ix.n, 1, ~0ull, "uoffset + len wraps");
        // (the sentinel's bit is at least 8: every entry is at least one bit long)
        expect_arg(ix, ix.e.back().bit / 8 - 1, total ? total - 1 : 0, total ? 1 : 0, "n cut below the sentinel's byte");
        {
            Index bad = ix;
            bad.e.back().bit = 8 * ix.n + 1;
            expect_arg(bad, ix.n, 0, total ? 1 : 0, "the sentinel's bit one beyond 8 n");
        }
        if (ix.count() >= 2) {
            Index bad = ix;
            const uint64_t k = 1 + rng() % (ix.count() - 1);
            bad.e[k].uoffset = bad.e[k - 1].uoffset;  // equal: not strictly increasing
            expect_arg(bad, ix.n, 0, 1, "two entries at one uoffset");
            bad.e[k].uoffset = bad.e[k - 1].uoffset > 0 ? bad.e[k - 1].uoffset - 1 : 0;
            expect_arg(bad, ix.n, 0, 1, "entries going back");
        }
        if (ix.e[ix.count() - 1].uoffset > 0) {
            Index bad = ix;
            bad.e.back().uoffset = ix.e[ix.count() - 1].uoffset - 1;
            expect_arg(bad, ix.n, 0, 0, "the sentinel before the last entry");
        }
        {
            Index bad = ix;
            const uint64_t k = rng() % ix.count();
            bad.e[k].flags = 0;
            bad.e[k].window = (uint32_t)(rng() % 32768);  // no NOWINDOW and not 32768
            expect_arg(bad, ix.n, 0, total ? 1 : 0, "a short window");
            bad.e[k].window = 32769;
            expect_arg(bad, ix.n, 0, total ? 1 : 0, "a long window");
        }
    }
    // no entry at all, and a null index
    std::vector<SeekSpan> spans;
    const dmx_seek_entry lone{0, 0, 0, 0};
    CHECK(seek_range_plan(&lone, 0, 10, 0, 0, &spans) == DMX_ERR_ARG, "count 0");
    CHECK(seek_range_plan(nullptr, 1, 10, 0, 0, &spans) == DMX_ERR_ARG, "null entries");
    // a range before entry 0 (an index cut out of a larger one)
    Index cut;
    cut.e = {dmx_seek_entry{800, 100, 0, DMX_SEEK_NOWINDOW}, dmx_seek_entry{1600, 200, 0, 0}};
    cut.n = 200;
    expect_arg(cut, cut.n, 99, 2, "a range before entry 0");
    check_range(cut, 100, 100, "an index that starts later");
    // the select's entries feed the plan: windows and flags carry over
    const std::vector<SeekCand> c = {{0, 0, false}, {4000, 40000, false}, {9000, 90000, true}, {12000, 140000, false}};
    std::vector<dmx_seek_entry> e = seek_select(c.data(), c.size(), 32768);
    e.push_back(dmx_seek_entry{16000, 150000, 0, 0});
    Index ix{e, 2000};
    check_range(ix, 39999, 60000, "select then plan");
    check_range(ix, 0, 150000, "select then plan, whole");
}

int main() {
    test_select();
    test_range();
    std::printf("seek_plan_test: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
