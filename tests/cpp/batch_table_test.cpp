// batch_table_test.cpp -- CPU test of deflate.hpp_amd/csrc/batch_table.h: the steps with which
// the kernels of batch_table.hip build a batch's tables from device-resident descriptor arrays
// (dmx_deflate_batch_async, dmx_inflate_batch_async).
//
// Stand-alone (no HIP, no GPU); tests/test_batch_table.py builds it plain and with
// AddressSanitizer + UBSan and runs both directly.  The steps (count, scan, fill, close) are run
// serially over all "threads" on exact-size heap arrays, so an access outside the table, the
// first-segment list or the flags is a sanitizer report; the table, bfirst, the segment count and
// the flags are compared with a plain serial loop -- the one of deflate_batch_locked, with the
// asynchronous call's two rules (a buffer above max_n has no segments; the table ends before the
// first buffer that does not fit its capacity).  The inflate side's class sort is run the same way.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../deflate.hpp_amd/csrc/batch_table.h"

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

typedef unsigned long long ull;

struct Built {
    std::vector<DeflateBatchSeg> tab;  // the entries below the segment count
    std::vector<uint64_t> first;       // count + 1
    std::vector<uint8_t> flag;         // count
    uint64_t nseg = 0;
};

static bool same_seg(const DeflateBatchSeg& a, const DeflateBatchSeg& b) {
    return a.src == b.src && a.tail == b.tail && a.nb == b.nb && a.buf == b.buf && a.dict == b.dict && a.dlen == b.dlen;
}

// The serial loop: deflate_batch_locked's, with the two rules of the asynchronous call.
static Built serial_table(const uint8_t* const* d_in, const uint64_t* n, size_t count, uint64_t max_n, uint64_t cap,
                          uint32_t seg, uint32_t du, const uint8_t* dtail) {
    Built r;
    r.first.resize(count + 1);
    r.flag.assign(count, 0);
    const size_t seg0 = seg - du;  // bytes of a buffer's first segment
    uint64_t s = 0;
    bool clipped = false;
    for (size_t i = 0; i < count; i++) {
        r.first[i] = s;
        if (n[i] > max_n) {
            r.flag[i] = 1;
            continue;
        }
        std::vector<DeflateBatchSeg> mine;
        for (size_t o = 0, len = seg0; o < n[i]; o += len, len = seg) {
            const size_t rest = n[i] - o;
            DeflateBatchSeg e;
            e.src = d_in[i] + o;
            e.tail = rest;
            e.nb = (uint32_t)std::min<size_t>(len, rest);
            e.buf = (uint32_t)i | (rest <= len ? DF_BATCH_LAST : 0u);
            e.dict = o == 0 ? dtail : nullptr;
            e.dlen = o == 0 ? du : 0u;
            mine.push_back(e);
        }
        if (clipped || s + mine.size() > cap) {
            clipped = true;
            r.flag[i] = 1;
        } else {
            r.tab.insert(r.tab.end(), mine.begin(), mine.end());
        }
        s += mine.size();
        if (!clipped) r.nseg = s;
    }
    r.first[count] = s;
    return r;
}

// The kernels' steps, every "thread" in turn, on arrays of exactly the sizes the host allocates.
static Built parallel_table(const uint8_t* const* d_in, const uint64_t* n, size_t count, uint64_t max_n, uint64_t cap,
                            uint32_t seg, uint32_t du, const uint8_t* dtail, const char* what) {
    std::unique_ptr<uint32_t[]> counts(new uint32_t[count]);
    std::unique_ptr<uint8_t[]> flag(new uint8_t[count]);
    std::unique_ptr<uint64_t[]> first(new uint64_t[count + 1]);
    std::unique_ptr<DeflateBatchSeg[]> tab(new DeflateBatchSeg[cap]);
    std::unique_ptr<uint8_t[]> written(new uint8_t[cap]);
    std::memset(written.get(), 0, cap);
    for (size_t i = 0; i < count; i++) counts[i] = bt_count(n[i], max_n, seg, du, &flag[i]);  // k_bt_count
    uint64_t run = 0;  // (stands for launch_scan_u32: the exclusive prefix sum and its total)
    for (size_t i = 0; i < count; i++) {
        first[i] = run;
        run += counts[i];
    }
    first[count] = run;
    const uint64_t threads = std::max<uint64_t>(cap, count);  // k_bt_fill, last thread first
    uint64_t nseg = ~0ull;
    int writers = 0;
    for (uint64_t t = threads; t-- > 0;) {
        if (t < cap) {
            DeflateBatchSeg e;
            if (bt_fill(t, first.get(), count, cap, d_in, n, seg, du, dtail, &e)) {
                tab[t] = e;
                written[t] = 1;
            }
        }
        if (t < count) {
            uint64_t ns = 0;
            if (bt_close(t, first.get(), count, cap, flag.get(), &ns)) {
                nseg = ns;
                writers++;
            }
        }
    }
    CHECK(writers == 1, "%s: %d threads wrote the segment count", what, writers);
    Built r;
    r.nseg = nseg;
    CHECK(nseg <= cap, "%s: segment count %llu above the capacity %llu", what, (ull)nseg, (ull)cap);
    for (uint64_t s = 0; s < cap; s++)
        CHECK((written[s] != 0) == (s < nseg), "%s: slot %llu %s (count %llu)", what, (ull)s,
              written[s] ? "written" : "not written", (ull)nseg);
    for (uint64_t s = 0; s < nseg && s < cap; s++) r.tab.push_back(tab[s]);
    r.first.assign(first.get(), first.get() + count + 1);
    r.flag.assign(flag.get(), flag.get() + count);
    return r;
}

static void compare(const std::vector<uint64_t>& sizes, uint64_t max_n, uint64_t cap, uint32_t seg, uint32_t du,
                    const char* what) {
    const size_t count = sizes.size();
    uint64_t sum = 0;
    for (uint64_t v : sizes) sum += v;
    std::unique_ptr<uint8_t[]> arena(new uint8_t[sum + 1]);  // the pointers are only compared
    std::unique_ptr<const uint8_t*[]> d_in(new const uint8_t*[count]);
    std::unique_ptr<uint64_t[]> n(new uint64_t[count]);
    uint64_t pos = 0;
    for (size_t i = 0; i < count; i++) {
        d_in[i] = arena.get() + pos;
        n[i] = sizes[i];
        pos += sizes[i];
    }
    static const uint8_t dict[16384] = {0};
    const uint8_t* const dtail = du ? dict + (sizeof(dict) - du) : nullptr;
    const Built a = serial_table(d_in.get(), n.get(), count, max_n, cap, seg, du, dtail);
    const Built b = parallel_table(d_in.get(), n.get(), count, max_n, cap, seg, du, dtail, what);
    CHECK(a.nseg == b.nseg, "%s: segment count %llu, serial %llu", what, (ull)b.nseg, (ull)a.nseg);
    CHECK(a.first == b.first, "%s: bfirst differs", what);
    CHECK(a.flag == b.flag, "%s: flags differ", what);
    CHECK(a.tab.size() == b.tab.size(), "%s: %zu entries, serial %zu", what, b.tab.size(), a.tab.size());
    for (size_t s = 0; s < a.tab.size() && s < b.tab.size(); s++)
        CHECK(same_seg(a.tab[s], b.tab[s]), "%s: entry %zu differs (buffer %u)", what, s, a.tab[s].buf & ~DF_BATCH_LAST);
}

// every capacity worth a look for one batch: the formula's for max_total = the sum, one segment
// short of what the batch needs, 0 (unknown); and the table cut at every point of a small batch
static void all_capacities(const std::vector<uint64_t>& sizes, uint64_t max_n, uint32_t seg, uint32_t du,
                           const char* what, bool every_cut) {
    const size_t count = sizes.size();
    uint64_t sum = 0, need = 0;
    for (uint64_t v : sizes) {
        sum += v;
        if (v <= max_n) need += bt_segments(v, seg, du);
    }
    char name[160];
    const uint64_t exact = std::max<uint64_t>(1, bt_capacity(count, max_n, sum, seg, du));
    std::snprintf(name, sizeof name, "%s S=%u Du=%u max_total=sum", what, seg, du);
    compare(sizes, max_n, exact, seg, du, name);
    std::snprintf(name, sizeof name, "%s S=%u Du=%u max_total=0", what, seg, du);
    compare(sizes, max_n, std::max<uint64_t>(1, bt_capacity(count, max_n, 0, seg, du)), seg, du, name);
    if (need > 1) {
        std::snprintf(name, sizeof name, "%s S=%u Du=%u one segment short", what, seg, du);
        compare(sizes, max_n, need - 1, seg, du, name);
    }
    std::snprintf(name, sizeof name, "%s S=%u Du=%u capacity = need", what, seg, du);
    compare(sizes, max_n, std::max<uint64_t>(1, need), seg, du, name);
    if (every_cut)
        for (uint64_t cap = 1; cap < need; cap++) {
            std::snprintf(name, sizeof name, "%s S=%u Du=%u capacity %llu", what, seg, du, (ull)cap);
            compare(sizes, max_n, cap, seg, du, name);
        }
}

static void test_deflate_tables() {
    std::mt19937_64 rng(20250612);
    for (uint32_t seg : {16384u, 32768u})
        for (uint32_t du : {0u, 1u, 16384u}) {
            const int64_t S = seg, D = du;
            std::vector<uint64_t> edges;
            for (int64_t v : {(int64_t)0, (int64_t)1, S - D - 1, S - D, S - D + 1, 2 * S - D, 2 * S - D + 1})
                if (v >= 0) edges.push_back((uint64_t)v);
            const uint64_t big = 1u << 20;
            // the bt_segments rule against the host loop's count, around every edge
            for (uint64_t v : edges)
                for (int64_t d = -2; d <= 2; d++) {
                    if ((int64_t)v + d < 0) continue;
                    const uint64_t nn = v + d;
                    uint64_t loop = 0;
                    for (size_t o = 0, len = seg - du; o < nn; o += len, len = seg) loop++;
                    CHECK(bt_segments(nn, seg, du) == loop, "S=%u Du=%u n=%llu: %llu segments, the loop %llu", seg, du,
                          (ull)nn, (ull)bt_segments(nn, seg, du), (ull)loop);
                }
            // each edge size alone and all of them in one batch
            for (uint64_t v : edges) all_capacities({v}, big, seg, du, "single", true);
            all_capacities(edges, big, seg, du, "edges", true);
            // runs of empty buffers: bfirst entries that repeat, at the start, inside and at the end
            all_capacities({0, 0, 0, 5, 0, 0, (uint64_t)S + 7, 0, 0, 0, 3 * (uint64_t)S, 0, 0}, big, seg, du, "empties", true);
            all_capacities({0, 0, 0, 0}, big, seg, du, "all empty", true);
            // n > max_n in the first, a middle and the last buffer (and in all of them)
            const uint64_t mx = 2 * (uint64_t)S;
            all_capacities({mx + 1, 100, mx, 7}, mx, seg, du, "over first", true);
            all_capacities({100, mx, mx + 1, 0, 7}, mx, seg, du, "over middle", true);
            all_capacities({100, mx, 0, 7, mx + 1}, mx, seg, du, "over last", true);
            all_capacities({mx + 1, mx + 2, mx + 3}, mx, seg, du, "over all", true);
            // 1000 random batches of 1-40 buffers
            for (int it = 0; it < 1000; it++) {
                const size_t count = 1 + rng() % 40;
                std::vector<uint64_t> sizes(count);
                for (auto& v : sizes) {
                    const uint64_t r = rng() % 10;
                    v = r < 3 ? edges[rng() % edges.size()] : r < 5 ? 0 : rng() % (3 * (uint64_t)S + 2);
                }
                const uint64_t max_n = (rng() & 1) ? big : sizes[rng() % count];
                all_capacities(sizes, max_n, seg, du, "random", false);
                uint64_t need = 0;
                for (uint64_t v : sizes)
                    if (v <= max_n) need += bt_segments(v, seg, du);
                if (need > 1) compare(sizes, max_n, 1 + rng() % need, seg, du, "random, random capacity");
            }
        }
    // the capacity formula: min(count * K, ceil(max_total / S) + count), saturating
    CHECK(bt_capacity(14, 100000, 0, 32768, 0) == 56, "%llu", (ull)bt_capacity(14, 100000, 0, 32768, 0));
    CHECK(bt_capacity(14, 100000, 32768 * 7, 32768, 0) == 21, "%llu", (ull)bt_capacity(14, 100000, 32768 * 7, 32768, 0));
    CHECK(bt_capacity(14, 100000, 32768 * 7 + 1, 32768, 0) == 22, "%llu", (ull)bt_capacity(14, 100000, 32768 * 7 + 1, 32768, 0));
    CHECK(bt_capacity(16384, 4096, 0, 32768, 0) == 16384, "%llu", (ull)bt_capacity(16384, 4096, 0, 32768, 0));
    // (count * max_n saturates at 2^64 - 1: ceil of that / S, + count; count * K saturates above it)
    CHECK(bt_capacity(1u << 30, ~0ull, 0, 16384, 0) == ~0ull / 16384 + 1 + (1u << 30), "saturation");
    CHECK(bt_capacity(~0ull, ~0ull, ~0ull, 16384, 0) == ~0ull, "saturation of the sum");
    CHECK(bt_capacity(3, ~0ull, 16384, 16384, 0) == 4, "%llu", (ull)bt_capacity(3, ~0ull, 16384, 16384, 0));
}

// ---- inflate: the class sort -----------------------------------------------------------------
static void class_sort(const std::vector<uint64_t>& n, const std::vector<uint8_t>& has_out, uint64_t max_n,
                       uint64_t route_bytes, const char* what) {
    const size_t count = n.size();
    std::unique_ptr<uint32_t[]> hist(new uint32_t[kBatchClasses]()), cursor(new uint32_t[kBatchClasses]()),
        start(new uint32_t[kBatchClasses]);
    std::unique_ptr<uint32_t[]> order(new uint32_t[count]);
    std::vector<uint32_t> mark(count);
    for (size_t i = 0; i < count; i++) {  // k_bt_desc
        mark[i] = bt_mark(n[i], max_n, route_bytes != 0, route_bytes, has_out[i] != 0);
        if (mark[i] == BT_KEEP) hist[bt_class(n[i])]++;
    }
    const uint32_t kept = bt_class_starts(hist.get(), start.get());
    CHECK(kept <= count, "%s: %u kept of %zu", what, kept, count);
    for (size_t i = count; i-- > 0;) {  // k_bt_order, last thread first: the order inside a class is arbitrary
        if (mark[i] != BT_KEEP) continue;
        const uint32_t c = bt_class(n[i]);
        const uint32_t p = start[c] + cursor[c]++;
        CHECK(p < kept, "%s: position %u of %u", what, p, kept);
        if (p < count) order[p] = (uint32_t)i;
    }
    std::vector<uint8_t> seen(count, 0);
    for (uint32_t k = 0; k < kept && k < count; k++) {
        const uint32_t i = order[k];
        CHECK(i < count && !seen[i] && mark[i] == BT_KEEP, "%s: position %u holds %u", what, k, i);
        if (i < count) seen[i] = 1;
        if (k && i < count && order[k - 1] < count)
            CHECK(bt_class(n[order[k - 1]]) >= bt_class(n[i]), "%s: class rises at position %u", what, k);
    }
    for (size_t i = 0; i < count; i++) {
        const bool want = n[i] <= max_n && !(route_bytes && n[i] > route_bytes && has_out[i]);
        CHECK((seen[i] != 0) == want, "%s: stream %zu (n = %llu) %s", what, i, (ull)n[i], seen[i] ? "listed" : "missing");
    }
}

static void test_class_sort() {
    for (uint32_t k = 0; k < 64; k++) {
        CHECK(bt_class(1ull << k) == k, "2^%u", k);
        if (k) CHECK(bt_class((1ull << k) - 1) == k - 1, "2^%u - 1", k);
        CHECK(bt_class((1ull << k) | ((1ull << k) >> 1)) == k, "1.5 * 2^%u", k);
    }
    CHECK(bt_class(0) == 0 && bt_class(~0ull) == 63, "ends");
    CHECK(bt_mark(5, 4, false, 0, true) == BT_OVER && bt_mark(4, 4, false, 0, true) == BT_KEEP, "max_n");
    CHECK(bt_mark(9, 100, true, 8, true) == BT_DEFER && bt_mark(8, 100, true, 8, true) == BT_KEEP, "threshold");
    CHECK(bt_mark(9, 100, true, 8, false) == BT_KEEP && bt_mark(9, 100, false, 8, true) == BT_KEEP, "no output / no routing");
    CHECK(bt_mark(200, 100, true, 8, true) == BT_OVER, "over max_n before deferred");
    std::mt19937_64 rng(777);
    const uint64_t route = 1u << 20;
    class_sort({0}, {1}, 10, route, "one empty");
    class_sort({11}, {1}, 10, route, "one over");
    class_sort({route + 1, route, route + 1}, {1, 1, 0}, ~0ull, route, "threshold");
    for (int it = 0; it < 1000; it++) {
        const size_t count = 1 + rng() % 40;
        std::vector<uint64_t> n(count);
        std::vector<uint8_t> has(count);
        for (size_t i = 0; i < count; i++) {
            n[i] = (rng() % 4 == 0) ? rng() % 8 : (rng() >> (rng() % 64));
            has[i] = rng() % 8 != 0;
        }
        const uint64_t max_n = (rng() & 1) ? ~0ull : n[rng() % count];
        class_sort(n, has, max_n, (rng() & 1) ? route : 0, "random");
    }
}

int main() {
    test_deflate_tables();
    test_class_sort();
    std::printf("batch_table_test: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
