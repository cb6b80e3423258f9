// huff_fit_test.cpp -- CPU test of deflate.hpp_amd/csrc/huff_fit.h: the arithmetic of the deflate's
// length-limited code build (init_len, fit_classes) and of its run-length header (plan_run), the
// functions deflate_kernels.hip compiles into the emission kernels.  Stand-alone (its own main, no
// HIP, no GPU).
//
//   (no argument)  every check; prints "<n> checks, <m> failed", the largest number of slack-fill
//                  passes seen, and the excess table (as --excess)
//   --lengths      stdin: one histogram per line, "<lit|dist|pre> f0 f1 ..."; stdout: its code
//                  lengths by the sequential restatement of the kernels' build, one line each
//   --plan         stdin: "<v> <r>" per line; stdout: "n18 last18 n17 r17 nlit n16 last16"
//   --excess       the cost of the build above package-merge at the same limit and above an
//                  unlimited Huffman code, worst and mean per alphabet, over the fuzz set and over
//                  level-1 histogram families of one 32 KiB segment
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../deflate.hpp_amd/csrc/huff_fit.h"

using namespace dmx;

static long g_checks = 0, g_failed = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        g_checks++;                                                           \
        if (!(c)) {                                                           \
            if (g_failed++ < 20) std::fprintf(stderr, "[FAIL] %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                                     \
    } while (0)

struct Alphabet {
    const char* name;
    int nsym, maxbits;
    bool by_freq;  // rank order: (frequency descending, symbol) -- the precode's 64-key sort;
                   // else (2 L0 + half, symbol) -- em_build_codes' ballots
};
static const Alphabet kAlpha[3] = {{"lit", 286, DF_LIT_MAXBITS, false},
                                   {"dist", 30, DF_DIST_MAXBITS, false},
                                   {"pre", 19, DF_PRE_MAXBITS, true}};

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
    g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }
static double rnd01() { return (double)(rnd() >> 11) / 9007199254740992.0; }

static int g_max_passes = 0;

// ---- the sequential restatement of the build: lengths from a histogram -----------------------
// em_build_codes (lit/len, distance) and wave_build_lengths64 (precode) in plain order: initial
// lengths, the rank order, fit_classes on the class sizes, lengths by rank ranges.
static std::vector<int> build_lengths(const Alphabet& A, const std::vector<uint32_t>& f) {
    const int n = A.nsym;
    std::vector<int> len(n, 0);
    uint32_t F = 0;
    int used = 0, hi = 0;
    for (int s = 0; s < n; s++) {
        F += f[s];
        if (f[s]) used++, hi = s + 1;
    }
    if (used <= 1) {  // two codes of length 1
        len[hi ? hi - 1 : 0] = 1;
        len[hi <= 1 ? 1 : 0] = 1;
        return len;
    }
    struct Key {
        uint64_t k;
        int s;
    };
    std::vector<Key> keys;
    uint32_t cnt[17] = {0};
    for (int s = 0; s < n; s++) {
        if (!f[s]) continue;
        const uint32_t L0 = init_len(f[s], F, A.maxbits);
        cnt[L0]++;
        const uint64_t k = A.by_freq ? ~(uint64_t)f[s] : 2 * L0 + init_half(f[s], F, L0);
        keys.push_back({k, s});
    }
    std::stable_sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.k < b.k; });
    int passes = 0;
    fit_classes(cnt, A.maxbits, &passes);
    g_max_passes = std::max(g_max_passes, passes);
    size_t r = 0;
    for (int L = 1; L <= 15; L++)
        for (uint32_t i = 0; i < cnt[L] && r < keys.size(); i++) len[keys[r++].s] = L;
    return len;
}

// ---- references ------------------------------------------------------------------------------
// package-merge (Larmore & Hirschberg): optimal code lengths of at most maxbits for the used
// symbols.  Level j's list is the leaves merged with the pairs of level j - 1's list; the first
// 2n - 2 items of the last list are the solution, and a leaf's length is the number of levels
// whose chosen prefix holds it.
static std::vector<int> package_merge(const std::vector<uint32_t>& f, int maxbits) {
    std::vector<std::pair<uint64_t, int>> leaf;
    for (size_t s = 0; s < f.size(); s++)
        if (f[s]) leaf.push_back({f[s], (int)s});
    std::sort(leaf.begin(), leaf.end());
    const size_t n = leaf.size();
    std::vector<int> len(f.size(), 0);
    if (n < 2) return len;
    struct Item {
        uint64_t w;
        bool is_leaf;
    };
    std::vector<std::vector<Item>> lists(maxbits);
    for (int j = 0; j < maxbits; j++) {
        std::vector<uint64_t> pk;
        if (j)
            for (size_t i = 0; i + 1 < lists[j - 1].size(); i += 2) pk.push_back(lists[j - 1][i].w + lists[j - 1][i + 1].w);
        size_t a = 0, b = 0;
        while (a < n || b < pk.size()) {
            if (b >= pk.size() || (a < n && leaf[a].first <= pk[b])) lists[j].push_back({leaf[a++].first, true});
            else lists[j].push_back({pk[b++], false});
        }
    }
    size_t need = 2 * n - 2;
    for (int j = maxbits - 1; j >= 0 && need; j--) {
        size_t leaves = 0, packs = 0;
        for (size_t i = 0; i < need && i < lists[j].size(); i++) (lists[j][i].is_leaf ? leaves : packs)++;
        for (size_t i = 0; i < leaves; i++) len[leaf[i].second]++;
        need = 2 * packs;
    }
    return len;
}

// cost of an unlimited Huffman code: the sum of its internal nodes' weights (two sorted queues)
static uint64_t huffman_cost(const std::vector<uint32_t>& f) {
    std::vector<uint64_t> a, b;
    for (uint32_t x : f)
        if (x) a.push_back(x);
    std::sort(a.begin(), a.end());
    if (a.size() < 2) return a.empty() ? 0 : a[0];
    size_t ia = 0, ib = 0;
    uint64_t cost = 0;
    auto pop = [&]() {
        if (ib >= b.size() || (ia < a.size() && a[ia] <= b[ib])) return a[ia++];
        return b[ib++];
    };
    while ((a.size() - ia) + (b.size() - ib) > 1) {
        const uint64_t s = pop() + pop();
        cost += s;
        b.push_back(s);
    }
    return cost;
}

static uint64_t cost_of(const std::vector<uint32_t>& f, const std::vector<int>& len) {
    uint64_t c = 0;
    for (size_t s = 0; s < f.size(); s++) c += (uint64_t)f[s] * len[s];
    return c;
}
static uint64_t kraft(const std::vector<int>& len, int maxbits) {
    uint64_t k = 0;
    for (int l : len)
        if (l) k += 1ull << (maxbits - l);
    return k;
}

// ---- fuzzed histograms -------------------------------------------------------------------------
// kind 0: frequencies 1..3; 1: log-uniform up to 2^16; 2: geometric (several ratios); 3: one
// dominant symbol; 4: uniform 1..2000.  `used` of the alphabet's symbols, at random places.
static std::vector<uint32_t> fuzz_hist(const Alphabet& A, int kind, int used) {
    std::vector<uint32_t> f(A.nsym, 0);
    std::vector<int> perm(A.nsym);
    for (int i = 0; i < A.nsym; i++) perm[i] = i;
    for (int i = A.nsym - 1; i > 0; i--) std::swap(perm[i], perm[rnd_below(i + 1)]);
    static const double ratios[] = {0.5, 0.7, 0.9, 0.97, 0.99};
    const double q = ratios[rnd_below(5)];
    double g = 60000.0;
    for (int i = 0; i < used; i++) {
        uint32_t v = 1;
        switch (kind) {
            case 0: v = 1 + rnd_below(3); break;
            case 1: v = (uint32_t)std::exp2(16.0 * rnd01()); break;
            case 2: v = (uint32_t)g, g *= q; break;
            case 3: v = i == 0 ? 20000 + rnd_below(40000) : 1 + rnd_below(4); break;
            default: v = 1 + rnd_below(2000); break;
        }
        f[perm[i]] = std::max(1u, std::min(v, 65536u));
    }
    return f;
}

// level-1 histograms of one 32 KiB segment: weights scaled to 32768 bytes (floor of 1 for a used
// value), plus the end-of-block symbol
static std::vector<uint32_t> scaled(const std::vector<double>& w, uint32_t total = 32768) {
    std::vector<uint32_t> f(286, 0);
    double sum = 0;
    for (double x : w) sum += x;
    uint64_t got = 0;
    size_t top = 0;
    for (size_t i = 0; i < w.size(); i++) {
        if (w[i] <= 0) continue;
        f[i] = std::max<uint32_t>(1, (uint32_t)(w[i] / sum * total));
        got += f[i];
        if (w[i] > w[top]) top = i;
    }
    if (got < total) f[top] += (uint32_t)(total - got);  // the rounding's rest goes to the largest
    f[256] = 1;
    return f;
}
struct Named {
    std::string name;
    std::vector<uint32_t> f;
};
static std::vector<Named> level1_families() {
    std::vector<Named> v;
    for (int m : {2, 3, 5, 17, 64, 128, 130, 200, 255})
        v.push_back({"uniform " + std::to_string(m), scaled(std::vector<double>(m, 1.0))});
    for (double q : {0.5, 0.7, 0.9, 0.97, 0.99}) {
        std::vector<double> w(256);
        double g = 1;
        for (auto& x : w) x = g, g *= q;
        char nm[32];
        std::snprintf(nm, sizeof nm, "geometric %.2f", q);
        v.push_back({nm, scaled(w)});
    }
    {
        std::vector<double> w(22);
        double a = 1, b = 1;
        for (auto& x : w) x = a, a = b, b += x;
        v.push_back({"fibonacci 22", scaled(w)});
    }
    for (double share : {0.90, 0.99}) {
        std::vector<uint32_t> f(286, 0);
        for (int i = 1; i < 256; i++) f[i] = 1;
        f[0] = 32768 - 255, f[256] = 1;
        if (share < 0.95) {  // 90 %: the rest spread over the other 255 values
            const uint32_t rest = (uint32_t)(32768 * (1 - share));
            for (int i = 1; i < 256; i++) f[i] = std::max(1u, rest / 255);
            f[0] = 32768;
            for (int i = 1; i < 256; i++) f[0] -= f[i];
        }
        v.push_back({share < 0.95 ? "one value at 90 %" : "one value at 99 %", f});
    }
    {
        std::vector<double> w(256, 1.0);
        for (int i = 0; i < 16; i++) w[i] = 400.0;
        v.push_back({"16 frequent + 240 rare", scaled(w)});
    }
    {
        std::vector<double> w(256);
        for (int i = 0; i < 256; i++) w[i] = 1.0 / (i + 1);
        v.push_back({"zipf", scaled(w)});
    }
    return v;
}

struct Excess {
    double worst_pm = 0, sum_pm = 0, worst_hf = 0, sum_hf = 0;
    long n = 0;
    std::string worst_name;
    void add(const Alphabet& A, const std::vector<uint32_t>& f, const std::string& name = "") {
        const uint64_t ours = cost_of(f, build_lengths(A, f));
        const uint64_t pm = cost_of(f, package_merge(f, A.maxbits)), hf = huffman_cost(f);
        if (!pm || !hf) return;
        const double e_pm = 100.0 * ((double)ours - (double)pm) / (double)pm;
        const double e_hf = 100.0 * ((double)ours - (double)hf) / (double)hf;
        if (e_pm > worst_pm) worst_pm = e_pm, worst_name = name;
        worst_hf = std::max(worst_hf, e_hf);
        sum_pm += e_pm, sum_hf += e_hf, n++;
    }
    void print(const char* set, const char* alpha, int maxbits) const {
        std::printf("excess %-8s %-4s limit %d: n %6ld  above package-merge worst %6.3f %% mean %6.3f %%  above huffman worst %6.3f %% mean %6.3f %%%s%s\n",
                    set, alpha, maxbits, n, worst_pm, n ? sum_pm / n : 0.0, worst_hf, n ? sum_hf / n : 0.0,
                    worst_name.empty() ? "" : "  worst: ", worst_name.c_str());
    }
};

static const int kFuzzPerKind = 1200;  // x 5 kinds = 6000 histograms per alphabet

static void excess_table() {
    g_rng = 0xD1B54A32D192ED03ull;
    for (const Alphabet& A : kAlpha) {
        Excess e;
        for (int kind = 0; kind < 5; kind++)
            for (int i = 0; i < kFuzzPerKind; i++) e.add(A, fuzz_hist(A, kind, 2 + (int)rnd_below(A.nsym - 1)));
        e.print("fuzz", A.name, A.maxbits);
    }
    Excess e;
    for (const Named& nm : level1_families()) {
        Excess one;
        one.add(kAlpha[0], nm.f);
        e.add(kAlpha[0], nm.f, nm.name);
        std::printf("excess level-1 %-24s above package-merge %6.3f %%  above huffman %6.3f %%\n", nm.name.c_str(),
                    one.worst_pm, one.worst_hf);
    }
    e.print("level-1", "lit", DF_LIT_MAXBITS);
}

// ---- checks ------------------------------------------------------------------------------------
static void check_fit(uint32_t (&cnt)[17], int maxbits, uint32_t used) {
    int passes = 0;
    fit_classes(cnt, maxbits, &passes);  // (returning at all: the repair loop ended)
    g_max_passes = std::max(g_max_passes, passes);
    uint64_t K = 0;
    uint32_t total = 0;
    for (int L = 1; L <= 15; L++) {
        total += cnt[L];
        if (L <= maxbits) K += (uint64_t)cnt[L] << (maxbits - L);
        else CHECK(cnt[L] == 0);  // no class beyond the limit
    }
    CHECK(cnt[0] == 0 && cnt[16] == 0);
    CHECK(K == (1ull << maxbits));  // complete: the slack fill ended on R == 0, neither on its
    CHECK(passes < 64);             // pass cap nor on a pass that changed nothing
    CHECK(total == used);
}

// every cnt[L..maxbits] with at most `left` more symbols; a vector of >= 2 symbols is checked
static void enum_classes(uint32_t (&v)[17], int L, int maxbits, uint32_t left, long* vectors) {
    if (L > maxbits) {
        if (8 - left < 2) return;
        uint32_t c[17];
        std::memcpy(c, v, sizeof c);
        check_fit(c, maxbits, 8 - left);
        ++*vectors;
        return;
    }
    for (uint32_t k = 0; k <= left; k++) {
        v[L] = k;
        enum_classes(v, L + 1, maxbits, left - k, vectors);
    }
    v[L] = 0;
}

static void test_fit_classes() {
    // class sizes of fuzzed histograms' initial lengths
    for (const Alphabet& A : kAlpha)
        for (int kind = 0; kind < 5; kind++)
            for (int i = 0; i < kFuzzPerKind; i++) {
                const int used = i < A.nsym - 1 ? 2 + i : 2 + (int)rnd_below(A.nsym - 1);  // every count 2..nsym
                const std::vector<uint32_t> f = fuzz_hist(A, kind, used);
                uint32_t F = 0, cnt[17] = {0};
                for (uint32_t x : f) F += x;
                for (uint32_t x : f)
                    if (x) cnt[init_len(x, F, A.maxbits)]++;
                check_fit(cnt, A.maxbits, (uint32_t)used);
            }
    // every class-size vector of 2..8 symbols
    for (int maxbits : {DF_LIT_MAXBITS, DF_DIST_MAXBITS, DF_PRE_MAXBITS}) {
        long vectors = 0;
        uint32_t v[17] = {0};
        enum_classes(v, 1, maxbits, 8, &vectors);
        CHECK(vectors > 1000);
    }
}

static uint32_t init_len_ref(uint32_t f, uint32_t F, int maxbits) {
    const long double x = log2l((long double)F / (long double)f);
    long double r = floorl(x + 0.5L);
    const long double fl = floorl(x);
    if (fabsl(x - (fl + 0.5L)) < 1e-12L) {
        // F / f at (or within rounding of) a half-power 2^(n + 1/2): the integer rule decides,
        // round up iff (f 2^(n+1))^2 <= 2 F^2
        const unsigned __int128 a = (unsigned __int128)f << ((int)fl + 1);
        r = fl + ((a * a <= (unsigned __int128)2 * F * F) ? 1 : 0);
    }
    return (uint32_t)std::max<long double>(1, std::min<long double>(maxbits, r));
}

static void test_init_len() {
    for (int maxbits : {DF_LIT_MAXBITS, DF_DIST_MAXBITS, DF_PRE_MAXBITS}) {
        CHECK(init_len(0, 100, maxbits) == 0);
        for (uint32_t F : {2u, 3u, 255u, 256u, 257u, 32769u, 65537u})
            for (uint32_t f = 1; f <= F; f++) CHECK(init_len(f, F, maxbits) == init_len_ref(f, F, maxbits));
        for (int i = 0; i < 200000; i++) {
            const uint32_t F = 1 + rnd_below(1u << 17), f = 1 + rnd_below(F);
            CHECK(init_len(f, F, maxbits) == init_len_ref(f, F, maxbits));
        }
    }
    // the half of a class: the less frequent half has f <= F / 2^L0
    for (uint32_t F : {255u, 256u, 32769u})
        for (uint32_t f = 1; f <= F; f++) {
            const uint32_t L0 = init_len(f, F, 15);
            CHECK(init_half(f, F, L0) == (((unsigned __int128)f << L0) <= F ? 1u : 0u));
        }
}

// the code-length symbols of a plan in writing order: (symbol, repeat count)
static std::vector<std::pair<int, int>> plan_symbols(uint32_t v, const RunPlan& p) {
    std::vector<std::pair<int, int>> s;
    if (v == 0) {
        for (uint32_t q = 0; q < p.n18; q++) s.push_back({18, (int)(q + 1 == p.n18 ? p.last18 : 138)});
        if (p.n17) s.push_back({17, (int)p.r17});
        for (uint32_t q = 0; q < p.nlit; q++) s.push_back({0, 1});
    } else {
        s.push_back({(int)v, 1});
        for (uint32_t q = 0; q < p.n16; q++) s.push_back({16, (int)(q + 1 == p.n16 ? p.last16 : 6)});
        for (uint32_t q = 1; q < p.nlit; q++) s.push_back({(int)v, 1});
    }
    return s;
}
// greedy RFC 1951 encoding of a run: the longest repeat first
static int greedy_symbols(uint32_t v, uint32_t r) {
    int n = 0;
    if (v == 0) {
        while (r >= 11) r -= std::min(r, 138u), n++;
        if (r >= 3) r = 0, n++;
        return n + (int)r;
    }
    r--, n++;
    while (r >= 3) r -= std::min(r, 6u), n++;
    return n + (int)r;
}

static void test_plan_run() {
    for (uint32_t v = 0; v <= 15; v++)
        for (uint32_t r = 1; r <= 316; r++) {
            const RunPlan p = plan_run(v, r);
            const auto s = plan_symbols(v, p);
            uint32_t total = 0;
            for (size_t i = 0; i < s.size(); i++) {
                total += (uint32_t)s[i].second;
                if (s[i].first == 18) CHECK(s[i].second >= 11 && s[i].second <= 138);
                else if (s[i].first == 17) CHECK(s[i].second >= 3 && s[i].second <= 10);
                else if (s[i].first == 16) CHECK(s[i].second >= 3 && s[i].second <= 6 && v != 0 && i > 0);
                else CHECK(s[i].first == (int)v && s[i].second == 1);
            }
            CHECK(total == r);
            CHECK(s[0].first != 16);
            if (v) CHECK(s[0].first == (int)v && p.n18 == 0 && p.n17 == 0);
            else CHECK(p.n16 == 0);
            CHECK((int)s.size() <= greedy_symbols(v, r));
            CHECK(s.size() == p.n18 + p.n17 + p.n16 + p.nlit);
        }
}

static void test_build() {
    // the restated build on fuzzed histograms: complete, inside the limit, exactly the used
    // symbols coded (or the two length-1 codes), never cheaper than package-merge
    for (const Alphabet& A : kAlpha) {
        for (int kind = 0; kind < 5; kind++)
            for (int i = 0; i < 400; i++) {
                const std::vector<uint32_t> f = fuzz_hist(A, kind, 2 + (int)rnd_below(A.nsym - 1));
                const std::vector<int> len = build_lengths(A, f), pm = package_merge(f, A.maxbits);
                CHECK(kraft(len, A.maxbits) == 1ull << A.maxbits);
                CHECK(kraft(pm, A.maxbits) == 1ull << A.maxbits);
                bool ok = true;
                for (int s = 0; s < A.nsym; s++) ok = ok && (len[s] != 0) == (f[s] != 0) && len[s] <= A.maxbits && pm[s] <= A.maxbits;
                CHECK(ok);
                CHECK(cost_of(f, len) >= cost_of(f, pm));
                CHECK(cost_of(f, pm) >= huffman_cost(f));
            }
        // zero and one used symbol
        std::vector<uint32_t> f(A.nsym, 0);
        std::vector<int> len = build_lengths(A, f);
        CHECK(len[0] == 1 && len[1] == 1 && kraft(len, A.maxbits) == 1ull << A.maxbits);
        for (int s = 0; s < A.nsym; s++) {
            std::fill(f.begin(), f.end(), 0u);
            f[s] = 7;
            len = build_lengths(A, f);
            CHECK(len[s] == 1 && len[s == 0 ? 1 : 0] == 1 && kraft(len, A.maxbits) == 1ull << A.maxbits);
        }
    }
    // package-merge against an unlimited Huffman code where the limit cannot bind (15 bits, <= 12
    // symbols ... 2^12 total): the costs agree
    for (int i = 0; i < 2000; i++) {
        std::vector<uint32_t> f(12, 0);
        for (auto& x : f) x = rnd_below(4) ? 1 + rnd_below(300) : 0;
        int used = 0;
        for (uint32_t x : f) used += x != 0;
        if (used < 2) continue;
        CHECK(cost_of(f, package_merge(f, 15)) == huffman_cost(f));
    }
}

static int mode_lengths() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string a;
        if (!(is >> a)) continue;
        const Alphabet* A = nullptr;
        for (const Alphabet& x : kAlpha)
            if (a == x.name) A = &x;
        if (!A) return 2;
        std::vector<uint32_t> f(A->nsym, 0);
        for (int s = 0; s < A->nsym && (is >> f[s]); s++) {}
        const std::vector<int> len = build_lengths(*A, f);
        for (int s = 0; s < A->nsym; s++) std::printf(s ? " %d" : "%d", len[s]);
        std::printf("\n");
    }
    return 0;
}

static int mode_plan() {
    uint32_t v, r;
    while (std::cin >> v >> r) {
        const RunPlan p = plan_run(v, r);
        std::printf("%u %u %u %u %u %u %u\n", p.n18, p.last18, p.n17, p.r17, p.nlit, p.n16, p.last16);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--lengths")) return mode_lengths();
    if (argc > 1 && !std::strcmp(argv[1], "--plan")) return mode_plan();
    if (argc > 1 && !std::strcmp(argv[1], "--excess")) {
        excess_table();
        return 0;
    }
    test_init_len();
    test_fit_classes();
    test_plan_run();
    test_build();
    excess_table();
    std::printf("huff_fit_test: slack-fill passes, maximum %d (cap 64)\n", g_max_passes);
    std::printf("huff_fit_test: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
