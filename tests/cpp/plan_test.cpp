// tests/cpp/plan_test.cpp -- the inflate planners (deflate.hpp_amd/csrc/inflate_plan.cpp) on
// records built by hand: no GPU, no HIP; links inflate_plan.cpp alone.  Every case asserts exact
// outputs.  Exit code 0 = all checks passed (tests/test_inflate_plan.py runs it plain and under
// ASan + UBSan).
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../deflate.hpp_amd/csrc/inflate_plan.h"
#include "../../include/dmx.h"

using namespace dmx;

static int fails = 0, checks = 0;
#define CHECK(c)                                                             \
    do {                                                                     \
        checks++;                                                            \
        if (!(c)) {                                                          \
            std::fprintf(stderr, "[FAIL] %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                                         \
        }                                                                    \
    } while (0)

template <class T>
static bool same(const std::vector<T>& v, std::initializer_list<T> want) {
    return v == std::vector<T>(want);
}
typedef std::initializer_list<uint64_t> U64;
typedef std::initializer_list<uint32_t> U32;

// ---- path 4: the chain walk over SegRecords ----

static SegRecord rec(uint64_t end_byte, uint32_t size, uint32_t flags) { return SegRecord{end_byte, 0, size, flags}; }

static void test_seg_chain() {
    {  // three uniform segments
        const uint64_t cands[] = {0, 100, 200};
        const SegRecord r[] = {rec(100, 32768, 0), rec(200, 32768, 0), rec(300, 1000, SEGF_FINAL)};
        const SegChain c = seg_chain_walk(r, cands, 3);
        CHECK(c.ok && same(c.chain, U64{0, 1, 2}) && same(c.offsets, U64{0, 32768, 65536}));
        CHECK(same(c.sizes, U32{32768, 32768, 1000}) && c.total == 66536);
    }
    {  // a false candidate in the middle: segment 0 ends at candidate 2
        const uint64_t cands[] = {0, 50, 100, 200};
        const SegRecord r[] = {rec(100, 1000, 0), rec(7, 9, SEGF_ERR_DATA), rec(200, 500, 0), rec(260, 7, SEGF_FINAL)};
        const SegChain c = seg_chain_walk(r, cands, 4);
        CHECK(c.ok && same(c.chain, U64{0, 2, 3}) && same(c.offsets, U64{0, 1000, 1500}));
        CHECK(same(c.sizes, U32{1000, 500, 7}) && c.total == 1507);
    }
    {  // an end that is no candidate
        const uint64_t cands[] = {0, 100, 200};
        const SegRecord r[] = {rec(77, 10, 0), rec(200, 10, 0), rec(300, 10, SEGF_FINAL)};
        const SegChain c = seg_chain_walk(r, cands, 3);
        CHECK(!c.ok && same(c.chain, U64{0}));
    }
    {  // an error flag on a chain member (also together with SEGF_FINAL)
        const uint64_t cands[] = {0, 100, 200};
        SegRecord r[] = {rec(100, 10, 0), rec(200, 10, SEGF_OVERFLOW), rec(300, 10, SEGF_FINAL)};
        CHECK(!seg_chain_walk(r, cands, 3).ok);
        r[1].flags = 0, r[2].flags = SEGF_FINAL | SEGF_EXOTIC;
        CHECK(!seg_chain_walk(r, cands, 3).ok);
    }
    {  // no final segment: the last end is past every candidate
        const uint64_t cands[] = {0, 100, 200};
        const SegRecord r[] = {rec(100, 10, 0), rec(200, 10, 0), rec(300, 10, 0)};
        const SegChain c = seg_chain_walk(r, cands, 3);
        CHECK(!c.ok && same(c.chain, U64{0, 1, 2}));
    }
    {  // a single final candidate
        const uint64_t cands[] = {0};
        const SegRecord r[] = {rec(9, 5, SEGF_FINAL)};
        const SegChain c = seg_chain_walk(r, cands, 1);
        CHECK(c.ok && same(c.chain, U64{0}) && same(c.offsets, U64{0}) && same(c.sizes, U32{5}) && c.total == 5);
    }
}

// ---- the pass plan ----

struct P {
    uint32_t mode, slot;
};
static bool passes(const PassPlan& p, std::initializer_list<P> want) {
    if (p.np != (int)want.size()) return false;
    int i = 0;
    for (const P& w : want) {
        if (p.pass[i][0] != w.mode || p.pass[i][1] != w.slot) return false;
        i++;
    }
    return true;
}

static void test_pass_plan() {
    const uint32_t S = 32768, H = 16384, B = 65536;
    const int ncu = 256;
    {  // the default plan at 32 KiB with the heavy route
        PassPlan p = inflate_pass_plan(S, 32ull * S, 32, -1, 0, ncu, true, true, true);
        CHECK(passes(p, {{4, S}, {6, S}, {3, S}, {2, S}, {3, S}, {2, H}, {3, H}, {1, 0}}));
        CHECK(p.heavy == 256 && p.heavy_limit == 0xFFFFFFFFu);  // ncand <= ncu
        p = inflate_pass_plan(S, 256ull * S, 256, -1, 0, ncu, true, true, true);
        CHECK(p.heavy == 256 && p.heavy_limit == 0xFFFFFFFFu);
        p = inflate_pass_plan(S, 257ull * S, 257, -1, 0, ncu, true, true, true);
        CHECK(p.heavy == 2048 && p.heavy_limit == 0xFFFFFFFFu);
        p = inflate_pass_plan(S, 2048ull * S, 2048, -1, 0, ncu, true, true, true);
        CHECK(p.heavy == 2048 && p.heavy_limit == 0xFFFFFFFFu);
        p = inflate_pass_plan(S, 2049ull * S, 2049, -1, 0, ncu, true, true, true);
        CHECK(p.heavy == 2048 && p.heavy_limit == 32u * 256u);
        CHECK(passes(p, {{4, S}, {6, S}, {3, S}, {2, S}, {3, S}, {2, H}, {3, H}, {1, 0}}));
        // dev_heavy_bytes set: that value, also for few candidates
        p = inflate_pass_plan(S, 32ull * S, 32, -1, 512, ncu, true, true, true);
        CHECK(p.heavy == 512 && p.heavy_limit == 0xFFFFFFFFu);
    }
    {  // ... and without it (the heavy list did not fit)
        const PassPlan p = inflate_pass_plan(S, 32ull * S, 32, -1, 0, ncu, true, false, true);
        CHECK(passes(p, {{4, S}, {3, S}, {2, S}, {3, S}, {2, H}, {3, H}, {1, 0}}));
        CHECK(p.heavy == 0 && p.heavy_limit == 0);
    }
    {  // 16 KiB segments: the workgroup decoder's other slot is 32 KiB
        const PassPlan p = inflate_pass_plan(H, 64ull * H, 64, -1, 0, ncu, true, true, true);
        CHECK(passes(p, {{4, H}, {6, H}, {3, H}, {2, H}, {3, H}, {2, S}, {3, S}, {1, 0}}));
    }
    {  // the default plan at 64 KiB: no mode 6 and no mode 2
        const PassPlan p = inflate_pass_plan(B, 64ull * B, 64, -1, 0, ncu, true, true, true);
        CHECK(passes(p, {{4, B}, {3, B}, {1, 0}}));
        CHECK(p.heavy == 0 && p.heavy_limit == 0);
        CHECK(!plan_wants_heavy(B, 64) && plan_wants_heavy(S, 64) && !plan_wants_heavy(S, 0xFFFFFFF0ull));
    }
    {  // few_bits: under 4096 stream bytes per candidate
        PassPlan p = inflate_pass_plan(S, 1000, 2, -1, 0, ncu, true, true, true);
        CHECK(passes(p, {{4, S}, {6, S}, {3, S}, {0, 0}, {1, 0}}));
        p = inflate_pass_plan(S, 2 * 4096, 2, -1, 0, ncu, true, true, true);  // exactly 4096: not few
        CHECK(passes(p, {{4, S}, {6, S}, {3, S}, {2, S}, {3, S}, {2, H}, {3, H}, {1, 0}}));
        p = inflate_pass_plan(S, 2 * 4096 - 1, 2, -1, 0, ncu, true, true, true);
        CHECK(passes(p, {{4, S}, {6, S}, {3, S}, {0, 0}, {1, 0}}));
    }
    {  // each forced pass
        const uint64_t n = 32ull * S;
        CHECK(passes(inflate_pass_plan(S, n, 32, 0, 0, ncu, false, false, true), {{0, 0}, {1, 0}}));
        CHECK(passes(inflate_pass_plan(S, n, 32, 1, 0, ncu, false, false, true), {{1, 0}}));
        CHECK(passes(inflate_pass_plan(S, n, 32, 2, 0, ncu, false, false, true), {{2, S}, {3, S}, {2, H}, {3, H}, {1, 0}}));
        CHECK(passes(inflate_pass_plan(S, 1000, 2, 2, 0, ncu, false, false, true), {{2, S}, {3, S}, {2, H}, {3, H}, {1, 0}}));
        CHECK(passes(inflate_pass_plan(S, n, 32, 3, 0, ncu, false, false, true), {{2, S}, {3, S}, {2, H}, {3, H}, {1, 0}}));
        CHECK(passes(inflate_pass_plan(S, n, 32, 4, 0, ncu, true, true, true), {{4, S}, {6, S}, {3, S}}));
        CHECK(passes(inflate_pass_plan(S, 1000, 2, 4, 0, ncu, true, true, true), {{4, S}, {6, S}, {3, S}}));
        CHECK(passes(inflate_pass_plan(S, n, 32, 5, 0, ncu, false, false, true), {}));
        CHECK(passes(inflate_pass_plan(S, n, 32, 6, 0, ncu, false, false, true), {{2, S}, {3, S}, {2, H}, {3, H}, {1, 0}}));
        CHECK(passes(inflate_pass_plan(S, n, 32, 7, 0, ncu, false, false, true), {}));
        // a forced pass other than 4 does not take the lane decoder, whatever was allocated
        CHECK(passes(inflate_pass_plan(S, n, 32, 1, 0, ncu, true, true, true), {{1, 0}}));
        CHECK(plan_wants_lanes(-1) && plan_wants_lanes(4) && !plan_wants_lanes(0) && !plan_wants_lanes(5));
    }
    {  // the lane decoder's buffers did not fit
        const PassPlan p = inflate_pass_plan(S, 32ull * S, 32, -1, 0, ncu, false, false, true);
        CHECK(passes(p, {{2, S}, {3, S}, {2, H}, {3, H}, {1, 0}}) && p.heavy == 0);
        CHECK(passes(inflate_pass_plan(S, 32ull * S, 32, 4, 0, ncu, false, false, true), {}));
    }
    // the output cannot hold every candidate's slot
    CHECK(passes(inflate_pass_plan(S, 32ull * S, 32, -1, 0, ncu, true, true, false), {}));
    {  // one candidate in a large stream: not the segment layout
        CHECK(passes(inflate_pass_plan(S, 65537, 1, -1, 0, ncu, true, true, true), {}));
        const PassPlan p = inflate_pass_plan(S, 65536, 1, -1, 0, ncu, true, true, true);
        CHECK(passes(p, {{4, S}, {6, S}, {3, S}, {2, S}, {3, S}, {2, H}, {3, H}, {1, 0}}) && p.heavy == 256);
        CHECK(passes(inflate_pass_plan(S, 65537, 1, 4, 0, ncu, true, true, true), {{4, S}, {6, S}, {3, S}}));
    }
    // the per-pass rules
    CHECK(pass_skipped(3, 0, 100) && pass_skipped(3, 13, 100) && !pass_skipped(3, 12, 100) && !pass_skipped(3, 1, 100));
    CHECK(pass_skipped(6, 0, 100) && !pass_skipped(6, 99, 100) && !pass_skipped(4, 0, 100) && !pass_skipped(1, 0, 100));
    CHECK(pass_ends_plan(4, 4, 0, 0) && pass_ends_plan(4, 4, 2, 5) && !pass_ends_plan(4, 4, 1, 5));
    CHECK(pass_ends_plan(4, 4, 1, 0) && pass_ends_plan(6, 4, 1, 0) && pass_ends_plan(3, 4, 1, 0));
    CHECK(!pass_ends_plan(2, 2, 1, 0) && !pass_ends_plan(3, 2, 1, 0) && !pass_ends_plan(0, 0, 1, 0));
    // the lane decoder's token words: 16404 per candidate, at most 8 per stream bit + 20
    CHECK(lane_tok_words(S, 10, 1u << 20) == 164040 && lane_tok_words(H, 10, 1u << 20) == 164040);
    CHECK(lane_tok_words(B, 10, 1u << 20) == 10 * 32788 && lane_tok_words(S, 10, 100) == 800 + 200);
}

// ---- path 5 ----

static const FbGeom G = {1ull << 18, 1ull << 12, 0, 0};  // 2^18-bit super blocks of 64 chunks
static const uint64_t ST = FbPlan::kStored, M = FB_STOP_MASK;

static FbUnit unit(uint64_t start, uint64_t end, uint64_t size, uint64_t hdr, uint32_t flags) {
    return FbUnit{start, end, size, hdr, 0, flags};
}

static void test_from_hits() {
    {
        FbPlan p(200000, G);  // 1,600,000 bits
        const uint64_t hits[] = {1000, 1000, 500, 2000 | FB_HIT_REJECT, 3000 | ST, 500000, 600000 | ST};
        p.from_hits(hits, 7);
        CHECK(p.K == 5 && p.Ku == 5);
        CHECK(same(p.starts, U64{0, 1000, 3000, 500000, 600000}));
        CHECK(same(p.strong, std::initializer_list<uint8_t>{1, 1, 0, 1, 0}));
        CHECK(same(p.stops, U64{1000, 500000 | FB_STOP_REGION, 500000 | FB_STOP_WEAK, M | FB_STOP_REGION, M | FB_STOP_WEAK}));
        // words_of: 2/3 word per bit + 4096 in 64-word groups; weak 64 Ki + 4096; a region head
        // at most 458752 + 65536 (+ 4096)
        CHECK(p.words_of(0, p.stops[0]) == 4800);         // 2 * 1000 / 3 + 4096 = 4762
        CHECK(p.words_of(1000, p.stops[1]) == 336768);    // 2 * 499000 / 3 + 4096 = 336762
        CHECK(p.words_of(3000, p.stops[2]) == 69632);
        CHECK(p.words_of(500000, p.stops[3]) == 528384);  // capped: 524288 + 4096
        CHECK(p.words_of(1700000, M) == 4096 && p.words_of(0, M) == 1070784);  // clamped to the stream
        CHECK(FbPlan::region_words(532487) == 181632 && FbPlan::region_words(0) == 4096);
        p.budgets();
        // regions: spans 499000 (3 units) and 1100000 (6 units)
        CHECK(p.R == 512 && p.Kcap == 5 + 9 + 512);
        CHECK(p.tokoff[0] == 0 && p.tokoff[1] == 4800 && p.tokoff[2] == 341568 && p.tokoff[5] == 1009216);
        CHECK(p.rep_words == 1009216 + 2 * 570439 + 4096 * 512 && p.rep_used == 0);
        CHECK(p.starts.size() == p.Kcap && p.stops.size() == p.Kcap && p.tokoff.size() == p.Kcap + 1 &&
              p.units.size() == p.Kcap && p.vmode.size() == p.Kcap && p.vhdr.size() == p.Kcap && p.ucb.size() == p.Kcap);
        CHECK(p.vmode[0] == FB_V_HEADER && p.ucb[0] == ~0u && p.expects(0) == FB_AT_HEADER);
    }
    {  // no hits: R has its floor of 512
        FbPlan p(1000, G);
        p.from_hits(nullptr, 0);
        p.budgets();
        CHECK(p.K == 1 && p.stops[0] == M && p.R == 512 && p.Kcap == 513);
        CHECK(p.rep_words == p.words_of(0, M) + 4096 * 512);
    }
    {  // FB_STOP_REGION: more than 1.5 super blocks (393216 bits) to the next strong start ...
        FbPlan p(1u << 20, G);
        uint64_t h[] = {393216, 393216 + 393217};
        p.from_hits(h, 2);
        CHECK(p.stops[0] == 393216 && p.stops[1] == ((393216 + 393217) | FB_STOP_REGION));
        uint64_t w[] = {393217 | ST, 400000};  // (a weak start in between does not count)
        p.from_hits(w, 2);
        CHECK(p.stops[0] == (400000 | FB_STOP_REGION) && p.stops[1] == (400000 | FB_STOP_WEAK));
    }
    {  // ... or to the end of the stream
        FbPlan a(49152, G), b(49153, G);
        a.from_hits(nullptr, 0);
        b.from_hits(nullptr, 0);
        CHECK(a.stops[0] == M && b.stops[0] == (M | FB_STOP_REGION));
    }
}

// three scanned units at 0, 1000, 2000 in a stream of 800,000 bits; unit 2 is final
static FbPlan three_units() {
    FbPlan p(100000, G);
    const uint64_t hits[] = {1000, 2000};
    p.from_hits(hits, 2);
    p.budgets();
    p.units[0] = unit(0, 1000, 10, FB_AT_HEADER, 0);
    p.units[1] = unit(1000, 2000, 20, FB_AT_HEADER, SEGF_CROSSED);
    p.units[2] = unit(2000, 5000, 30, FB_AT_HEADER, SEGF_FINAL);
    p.select_regions();
    CHECK(p.regs.empty() && p.nsb == 0);
    const FbRegionUnits ru = p.region_units(nullptr);
    CHECK(ru.ok && ru.regions == 0 && p.Ku == 3);
    return p;
}
// a unit appended by hand (as a region or repair unit would be)
static void append(FbPlan& p, uint64_t start, uint8_t vmode, uint64_t vhdr, const FbUnit& u) {
    p.starts[p.Ku] = start, p.vmode[p.Ku] = vmode, p.vhdr[p.Ku] = vhdr, p.units[p.Ku] = u;
    p.Ku++;
}

static void test_walk() {
    {  // a clean chain
        FbPlan p = three_units();
        const FbWalk w = p.walk(0);
        CHECK(w.kind == FbWalk::DONE && same(p.chain, U32{0, 1, 2}));
        CHECK(same(p.coffs, U64{0, 10, 30}) && same(p.csizes, U64{10, 20, 30}) && p.total == 60);
    }
    for (int state = 0; state < 2; state++) {  // a break: unit 0 ends where no unit starts
        FbPlan p = three_units();
        const uint64_t hdr = state ? (FB_STATE_FIXED | FB_STATE_FINAL) : FB_AT_HEADER;
        p.units[0] = unit(0, 1500, 10, hdr, 0);
        FbWalk w = p.walk(0);
        CHECK(w.kind == FbWalk::REPAIR && w.k0 == 3 && p.Ku == 4);
        CHECK(p.starts[3] == 1500 && p.stops[3] == 2000 && p.ucb[3] == ~0u);
        CHECK(p.vmode[3] == (state ? FB_V_EXACT : FB_V_HEADER) && p.vhdr[3] == (state ? hdr : 0) && p.expects(3) == hdr);
        CHECK(p.tokoff[4] - p.tokoff[3] == 4480 && p.rep_used == 4480);  // 2 * 500 / 3 + 4096 = 4429
        p.units[3] = unit(1500, 2000, 5, FB_AT_HEADER, 0);
        w = p.walk(1);
        CHECK(w.kind == FbWalk::DONE && same(p.chain, U32{0, 3, 2}));
        CHECK(same(p.coffs, U64{0, 10, 15}) && same(p.csizes, U64{10, 5, 30}) && p.total == 45);
    }
    {  // two units at the same start and state: the larger end wins, the later one on a tie
        FbPlan p = three_units();
        p.units[1] = unit(1000, 1500, 20, FB_AT_HEADER, 0);
        append(p, 1000, FB_V_HEADER, 0, unit(1000, 2000, 21, FB_AT_HEADER, 0));
        CHECK(p.walk(0).kind == FbWalk::DONE && same(p.chain, U32{0, 3, 2}) && p.total == 61);
        p.units[1].end = 2000;
        CHECK(p.walk(0).kind == FbWalk::DONE && same(p.chain, U32{0, 3, 2}));
        p.units[3].end = 1500;
        CHECK(p.walk(0).kind == FbWalk::DONE && same(p.chain, U32{0, 1, 2}) && p.total == 60);
    }
    {  // a unit at the right bit in the wrong code state is not linked
        FbPlan p = three_units();
        p.units[0].hdr = FB_STATE_FIXED;
        const FbWalk w = p.walk(0);
        CHECK(w.kind == FbWalk::REPAIR && w.k0 == 3 && p.Ku == 4 && p.starts[3] == 1000);
        CHECK(p.vmode[3] == FB_V_EXACT && p.vhdr[3] == FB_STATE_FIXED && p.stops[3] == 2000);
        // ... and an exact unit in that state is, before the header unit there
        p.units[3] = unit(1000, 2000, 7, FB_AT_HEADER, 0);
        CHECK(p.walk(1).kind == FbWalk::DONE && same(p.chain, U32{0, 3, 2}) && p.total == 47);
    }
    {  // unit 0 in error
        FbPlan p = three_units();
        p.units[0].flags = SEGF_OVERREAD;
        FbWalk w = p.walk(0);
        CHECK(w.kind == FbWalk::STREAM_ERROR && w.err == DMX_ERR_OVERREAD && w.unit == 0 && p.chain.empty());
        p.units[0].flags = SEGF_ERR_DATA | SEGF_CROSSED;
        w = p.walk(0);
        CHECK(w.kind == FbWalk::STREAM_ERROR && w.err == DMX_ERR_DATA && w.unit == 0);
        p.units[0].flags = SEGF_OVERREAD | SEGF_ERR_DATA;
        CHECK(p.walk(0).err == DMX_ERR_OVERREAD);
        p.units[0].flags = SEGF_OVERREAD | SEGF_OVERFLOW;
        w = p.walk(0);
        CHECK(w.kind == FbWalk::DECLINE && !std::strcmp(w.why, "unit error") && w.unit == 0);
    }
    {  // an errored unit where the chain arrives is the stream's error; off the chain it is ignored
        FbPlan p = three_units();
        p.units[1].flags = SEGF_ERR_DATA;
        FbWalk w = p.walk(0);
        CHECK(w.kind == FbWalk::STREAM_ERROR && w.err == DMX_ERR_DATA && w.unit == 1 && same(p.chain, U32{0}));
        p.units[0].end = 2000;
        w = p.walk(0);
        CHECK(w.kind == FbWalk::DONE && same(p.chain, U32{0, 2}) && p.total == 40);
        // (its own limits are no stream error: a repair unit is tried)
        p.units[0].end = 1000;
        p.units[1].flags = SEGF_ERR_DATA | SEGF_TIMEOUT;
        CHECK(p.walk(0).kind == FbWalk::REPAIR && p.starts[3] == 1000 && p.vmode[3] == FB_V_HEADER);
    }
    {  // the same break twice
        FbPlan p = three_units();
        p.units[0].end = 1500;
        CHECK(p.walk(0).kind == FbWalk::REPAIR);
        p.units[3] = unit(1500, 1600, 0, FB_AT_HEADER, SEGF_OVERFLOW);
        const FbWalk w = p.walk(1);
        CHECK(w.kind == FbWalk::DECLINE && !std::strcmp(w.why, "repair failed") && w.unit == 2 && p.Ku == 4);
    }
    {  // token space used up
        FbPlan p = three_units();
        p.units[0].end = 1500;
        p.rep_used = p.rep_words - 4479;
        FbWalk w = p.walk(0);
        CHECK(w.kind == FbWalk::DECLINE && !std::strcmp(w.why, "repair token space") && w.unit == 2 && p.Ku == 3);
        p.rep_used = p.rep_words - 4480;
        CHECK(p.walk(0).kind == FbWalk::REPAIR && p.rep_used == p.rep_words);
    }
    {  // the last round
        FbPlan p = three_units();
        p.units[0].end = 1500;
        FbWalk w = p.walk(FbPlan::kRepairRounds);
        CHECK(FbPlan::kRepairRounds == 48 && w.kind == FbWalk::DECLINE && !std::strcmp(w.why, "repairs exhausted"));
        CHECK(w.unit == 2 && p.Ku == 3);
        p.units[2].flags = 0;  // (no final unit either: the end of unit 2 is a second break)
        w = p.walk(48);
        CHECK(w.kind == FbWalk::DECLINE && !std::strcmp(w.why, "no final block") && w.unit == 2);
        CHECK(p.walk(47).kind == FbWalk::REPAIR && p.Ku == 5 && p.starts[3] == 1500 && p.starts[4] == 5000 &&
              p.stops[4] == M);
    }
    {  // more breaks than units left
        FbPlan p = three_units();
        p.units[0].end = 1500;
        p.Kcap = 3;
        const FbWalk w = p.walk(0);
        CHECK(w.kind == FbWalk::DECLINE && !std::strcmp(w.why, "repairs exhausted"));
    }
}

static void test_region_units() {
    for (int walked = 0; walked < 2; walked++) {
        FbPlan p(200000, G);  // 1,600,000 bits
        const uint64_t hits[] = {1000, 10000 | ST, 1200000, 1300000 | ST};
        p.from_hits(hits, 4);
        CHECK(p.K == 5 && p.stops[1] == (1200000 | FB_STOP_REGION) && p.stops[3] == (M | FB_STOP_REGION));
        p.budgets();
        p.units[0] = unit(0, 1000, 1, FB_AT_HEADER, 0);
        p.units[1] = unit(1000, 5000, 2, FB_AT_HEADER, SEGF_CROSSED);  // stopped at a far fixed-code header
        p.units[2] = unit(10000, 10100, 0, FB_AT_HEADER, SEGF_ERR_DATA);
        p.units[3] = unit(1200000, 1500000, 3, FB_AT_HEADER, SEGF_FINAL);  // (final: no region after it)
        p.units[4] = unit(1300000, 1300100, 0, FB_AT_HEADER, SEGF_ERR_DATA);
        p.select_regions();
        CHECK(p.regs.size() == 1 && p.nsb == 5);
        CHECK(p.regs[0].E == 5000 && p.regs[0].T == 1200000 && p.regs[0].sb0 == 0 && p.regs[0].nsb == 5);
        // super block 1 and 4 skipped; the walk failed (or reached the end)
        const uint32_t vis[6] = {0, ~0u, (130u << 6) | (1u << 5) | 7u, (200u << 6) | 9u, ~0u,
                                 walked ? FB_REGION_END : 0u};
        const FbRegionUnits ru = p.region_units(vis);
        CHECK(ru.ok && ru.regions == 1 && p.Ku == 8);
        CHECK(p.starts[5] == 5000 && p.starts[6] == 5000 + 130 * 4096 + 7 && p.starts[7] == 5000 + 200 * 4096 + 9);
        CHECK(p.vmode[5] == FB_V_HEADER && p.vmode[6] == FB_V_EXACT && p.vmode[7] == FB_V_EXACT);
        CHECK(p.vhdr[5] == 0 && p.vhdr[6] == (FB_STATE_FIXED | FB_STATE_FINAL) && p.vhdr[7] == FB_STATE_FIXED);
        CHECK(p.ucb[5] == 0 && p.ucb[6] == 128 && p.ucb[7] == 192);
        CHECK(p.stops[5] == (537487 | FB_STOP_SOFT) && p.stops[6] == (824209 | FB_STOP_SOFT) && p.stops[7] == 1200000);
        // a third of a word per bit + 4096; the last unit of a failed walk: the open budget
        // (2/3 of a word per bit up to T, at most kOpenWords)
        const uint64_t last = walked ? 129408 : 254656;
        CHECK(p.tokoff[6] - p.tokoff[5] == 181632 && p.tokoff[7] - p.tokoff[6] == 99712 && p.tokoff[8] - p.tokoff[7] == last);
        CHECK(p.rep_used == 181632 + 99712 + last && FbPlan::kOpenWords == 4198400);
        // the weak start at 10000 is superseded (a repair unit stops softly at the next region
        // unit), the one at 1300000 is not a stop at all
        CHECK(p.stop_of(2000) == 5000 && p.stop_of(6000) == (537487 | FB_STOP_SOFT) && p.stop_of(5000) == (537487 | FB_STOP_SOFT));
        CHECK(p.stop_of(537487) == (824209 | FB_STOP_SOFT) && p.stop_of(900000) == 1200000 && p.stop_of(1250000) == M);
        CHECK(p.stop_of(500) == 1000 && p.stop_of(0) == 1000);
    }
    {  // a far open stop: the budget is capped at kOpenWords
        FbPlan p(4000000, G);  // 32,000,000 bits
        const uint64_t hits[] = {1000, 30000000};
        p.from_hits(hits, 2);
        p.budgets();
        p.units[0] = unit(0, 1000, 1, FB_AT_HEADER, 0);
        p.units[1] = unit(1000, 5000, 2, FB_AT_HEADER, 0);
        p.units[2] = unit(30000000, 30000100, 3, FB_AT_HEADER, SEGF_FINAL);
        p.select_regions();
        CHECK(p.regs.size() == 1 && p.nsb == 115);  // ceil(29,995,000 / 2^18)
        std::vector<uint32_t> vis(116, ~0u);
        vis[0] = 0, vis[115] = 0;
        const FbRegionUnits ru = p.region_units(vis.data());
        CHECK(ru.ok && p.Ku == 4 && p.stops[3] == 30000000 && p.tokoff[4] - p.tokoff[3] == FbPlan::kOpenWords);
    }
    {  // the region units do not fit the token space
        FbPlan p(200000, G);
        const uint64_t hits[] = {1000, 1200000};
        p.from_hits(hits, 2);
        p.budgets();
        p.units[1] = unit(1000, 5000, 2, FB_AT_HEADER, 0);
        p.units[2] = unit(1200000, 1500000, 3, FB_AT_HEADER, SEGF_FINAL);
        p.select_regions();
        const uint32_t vis[6] = {0, ~0u, (130u << 6) | 7u, ~0u, ~0u, FB_REGION_END};
        p.rep_words = 181632 + 100000;
        const FbRegionUnits ru = p.region_units(vis);
        CHECK(!ru.ok && ru.token_space && ru.unit == 4 && ru.regions == 1);
    }
    {  // region selection: only heads that stopped clean at a header, more than a super block before T
        FbPlan p(200000, G);
        const uint64_t hits[] = {1000, 1200000};
        p.from_hits(hits, 2);
        p.budgets();
        p.units[2] = unit(1200000, 1500000, 3, FB_AT_HEADER, SEGF_FINAL);
        p.units[1] = unit(1000, 5000, 2, FB_STATE_FIXED, 0);
        p.select_regions();
        CHECK(p.regs.empty());
        p.units[1] = unit(1000, 5000, 2, FB_AT_HEADER, SEGF_OVERFLOW);
        p.select_regions();
        CHECK(p.regs.empty());
        p.units[1] = unit(1000, 1200000 - 262144, 2, FB_AT_HEADER, 0);
        p.select_regions();
        CHECK(p.regs.empty());
        p.units[1] = unit(1000, 1200000 - 262145, 2, FB_AT_HEADER, 0);
        p.select_regions();
        CHECK(p.regs.size() == 1 && p.regs[0].nsb == 2 && p.nsb == 2);
    }
}

int main() {
    test_seg_chain();
    test_pass_plan();
    test_from_hits();
    test_walk();
    test_region_units();
    std::printf("plan_test: %d checks, %d failed\n", checks, fails);
    return fails ? 1 : 0;
}
