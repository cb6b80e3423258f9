// tests/cpp/inflate_spec_test.cpp -- the decisions around the synchronous inflate's speculative
// first pass (deflate.hpp_amd/csrc/inflate_plan.cpp: spec_knob, spec_wanted, spec_provision,
// spec_decide) over a table of cases: no GPU, no HIP; links inflate_plan.cpp alone.  Exit code
// 0 = all checks passed (tests/test_inflate_spec.py runs it plain and under ASan + UBSan).
#include <cstdio>

#include "../../deflate.hpp_amd/csrc/inflate_plan.h"

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

constexpr int NCU = 256;
constexpr SpecVerdict D = SpecVerdict::Discard, A = SpecVerdict::Accept, C = SpecVerdict::Continue;

// the plan the driver makes for `ncand` candidates of an n-byte stream (every allocation fits)
static PassPlan plan(uint32_t seg, uint64_t n, uint64_t ncand, int forced = -1, bool lanes_ok = true,
                     uint32_t heavy_bytes = 0) {
    const bool heavy_ok = lanes_ok && plan_wants_lanes(forced) && plan_wants_heavy(seg, ncand);
    return inflate_pass_plan(seg, n, ncand, forced, heavy_bytes, NCU, lanes_ok, heavy_ok, true);
}

static void test_knob() {
    CHECK(spec_knob(nullptr) == SpecKnob::On);
    CHECK(spec_knob("") == SpecKnob::On);
    CHECK(spec_knob("1") == SpecKnob::On);
    CHECK(spec_knob("0") == SpecKnob::Off);
    CHECK(spec_knob("force") == SpecKnob::Force);
    CHECK(spec_knob("forced") == SpecKnob::On && spec_knob("00") == SpecKnob::On && spec_knob("x") == SpecKnob::On);
}

static void test_gate() {
    for (const uint32_t seg : {16384u, 32768u, 65536u}) {
        const uint64_t at = 2048ull * seg;  // cap / seg == 2048: not above the gate
        const uint64_t big = 1ull << 40;  // stream bytes: never the smaller bound
        CHECK(spec_provision(seg, at, big) == 2048 + 64);
        CHECK(spec_provision(seg, at + seg - 1, big) == 2048 + 64 && spec_provision(seg, at + seg, big) == 2049 + 64);
        CHECK(spec_provision(seg, 0, big) == 64);
        // a capacity far above what the stream can hold: four bytes per marker bound the count
        CHECK(spec_provision(seg, big, 4000) == 1001 && spec_provision(seg, big, 3) == 1);
        CHECK(spec_provision(seg, at, 4 * 2111) == 2112 && spec_provision(seg, at, 4 * 2110) == 2111);
        // the capacity gate
        CHECK(!spec_wanted(SpecKnob::On, true, false, false, -1, seg, at));
        CHECK(!spec_wanted(SpecKnob::On, true, false, false, -1, seg, at + seg - 1));
        CHECK(spec_wanted(SpecKnob::On, true, false, false, -1, seg, at + seg));
        CHECK(spec_wanted(SpecKnob::On, true, false, false, -1, seg, 1ull << 40));
        // force drops it, and nothing else
        CHECK(spec_wanted(SpecKnob::Force, true, false, false, -1, seg, 0));
        CHECK(spec_wanted(SpecKnob::Force, true, false, false, -1, seg, at));
        CHECK(!spec_wanted(SpecKnob::Force, false, false, false, -1, seg, at + seg));  // the context's buffer
        CHECK(!spec_wanted(SpecKnob::Force, true, true, false, -1, seg, at + seg));    // a piece
        CHECK(!spec_wanted(SpecKnob::Force, true, false, true, -1, seg, at + seg));    // a diagnostic
        CHECK(!spec_wanted(SpecKnob::On, false, false, false, -1, seg, at + seg));
        CHECK(!spec_wanted(SpecKnob::On, true, true, false, -1, seg, at + seg));
        CHECK(!spec_wanted(SpecKnob::On, true, false, true, -1, seg, at + seg));
        // off
        CHECK(!spec_wanted(SpecKnob::Off, true, false, false, -1, seg, 1ull << 40));
        // each forced pass value: only the plan (-1) and the forced lane pass (4) start with the lanes
        for (int forced = -1; forced <= 7; forced++) {
            const bool want = forced == -1 || forced == 4;
            CHECK(spec_wanted(SpecKnob::On, true, false, false, forced, seg, at + seg) == want);
            CHECK(spec_wanted(SpecKnob::Force, true, false, false, forced, seg, 3 * seg) == want);
        }
    }
    CHECK(!spec_wanted(SpecKnob::Force, true, false, false, -1, 0, 1 << 20));  // (never divides by zero)
}

static void test_decide() {
    for (const uint32_t seg : {16384u, 32768u, 65536u}) {
        const uint64_t cap = 4096ull * seg, n = cap / 3, ncap = spec_provision(seg, cap, n);
        CHECK(ncap == 4160);
        const PassPlan sp = plan(seg, n, ncap);
        CHECK(sp.np > 0 && sp.pass[0][0] == 4 && sp.pass[0][1] == seg);
        // counts: 1 (no marker), 2048, 2049, provisioned, provisioned + 1
        CHECK(spec_decide(sp, plan(seg, n, 1), 1, ncap, 0, 0) == D);
        CHECK(spec_decide(sp, plan(seg, n, 1), 1, ncap, 2, 0) == D);
        CHECK(spec_decide(sp, plan(seg, n, 2048), 2048, ncap, 0, 0) == D);
        CHECK(spec_decide(sp, plan(seg, n, 2049), 2049, ncap, 0, 0) == A);
        CHECK(spec_decide(sp, plan(seg, n, ncap), ncap, ncap, 0, 0) == A);
        CHECK(spec_decide(sp, PassPlan{}, ncap + 1, ncap, 0, 0) == D);
        CHECK(spec_decide(sp, plan(seg, n, ncap + 1), ncap + 1, ncap, 0, 0) == D);  // (whatever plan comes along)
        CHECK(spec_decide(sp, PassPlan{}, ~0ull, ncap, 0, 0) == D);
        // the validation's status
        const PassPlan cl = plan(seg, n, 4000);
        CHECK(spec_decide(sp, cl, 4000, ncap, 0, 0) == A);
        CHECK(spec_decide(sp, cl, 4000, ncap, 2, 0) == D);       // not settled by a segmented pass
        CHECK(spec_decide(sp, cl, 4000, ncap, 2, 17) == D);
        CHECK(spec_decide(sp, cl, 4000, ncap, -3, 0) == D);      // (no such status: as today, from the start)
        CHECK(spec_decide(sp, cl, 4000, ncap, 1, 5) == C);       // declined candidates: the heavy / patch passes
        CHECK(spec_decide(sp, cl, 4000, ncap, 1, 4000) == C);
        CHECK(spec_decide(sp, cl, 4000, ncap, 1, 0) == A);       // sizes not uniform: the plan is over, chain repair
        CHECK(pass_ends_plan(4, 4, 1, 0) && !pass_ends_plan(4, 4, 1, 5));
        // the classic plan must have the same first pass and parameters
        PassPlan other = cl;
        other.heavy += 1;
        CHECK(spec_decide(sp, other, 4000, ncap, 0, 0) == D);
        other = cl;
        other.heavy_limit -= 1;
        CHECK(spec_decide(sp, other, 4000, ncap, 0, 0) == D);
        other = cl;
        other.pass[0][1] = seg / 2;
        CHECK(spec_decide(sp, other, 4000, ncap, 0, 0) == D);
        other = cl;
        other.pass[0][0] = 2;
        CHECK(spec_decide(sp, other, 4000, ncap, 0, 0) == D);
        other = cl;
        other.np = 0;
        CHECK(spec_decide(sp, other, 4000, ncap, 0, 0) == D);
        // a developer's heavy threshold is the same on both sides
        CHECK(spec_decide(plan(seg, n, ncap, -1, true, 999), plan(seg, n, 4000, -1, true, 999), 4000, ncap, 0, 0) == A);
        CHECK(spec_decide(plan(seg, n, ncap, -1, true, 999), cl, 4000, ncap, 0, 0) == (seg <= 32768 ? D : A));
        // the forced lane pass speculates like the plan; lanes_ok false: no lane pass, nothing to stand
        CHECK(spec_decide(plan(seg, n, ncap, 4), plan(seg, n, 4000, 4), 4000, ncap, 0, 0) == A);
        CHECK(spec_decide(plan(seg, n, ncap, 4), plan(seg, n, 4000, 4), 4000, ncap, 1, 3) == C);
        const PassPlan nol = plan(seg, n, ncap, -1, false);
        CHECK(nol.np == 0 || nol.pass[0][0] != 4);
        CHECK(spec_decide(nol, plan(seg, n, 4000, -1, false), 4000, ncap, 0, 0) == D);
        CHECK(spec_decide(sp, plan(seg, n, 4000, -1, false), 4000, ncap, 0, 0) == D);
        // every other forced pass value: the plan does not start with the lanes
        for (const int forced : {0, 1, 2, 3, 5, 6, 7}) {
            const PassPlan f = plan(seg, n, ncap, forced);
            CHECK(f.np == 0 || f.pass[0][0] != 4);
            CHECK(spec_decide(f, plan(seg, n, 4000, forced), 4000, ncap, 0, 0) == D);
        }
        // force at a small capacity: the provisioned plan's heavy limit is the small streams', and
        // counts at or below the gate never stand
        const uint64_t ncap3 = spec_provision(seg, 3ull * seg, 50000);
        CHECK(ncap3 == 67);
        CHECK(spec_decide(plan(seg, 50000, ncap3), plan(seg, 50000, 3), 3, ncap3, 0, 0) == D);
        CHECK(spec_decide(plan(seg, 50000, ncap3), PassPlan{}, 68, ncap3, 0, 0) == D);
        // force, a capacity at the gate and a count above it: provisioned 2112, heavy limit of the
        // large streams on both sides
        const uint64_t ncapg = spec_provision(seg, 2049ull * seg - 1, n);
        CHECK(ncapg == 2112);
        CHECK(spec_decide(plan(seg, n, ncapg), plan(seg, n, 2049), 2049, ncapg, 0, 0) == A);
        // the gate's two sides of a provisioned plan: 2048 provisioned (heavy limit of small
        // streams) against 2049 candidates cannot happen, and would be discarded by the count
        CHECK(spec_decide(plan(seg, n, 2048), plan(seg, n, 2049), 2049, 2048, 0, 0) == D);
    }
}

int main() {
    test_knob();
    test_gate();
    test_decide();
    std::printf("inflate_spec_test: %d checks, %d failed\n", checks, fails);
    return fails ? 1 : 0;
}
