// deflate_pipe_test.cpp -- CPU test of deflate.hpp_amd/csrc/deflate_pipe.h: the chunk arithmetic
// of the deflate's chunk pipeline and its knob.  Stand-alone (its own main, no HIP, no GPU).
#include <cstdio>
#include <vector>

#include "../../deflate.hpp_amd/csrc/deflate_pipe.h"

using namespace dmx;

static int g_checks = 0, g_failed = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        g_checks++;                                                           \
        if (!(c)) {                                                           \
            g_failed++;                                                       \
            std::fprintf(stderr, "[FAIL] %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                                     \
    } while (0)

// every segment and every front segment exactly once, the halves of a block in the block's chunk
static void check_cover(uint64_t nseg, uint64_t chunk, uint32_t halves, uint64_t nfront) {
    const uint64_t k = pipe_chunk_count(nseg, chunk);
    CHECK(k >= 2);
    std::vector<uint8_t> seen(nseg, 0), fseen(nfront, 0);
    uint64_t prev = 0, fprev = 0;
    for (uint64_t i = 0; i < k; i++) {
        const PipeRange r = pipe_range(nseg, chunk, i);
        CHECK(r.first == prev && r.first < r.end && r.end <= nseg);
        CHECK(i + 1 == k ? r.end == nseg : r.end - r.first == chunk);
        prev = r.end;
        for (uint64_t s = r.first; s < r.end; s++) seen[s]++;
        const PipeRange f = pipe_front_range(r, halves, nfront);
        CHECK(f.first == fprev && f.first < f.end && f.end <= nfront);
        fprev = f.end;
        for (uint64_t s = f.first; s < f.end; s++) {
            fseen[s]++;
            CHECK(s / halves >= r.first && s / halves < r.end);  // a half lies in its block's chunk
        }
    }
    CHECK(prev == nseg && fprev == nfront);
    for (uint64_t s = 0; s < nseg; s++) CHECK(seen[s] == 1);
    for (uint64_t s = 0; s < nfront; s++) CHECK(fseen[s] == 1);
}

int main() {
    // below two grids' worth of segments: no pipeline
    for (uint64_t fit : {1ull, 7ull, 256ull, 512ull})
        for (uint64_t nseg = 0; nseg < 2 * fit; nseg += (fit > 16 ? 37 : 1))
            for (uint32_t k : {2u, 4u, 8u}) CHECK(pipe_chunk_segs(nseg, fit, k, 0) == 0);
    CHECK(pipe_chunk_segs(1000, 256, 1, 0) == 0 && pipe_chunk_segs(1000, 256, 0, 0) == 0);
    CHECK(pipe_chunk_segs(1000, 0, 4, 0) == 0);

    // from there on: multiples of the grid, at most the wanted count, full cover
    for (uint64_t fit : {1ull, 3ull, 64ull, 256ull, 512ull}) {
        for (uint64_t nseg : std::vector<uint64_t>{2 * fit, 2 * fit + 1, 3 * fit - 1, 4 * fit, 4 * fit + 1, 7 * fit + 5, 32768,
                                                   32769, 16384, 100003}) {
            if (nseg < 2 * fit) continue;
            for (uint32_t k : {2u, 3u, 4u, 8u, 64u}) {
                const uint64_t c = pipe_chunk_segs(nseg, fit, k, 0);
                if (c == 0) {  // only when rounding the chunk up to the grid leaves a single chunk
                    CHECK(((nseg + k - 1) / k + fit - 1) / fit * fit >= nseg);
                    continue;
                }
                CHECK(c % fit == 0 && c < nseg);
                CHECK(pipe_chunk_count(nseg, c) <= k);
                for (uint32_t halves : {1u, 2u}) {
                    check_cover(nseg, c, halves, nseg * halves);
                    if (halves == 2) check_cover(nseg, c, halves, nseg * halves - 1);  // a last block of one half
                }
            }
        }
    }
    // 2 x fit exactly splits into two chunks of one grid each
    CHECK(pipe_chunk_segs(512, 256, 2, 0) == 256 && pipe_chunk_segs(512, 256, 8, 0) == 256);
    // the headline: 32768 segments on 256 CUs, four chunks of 8192
    CHECK(pipe_chunk_segs(32768, 256, 4, 0) == 8192 && pipe_chunk_count(32768, 8192) == 4);

    // a forced chunk (tests): may be smaller than the grid; engages from a chunk and one segment
    CHECK(pipe_chunk_segs(64, 256, 4, 64) == 0 && pipe_chunk_segs(65, 256, 4, 64) == 64);
    for (uint64_t nseg : {65ull, 128ull, 129ull, 192ull, 193ull, 1000ull})
        for (uint32_t halves : {1u, 2u}) {
            check_cover(nseg, 64, halves, nseg * halves);
            if (halves == 2) check_cover(nseg, 64, halves, nseg * halves - 1);
        }

    // the knob
    PipeKnob k = pipe_knob(nullptr);
    CHECK(k.on == kPipeDefaultOn && !k.explicit_on && k.chunks == kPipeDefaultChunks && k.forced == 0);
    k = pipe_knob("");
    CHECK(k.on == kPipeDefaultOn && !k.explicit_on);
    k = pipe_knob("0");
    CHECK(!k.on && !k.explicit_on);
    k = pipe_knob("1");
    CHECK(k.on && k.explicit_on && k.chunks == kPipeDefaultChunks && k.forced == 0);
    k = pipe_knob("8");
    CHECK(k.on && k.explicit_on && k.chunks == 8 && k.forced == 0);
    k = pipe_knob("s64");
    CHECK(k.on && k.explicit_on && k.forced == 64);
    for (const char* bad : {"x", "s", "s0", "65", "4x", "-1", "99999999999999999999"}) {
        k = pipe_knob(bad);
        CHECK(k.on == kPipeDefaultOn && !k.explicit_on && k.chunks == kPipeDefaultChunks && k.forced == 0);
    }
    std::printf("deflate_pipe_test: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
