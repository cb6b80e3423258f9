// deflate_pipe.h -- the chunk arithmetic of the deflate's chunk pipeline (launch_deflate): plain
// C++, shared by the host runtime and tests/cpp/deflate_pipe_test.cpp.
//
// The single-stream deflate splits its segments into chunks; chunk i's emission runs on a side
// stream while the front kernel works on chunk i + 1.  A segment here is what the emission
// kernel takes (a block of 16, 32 or 64 KiB); a 64 KiB block is two front segments (halves) of
// 32 KiB, and both halves of a block belong to the block's chunk.
#pragma once
#include <stdint.h>

namespace dmx {

struct PipeRange {
    uint64_t first, end;  // [first, end)
};

// The chunk size in segments, or 0: no pipeline (one launch over all segments).
//   nseg    segments of the call
//   fit     the front kernel's persistent grid (deflate_front_fit), >= 1
//   chunks  the wanted chunk count (>= 2; fewer come out when the rounding says so)
//   forced  != 0: the chunk size itself (tests; may be smaller than the grid)
// A chunk is a multiple of the grid, so that every persistent workgroup gets the same number of
// segments in every chunk but the last; the pipeline engages from two grids' worth of segments
// (forced: from one segment more than a chunk).
inline uint64_t pipe_chunk_segs(uint64_t nseg, uint64_t fit, uint32_t chunks, uint64_t forced) {
    if (forced) return nseg > forced ? forced : 0;
    if (fit == 0 || chunks < 2 || nseg < 2 * fit) return 0;
    const uint64_t per = (nseg + chunks - 1) / chunks;
    const uint64_t c = (per + fit - 1) / fit * fit;
    return c < nseg ? c : 0;
}
inline uint64_t pipe_chunk_count(uint64_t nseg, uint64_t chunk) { return (nseg + chunk - 1) / chunk; }
// chunk i of pipe_chunk_count(nseg, chunk)
inline PipeRange pipe_range(uint64_t nseg, uint64_t chunk, uint64_t i) {
    const uint64_t a = i * chunk, b = a + chunk;
    return {a, b < nseg ? b : nseg};
}
// the front kernel's segments of a chunk: `halves` front segments per segment (2 for 64 KiB
// blocks, else 1), nfront of them in all (the last block may have one half only)
inline PipeRange pipe_front_range(PipeRange r, uint32_t halves, uint64_t nfront) {
    const uint64_t a = r.first * halves, b = r.end * halves;
    return {a < nfront ? a : nfront, b < nfront ? b : nfront};
}

// DMX_DEFLATE_PIPE (developer knob, read at dmx_create): "0" off; "1" on with the default chunk
// count; "<k>" (2..64) on with k chunks; "s<n>" on with chunks of n segments (tests).  Unset or
// unparsable: the default (on = kPipeDefaultOn, explicit = false): the synchronous call with
// 32 KiB segments takes the pipeline; 64 KiB blocks and the asynchronous call only when the knob
// asks for it (explicit).
struct PipeKnob {
    bool on;
    bool explicit_on;  // asked for by the knob: 64 KiB blocks and the asynchronous call follow it too
    uint32_t chunks;
    uint64_t forced;
};
constexpr bool kPipeDefaultOn = true;
constexpr uint32_t kPipeDefaultChunks = 4;
inline PipeKnob pipe_knob(const char* e) {
    PipeKnob k{kPipeDefaultOn, false, kPipeDefaultChunks, 0};
    if (!e || !*e) return k;
    const bool seg = *e == 's';
    uint64_t v = 0;
    const char* p = e + (seg ? 1 : 0);
    if (!*p) return k;
    for (; *p; p++) {
        if (*p < '0' || *p > '9' || v > (1u << 24)) return k;
        v = v * 10 + (uint64_t)(*p - '0');
    }
    if (seg) {
        if (v) k.on = k.explicit_on = true, k.forced = v;
    } else if (v == 0) {
        k.on = false;
    } else if (v == 1) {
        k.on = k.explicit_on = true;
    } else if (v <= 64) {
        k.on = k.explicit_on = true, k.chunks = (uint32_t)v;
    }
    return k;
}

}  // namespace dmx
