// seek_plan.h -- the host-side decisions of the seek index (dmx_inflate_index_device,
// dmx_inflate_range_device), free of HIP: which checkpoints of a decode become index entries
// (seek_select) and which spans a ranged read decodes (seek_range_plan).  The drivers
// (the two calls in dmx_host.cpp; the hand-over in host_fb.cpp and host_inflate.cpp) allocate, upload and launch
// what these decide; tests/cpp/seek_plan_test.cpp checks them against models on the CPU.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/dmx.h"

namespace dmx {

// A point of a finished decode where a decoder can start again: the stream bit of a block header
// and the plain bytes before it.  nowindow: nothing before the point is referenced (a libdmx
// segment start).
struct SeekCand {
    uint64_t bit, uoffset;
    bool nowindow;
};

// What a decode hands over when an index is asked for (dmx_ctx::seek_tap, null otherwise): the
// path that decoded the stream lists its checkpoints in stream order.  Paths without checkpoints
// (the serial decoder, the workgroup decoders) leave the list empty.
struct SeekTap {
    std::vector<SeekCand> cands;
};

// The index entries of a decode: entry 0 = {0, 0, 0, NOWINDOW}, then the candidates taken
// greedily -- one is kept when its uoffset is at least `spacing` past the last kept entry's.
// cands are in stream order (bit and uoffset not decreasing); spacing >= DMX_SEEK_WINDOW, so a
// kept entry that needs a window has all 32768 bytes of it.  The sentinel is the caller's.
std::vector<dmx_seek_entry> seek_select(const SeekCand* cands, uint64_t ncand, uint64_t spacing);

// One span of a ranged read: the decoder starts at `bit` behind window slot `slot` (window bytes:
// 0 or 32768), decodes `limit` plain bytes and writes those from `skip` on to d_out + out_off.
struct SeekSpan {
    uint64_t bit;
    uint64_t limit;
    uint64_t skip;
    uint64_t out_off;
    uint64_t slot;
    uint32_t window;
    uint32_t pad_;
};
static_assert(sizeof(SeekSpan) == 48, "SeekSpan is shared with the kernel");
// What the span decoder's launch starts from, uploaded in front of the spans: the ticket the
// workgroups draw spans from (0) and the status key (all ones; the kernel leaves the minimum of
// span index << 32 | (uint32_t)status over the failing spans).
struct SeekSpanHead {
    uint32_t ticket, pad_;
    unsigned long long key;
};
static_assert(sizeof(SeekSpanHead) == 16, "SeekSpanHead is shared with the kernel");
// A window slot the gather kernel fills: plain bytes [uoffset - 32768, uoffset) into slot `slot`.
struct SeekSlot {
    uint64_t slot, uoffset;
};

// The spans of plain bytes [uoffset, uoffset + len) over entries[0 .. count] (the last one the
// sentinel), n = the stream's bytes.  Entry k covers [uoffset_k, uoffset_{k+1}); the touched ones
// are found by two binary searches.  DMX_ERR_ARG: no entry, a range beyond the sentinel's uoffset
// or before entry 0's, a sentinel bit beyond 8 n, entries not strictly increasing in uoffset (the
// sentinel may equal the last entry), an entry without NOWINDOW whose window is not 32768.
// len == 0: DMX_OK and no span.
int seek_range_plan(const dmx_seek_entry* entries, uint64_t count, uint64_t n, uint64_t uoffset, uint64_t len,
                    std::vector<SeekSpan>* spans);

}  // namespace dmx
