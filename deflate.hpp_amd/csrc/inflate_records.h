// inflate_records.h -- the records the inflate kernels write and the host plans from, with their
// flag and stop constants.  Plain C++ (no HIP): shared by the kernels (through dmx_internal.h)
// and the host-side planners (inflate_plan.h).
#pragma once
#include <stdint.h>

namespace dmx {

// per-candidate record of the segment-parallel inflate
struct SegRecord {
    uint64_t end_byte;  // byte offset (relative to the stream) just past the segment's marker
    uint64_t offset;    // output offset the segment was written at
    uint32_t out_size;
    uint32_t flags;     // SEGF_*
};
static_assert(sizeof(SegRecord) == 24, "SegRecord is shared with the kernels");
enum : uint32_t {
    SEGF_FINAL = 1u,      // the segment ended with a BFINAL block
    SEGF_ERR_DATA = 2u,   // undecodable code / table
    SEGF_OVERREAD = 4u,   // ran past the end of the input
    SEGF_OVERFLOW = 8u,   // output exceeded the LDS window
    SEGF_XREF = 16u,      // back-reference reaches before the segment start
    SEGF_TIMEOUT = 32u,   // look-back spin bound hit
    SEGF_EXOTIC = 64u,    // layout the workgroup decoder does not take (several blocks, > 32 KiB,
                          // unsettled split): the wave-per-segment decoder redoes the stream
};

// block-parallel inflate of arbitrary streams (inflate_blocks.hip, path 5)
struct FbUnit {         // per-unit record written by k_fb_pdecode / k_fb_decode
    uint64_t start;     // stream bit of the unit's first token (a block header, or a token
                        // boundary inside a block: region and repair units)
    uint64_t end;       // stream bit where it stopped: past its last block, or (soft stop) the
                        // first token boundary at or past its stop
    uint64_t size;      // output bytes
    uint64_t hdr;       // state at `end`: FB_AT_HEADER, else the code in force (FB_STATE_*)
    uint32_t ntok;      // token words
    uint32_t flags;     // SEGF_*
};
static_assert(sizeof(FbUnit) == 40, "FbUnit is shared with the kernels");
// Units and their stops (path 5).  stops[u]: the stream bit where unit u ends, with
constexpr uint64_t FB_STOP_WEAK = 1ull << 63;  // a stored-header (weak) unit
constexpr uint64_t FB_STOP_SOFT = 1ull << 62;  // the next unit starts inside a block: end at the
                                               // first token boundary at or past the stop
constexpr uint64_t FB_STOP_REGION = 1ull << 61;  // the head of a long gap between dynamic-header
                                                 // starts: a first block that is not dynamic ends
                                                 // the unit at once (the region map decodes the run)
constexpr uint64_t FB_STOP_MASK = FB_STOP_REGION - 1;
// A code state (FbUnit.hdr, the per-unit vhdr): the stream bit of the dynamic block header whose
// code is in force, or FB_STATE_FIXED for the fixed code; FB_STATE_FINAL: that block has BFINAL.
constexpr uint64_t FB_STATE_FIXED = 1ull << 62;
constexpr uint64_t FB_STATE_FINAL = 1ull << 61;
constexpr uint64_t FB_STATE_POS = FB_STATE_FINAL - 1;
constexpr uint64_t FB_AT_HEADER = ~0ull;       // the unit ended at a block header
// how a unit starts (vmode)
enum : uint8_t {
    FB_V_HEADER = 0,   // at a block header (bit 0, a scanned dynamic or stored header)
    FB_V_EXACT = 2,    // exactly at its start bit inside a block whose code is vhdr (a repair)
};
constexpr uint32_t SEGF_SOFT = 1u << 30;  // internal: decode_huffman reached the soft stop
// FbUnit flag (not an error): the unit's decode passed at least one block header after its
// start (diagnostics)
constexpr uint32_t SEGF_CROSSED = 1u << 29;
constexpr uint32_t SEGF_ERRORS = ~(SEGF_FINAL | SEGF_CROSSED);
// a scan candidate that failed the full header test (k_fb_check)
constexpr uint64_t FB_HIT_REJECT = 1ull << 63;
// the region walk's outcome per region (rstat of launch_fb_regions)
constexpr uint32_t FB_REGION_END = 0x80000001u, FB_REGION_LINK = 0x80000002u;

}  // namespace dmx
