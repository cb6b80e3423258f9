// inflate_plan.h -- the host-side decisions of the inflate paths, free of HIP: which passes the
// segmented plan runs, the path-4 chain walk over the candidates' records, and path 5's units
// (starts, stops, token budgets, region units, the chain walk and its repair rounds).  The
// drivers (host_inflate.cpp, host_fb.cpp) allocate, upload and launch what these decide.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

#include "inflate_records.h"

namespace dmx {

constexpr uint64_t LN_OUT_CAP_BYTES = 32768;  // largest segment output of the lane decoder

// ---- the segmented plan (paths 0-4) -------------------------------------------------------

// token words of the lane decoder (k_lane_caps): min(8 bits, slot / 2 + 2) + 16 words per
// candidate, in groups of four
inline uint64_t lane_tok_words(uint32_t seg, uint64_t ncand, uint64_t n) {
    const uint64_t per = ((LN_OUT_CAP_BYTES > seg ? LN_OUT_CAP_BYTES : seg) / 2 + 2 + 16 + 3) & ~3ull;
    const uint64_t a = ncand * per, b = 8ull * n + 20ull * ncand;
    return a < b ? a : b;
}

struct PassPlan {
    uint32_t pass[8][2];  // {InflateArgs::mode, slot bytes}
    int np = 0;
    uint32_t heavy = 0, heavy_limit = 0;  // mode 6: the lanes decline candidates above `heavy`
                                          // compressed bytes when at most `heavy_limit` are
    void add(uint32_t mode, uint32_t slot) { pass[np][0] = mode, pass[np][1] = slot, np++; }
};
// forced: dmx_config.dev_inflate_pass - 1 (-1 = the plan).  The caller allocates: the lane
// decoder's buffers when plan_wants_lanes (lanes_ok), then the heavy list when
// plan_wants_heavy (heavy_ok); parallel_ok: the output holds every candidate's slot.
inline bool plan_wants_lanes(int forced) { return forced == -1 || forced == 4; }
// (the workgroup decoder of the heavy route takes segments of <= 32 KiB)
inline bool plan_wants_heavy(uint32_t seg, uint64_t ncand) { return seg <= 32768 && ncand < 0xFFFFFFF0ull; }
PassPlan inflate_pass_plan(uint32_t seg, uint64_t n, uint64_t ncand, int forced, uint32_t heavy_bytes, int ncu,
                           bool lanes_ok, bool heavy_ok, bool parallel_ok);
// a pass that has nothing to do after the previous pass's validation (`exotic` candidates declined)
inline bool pass_skipped(uint32_t mode, uint64_t exotic, uint64_t ncand) {
    if (mode == 3) return exotic == 0 || exotic > ncand / 8;  // nothing / too many
    return mode == 6 && exotic == 0;
}
// the plan ends after a pass that validated with `status`
inline bool pass_ends_plan(uint32_t mode, uint32_t lead_mode, int32_t status, uint64_t exotic) {
    if (status != 1) return true;  // 1: not this layout
    // the lane pass decoded every candidate but the segment sizes are not uniform (a shard
    // ending on a short segment, 16 KiB segments): the chain repair places them, the other
    // passes would only decode everything again
    return lead_mode == 4 && exotic == 0 && (mode == 4 || mode == 6 || mode == 3);
}

// ---- the speculative first pass of the synchronous inflate ---------------------------------
// dmx_inflate_device into a caller's buffer launches the marker list, the lane pass and its
// validation before the host knows the candidate count (the kernels stop at the device-side
// count, as in dmx_inflate_device_async), so that the call waits for the GPU once.  The scratch
// is provisioned for cap / segment + 64 candidates: a libdmx stream has one per segment.

// DMX_INFLATE_SPEC (developer knob, read at dmx_create): "0" off, "1" (and unset or unparsable)
// on, "force" on without the capacity gate, so that tests reach every branch at small sizes
enum class SpecKnob : uint8_t { Off, On, Force };
SpecKnob spec_knob(const char* e);
// Up to this many candidates the first pass's heavy threshold and limit depend on the count
// (inflate_pass_plan): no speculation at or below it.
constexpr uint64_t kSpecMinCands = 2048;
// (a marker is four bytes, so an n-byte stream has at most n / 4 + 1 candidates: a capacity far
// above the stream's output does not size the scratch)
inline uint64_t spec_provision(uint32_t seg, uint64_t cap, uint64_t n) {
    const uint64_t by_cap = cap / seg + 64, by_n = n / 4 + 1;
    return by_cap < by_n ? by_cap : by_n;
}
// Whether the call launches its first pass ahead of the count.  fixed_out: the caller supplies
// the output buffer; piece: dmx_inflate_piece_device; diag: a diagnostic that sizes its buffers
// by the count is on (DMX_PHASES, DMX_RECS); forced: dmx_config.dev_inflate_pass - 1.
bool spec_wanted(SpecKnob knob, bool fixed_out, bool piece, bool diag, int forced, uint32_t seg, uint64_t cap);
// What becomes of the speculative pass once the count and its validation are known.
//   spec     the plan made for the provisioned count (its first pass is what ran)
//   classic  the plan for the true count (np = 0 when ncand > ncap: not made)
//   status / exotic: the pass's validation (InflateResult)
// Discard: today's flow runs from the marker list on, as if nothing had been launched.
// Accept: the pass stands as the classic plan's first pass and that plan is over (decoded, or a
// layout the chain repair takes).  Continue: it stands, the classic plan goes on from its second pass.
enum class SpecVerdict : uint8_t { Discard, Accept, Continue };
SpecVerdict spec_decide(const PassPlan& spec, const PassPlan& classic, uint64_t ncand, uint64_t ncap, int32_t status,
                        uint64_t exotic);

// Path-4 chain repair: the walk from candidate 0 over the records of a lane pass.  Each
// segment's end must be a candidate start, up to the first BFINAL; a flag other than
// SEGF_FINAL on a chain member, or an end that is no candidate, ends it not ok.
struct SegChain {
    bool ok = false;
    std::vector<uint64_t> chain, offsets;  // candidate index, output offset
    std::vector<uint32_t> sizes;
    uint64_t total = 0;
};
SegChain seg_chain_walk(const SegRecord* recs, const uint64_t* cands, uint64_t ncand);

// ---- path 5: the block-parallel decode of arbitrary streams -------------------------------

struct FbGeom {  // the region map's geometry (fb_region_*() of inflate_blocks.hip)
    uint64_t super_bits, chunk_bits;
    uint32_t nodes, entries;
};

// the outcome of one chain-walk round
struct FbWalk {
    enum Kind { DONE, REPAIR, DECLINE, STREAM_ERROR } kind;
    uint64_t k0;      // REPAIR: units [k0, Ku) are new -- upload and decode them, then walk again
    const char* why;  // DECLINE: the reason (DMX_FB_DEBUG prints it); the serial decoder takes over
    int err;          // STREAM_ERROR: the DMX_ERR_* code the stream ends with
    uint64_t unit;    // DECLINE / STREAM_ERROR: the unit it happened at
};
// the outcome of the region units
struct FbRegionUnits {
    bool ok;           // false: the serial decoder takes the stream
    uint64_t regions;  // regions visited (all of them when ok)
    bool token_space;  // !ok because the token space ran out at `unit` (else: the unit table)
    uint64_t unit;
};

class FbPlan {
public:
    static constexpr uint64_t kStored = 1ull << 62;  // a hit at a stored-block header
    static constexpr int kRepairRounds = 48;
    // a repair unit (or the last unit of a failed region walk) whose stop is far: at most this
    // many words (>= 6 Mbit of the densest code); when they fill, it stops softly and the next
    // repair round continues it, instead of reserving 2/3 of a word per bit up to the stop
    static constexpr uint64_t kOpenWords = (1ull << 22) + 4096;
    struct Reg {
        uint64_t E, T, sb0, nsb;
    };

    FbPlan(uint64_t n_bytes, const FbGeom& g) : geom(g), nbits(8ull * n_bytes) {}

    // the phases, in order
    void from_hits(const uint64_t* hits, uint64_t nhits);  // the scanned units [0, K) and their stops
    void budgets();         // tokoff[0..K], R, Kcap, rep_words; sizes the per-unit arrays for Kcap
    void select_regions();  // regs / nsb from the first pass's records units[0, K)
    FbRegionUnits region_units(const uint32_t* vis);  // vis: nsb visit words, then one status per region
    FbWalk walk(int round);  // over units[0, Ku)

    uint64_t words_of(uint64_t pos, uint64_t stop) const;
    static uint64_t region_words(uint64_t span) { return ((span / 3 + 4096) + 63) & ~63ull; }
    // the stop of a repair unit at pos: a soft stop at the next region unit, else the next
    // strong start (or region head)
    uint64_t stop_of(uint64_t pos) const;
    // the code state a unit assumes at its start: FB_AT_HEADER, or the code in force
    uint64_t expects(uint64_t k) const { return vmode[k] == FB_V_HEADER ? FB_AT_HEADER : vhdr[k]; }

    const FbGeom geom;
    const uint64_t nbits;
    uint64_t K = 0, Ku = 0, Kcap = 0;  // scanned units, units so far, the most there can be
    uint64_t R = 0;                    // repair units provided for
    uint64_t rep_words = 0, rep_used = 0;  // token words past tokoff[K]: provided / given out
    // per unit (Kcap entries after budgets()): what the decode kernels read ...
    std::vector<uint64_t> starts, stops, vhdr, tokoff;
    std::vector<uint8_t> vmode;
    std::vector<uint32_t> ucb;  // region units: the first global chunk of their super block
    // ... and write (the driver copies the records of every decoded batch here)
    std::vector<FbUnit> units;
    std::vector<uint8_t> strong;  // scanned units: a dynamic-header start
    std::vector<Reg> regs;  // the fixed-code regions (select_regions)
    uint64_t nsb = 0;       // super blocks of all regions
    // the chain of the last walk
    std::vector<uint32_t> chain;
    std::vector<uint64_t> coffs, csizes;
    uint64_t total = 0;

private:
    // Sorted list of the starts a repair unit stops at: the scanned ones (a weak start inside a
    // region is superseded by the region's units) and the region units' (soft: inside a block,
    // except the region head E, a block header).
    struct Prim {
        uint64_t pos;
        uint8_t kind;  // 0 strong / region head, 1 weak, 2 soft
    };
    std::vector<Prim> prim;
    std::vector<std::pair<uint64_t, uint64_t>> repaired;  // (end bit, state) already given a repair unit
    std::vector<std::pair<uint64_t, uint32_t>> by, bad;   // (start, unit) decoded without / with an error
    std::vector<std::pair<uint64_t, uint64_t>> breaks;    // (end bit, code state)
};

}  // namespace dmx
