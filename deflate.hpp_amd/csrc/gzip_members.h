// gzip_members.h -- multi-member gzip files (RFC 1952 2.2, dmx_inflate_gzip_members): the records
// the device passes write and the host-side chain walk over them.  Plain C++, no HIP: the walk and
// the cut rule of gzip_members.cpp are what tests/cpp/gzip_members_test.cpp runs on the CPU.
//
// A member's end is known only from a decode, so the device (gzip_members.hip) lists every offset
// that could start a member (GzmCand: 1f 8b 08 and a header that parses) and measures every one of
// them (GzmRec: where its DEFLATE stream ends and how many plain bytes it holds, over a window of
// at most kBatchRouteBytes).  The chain itself -- member k + 1 starts behind member k's trailer and
// the zeros that follow it -- is then a walk over those two lists, which the host does.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/dmx.h"

namespace dmx {

struct GzmCand {
    uint64_t off;   // a header that parses starts here
    uint64_t head;  // its length: the raw stream starts at off + head
};
static_assert(sizeof(GzmCand) == 16, "copied as 16-byte records");

// one candidate's measurement (k_gzm_measure)
struct GzmRec {
    uint64_t end;    // status DMX_OK: the file offset just past the stream's final block
    uint64_t plain;  // status DMX_OK: the stream's plain bytes
    int32_t status;  // DMX_OK, DMX_ERR_DATA or DMX_ERR_OVERREAD
    uint32_t cut;    // the window was shortened to the measuring limit and the decode ran off its
                     // end: a LONG member, not a broken one
    uint64_t pad_;
};
static_assert(sizeof(GzmRec) == 32, "copied as 32-byte records");

struct GzmRow {  // a member on the chain
    uint64_t coff, head, end, plain;  // [coff, end + 8) in the file; the raw stream is [coff + head, end)
};
struct GzmGap {  // [a, b): bytes between a trailer and the next member (or the file's end) -- must be zeros
    uint64_t a, b;
};

// what a walk ended in; a status (DMX_ERR_*, negative) otherwise
enum : int {
    GZM_DONE = 1,       // reached n
    GZM_LONG = 2,       // candidate `k` is on the chain and its record is `cut`
    GZM_BAD_START = 3,  // no member starts at offset 0: the status is the header's at offset 0
};
struct GzmWalk {
    int what;      // GZM_* or the first failing member's status
    uint64_t k;    // GZM_LONG, or a status: the candidate
    uint64_t pos;  // where the walk stood (GZM_LONG: the member's first byte)
};

// The first candidate at or behind file offset `at` (ncand: none); cands are in offset order.
uint64_t gzm_cand_at(const GzmCand* cands, uint64_t ncand, uint64_t at);

// The chain from file offset `from` (0, or the byte behind a long member's trailer): appends the
// members to *rows and the spaces in front of them to *gaps.  From a position p the next member is
// the first candidate at or behind p; [p, its offset) goes on the gap list, or [p, n) when there
// is none, and the walk is done.  A member whose trailer runs past n is DMX_ERR_OVERREAD; a record
// with an error is that error.  Candidates that lie inside a member are never looked at.
GzmWalk gzm_walk(const GzmCand* cands, const GzmRec* recs, uint64_t ncand, uint64_t n, uint64_t from,
                 std::vector<GzmRow>* rows, std::vector<GzmGap>* gaps);

// Where the single-stream decode of the long member at candidate k ends its input: at candidate
// `idx` (offset `end`), or at the file's end (idx == ncand, end == n).
struct GzmCut {
    uint64_t idx, end;
};
// the first cut: the first candidate at or beyond cands[k].off + cands[k].head + limit
GzmCut gzm_first_cut(const GzmCand* cands, uint64_t ncand, uint64_t k, uint64_t n, uint64_t limit);
// After DMX_ERR_OVERREAD from a decode cut at *c: the cut was a false candidate inside the member
// when more of the file lies behind it -- the cut moves to the next candidate (true).  false: the
// cut was the file's end, the member is truncated.
bool gzm_next_cut(const GzmCand* cands, uint64_t ncand, uint64_t n, GzmCut* c);

}  // namespace dmx
