// bgzf_chain.h -- the member chain of a BGZF file, found in parallel: the steps the kernels of
// bgzf_chain.hip run, one call per "thread".  Plain C++, no HIP (DMX_HD as in container_parse.h):
// tests/cpp/bgzf_chain_test.cpp runs the same calls serially and compares with the serial
// bgzf_next walk.
//
//   1. candidates  every offset where bgzf_next succeeds, in offset order (bgzf_candidate)
//   2. links       a candidate's successor is the candidate at off + size (bgzf_link)
//   3. doubling    level k + 1 holds the 2^(k+1)-th successor (bgzf_double)
//   4. length      the members reachable from candidate 0, which must sit at offset 0
//                  (bgzf_chain_length); false candidates inside payloads are never counted,
//                  whatever chains they form among themselves
//   5. rank        member r is reached from candidate 0 along the bits of r (bgzf_rank_lookup)
//   6. end         DMX_OK when the last member ends at n, else bgzf_next's verdict at the offset
//                  where the chain breaks (bgzf_chain_status)
//
// No function here reads a byte at or beyond in + n.
#pragma once
#include "container_parse.h"

namespace dmx {

constexpr uint32_t kBgzfEnd = 0xFFFFFFFFu;   // link: the member ends exactly at n
constexpr uint32_t kBgzfNone = 0xFFFFFFFEu;  // link: no member starts where this one ends
// (a link below kBgzfNone is a candidate index: the lists hold fewer than 2^32 - 2 candidates)

struct BgzfCand {
    uint64_t off;          // the member is [off, off + size)
    uint32_t size, isize;  // BSIZE + 1; the trailer's ISIZE
};
static_assert(sizeof(BgzfCand) == 16, "candidate lists are arrays of 16-byte records");

// the first four bytes of a member (little-endian word): 1f 8b 08 and FLG with FEXTRA
DMX_HD inline bool bgzf_magic(uint32_t w) { return (w & 0x04FFFFFFu) == 0x04088B1Fu; }

// The candidate predicate: bgzf_next itself, so kernel and host walk agree by construction.
DMX_HD inline bool bgzf_candidate(const uint8_t* in, uint64_t n, uint64_t off, BgzfCand* c) {
    BgzfMember m;
    if (bgzf_next(in, n, off, &m) != DMX_OK) return false;
    c->off = off;
    c->size = (uint32_t)m.size;  // BSIZE + 1 <= 65536
    c->isize = m.isize;
    return true;
}

// The link rule.  size >= head + 8 > 0: the successor lies behind candidate i.
DMX_HD inline uint32_t bgzf_link(const BgzfCand* cands, uint64_t ncand, uint64_t i, uint64_t n) {
    const uint64_t target = cands[i].off + cands[i].size;
    if (target == n) return kBgzfEnd;
    uint64_t lo = i + 1, hi = ncand;  // the first candidate at or behind target
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (cands[mid].off < target) lo = mid + 1;
        else hi = mid;
    }
    return (lo < ncand && cands[lo].off == target) ? (uint32_t)lo : kBgzfNone;
}

// Jump levels for ncand candidates: a chain has at most ncand - 1 hops = 2^levels - 1.
DMX_HD inline uint32_t bgzf_levels(uint64_t ncand) {
    uint32_t k = 1;
    while (k < 32 && (1ull << k) < ncand) k++;
    return k;
}

// One doubling step: Jk[i] is the 2^k-th successor of i (or END / NONE when the chain is
// shorter); the result is the 2^(k+1)-th.
DMX_HD inline uint32_t bgzf_double(const uint32_t* Jk, uint64_t i) {
    const uint32_t j = Jk[i];
    return j >= kBgzfNone ? j : Jk[j];
}

// The members reachable from candidate 0 (J: levels tables of ncand links, level k at
// J + k * ncand); *last is the last one.  The caller has checked that candidate 0 is at offset 0.
DMX_HD inline uint64_t bgzf_chain_length(const uint32_t* J, uint64_t ncand, uint32_t levels, uint32_t* last) {
    uint32_t cur = 0;
    uint64_t len = 1;
    for (uint32_t k = levels; k-- > 0;) {
        const uint32_t j = J[(uint64_t)k * ncand + cur];
        if (j < kBgzfNone) {
            cur = j;
            len += 1ull << k;
        }
    }
    *last = cur;
    return len;
}

// Member r < length: the candidate r hops behind candidate 0.
DMX_HD inline uint32_t bgzf_rank_lookup(const uint32_t* J, uint64_t ncand, uint32_t levels, uint64_t r) {
    uint32_t cur = 0;
    for (uint32_t k = 0; k < levels; k++)
        if ((r >> k) & 1) cur = J[(uint64_t)k * ncand + cur];
    return cur;
}

// The chain's members and status, as the serial walk `for (off = 0; off < n;) bgzf_next(...)`
// reports them: *members counts the members before the walk stops.
DMX_HD inline int bgzf_chain_status(const uint8_t* in, uint64_t n, const BgzfCand* cands, uint64_t ncand,
                                    const uint32_t* J, uint32_t levels, uint64_t* members) {
    BgzfMember m;
    *members = 0;
    if (n == 0) return DMX_OK;
    if (ncand == 0 || cands[0].off != 0) return bgzf_next(in, n, 0, &m);  // (not DMX_OK: 0 is no candidate)
    uint32_t last = 0;
    *members = bgzf_chain_length(J, ncand, levels, &last);
    if (J[last] == kBgzfEnd) return DMX_OK;
    // no candidate where the last member ends: the serial walk stops there with this verdict
    const int rc = bgzf_next(in, n, cands[last].off + cands[last].size, &m);
    return rc != DMX_OK ? rc : DMX_ERR_DATA;  // (DMX_OK cannot happen: it would be a candidate)
}

}  // namespace dmx
