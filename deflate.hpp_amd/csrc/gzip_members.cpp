// gzip_members.cpp -- the chain walk and the cut rule of dmx_inflate_gzip_members (gzip_members.h).
// Plain C++, no HIP; tests/cpp/gzip_members_test.cpp includes this file.
#include "gzip_members.h"

namespace dmx {

uint64_t gzm_cand_at(const GzmCand* cands, uint64_t ncand, uint64_t at) {
    uint64_t lo = 0, hi = ncand;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (cands[mid].off < at) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

GzmWalk gzm_walk(const GzmCand* cands, const GzmRec* recs, uint64_t ncand, uint64_t n, uint64_t from,
                 std::vector<GzmRow>* rows, std::vector<GzmGap>* gaps) {
    if (from > n) return GzmWalk{DMX_ERR_OVERREAD, ncand, from};
    uint64_t p = from;
    for (;;) {
        if (p == n) return GzmWalk{GZM_DONE, ncand, p};
        const uint64_t k = gzm_cand_at(cands, ncand, p);
        if (p == 0 && (k == ncand || cands[k].off != 0)) return GzmWalk{GZM_BAD_START, ncand, 0};
        if (k == ncand) {
            gaps->push_back(GzmGap{p, n});
            return GzmWalk{GZM_DONE, ncand, p};
        }
        const GzmCand c = cands[k];
        if (c.off > p) gaps->push_back(GzmGap{p, c.off});
        const GzmRec r = recs[k];
        if (r.cut) return GzmWalk{GZM_LONG, k, c.off};
        if (r.status != DMX_OK) return GzmWalk{r.status, k, c.off};
        if (r.end > n || n - r.end < 8) return GzmWalk{DMX_ERR_OVERREAD, k, c.off};
        rows->push_back(GzmRow{c.off, c.head, r.end, r.plain});
        p = r.end + 8;
    }
}

GzmCut gzm_first_cut(const GzmCand* cands, uint64_t ncand, uint64_t k, uint64_t n, uint64_t limit) {
    uint64_t idx = gzm_cand_at(cands, ncand, cands[k].off + cands[k].head + limit);
    if (idx <= k) idx = k + 1;  // (limit == 0 and an empty header cannot happen; the cut lies behind k)
    return GzmCut{idx < ncand ? idx : ncand, idx < ncand ? cands[idx].off : n};
}

bool gzm_next_cut(const GzmCand* cands, uint64_t ncand, uint64_t n, GzmCut* c) {
    if (c->idx >= ncand) return false;
    c->idx++;
    c->end = c->idx < ncand ? cands[c->idx].off : n;
    return true;
}

}  // namespace dmx
