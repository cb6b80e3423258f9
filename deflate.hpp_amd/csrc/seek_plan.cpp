// seek_plan.cpp -- seek_select and seek_range_plan (seek_plan.h).  Plain C++, no HIP.
#include "seek_plan.h"

#include <algorithm>

namespace dmx {

std::vector<dmx_seek_entry> seek_select(const SeekCand* cands, uint64_t ncand, uint64_t spacing) {
    std::vector<dmx_seek_entry> e;
    e.push_back(dmx_seek_entry{0, 0, 0, DMX_SEEK_NOWINDOW});
    uint64_t last = 0;
    for (uint64_t i = 0; i < ncand; i++) {
        const SeekCand& c = cands[i];
        if (c.uoffset < last || c.uoffset - last < spacing) continue;
        e.push_back(dmx_seek_entry{c.bit, c.uoffset, c.nowindow ? 0u : DMX_SEEK_WINDOW,
                                   c.nowindow ? DMX_SEEK_NOWINDOW : 0u});
        last = c.uoffset;
    }
    return e;
}

int seek_range_plan(const dmx_seek_entry* entries, uint64_t count, uint64_t n, uint64_t uoffset, uint64_t len,
                    std::vector<SeekSpan>* spans) {
    spans->clear();
    if (!entries || count == 0) return DMX_ERR_ARG;
    const dmx_seek_entry& end = entries[count];
    if (n > (~0ull >> 3) || end.bit > 8 * n) return DMX_ERR_ARG;
    for (uint64_t k = 0; k < count; k++) {
        if (k + 1 < count ? entries[k + 1].uoffset <= entries[k].uoffset : end.uoffset < entries[k].uoffset)
            return DMX_ERR_ARG;
        if (!(entries[k].flags & DMX_SEEK_NOWINDOW) && entries[k].window != DMX_SEEK_WINDOW) return DMX_ERR_ARG;
    }
    if (uoffset < entries[0].uoffset || uoffset > end.uoffset || len > end.uoffset - uoffset) return DMX_ERR_ARG;
    if (!len) return DMX_OK;
    // the entries that overlap [u0, u1): from the last one that starts at or before u0 up to the
    // first entry (or the sentinel) at or behind u1
    const uint64_t u0 = uoffset, u1 = uoffset + len;
    const dmx_seek_entry* const e = entries + count;
    const uint64_t k0 = (uint64_t)(std::upper_bound(entries, e, u0, [](uint64_t u, const dmx_seek_entry& x) {
                                       return u < x.uoffset;
                                   }) - entries) - 1;
    const uint64_t k1 = (uint64_t)(std::lower_bound(entries, e + 1, u1, [](const dmx_seek_entry& x, uint64_t u) {
                                       return x.uoffset < u;
                                   }) - entries);
    spans->reserve(k1 - k0);
    for (uint64_t k = k0; k < k1; k++) {
        const uint64_t uk = entries[k].uoffset, un = entries[k + 1].uoffset;
        SeekSpan s{};
        s.bit = entries[k].bit;
        s.limit = (un < u1 ? un : u1) - uk;
        s.skip = k == k0 ? u0 - uk : 0;
        s.out_off = (uk > u0 ? uk : u0) - u0;
        s.slot = k;
        s.window = (entries[k].flags & DMX_SEEK_NOWINDOW) ? 0u : DMX_SEEK_WINDOW;
        spans->push_back(s);
    }
    return DMX_OK;
}

}  // namespace dmx
