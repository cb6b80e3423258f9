// inflate_plan.cpp -- the inflate planners (inflate_plan.h): pure functions of host arrays.
#include "inflate_plan.h"

#include <algorithm>
#include <string_view>

#include "../../include/dmx.h"

namespace dmx {

// Plan: the lane decoder (one lane per segment decodes tokens, one wave per segment
// resolves them; segment j lands at j * seg) with a patch pass of the exact wave decoder
// for the candidates it declines; then the older workgroup-per-segment decoder with both
// segment sizes; then the wave-per-segment decoder, which places segments of any size
// <= 32 KiB by look-back.  Each pass runs only if the previous one reported status 1 (a
// segment outside its layout or sizes not uniform); status 2 goes to the serial decoder.
//
// Heavy candidates (mode 6): a lane decodes about one symbol per 1000 cycles, so the lane
// decoder takes as long as the serial decode of the densest segment in a wave (a 24 MiB
// bitmap: 6 ms for ~10K symbols).  Candidates spanning more than heavy_bytes compressed
// bytes go to the workgroup decoder instead (k_inflate_pj: the segment's bits split over 512
// lanes, ~0.17 ms per dense segment on one CU): always up to 2048 candidates, beyond that
// when the device-side count finds at most 32 per CU (32 rounds of workgroups, ~5.5 ms;
// more dense segments than that keep the lanes' throughput: 1 GiB of text).
// A stream of at most one candidate per CU takes one round of workgroups, which beats the
// lanes' ~0.3 ms floor (a wave's header, table and token phases) from 256 bytes up.
PassPlan inflate_pass_plan(uint32_t seg, uint64_t n, uint64_t ncand, int forced, uint32_t heavy_bytes, int ncu,
                           bool lanes_ok, bool heavy_ok, bool parallel_ok) {
    PassPlan p;
    const bool heavy_env = heavy_bytes != 0;  // developer A/B (dmx_config.dev_heavy_bytes)
    const bool few_bits = n / ncand < 4096;
    if (plan_wants_lanes(forced) && lanes_ok) {
        p.add(4, seg);
        if (plan_wants_heavy(seg, ncand) && heavy_ok) {
            p.heavy = (!heavy_env && ncand <= (uint64_t)ncu) ? 256u : heavy_env ? heavy_bytes : 2048u;
            p.heavy_limit = ncand <= 2048 ? 0xFFFFFFFFu : 32u * (uint32_t)std::max(ncu, 1);
            p.add(6, seg);  // the heavy candidates
        }
        p.add(3, seg);  // patch the declined candidates
    }
    if (forced == 0 || forced == 1) {
        p.add((uint32_t)forced, 0);
    } else if (forced != 4) {
        if (few_bits && forced != 2) {
            p.add(0, 0);
        } else if (seg <= 32768) {  // (the workgroup decoder's slots are 16 or 32 KiB)
            p.add(2, seg);
            p.add(3, seg);
            p.add(2, seg == 32768 ? 16384u : 32768u);
            p.add(3, seg == 32768 ? 16384u : 32768u);
        }
    }
    if (forced != 1 && forced != 4) p.add(1, 0);
    if (!parallel_ok) p.np = 0;
    // no marker in a large stream: not libdmx's segment layout, the block-parallel path next
    if (ncand == 1 && n > 65536 && forced == -1) p.np = 0;
    if (forced == 5 || forced == 7) p.np = 0;  // 7: the serial decoder alone
    return p;
}

SpecKnob spec_knob(const char* e) {
    if (!e) return SpecKnob::On;
    const std::string_view s(e);
    if (s == "0") return SpecKnob::Off;
    if (s == "force") return SpecKnob::Force;
    return SpecKnob::On;
}

bool spec_wanted(SpecKnob knob, bool fixed_out, bool piece, bool diag, int forced, uint32_t seg, uint64_t cap) {
    if (knob == SpecKnob::Off || !fixed_out || piece || diag || seg == 0) return false;
    if (!plan_wants_lanes(forced)) return false;
    return knob == SpecKnob::Force || cap / seg > kSpecMinCands;
}

SpecVerdict spec_decide(const PassPlan& spec, const PassPlan& classic, uint64_t ncand, uint64_t ncap, int32_t status,
                        uint64_t exotic) {
    if (ncand > ncap || ncand <= kSpecMinCands) return SpecVerdict::Discard;
    if (spec.np == 0 || classic.np == 0 || spec.pass[0][0] != 4) return SpecVerdict::Discard;
    if (classic.pass[0][0] != spec.pass[0][0] || classic.pass[0][1] != spec.pass[0][1] || classic.heavy != spec.heavy ||
        classic.heavy_limit != spec.heavy_limit)
        return SpecVerdict::Discard;
    if (status == 0) return SpecVerdict::Accept;
    if (status != 1) return SpecVerdict::Discard;  // nothing the segmented passes settle: as today, from the start
    return pass_ends_plan(4, 4, status, exotic) ? SpecVerdict::Accept : SpecVerdict::Continue;
}

SegChain seg_chain_walk(const SegRecord* recs, const uint64_t* cands, uint64_t ncand) {
    SegChain c;
    uint64_t k = 0;
    for (;;) {
        const SegRecord& s = recs[k];
        if (s.flags & ~SEGF_FINAL) break;
        c.chain.push_back(k);
        c.offsets.push_back(c.total);
        c.sizes.push_back(s.out_size);
        c.total += s.out_size;
        if (s.flags & SEGF_FINAL) {
            c.ok = true;
            break;
        }
        const uint64_t* const it = std::lower_bound(cands + k + 1, cands + ncand, s.end_byte);
        if (it == cands + ncand || *it != s.end_byte) break;
        k = (uint64_t)(it - cands);
    }
    return c;
}

// units: bit 0, then every hit (sorted: chunks in order, lanes in order within a chunk);
// dynamic-header hits are "strong" (practically never false), stored-header hits "weak".
// A gap of more than kRegionGap bits between two strong starts is a run of blocks the scan
// cannot split (fixed-code blocks -- zlib's Z_FIXED, the reference's own level-1/2 chunks --
// or one huge block).  Its head unit decodes only a dynamic first block (and what follows
// it up to the first far fixed-code header, FB_STOP_REGION); from where it stops, E, to the
// next strong start T the region map (k_fb_smap / k_fb_swalk) finds the exact token path,
// and one unit per 2^18 bits starts exactly on it.  The chain walk below verifies every link
// (end bit and code state); a break gets a repair unit that starts exactly there.
void FbPlan::from_hits(const uint64_t* hits, uint64_t nhits) {
    const uint64_t kRegionGap = geom.super_bits + geom.super_bits / 2;
    starts.assign(1, 0);
    strong.assign(1, 1);
    for (uint64_t i = 0; i < nhits; i++) {
        const uint64_t h = hits[i];
        if (h & FB_HIT_REJECT) continue;
        const uint64_t b = h & ~kStored;
        if (b > starts.back()) {
            starts.push_back(b);
            strong.push_back((h & kStored) ? 0 : 1);
        }
    }
    K = Ku = starts.size();
    stops.assign(K, 0);
    uint64_t next_strong = FB_STOP_MASK;
    for (uint64_t k = K; k-- > 0;) {
        stops[k] = next_strong;
        if (!strong[k]) stops[k] |= FB_STOP_WEAK;
        else if (std::min(next_strong, nbits) - starts[k] > kRegionGap) stops[k] |= FB_STOP_REGION;
        if (strong[k]) next_strong = starts[k];
    }
}

// Token words: up to where a unit can stop, plus room for the block that crosses its stop.
// A token word takes at least 1.5 bits of stream: a match at least 2 (a lit/len and a
// distance code, each at least 1 bit), a word of literals up to three of them; the densest
// packing is a 1-bit literal then a 2-bit match, two words per 3 bits -- so 2/3 of a word per
// bit always suffices (C3 uses 0.37).  A weak unit with a hard stop (a stored block -- two
// words -- then possibly fixed-code blocks up to the next dynamic one) gets 64 Ki words; a
// region head at most its staged first block.  A unit that fills its space stops softly and
// a repair unit continues it.  Inside a fixed-code region a token word covers at least 7 bits
// (fixed codes are 7-9 bits, three literals per word), so a third of a word per bit
// (region_words).  16-B groups.
uint64_t FbPlan::words_of(uint64_t pos, uint64_t stop) const {
    const uint64_t s = std::min<uint64_t>(stop & FB_STOP_MASK, nbits), p = std::min(pos, nbits);
    uint64_t w = 4096 + 65536;
    if (stop & FB_STOP_REGION) w = std::min<uint64_t>(2 * (s - p) / 3, 458752 + 65536) + 4096;
    else if (!(stop & FB_STOP_WEAK)) w = 2 * (s - p) / 3 + 4096;
    return (w + 63) & ~63ull;
}

void FbPlan::budgets() {
    // region budget: every long gap could become one region of units, each with a repair
    uint64_t reg_budget = 0, reg_units_max = 0;
    for (uint64_t k = 0; k < K; k++)
        if (stops[k] & FB_STOP_REGION) {
            const uint64_t span = std::min(stops[k] & FB_STOP_MASK, nbits) - starts[k];
            const uint64_t nu = span / geom.super_bits + 2;
            reg_units_max += nu;
            reg_budget += span / 3 + nu * (4096 + 64);
        }
    R = 2 * std::max<uint64_t>(256, K + reg_units_max);  // repair units
    Kcap = K + reg_units_max + R;
    tokoff.assign(Kcap + 1, 0);
    starts.resize(Kcap);
    vhdr.assign(Kcap, 0);
    vmode.assign(Kcap, FB_V_HEADER);
    ucb.assign(Kcap, ~0u);
    stops.resize(Kcap);
    units.assign(Kcap, FbUnit{});
    for (uint64_t k = 0; k < K; k++) tokoff[k + 1] = tokoff[k] + words_of(starts[k], stops[k]);
    rep_words = std::min<uint64_t>(tokoff[K] + 2 * reg_budget + 4096 * R, 1ull << 29);
    rep_used = 0;
}

// ---- fixed-code regions ----
void FbPlan::select_regions() {
    regs.clear();
    nsb = 0;
    for (uint64_t k = 0; k < K; k++) {
        if (!(stops[k] & FB_STOP_REGION)) continue;
        const FbUnit& u = units[k];
        if ((u.flags & (SEGF_ERRORS | SEGF_FINAL)) || u.hdr != FB_AT_HEADER) continue;
        const uint64_t T = std::min(stops[k] & FB_STOP_MASK, nbits);
        if (u.end >= T || T - u.end <= geom.super_bits) continue;  // a repair unit takes the rest
        const uint64_t m = (T - u.end + geom.super_bits - 1) / geom.super_bits;
        regs.push_back({u.end, T, nsb, m});
        nsb += m;
    }
}

FbRegionUnits FbPlan::region_units(const uint32_t* vis) {
    std::vector<uint8_t> in_region(K, 0);
    const uint64_t ch = geom.chunk_bits, nreg = regs.size();
    for (uint64_t r = 0; r < nreg; r++) {
        const uint32_t rs = vis[nsb + r];
        // A failed walk (the map met a dynamic header that was not a listed start, a
        // stored block past T, ...): the super blocks it visited before failing are still
        // on the true path, so they keep their units; the last one decodes on towards T
        // (through the unlisted block, as far as its token space goes) and repair units
        // take the rest -- only that span loses parallelism, not the stream.
        const bool walked = rs == FB_REGION_END || rs == FB_REGION_LINK;
        const uint64_t first = Ku;
        for (uint64_t j = 0; j < regs[r].nsb; j++) {
            const uint32_t v = vis[regs[r].sb0 + j];
            if (v == ~0u) continue;
            if (Ku >= Kcap) return {false, r + 1, false, Ku};
            const bool head = Ku == first;
            starts[Ku] = regs[r].E + (uint64_t)(v >> 6) * ch + (v & 31u);
            vmode[Ku] = head ? FB_V_HEADER : FB_V_EXACT;
            vhdr[Ku] = head ? 0 : (FB_STATE_FIXED | ((v >> 5) & 1u ? FB_STATE_FINAL : 0ull));
            ucb[Ku] = (uint32_t)((regs[r].sb0 + j) * 64);  // its super block's first chunk
            Ku++;
        }
        for (uint64_t k = first; k < Ku; k++) {
            stops[k] = k + 1 < Ku ? (starts[k + 1] | FB_STOP_SOFT) : regs[r].T;
            const uint64_t w = k + 1 < Ku || walked ? region_words(std::min(stops[k] & FB_STOP_MASK, nbits) - starts[k])
                                                    : std::min(words_of(starts[k], stops[k]), kOpenWords);
            if (rep_used + w > rep_words) return {false, r + 1, true, k};
            tokoff[k + 1] = tokoff[k] + w;
            rep_used += w;
            prim.push_back({starts[k], (uint8_t)(k == first ? 0 : 2)});
        }
        // weak starts inside the region: superseded
        for (uint64_t k = (uint64_t)(std::upper_bound(starts.begin(), starts.begin() + K, regs[r].E) - starts.begin());
             k < K && starts[k] < regs[r].T; k++)
            in_region[k] = 1;
    }
    for (uint64_t k = 0; k < K; k++)
        if (!in_region[k]) prim.push_back({starts[k], (uint8_t)(strong[k] ? 0 : 1)});
    std::sort(prim.begin(), prim.end(), [](const Prim& a, const Prim& b) { return a.pos < b.pos; });
    return {true, nreg, false, 0};
}

uint64_t FbPlan::stop_of(uint64_t pos) const {
    auto it = std::upper_bound(prim.begin(), prim.end(), pos, [](uint64_t p, const Prim& q) { return p < q.pos; });
    if (it != prim.end() && it->kind == 2) return it->pos | FB_STOP_SOFT;
    for (; it != prim.end(); ++it)
        if (it->kind != 1) return it->pos;
    return FB_STOP_MASK;
}

// A unit that starts on the chain (at bit 0, or exactly where the chain's last unit ended, in
// the code state it ended in) decodes the stream's own blocks from there, so an over-read or
// an undecodable code it reports is the error realDecompress meets (inflate.hpp:277-322):
// the stream ends with that error at once instead of a serial re-decode from bit 0 to find
// it again (a truncated 1 GiB stream took ~75 s on the serial decoder).  Only
// pure stream errors count; token space, staging or exotic-layout flags are this decoder's
// own limits and still go to the serial decoder.
static int stream_error(const FbUnit& u) {
    constexpr uint32_t kStreamErr = SEGF_OVERREAD | SEGF_ERR_DATA;
    if (!(u.flags & kStreamErr) || (u.flags & ~(kStreamErr | SEGF_CROSSED | SEGF_FINAL))) return DMX_OK;
    return (u.flags & SEGF_OVERREAD) ? DMX_ERR_OVERREAD : DMX_ERR_DATA;  // as k_inflate_serial maps it
}

// chain from bit 0: each unit must end exactly where the next one on the chain starts, in
// the code state that one assumes (a block header, or the code in force and its BFINAL bit).
// Every break -- an end where no such unit starts -- gets a repair unit that starts exactly
// there in that state; the walk goes on optimistically past a break (from the next unit in
// start order), so one round repairs all the breaks it can see.
FbWalk FbPlan::walk(int round) {
    by.clear();
    bad.clear();
    by.reserve(Ku);
    for (uint64_t k = 0; k < Ku; k++) (units[k].flags & SEGF_ERRORS ? bad : by).emplace_back(units[k].start, (uint32_t)k);
    std::sort(by.begin(), by.end());
    std::sort(bad.begin(), bad.end());
    chain.clear();
    coffs.clear();
    csizes.clear();
    total = 0;
    breaks.clear();
    bool fin = false;
    if (units[0].flags & SEGF_ERRORS) {
        if (const int rc = stream_error(units[0])) return {FbWalk::STREAM_ERROR, 0, nullptr, rc, 0};
        return {FbWalk::DECLINE, 0, "unit error", 0, 0};
    }
    uint64_t k = 0;
    for (;;) {
        const FbUnit& u = units[k];
        chain.push_back((uint32_t)k);
        coffs.push_back(total);
        csizes.push_back(u.size);
        total += u.size;
        if (u.flags & SEGF_FINAL) {
            fin = true;
            break;
        }
        const uint64_t state = u.hdr;
        // (several units may start there in that state -- a scanned one, a region unit, a
        // repair: all decode the same tokens, the one that reaches farthest is taken)
        uint64_t best = ~0ull;
        for (auto it = std::lower_bound(by.begin(), by.end(), std::make_pair(u.end, 0u));
             it != by.end() && it->first == u.end; ++it)
            if (it->second != k && expects(it->second) == state &&
                (best == ~0ull || units[it->second].end >= units[best].end))
                best = it->second;
        if (best != ~0ull) {
            k = best;
            continue;
        }
        if (breaks.empty()) {  // the first break: everything before it is the stream's true path
            for (auto it = std::lower_bound(bad.begin(), bad.end(), std::make_pair(u.end, 0u));
                 it != bad.end() && it->first == u.end; ++it)
                if (expects(it->second) == state)
                    if (const int rc = stream_error(units[it->second]))
                        return {FbWalk::STREAM_ERROR, 0, nullptr, rc, it->second};
        }
        breaks.emplace_back(u.end, state);
        // (optimistic: on with the unit after this one in start order)
        auto self = std::lower_bound(by.begin(), by.end(), std::make_pair(u.start, (uint32_t)k));
        if (self == by.end() || self->second != k || ++self == by.end()) break;
        k = self->second;
    }
    if (fin && breaks.empty()) return {FbWalk::DONE, 0, nullptr, 0, 0};
    if (breaks.empty() || round == kRepairRounds || Ku + breaks.size() > Kcap)
        return {FbWalk::DECLINE, 0, fin ? "repairs exhausted" : "no final block", 0, chain.back()};
    std::sort(breaks.begin(), breaks.end());
    breaks.erase(std::unique(breaks.begin(), breaks.end()), breaks.end());
    // repair units, appended at [Ku, Ku + breaks)
    const uint64_t k0 = Ku;
    for (const auto& br : breaks) {
        // a repair that was already made there failed: the serial decoder reports why
        if (std::binary_search(repaired.begin(), repaired.end(), br))
            return {FbWalk::DECLINE, 0, "repair failed", 0, chain.back()};
        const uint64_t e = br.first;
        starts[Ku] = e;
        vmode[Ku] = br.second == FB_AT_HEADER ? FB_V_HEADER : FB_V_EXACT;
        vhdr[Ku] = br.second == FB_AT_HEADER ? 0 : br.second;
        stops[Ku] = stop_of(e);
        // No exact chunk entries for a repair unit, also inside a fixed-code region where the
        // true path's are known: starting its ranges on them measured Z_FIXED 64 MiB text
        // 4.7 -> 4.2 ms but 32 MiB mixed 8.7 -> 13.4 ms (a repair unit after a stored block
        // then ends serially), also with soft stops only.
        ucb[Ku] = ~0u;
        const uint64_t w = (stops[Ku] & FB_STOP_SOFT) ? region_words((stops[Ku] & FB_STOP_MASK) - std::min(e, nbits))
                                                      : std::min(words_of(e, stops[Ku]), kOpenWords);
        if (rep_used + w > rep_words) return {FbWalk::DECLINE, 0, "repair token space", 0, chain.back()};
        tokoff[Ku + 1] = tokoff[Ku] + w;
        rep_used += w;
        Ku++;
    }
    repaired.insert(repaired.end(), breaks.begin(), breaks.end());
    std::sort(repaired.begin(), repaired.end());
    return {FbWalk::REPAIR, k0, nullptr, 0, 0};
}

}  // namespace dmx
