// host_members.cpp -- files made of framed members (see include/dmx.h): BGZF on host buffers and
// in device memory (the member chain, ranged reads), and multi-member gzip.  Both decode a
// device-resident list of members through members_decode_locked; the batch drivers underneath
// are host_batch.cpp's (dmx_ctx.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "dmx_ctx.h"

using namespace dmx;

namespace {

const uint8_t kBgzfEof[kBgzfEofBytes] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                                         0x02, 0,    0x1b, 0,    0x03, 0, 0, 0, 0, 0,    0,    0, 0,    0};

// The BGZF deflate's batch: block i of in[0, n) into slot i of `slots` (host or device memory)
struct BgzfSlots {
    size_t nblk, slot;
    std::vector<const uint8_t*> ins;
    std::vector<uint8_t*> outs;
    std::vector<size_t> ns, caps;
    std::vector<dmx_batch_result> res;
    explicit BgzfSlots(size_t n)
        : nblk((n + kBgzfBlock - 1) / kBgzfBlock), slot(dmx_batch_framed_bound(DMX_FRAME_BGZF, kBgzfBlock)) {}
    void fill(const uint8_t* in, size_t n, uint8_t* slots) {  // (may throw std::bad_alloc)
        ins.resize(nblk);
        outs.resize(nblk);
        ns.resize(nblk);
        caps.assign(nblk, slot);
        res.resize(nblk);
        for (size_t i = 0; i < nblk; i++) {
            ins[i] = in + i * kBgzfBlock;
            ns[i] = std::min<size_t>(kBgzfBlock, n - i * kBgzfBlock);
            outs[i] = slots + i * slot;
        }
    }
};

// ---- BGZF files in device memory (bgzf_chain.hip) ---------------------------------------------

// The member chain of d_in[0, n), found on the device; two host synchronisations (the candidate
// count sizes the scratch; then the member count, the plain bytes and the chain status).
struct BgzfChain {
    uint64_t members = 0, total = 0;
    int status = DMX_OK;
    BgzfCand* rows = nullptr;     // device: members entries, chain order
    uint64_t* uoff = nullptr;     // device: their output offsets
    BgzfChainHead* head = nullptr;
};
int bgzf_chain_locked(dmx_ctx* c, const uint8_t* d_in, size_t n, hipStream_t st, BgzfChain* ch) {
    if (!n) return DMX_OK;  // no member, DMX_OK
    ScanScratch S;
    if (!S.carve(c, scan_tiles(d_in, n), sizeof(BgzfChainHead))) return DMX_ERR_NOMEM;
    ch->head = reinterpret_cast<BgzfChainHead*>(S.words);
    // (links are 32-bit candidate indices)
    const int rc = S.count(launch_bgzf_count(d_in, n, S.counts, S.offs, S.d_ncand, st), kBgzfNone, st);
    if (rc != DMX_OK) return rc;
    const uint64_t ncand = S.ncand;
    const uint32_t levels = bgzf_levels(ncand);
    const size_t off_rows = up16(ncand * sizeof(BgzfCand)), off_J = off_rows * 2;
    const size_t off_isz = off_J + up16((size_t)levels * ncand * 4), off_uoff = off_isz + up16(ncand * 4);
    if (!c->bgzc.ensure(off_uoff + scan_words(ncand) * 8)) return DMX_ERR_NOMEM;
    uint8_t* const cb = c->bgzc.as<uint8_t>();
    ch->rows = reinterpret_cast<BgzfCand*>(cb + off_rows);
    ch->uoff = reinterpret_cast<uint64_t*>(cb + off_uoff);
    HIPCHK(launch_bgzf_chain(d_in, n, S.offs, ncand, reinterpret_cast<BgzfCand*>(cb),
                             reinterpret_cast<uint32_t*>(cb + off_J), ch->rows,
                             reinterpret_cast<uint32_t*>(cb + off_isz), ch->uoff, ch->head, st));
    BgzfChainHead h{};
    HIPCHK(hipMemcpyAsync(&h, ch->head, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ch->members = h.members;
    ch->total = h.total;
    ch->status = h.status;
    return DMX_OK;
}

// ---- the decode of a device-resident list of framed members -------------------------------------

// Its scratch for `count` members at `base` (16-byte aligned; null: for `bytes` alone):
//   desc | order | results | tickets (decode, checksum) | side | key
// member_tab is the only place that knows this layout.
struct MemberTab {
    InflateBatchDesc* desc;
    uint32_t* order;
    dmx_batch_result* res;
    unsigned int* ticket;
    FrameHead* side;
    unsigned long long* key;
    size_t list_bytes;  // desc | order: what a list built on the host uploads in one copy
    size_t bytes;
};
MemberTab member_tab(uint8_t* base, size_t count) {
    const size_t off_order = count * sizeof(InflateBatchDesc), off_res = off_order + up16(count * 4);
    const size_t off_ticket = off_res + count * sizeof(dmx_batch_result), off_side = off_ticket + 32;
    const size_t off_key = off_side + count * sizeof(FrameHead);
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    return MemberTab{reinterpret_cast<InflateBatchDesc*>(b),
                     reinterpret_cast<uint32_t*>(b + off_order),
                     reinterpret_cast<dmx_batch_result*>(b + off_res),
                     reinterpret_cast<unsigned int*>(b + off_ticket),
                     reinterpret_cast<FrameHead*>(b + off_side),
                     reinterpret_cast<unsigned long long*>(b + off_key),
                     off_res,
                     off_key + 16};
}

// The framed batch inflate over arrays that are already on the device: `build` fills T.desc and
// T.order with `count` members (path 6 throughout: every member is below kBatchRouteBytes),
// `after` may add a launch behind the decode.  One host synchronisation, the read-back of *key:
// all ones, or index << 32 | (uint32_t)status of the first member that failed 
// (launch_member_status).  main_events: dmx_stats.ms_main_kernel brackets the decode kernel.
template <class Build, class After>
int members_decode_locked(dmx_ctx* c, const MemberTab& T, size_t count, uint32_t format, bool verify,
                          bool main_events, hipStream_t st, Build build, After after, unsigned long long* key) {
    HIPCHK(hipMemsetAsync(T.res, 0xFF, count * sizeof(dmx_batch_result), st));
    HIPCHK(hipMemsetAsync(T.key, 0xFF, 8, st));
    HIPCHK(build());
    HIPCHK(launch_frame_parse(T.desc, T.side, count, format, st));
    if (main_events) (void)hipEventRecord(c->ev[1], st);
    HIPCHK(launch_inflate_batch(T.desc, T.order, count, T.res, T.ticket, c->flags, st));
    if (main_events) (void)hipEventRecord(c->ev[2], st);
    if (verify) HIPCHK(launch_checksum_batch(T.desc, T.res, T.side, count, true, T.ticket + 4, st));
    HIPCHK(launch_frame_verdict(T.side, T.res, count, format, verify, st));
    // (a size other than the expected one: BGZF's ISIZE is wrong; gzip's measuring pass and decode disagree)
    HIPCHK(launch_member_status(T.res, T.desc, count, format == DMX_FRAME_GZIP ? DMX_ERR_INTERNAL : DMX_ERR_CHECKSUM,
                                T.key, st));
    HIPCHK(after());
    HIPCHK(hipEventRecord(c->ev_inf, st));
    c->inf_pending = true;
    HIPCHK(hipMemcpyAsync(key, T.key, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    end_timing(c, st);
    return DMX_OK;
}

// The BGZF calls' use of it: the file's status, and the stats both calls share
template <class Build, class After>
int bgzf_inflate_locked(dmx_ctx* c, const MemberTab& T, size_t count, bool verify, hipStream_t st, Build build,
                        After after) {
    unsigned long long k = 0;
    const int rc = members_decode_locked(c, T, count, DMX_FRAME_BGZF, verify, c->timing, st, build, after, &k);
    if (rc != DMX_OK) return rc;
    c->stats.segments = count;
    c->stats.path = 6;
    return k == ~0ull ? DMX_OK : (int)(int32_t)(uint32_t)k;
}

// ---- multi-member gzip files (gzip_members.hip; the walk: gzip_members.h) ----------------------

// Developer switch, read per call and only with dmx_set_timing on: which phase
// dmx_stats.ms_main_kernel brackets -- DMX_GZM_MAIN=scan (candidate count, its host read and the
// candidate list), =measure (the measuring pass); anything else: the batch decode.
int gzm_main_phase(const dmx_ctx* c) {
    if (!c->timing) return 2;
    const char* e = std::getenv("DMX_GZM_MAIN");
    return e && !std::strcmp(e, "scan") ? 0 : e && !std::strcmp(e, "measure") ? 1 : 2;
}

// One call: the file d_in[0, n) -> out[0, cap), and what its phases hand on.  Scratch: c->bgzt
// (tile counts and offsets, the small words), c->bgzc (candidates and records), c->bgzd (the gap
// list, then the batch's arrays) -- the BGZF device calls' buffers, which like this call end
// synchronised and wait for c->ev_inf.
struct GzmCall {
    const uint8_t* in;
    size_t n;
    bool verify;
    uint8_t* out;
    size_t cap;
    int phase;  // gzm_main_phase
    hipStream_t st;
    // c->bgzt's small words (ScanScratch::words): gap flag | gap result (2) | at 32 the measuring ticket
    uint8_t* d_words = nullptr;
    float phase_ms = 0;  // phase < 2: the events' time, read before a long member's own call records them anew
    std::vector<GzmCand> hc;
    std::vector<GzmRec> hr;
    std::vector<GzmRow> rows;
    std::vector<GzmGap> gaps;
    std::vector<uint64_t> uoffs;  // rows[k]'s first plain byte
    std::vector<uint32_t> small;  // the rows the batch decodes (the others are long: decoded in the walk)
    uint64_t total = 0;
    int tail = DMX_OK;  // what ended the chain early: the first failure that is not a batch member's
    bool bad_start = false;
};

// Phase 1: the candidates and their records, measured on the device and read back
int gzm_measure(dmx_ctx* c, GzmCall& G) {
    const hipStream_t st = G.st;
    ScanScratch S;
    if (!S.carve(c, scan_tiles(G.in, G.n), 48)) return DMX_ERR_NOMEM;
    G.d_words = S.words;
    unsigned int* const d_mticket = reinterpret_cast<unsigned int*>(G.d_words + 32);
    if (G.phase == 0) (void)hipEventRecord(c->ev[1], st);
    // (tickets and order entries are 32-bit)
    const int rc = S.count(launch_gzm_count(G.in, G.n, S.counts, S.offs, S.d_ncand, st), 0xFFFFFFFFull, st);
    if (rc != DMX_OK) return rc;
    const uint64_t ncand = S.ncand;
    G.hc.resize(ncand);
    G.hr.resize(ncand);
    const size_t off_recs = up16(ncand * sizeof(GzmCand));
    if (!c->bgzc.ensure(off_recs + ncand * sizeof(GzmRec) + 16)) return DMX_ERR_NOMEM;
    GzmCand* const d_cands = c->bgzc.as<GzmCand>();
    GzmRec* const d_recs = reinterpret_cast<GzmRec*>(c->bgzc.as<uint8_t>() + off_recs);
    HIPCHK(launch_gzm_write(G.in, G.n, S.offs, d_cands, ncand, st));
    if (G.phase == 0) (void)hipEventRecord(c->ev[2], st);
    if (G.phase == 1) (void)hipEventRecord(c->ev[1], st);
    int occupancy = 0;
    HIPCHK(launch_gzm_measure(G.in, G.n, d_cands, ncand, d_recs, d_mticket, c->flags, kBatchRouteBytes, st, &occupancy));
    if (G.phase == 1) (void)hipEventRecord(c->ev[2], st);
    if (c->diag & DIAG_DEBUG)
        std::fprintf(stderr, "dmx: gzip members: %llu candidates, measuring pass at %d workgroups per CU\n",
                     (unsigned long long)ncand, occupancy);
    if (ncand) {
        HIPCHK(hipMemcpyAsync(G.hc.data(), d_cands, ncand * sizeof(GzmCand), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(G.hr.data(), d_recs, ncand * sizeof(GzmRec), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    if (G.phase < 2 && ncand) {
        (void)hipEventElapsedTime(&G.phase_ms, c->ev[1], c->ev[2]);
        (void)hipGetLastError();
    }
    return DMX_OK;
}

// Phase 2: the chain -- the host's walk, a long member decoded where the walk meets it.  A return
// other than DMX_OK ends the call; what ends the chain goes to G.tail / G.bad_start.
int gzm_walk_chain(dmx_ctx* c, GzmCall& G) {
    const hipStream_t st = G.st;
    const uint64_t ncand = G.hc.size();
    uint64_t from = 0;
    for (;;) {
        const GzmWalk w = gzm_walk(G.hc.data(), G.hr.data(), ncand, G.n, from, &G.rows, &G.gaps);
        for (size_t k = G.uoffs.size(); k < G.rows.size(); k++) {
            G.uoffs.push_back(G.total);
            G.small.push_back((uint32_t)k);
            G.total += G.rows[k].plain;
        }
        if (w.what == GZM_DONE) return DMX_OK;
        if (w.what == GZM_BAD_START) {
            G.bad_start = true;
            return DMX_OK;
        }
        if (w.what != GZM_LONG) {
            G.tail = w.what;
            return DMX_OK;
        }
        // a long member: the single-stream plan, straight into its place
        if (!G.out || G.total > G.cap) {
            G.tail = DMX_ERR_CAPACITY;  // (its size is not known)
            return DMX_OK;
        }
        const GzmCand lc = G.hc[w.k];
        const uint64_t s0 = lc.off + lc.head;
        GzmCut cut = gzm_first_cut(G.hc.data(), ncand, w.k, G.n, kBatchRouteBytes);
        size_t len = 0;
        int rc;
        for (;;) {
            rc = inflate_device_locked(c, G.in + s0, (size_t)(cut.end - s0), G.out + G.total, G.cap - G.total, &len,
                                       nullptr, st);
            if (rc == DMX_ERR_NOMEM || rc == DMX_ERR_DEVICE || rc == DMX_ERR_INTERNAL) return rc;
            // DMX_ERR_OVERREAD with more of the file behind the cut: a false candidate inside the member
            if (rc != DMX_ERR_OVERREAD || !gzm_next_cut(G.hc.data(), ncand, G.n, &cut)) break;
        }
        if (rc != DMX_OK) {
            G.tail = rc;
            return DMX_OK;
        }
        const uint64_t end = s0 + c->last_end;
        if (end > G.n || G.n - end < 8) {
            G.tail = DMX_ERR_OVERREAD;
            return DMX_OK;
        }
        if (G.verify) {
            uint8_t t8[8];
            uint32_t ck = 0;
            HIPCHK(hipMemcpyAsync(t8, G.in + end, 8, hipMemcpyDeviceToHost, st));
            const int rk = checksum_locked(c, true, G.out + G.total, len, 0u, &ck, st);  // (waits for the copy too)
            if (rk != DMX_OK) return rk;
            if (frame_le32(t8) != ck || frame_le32(t8 + 4) != (uint32_t)len) {
                G.tail = DMX_ERR_CHECKSUM;
                return DMX_OK;
            }
        }
        G.rows.push_back(GzmRow{lc.off, lc.head, end, len});
        G.uoffs.push_back(G.total);
        G.total += len;
        from = end + 8;
    }
}

// Phase 3: the spaces between the members -- zeros, or the status of the header expected there,
// which takes the rows behind it away
int gzm_check_gaps(dmx_ctx* c, GzmCall& G) {
    if (!G.bad_start && G.gaps.empty()) return DMX_OK;
    const hipStream_t st = G.st;
    unsigned long long* const d_flag = reinterpret_cast<unsigned long long*>(G.d_words);
    uint64_t* const d_gapres = reinterpret_cast<uint64_t*>(G.d_words + 8);
    uint64_t longest = 0;
    for (const GzmGap& g : G.gaps) longest = std::max(longest, g.b - g.a);
    GzmGap* d_gaps = nullptr;
    if (!G.bad_start) {
        if (!c->bgzd.ensure(G.gaps.size() * sizeof(GzmGap))) return DMX_ERR_NOMEM;
        d_gaps = c->bgzd.as<GzmGap>();
        HIPCHK(hipMemcpyAsync(d_gaps, G.gaps.data(), G.gaps.size() * sizeof(GzmGap), hipMemcpyHostToDevice, st));
    }
    HIPCHK(launch_gzm_gaps(G.in, G.n, d_gaps, G.bad_start ? 0 : G.gaps.size(), longest, G.bad_start ? 0ull : ~0ull,
                           d_flag, d_gapres, st));
    uint64_t gr[2] = {~0ull, 0};
    HIPCHK(hipMemcpyAsync(gr, d_gapres, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (gr[0] != ~0ull) {  // the members in front of it stay; it comes before whatever ended the walk
        while (!G.rows.empty() && G.rows.back().coff > gr[0]) {
            if (!G.small.empty() && G.small.back() == G.rows.size() - 1) G.small.pop_back();
            G.rows.pop_back();
            G.uoffs.pop_back();
        }
        G.total = G.rows.empty() ? 0 : G.uoffs.back() + G.rows.back().plain;
        G.tail = (int)(int64_t)gr[1];
    }
    return DMX_OK;
}

// Phase 4: the members within the measuring limit (G.small, at least one) -- one decode of the
// list, which the host builds and uploads.  *key: as members_decode_locked, an index into G.small.
int gzm_decode_small(dmx_ctx* c, GzmCall& G, unsigned long long* key) {
    const size_t count = G.small.size();
    if (!c->bgzd.ensure(member_tab(nullptr, count).bytes)) return DMX_ERR_NOMEM;
    const MemberTab T = member_tab(c->bgzd.as<uint8_t>(), count);
    std::vector<uint64_t> image(T.list_bytes / 8);  // (outlives the decode's synchronise)
    InflateBatchDesc* const hd = reinterpret_cast<InflateBatchDesc*>(image.data());
    uint32_t* const ho = reinterpret_cast<uint32_t*>(hd + count);
    for (size_t i = 0; i < count; i++) {  // buffer i = the member with its header and trailer
        const GzmRow& r = G.rows[G.small[i]];
        hd[i] = InflateBatchDesc{G.in + r.coff, r.end + 8 - r.coff, G.out + G.uoffs[G.small[i]], r.plain};
        ho[i] = (uint32_t)i;
    }
    std::stable_sort(ho, ho + count, [&](uint32_t a, uint32_t b) { return hd[a].n > hd[b].n; });  // longest first
    return members_decode_locked(
        c, T, count, DMX_FRAME_GZIP, G.verify, G.phase == 2 && c->timing, G.st,
        [&] { return hipMemcpyAsync(T.desc, image.data(), T.list_bytes, hipMemcpyHostToDevice, G.st); },
        [] { return hipSuccess; }, key);
}

int gzip_members_locked(dmx_ctx* c, const uint8_t* in, size_t n, bool verify, uint8_t* out, size_t cap,
                        dmx_bgzf_entry* entries, size_t entry_cap, size_t* members, size_t* out_len, hipStream_t st) try {
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    begin_timing(c, st);
    GzmCall G{in, n, verify, out, cap, gzm_main_phase(c), st};
    if (const int rc = gzm_measure(c, G); rc != DMX_OK) return rc;
    if (const int rc = gzm_walk_chain(c, G); rc != DMX_OK) return rc;
    if (const int rc = gzm_check_gaps(c, G); rc != DMX_OK) return rc;
    const size_t nrows = G.rows.size();
    if (members) *members = nrows;
    c->stats.in_bytes = n;
    c->stats.segments = nrows;
    c->stats.path = 6;
    if (G.tail != DMX_OK) {
        // Under DMX_VERIFY a member in front of the failure may fail its checksum, which then comes
        // first; that needs the members' bytes, so only where they fit.
        if (!verify || G.small.empty() || G.total > cap) return G.tail;
    } else {
        if (entries && entry_cap < nrows + 1) return DMX_ERR_CAPACITY;
        if (G.total > cap) {  // before any member within the measuring limit is decoded
            *out_len = (size_t)G.total;
            return DMX_ERR_CAPACITY;
        }
    }
    if (!G.small.empty()) {
        unsigned long long key = 0;
        if (const int rc = gzm_decode_small(c, G, &key); rc != DMX_OK) return rc;
        if (key != ~0ull) {
            if (members) *members = G.small[(size_t)(key >> 32)];
            return (int)(int32_t)(uint32_t)key;
        }
    } else {
        end_timing(c, st);
    }
    // ---- the call's figures; the index ----
    if (G.phase < 2) c->stats.ms_main_kernel = G.phase_ms;
    if (G.tail != DMX_OK) return G.tail;
    if (entries) {
        for (size_t k = 0; k < nrows; k++) entries[k] = dmx_bgzf_entry{G.rows[k].coff, G.uoffs[k]};
        entries[nrows] = dmx_bgzf_entry{n, G.total};
    }
    c->stats.out_bytes = G.total;
    *out_len = (size_t)G.total;
    return DMX_OK;
} catch (const std::bad_alloc&) {
    return DMX_ERR_NOMEM;
}

}  // namespace

extern "C" {

// ---- BGZF files on host buffers: one framed batch call each -----------------------------------
size_t dmx_bgzf_bound(size_t n) {
    const size_t full = n / kBgzfBlock, rem = n % kBgzfBlock;
    return full * dmx_batch_framed_bound(DMX_FRAME_BGZF, kBgzfBlock) +
           (rem ? dmx_batch_framed_bound(DMX_FRAME_BGZF, rem) : 0) + kBgzfEofBytes;
}

int dmx_deflate_bgzf(dmx_ctx* c, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap, size_t* out_len) {
    if (!c && !(c = dmx_default_ctx())) return DMX_ERR_DEVICE;
    if ((!in && n) || !out_len || !out) return DMX_ERR_ARG;
    *out_len = 0;
    BgzfSlots B(n);
    std::vector<uint8_t> members;  // one slot per member; concatenated into `out` below
    try {
        members.resize(B.nblk * B.slot);
        B.fill(in, n, members.data());
    } catch (const std::bad_alloc&) {
        return DMX_ERR_NOMEM;
    }
    const int rc = dmx_deflate_batch_framed(c, B.ins.data(), B.ns.data(), B.nblk, level, DMX_FRAME_BGZF, B.outs.data(),
                                            B.caps.data(), B.res.data());
    if (rc != DMX_OK) return rc;
    size_t total = kBgzfEofBytes;
    for (size_t i = 0; i < B.nblk; i++) {
        if (B.res[i].status != DMX_OK) return B.res[i].status;
        total += B.res[i].bytes;
    }
    *out_len = total;
    if (total > cap) return DMX_ERR_CAPACITY;
    uint8_t* o = out;
    for (size_t i = 0; i < B.nblk; i++) {
        std::memcpy(o, B.outs[i], B.res[i].bytes);
        o += B.res[i].bytes;
    }
    std::memcpy(o, kBgzfEof, kBgzfEofBytes);
    return DMX_OK;
}

int dmx_inflate_bgzf(dmx_ctx* c, const uint8_t* in, size_t n, uint32_t flags, uint8_t** out, size_t* len) {
    if (!c && !(c = dmx_default_ctx())) return DMX_ERR_DEVICE;
    if ((!in && n) || !out || !len || (flags & ~DMX_VERIFY)) return DMX_ERR_ARG;
    *out = nullptr;
    *len = 0;
    std::vector<const uint8_t*> ins;
    std::vector<uint8_t*> outs;
    std::vector<size_t> ns, caps;
    std::vector<dmx_batch_result> res;
    size_t total = 0;
    try {
        for (uint64_t off = 0; off < n;) {  // the member chain, by BSIZE
            BgzfMember m;
            const int rc = bgzf_next(in, n, off, &m);
            if (rc != DMX_OK) return rc;
            ins.push_back(in + m.off);
            ns.push_back((size_t)m.size);
            caps.push_back(m.isize);
            total += m.isize;
            off += m.size;
        }
        outs.resize(ins.size());
        res.resize(ins.size());
    } catch (const std::bad_alloc&) {
        return DMX_ERR_NOMEM;
    }
    uint8_t* h = static_cast<uint8_t*>(std::malloc(total ? total : 1));
    if (!h) return DMX_ERR_NOMEM;
    size_t o = 0;
    for (size_t i = 0; i < ins.size(); i++) {  // the layout: the prefix sum of ISIZE
        outs[i] = h + o;
        o += caps[i];
    }
    int rc = dmx_inflate_batch_framed(c, ins.data(), ns.data(), ins.size(), DMX_FRAME_BGZF, outs.data(), caps.data(),
                                      res.data(), (flags & DMX_VERIFY) ? DMX_BATCH_VERIFY : 0u);
    for (size_t i = 0; rc == DMX_OK && i < ins.size(); i++) {
        rc = res[i].status;
        // a member that decodes to more or fewer bytes than its ISIZE breaks the layout
        if (rc == DMX_ERR_CAPACITY || (rc == DMX_OK && res[i].bytes != caps[i])) rc = DMX_ERR_CHECKSUM;
    }
    if (rc != DMX_OK) {
        std::free(h);
        return rc;
    }
    *out = h;
    *len = total;
    return DMX_OK;
}

// ---- BGZF files in device memory ----------------------------------------------------------------
int dmx_deflate_bgzf_device(dmx_ctx* c, const void* d_in, size_t n, int level, void* d_out, size_t cap,
                            size_t* out_len, void* stream) {
    if (!c || (!d_in && n) || !out_len || (!d_out && cap)) return DMX_ERR_ARG;
    if (!has_batch_deflate(c)) return DMX_ERR_ARG;  // as dmx_deflate_batch_framed_device
    *out_len = 0;
    BgzfSlots B(n);
    const size_t nblk = B.nblk;
    if (nblk >= (size_t)DF_BATCH_LAST) return DMX_ERR_ARG;
    DMX_ENTER(g, c, stream);
    const hipStream_t st = g.st;
    if (!nblk) {  // the EOF member alone
        *out_len = kBgzfEofBytes;
        if (cap < kBgzfEofBytes) return DMX_ERR_CAPACITY;
        HIPCHK(hipMemcpyAsync(d_out, kBgzfEof, kBgzfEofBytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        return DMX_OK;
    }
    // member i into slot i, as dmx_deflate_bgzf does on the host
    const size_t off_offs = up16(nblk * 4), off_key = off_offs + up16(scan_words(nblk) * 8);
    if (!c->bgzs.ensure(nblk * B.slot + 16) || !c->bgzc.ensure(off_key + 16 + sizeof(BgzfChainHead))) return DMX_ERR_NOMEM;
    try {
        B.fill(static_cast<const uint8_t*>(d_in), n, c->bgzs.as<uint8_t>());
    } catch (const std::bad_alloc&) {
        return DMX_ERR_NOMEM;
    }
    const int rc = deflate_batch_framed_locked(c, B.ins.data(), B.ns.data(), nblk, level, DMX_FRAME_BGZF, B.outs.data(),
                                               B.caps.data(), B.res.data(), st);
    if (rc != DMX_OK) return rc;
    // the members back to back into d_out, the EOF member behind them; the results are still in
    // c->bres, where the batch left them
    uint8_t* const cb = c->bgzc.as<uint8_t>();
    unsigned long long* const key = reinterpret_cast<unsigned long long*>(cb + off_key);
    BgzfChainHead* const head = reinterpret_cast<BgzfChainHead*>(cb + off_key + 16);
    HIPCHK(hipMemsetAsync(key, 0xFF, 8, st));
    HIPCHK(launch_bgzf_pack(c->bgzs.as<uint8_t>(), B.slot, c->bres.as<dmx_batch_result>(), nblk,
                            reinterpret_cast<uint32_t*>(cb), reinterpret_cast<uint64_t*>(cb + off_offs), key,
                            static_cast<uint8_t*>(d_out), cap, head, st));
    HIPCHK(hipEventRecord(c->ev_df, st));
    c->df_pending = true;
    BgzfChainHead h{};
    HIPCHK(hipMemcpyAsync(&h, head, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h.status == DMX_OK || h.status == DMX_ERR_CAPACITY) *out_len = (size_t)h.members;
    c->stats.out_bytes = h.status == DMX_OK ? h.members : 0;
    return h.status;
}

int dmx_bgzf_index_device(dmx_ctx* c, const void* d_in, size_t n, dmx_bgzf_entry* entries, size_t entry_cap,
                          size_t* members, uint64_t* plain_bytes, void* stream) {
    if (!c || (!d_in && n)) return DMX_ERR_ARG;
    if (members) *members = 0;
    if (plain_bytes) *plain_bytes = 0;
    DMX_ENTER(g, c, stream);
    const hipStream_t st = g.st;
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    begin_timing(c, st);
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    BgzfChain ch;
    const int rc = bgzf_chain_locked(c, static_cast<const uint8_t*>(d_in), n, st, &ch);
    if (rc != DMX_OK) return rc;
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    HIPCHK(hipEventRecord(c->ev_inf, st));
    c->inf_pending = true;
    end_timing(c, st);
    c->stats.segments = ch.members;
    c->stats.in_bytes = n;
    if (members) *members = (size_t)ch.members;
    if (ch.status != DMX_OK) return ch.status;
    if (plain_bytes) *plain_bytes = ch.total;
    if (!entries) return DMX_OK;
    if (entry_cap < ch.members + 1) return DMX_ERR_CAPACITY;
    if (!ch.members) {
        entries[0] = dmx_bgzf_entry{n, 0};
        return DMX_OK;
    }
    const size_t bytes = (ch.members + 1) * sizeof(dmx_bgzf_entry);
    if (!c->bgzd.ensure(bytes)) return DMX_ERR_NOMEM;
    HIPCHK(launch_bgzf_entries(ch.rows, ch.uoff, ch.members, n, &ch.head->total, c->bgzd.as<dmx_bgzf_entry>(), st));
    HIPCHK(hipEventRecord(c->ev_inf, st));
    HIPCHK(hipMemcpyAsync(entries, c->bgzd.p, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DMX_OK;
}

int dmx_inflate_bgzf_device(dmx_ctx* c, const void* d_in, size_t n, uint32_t flags, void* d_out, size_t cap,
                            size_t* out_len, void* stream) {
    if (!c || (!d_in && n) || !out_len || (!d_out && cap) || (flags & ~DMX_VERIFY)) return DMX_ERR_ARG;
    *out_len = 0;
    DMX_ENTER(g, c, stream);
    const hipStream_t st = g.st;
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    begin_timing(c, st);
    BgzfChain ch;
    int rc = bgzf_chain_locked(c, static_cast<const uint8_t*>(d_in), n, st, &ch);
    if (rc != DMX_OK) return rc;
    if (ch.status != DMX_OK) return ch.status;
    if (ch.total > cap) {  // before any member is looked at
        *out_len = (size_t)ch.total;
        return DMX_ERR_CAPACITY;
    }
    if (!ch.members) return DMX_OK;
    if (ch.members >= (uint64_t)DF_BATCH_LAST) return DMX_ERR_NOMEM;
    if (!c->bgzd.ensure(member_tab(nullptr, ch.members).bytes)) return DMX_ERR_NOMEM;
    const MemberTab T = member_tab(c->bgzd.as<uint8_t>(), ch.members);
    const uint8_t* const in = static_cast<const uint8_t*>(d_in);
    uint8_t* const out = static_cast<uint8_t*>(d_out);
    rc = bgzf_inflate_locked(
        c, T, ch.members, (flags & DMX_VERIFY) != 0, st,
        [&] { return launch_bgzf_desc(in, ch.rows, ch.uoff, ch.members, out, T.desc, T.order, st); },
        [] { return hipSuccess; });
    c->stats.in_bytes = n;
    if (rc != DMX_OK) return rc;
    c->stats.out_bytes = ch.total;
    *out_len = (size_t)ch.total;
    return DMX_OK;
}

int dmx_inflate_bgzf_range_device(dmx_ctx* c, const void* d_in, size_t n, const dmx_bgzf_entry* index, size_t members,
                                  uint64_t uoffset, size_t len, uint32_t flags, void* d_out, void* stream) {
    if (!c || (!d_in && n) || !index || (flags & ~DMX_VERIFY)) return DMX_ERR_ARG;
    for (size_t k = 0; k < members; k++)
        if (index[k + 1].coffset < index[k].coffset || index[k + 1].uoffset < index[k].uoffset) return DMX_ERR_ARG;
    const uint64_t plain = index[members].uoffset;
    if (index[members].coffset > n || uoffset > plain || len > plain - uoffset || uoffset < index[0].uoffset)
        return DMX_ERR_ARG;
    if (!len) return DMX_OK;
    if (!d_out) return DMX_ERR_ARG;
    // the members that overlap [u0, u1): from the last one that starts at or before u0 (it is not
    // empty) up to the first entry at or behind u1
    const uint64_t u0 = uoffset, u1 = uoffset + len;
    const dmx_bgzf_entry* const e = index + members + 1;
    const size_t k0 = (size_t)(std::upper_bound(index, e, u0, [](uint64_t u, const dmx_bgzf_entry& x) {
                                   return u < x.uoffset;
                               }) - index) - 1;
    const size_t k1 = (size_t)(std::lower_bound(index, e, u1, [](const dmx_bgzf_entry& x, uint64_t u) {
                                   return x.uoffset < u;
                               }) - index);
    const size_t count = k1 - k0;  // >= 1: index[k0].uoffset <= u0 < u1 <= index[k1].uoffset
    if (count >= (size_t)DF_BATCH_LAST) return DMX_ERR_ARG;
    const uint64_t edge0 = index[k0 + 1].uoffset - index[k0].uoffset, edge1 = index[k1].uoffset - index[k1 - 1].uoffset;
    DMX_ENTER(g, c, stream);
    const hipStream_t st = g.st;
    // c->bgzd: the index slice, then the decode's arrays
    const size_t idx_bytes = up16((count + 1) * sizeof(dmx_bgzf_entry));
    if (!c->bgzs.ensure(edge0 + edge1 + 16) || !c->bgzd.ensure(idx_bytes + member_tab(nullptr, count).bytes))
        return DMX_ERR_NOMEM;
    const MemberTab T = member_tab(c->bgzd.as<uint8_t>() + idx_bytes, count);
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    begin_timing(c, st);
    dmx_bgzf_entry* const d_idx = c->bgzd.as<dmx_bgzf_entry>();
    HIPCHK(hipMemcpyAsync(d_idx, index + k0, (count + 1) * sizeof(dmx_bgzf_entry), hipMemcpyHostToDevice, st));
    const uint8_t* const in = static_cast<const uint8_t*>(d_in);
    uint8_t* const out = static_cast<uint8_t*>(d_out);
    uint8_t* const edge = c->bgzs.as<uint8_t>();
    const int rc = bgzf_inflate_locked(
        c, T, count, (flags & DMX_VERIFY) != 0, st,
        [&] { return launch_bgzf_range_desc(in, d_idx, count, u0, u1, out, edge, T.desc, T.order, st); },
        [&] { return launch_bgzf_range_copy(d_idx, count, u0, u1, edge, out, st); });
    c->stats.out_bytes = rc == DMX_OK ? len : 0;
    return rc;
}

// ---- multi-member gzip files ------------------------------------------------------------------
int dmx_inflate_gzip_members_device(dmx_ctx* c, const void* d_in, size_t n, uint32_t flags, void* d_out, size_t cap,
                                    dmx_bgzf_entry* entries, size_t entry_cap, size_t* members, size_t* out_len,
                                    void* stream) {
    if (!c || !out_len || (!d_in && n) || (!d_out && cap) || (flags & ~DMX_VERIFY)) return DMX_ERR_ARG;
    *out_len = 0;
    if (members) *members = 0;
    if (!n) {  // no member
        if (entries && entry_cap < 1) return DMX_ERR_CAPACITY;
        if (entries) entries[0] = dmx_bgzf_entry{0, 0};
        return DMX_OK;
    }
    DMX_ENTER(g, c, stream);
    return gzip_members_locked(c, static_cast<const uint8_t*>(d_in), n, (flags & DMX_VERIFY) != 0,
                               static_cast<uint8_t*>(d_out), cap, entries, entry_cap, members, out_len, g.st);
}

int dmx_inflate_gzip_members(dmx_ctx* c, const uint8_t* in, size_t n, uint32_t flags, uint8_t* out, size_t cap,
                             size_t* members, size_t* out_len) {
    if (!c || !out_len || (!in && n) || (!out && cap) || (flags & ~DMX_VERIFY)) return DMX_ERR_ARG;
    *out_len = 0;
    if (members) *members = 0;
    if (!n) return DMX_OK;
    DMX_ENTER(g, c);
    // the file and the output area, staged in context scratch (nothing else in this call uses it)
    const size_t off_out = up16(n + 16);
    if (!c->bgzs.ensure(off_out + cap + 16)) return DMX_ERR_NOMEM;
    uint8_t* const d_in = c->bgzs.as<uint8_t>();
    uint8_t* const d_out = cap ? d_in + off_out : nullptr;
    HIPCHK(hipMemcpyAsync(d_in, in, n, hipMemcpyHostToDevice, c->stream));
    const int rc = gzip_members_locked(c, d_in, n, (flags & DMX_VERIFY) != 0, d_out, cap, nullptr, 0, members, out_len,
                                       c->stream);
    if (rc != DMX_OK || !*out_len) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out, *out_len, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return DMX_OK;
}

}  // extern "C"
