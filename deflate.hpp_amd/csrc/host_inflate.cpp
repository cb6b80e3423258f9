// host_inflate.cpp -- the inflate drivers: the segmented plan (inflate_plan.h decides the
// passes), the path-4 chain repair, path 5 (host_fb.cpp), the serial fallback, and the
// asynchronous lane path.
#include <algorithm>
#include <cstdio>

#include "dmx_ctx.h"
#include "inflate_plan.h"

namespace dmx {

int marker_scan(dmx_ctx* c, const StreamWords& w, size_t n, uint64_t* ntiles, hipStream_t st, bool sync_call,
                const uint32_t** hl_zeroed) {
    const uint64_t nt = *ntiles = marker_tiles(n, w.misalign);
    if (!c->tiles.ensure(nt * 4) || !c->tileoffs.ensure(scan_words(nt) * 8)) return DMX_ERR_NOMEM;
    Scal* ds = c->scal.as<Scal>();
    if (!sync_call) {
        HIPCHK(launch_marker_count(w.words, w.misalign, n, c->tiles.as<uint32_t>(), nt, st));
        HIPCHK(launch_scan_u32(c->tiles.as<uint32_t>(), c->tileoffs.as<uint64_t>(), nt, &ds->nmarkers, st));
        return DMX_OK;
    }
    uint32_t* const hl = c->lheavy.as<uint32_t>();  // (nullptr before the first heavy route)
    if (hl_zeroed) *hl_zeroed = hl;
    HIPCHK(launch_marker_count(w.words, w.misalign, n, c->tiles.as<uint32_t>(), nt, st, &ds->vw, hl));
    HIPCHK(launch_scan_u32(c->tiles.as<uint32_t>(), c->tileoffs.as<uint64_t>(), nt, &ds->nmarkers, st,
                           c->hres ? &c->hres_dev->nmarkers : nullptr, &ds->ncand));
    return DMX_OK;
}
int marker_write(dmx_ctx* c, const StreamWords& w, size_t n, uint64_t ntiles, uint64_t cand_cap, hipStream_t st) {
    HIPCHK(launch_marker_write(w.words, w.misalign, n, c->tileoffs.as<uint64_t>(), ntiles, c->cands.as<uint64_t>(),
                               cand_cap, st));
    return DMX_OK;
}

namespace {

constexpr uint32_t kSegCap = 32768;  // LDS window of k_inflate_segments

// the per-candidate scratch of the segmented passes, then their arguments (mode, slot and dbg
// are the pass's)
bool cand_bufs(dmx_ctx* c, uint64_t ncand) {
    return c->cands.ensure(ncand * 8) && c->recs.ensure(ncand * sizeof(SegRecord)) && c->status.ensure(ncand * 8);
}
InflateArgs inflate_args(dmx_ctx* c, const StreamWords& w, size_t n, uint64_t ncand, uint8_t* out, uint64_t cap,
                         uint32_t iflags) {
    InflateArgs A;
    A.in_words = w.words;
    A.misalign = w.misalign;
    A.n = n;
    A.cands = c->cands.as<uint64_t>();
    A.ncand = ncand;
    A.out = out;
    A.cap = cap;
    A.recs = c->recs.as<SegRecord>();
    A.status = c->status.as<unsigned long long>();
    A.ticket = &c->scal.as<Scal>()->ticket;
    A.flags = c->flags | iflags;
    A.dbg = nullptr;
    return A;
}
// the lane decoder's token lists (mode 4)
bool lane_bufs(dmx_ctx* c, uint64_t ncand, size_t n) {
    return c->ltok.ensure(lane_tok_words(c->seg, ncand, n) * 4) && c->ltokoff.ensure(scan_words(ncand) * 8) &&
           c->lntok.ensure(ncand * 4) && c->lcaps.ensure(ncand * 4) && c->lsplit.ensure(ncand * 4 + 8);
}
int lanes_pass(dmx_ctx* c, const InflateArgs& A, uint32_t heavy, uint32_t heavy_limit, uint32_t* hl, hipStream_t st,
               hipEvent_t e0, hipEvent_t e1, bool hl_zeroed = false) {
    HIPCHK(launch_inflate_lanes(A, c->ltok.as<uint32_t>(), c->ltokoff.as<uint64_t>(), c->lntok.as<uint32_t>(),
                                c->lcaps.as<uint32_t>(), heavy, heavy_limit, hl, c->lsplit.as<uint32_t>(), c->ncu, st,
                                e0, e1, hl_zeroed));
    return DMX_OK;
}

// the plan for this stream: allocates what the lane and heavy passes need and says what fitted
PassPlan make_plan(dmx_ctx* c, size_t n, uint64_t ncand, bool parallel_ok) {
    bool lanes_ok = false, heavy_ok = false;
    if (plan_wants_lanes(c->inflate_pass)) {
        // short of device memory: drop the scratch this call does not use (the deflate's token
        // words and slots, path 5's token space and images, chain-repair scratch) and try again
        // before the plan goes past the lane decoder
        lanes_ok = lane_bufs(c, ncand, n);
        if (!lanes_ok) {
            for (DevBuf* b : {&c->dtok, &c->slots, &c->rtmp, &c->fbt, &c->fbimg, &c->fbwin, &c->fbopen, &c->fbk,
                              &c->fbu, &c->fbJ, &c->fbJraw, &c->fbJsub})
                b->release();
            lanes_ok = lane_bufs(c, ncand, n);
        }
        heavy_ok = lanes_ok && plan_wants_heavy(c->seg, ncand) && c->lheavy.ensure((ncand + 2) * 4);
    }
    return inflate_pass_plan(c->seg, n, ncand, c->inflate_pass, c->heavy_bytes, c->ncu, lanes_ok, heavy_ok, parallel_ok);
}

// DMX_RECS: per-candidate outcome of a pass (developer aid)
void dump_recs(const InflateArgs& A, int32_t status) {
    const uint64_t ncand = A.ncand;
    const uint32_t mode = A.mode;
    std::vector<SegRecord> h(ncand);
    (void)hipMemcpy(h.data(), A.recs, ncand * sizeof(SegRecord), hipMemcpyDeviceToHost);
    uint64_t fl[8] = {0}, shown = 0;
    for (uint64_t i = 0; i < ncand; i++) {
        for (int b = 0; b < 8; b++) fl[b] += (h[i].flags >> b) & 1;
        if ((h[i].flags & ~1u) && shown++ < 8)
            std::fprintf(stderr, "dmx: mode %u cand %llu flags %u size %u end %llu\n", mode,
                         (unsigned long long)i, h[i].flags, h[i].out_size,
                         (unsigned long long)h[i].end_byte);
    }
    std::fprintf(stderr, "dmx: mode %u ncand %llu status %u flags fin %llu data %llu over %llu ovf %llu xref %llu tmo %llu exo %llu\n",
                 mode, (unsigned long long)ncand, status, (unsigned long long)fl[0], (unsigned long long)fl[1],
                 (unsigned long long)fl[2], (unsigned long long)fl[3], (unsigned long long)fl[4],
                 (unsigned long long)fl[5], (unsigned long long)fl[6]);
}

void dump_serial_cycles(const InflateResult& r) {
    std::fprintf(stderr, "dmx serial: cycles %llu %llu %llu %llu %llu, regions %llu; walk phases %llu %llu %llu %llu %llu, "
                 "rounds %llu (k_inflate_serial_wg: doubling, members+scan+cuts, parallel writes, wave-0 copies + "
                 "flush, decode + walks; walks: first pass, rounds, output sums, writes, dependent copies)\n",
                 (unsigned long long)r.cycles[0], (unsigned long long)r.cycles[1], (unsigned long long)r.cycles[2],
                 (unsigned long long)r.cycles[3], (unsigned long long)r.cycles[4], (unsigned long long)r.cycles[5],
                 (unsigned long long)r.cycles[6], (unsigned long long)r.cycles[7], (unsigned long long)r.cycles[8],
                 (unsigned long long)r.cycles[9], (unsigned long long)r.cycles[10], (unsigned long long)r.cycles[11]);
}

struct PlanRun {
    dmx_ctx* c;
    hipStream_t st;
    InflateArgs A;  // out / cap: where the passes decode to
    PassPlan plan;
    uint32_t lead_mode = 0;  // the last pass run that decodes every candidate (not a patch pass)
    int first = 0;           // the pass to start from (> 0: r holds the validation of the pass before)
    bool one_pass = false;   // stop behind the first pass run (the speculative pass)
    // the call's marker count kernel has zeroed the validation words / the heavy list's counters
    // (marker_scan); used up by the first pass run
    bool vw_zeroed = false;
    const uint32_t* hl_zeroed = nullptr;
};

// the plan's passes into A.out / A.cap; r: the last validation result
int run_plan(PlanRun& s, InflateResult& r) {
    dmx_ctx* c = s.c;
    hipStream_t st = s.st;
    InflateArgs& A = s.A;
    Scal* ds = c->scal.as<Scal>();
    if (s.first == 0) r.status = 2;
    for (int pi = s.first; pi < s.plan.np; pi++) {
        const uint32_t mode = s.plan.pass[pi][0];
        if (pass_skipped(mode, r.exotic, A.ncand)) continue;
        A.mode = mode;
        A.slot = s.plan.pass[pi][1];
        // main-kernel window: from the first pass's launch to the end of the last pass run
        hipEvent_t e0 = (c->timing && pi == 0) ? c->ev[1] : nullptr, e1 = c->timing ? c->ev[2] : nullptr;
        if (mode != 3 && mode != 6) s.lead_mode = mode;
        if (mode == 4) {
            uint32_t* const hl = c->lheavy.as<uint32_t>();
            if (lanes_pass(c, A, s.plan.heavy, s.plan.heavy_limit, hl, st, e0, e1, hl && hl == s.hl_zeroed) != DMX_OK)
                return DMX_ERR_DEVICE;
        } else if (mode == 6) {
            const uint32_t grid = (uint32_t)std::min<uint64_t>(r.exotic, (uint64_t)std::max(c->ncu, 1));
            HIPCHK(launch_inflate_pj_list(A, A.slot, c->lheavy.as<uint32_t>(), grid, st, e1));
        } else if (mode == 2) {
            HIPCHK(launch_inflate_pj(A, A.slot, st, e0, e1));
        } else {
            HIPCHK(hipMemsetAsync(A.status, 0, A.ncand * 8, st));
            HIPCHK(hipMemsetAsync(&ds->ticket, 0, 4, st));
            HIPCHK(launch_inflate_segments(A, st, e0, e1));
        }
        // the result comes through the host result block (k_inflate_validate stores it there too)
        HIPCHK(launch_inflate_validate(A, &ds->vw, &ds->res, st, s.vw_zeroed, c->hres ? &c->hres_dev->res : nullptr));
        s.vw_zeroed = false;
        s.hl_zeroed = nullptr;
        if (A.dbg) phase_dump(c, "inflate", A.ncand, st);
        if (!c->hres) HIPCHK(hipMemcpyAsync(&r, &ds->res, sizeof r, hipMemcpyDeviceToHost, st));
        mark_end(c, st);  // (the last pass's stands: end_timing does not wait again)
        HIPCHK(hipStreamSynchronize(st));
        if (c->hres) r = c->hres->res;
        if (c->diag & DIAG_RECS) dump_recs(A, r.status);
        if (s.one_pass || pass_ends_plan(mode, s.lead_mode, r.status, r.exotic)) break;
    }
    return DMX_OK;
}

// dmx_inflate_index_device: the validated chain's segment starts as the index's checkpoints.  No
// back-reference crosses a segment start, so none needs a window.
void seek_tap_segments(SeekTap* tap, const SegChain& ch, const uint64_t* cands) {
    tap->cands.clear();
    for (size_t i = 0; i < ch.chain.size(); i++) tap->cands.push_back({8 * cands[ch.chain[i]], ch.offsets[i], true});
}
// The same for the uniform layout, whose chain the validation kernels checked on the device: the
// records and candidates up to the BFINAL segment come back (one more host synchronisation, in
// the index call only) and the host walks them.  A walk that does not confirm the chain leaves
// the tap empty (entry 0 alone: correct, degenerate).
int seek_tap_uniform(dmx_ctx* c, const InflateArgs& A, const InflateResult& r, hipStream_t st) {
    const uint64_t nc = std::min<uint64_t>((uint64_t)r.fin_index + 1, A.ncand);
    std::vector<SegRecord> h(nc);
    std::vector<uint64_t> hc(nc);
    HIPCHK(hipMemcpyAsync(h.data(), A.recs, nc * sizeof(SegRecord), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hc.data(), A.cands, nc * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const SegChain ch = seg_chain_walk(h.data(), hc.data(), nc);
    c->seek_tap->cands.clear();
    if (ch.ok && ch.total == r.total) seek_tap_segments(c->seek_tap, ch, hc.data());
    return DMX_OK;
}

// Chain repair.  A "00 00 FF FF" inside stored data (random data: once per ~4 GiB) is a
// candidate no segment starts at, so the candidate chain skips it and every later segment
// sits one slot too far; the whole stream used to go to the serial decoder (hours at
// multi-GiB sizes).  Segments of other sizes than the slot (a short segment in the middle,
// 16 KiB segments) are placed the same way.  The records say where each segment ends: the host walks the chain
// from candidate 0 (seg_chain_walk), the segments are decoded into a scratch buffer at their
// slots if the first decode did not hold every slot, and one kernel moves the chain's segments
// to their offsets.  out / cap: the plan's output buffer (the caller's when fixed).
// *repaired = false: not repaired (the later paths decode the stream).
int chain_repair(PlanRun& s, bool fixed, uint8_t* out, size_t cap, size_t* total_out, uint8_t** dev_out,
                 bool* repaired) {
    dmx_ctx* c = s.c;
    hipStream_t st = s.st;
    InflateArgs& A = s.A;
    const uint64_t ncand = A.ncand;
    *repaired = false;
    std::vector<SegRecord> h(ncand);
    std::vector<uint64_t> hc(ncand);
    HIPCHK(hipMemcpyAsync(h.data(), A.recs, ncand * sizeof(SegRecord), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hc.data(), A.cands, ncand * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const SegChain ch = seg_chain_walk(h.data(), hc.data(), ncand);
    if (!ch.ok) return DMX_OK;
    // (when the repair's own scratch does not fit, the stream still decodes on path 5 or the
    // serial decoder, which need only the output: ADVICE r3)
    if (fixed && ch.total > cap) return DMX_ERR_CAPACITY;
    uint64_t slot = A.slot ? A.slot : c->seg;
    const uint64_t need = (ch.chain.back() + 1) * slot;
    const uint32_t maxsz = *std::max_element(ch.sizes.begin(), ch.sizes.end());
    const uint8_t* src = out;
    uint8_t* place = out;  // where the kernel writes; then copied to out if scratch
    if (need > A.cap || maxsz > slot) {
        // slots past the buffer were not written, or segments larger than the slot
        // overlapped: decode again into scratch with 32 KiB slots, place into out
        if (maxsz > slot) {
            slot = LN_OUT_CAP_BYTES;
            for (int pi = 0; pi < s.plan.np; pi++)
                if (const uint32_t m = s.plan.pass[pi][0]; m == 4 || m == 6 || m == 3) s.plan.pass[pi][1] = (uint32_t)slot;
        }
        if (!c->rtmp.ensure(ncand * slot)) return DMX_OK;
        A.out = c->rtmp.as<uint8_t>();
        A.cap = ncand * slot;
        InflateResult r2{};
        if (const int rc = run_plan(s, r2); rc != DMX_OK) return rc;
        src = A.out;
    } else {  // every slot is in `out`: place into scratch, copy back
        if (!c->rtmp.ensure(ch.total ? ch.total : 1)) return DMX_OK;
        place = c->rtmp.as<uint8_t>();
    }
    const uint64_t nch = ch.chain.size();
    if (!c->rchain.ensure(nch * 20)) return DMX_OK;
    uint64_t* dch = c->rchain.as<uint64_t>();
    uint64_t* doffs = dch + nch;
    uint32_t* dsz = reinterpret_cast<uint32_t*>(doffs + nch);
    HIPCHK(hipMemcpyAsync(dch, ch.chain.data(), nch * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(doffs, ch.offsets.data(), nch * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dsz, ch.sizes.data(), nch * 4, hipMemcpyHostToDevice, st));
    HIPCHK(launch_place_segments(src, (uint32_t)slot, dch, doffs, dsz, nch, place, st));
    if (place != out && ch.total) HIPCHK(hipMemcpyAsync(out, place, ch.total, hipMemcpyDeviceToDevice, st));
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    mark_end(c, st);
    HIPCHK(hipStreamSynchronize(st));
    end_timing(c, st);
    c->last_end = h[ch.chain.back()].end_byte;
    if (c->seek_tap) seek_tap_segments(c->seek_tap, ch, hc.data());
    c->stats.path = 4;
    c->stats.out_bytes = ch.total;
    *total_out = ch.total;
    if (dev_out) *dev_out = out;
    *repaired = true;
    return DMX_OK;
}

int serial_pass(dmx_ctx* c, const InflateArgs& A, InflateResult& r, hipStream_t st) {
    InflateResult* dres = &c->scal.as<Scal>()->res;
    HIPCHK(launch_inflate_serial(A, 0, dres, st));
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    HIPCHK(hipMemcpyAsync(&r, dres, sizeof r, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DMX_OK;
}

// serial path: one pass into the caller's buffer, or into c->out sized generously (bytes
// past the capacity are counted, not written); a second pass only when that did not fit
int inflate_serial(dmx_ctx* c, InflateArgs A, size_t n, uint8_t* fixed_out, size_t cap, size_t* total_out,
                   uint8_t** dev_out, hipStream_t st) {
    c->stats.path = 2;
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    uint64_t dummy_dbg = 0;
    A.dbg = (c->diag & DIAG_FB) ? &dummy_dbg : nullptr;  // (a flag for the kernel: count phases)
    if (!fixed_out) {
        size_t freeb = 0, totb = 0;
        if (hipMemGetInfo(&freeb, &totb) != hipSuccess) freeb = 0;
        // a generous first buffer saves the second pass on high-ratio streams, but it is kept
        // by the context: bounded by 4 GiB (64 n alone held ~72 GiB for a 1 GiB
        // stream); a larger output is counted by the first pass and decoded by a second
        const uint64_t guess = std::min<uint64_t>({64ull * n + (16ull << 20), 4ull << 30, freeb / 4});
        if (c->out.cap < guess && !c->out.ensure(guess)) (void)c->out.ensure(1);
        A.out = c->out.as<uint8_t>();
        A.cap = c->out.p ? c->out.cap : 0;
    } else {
        A.out = fixed_out;
        A.cap = cap;
    }
    InflateResult r{};
    if (serial_pass(c, A, r, st) != DMX_OK) return DMX_ERR_DEVICE;
    if (r.status != 0) return r.status;
    if (r.total > A.cap) {
        if (fixed_out) return DMX_ERR_CAPACITY;
        if (!c->out.ensure(r.total)) return DMX_ERR_NOMEM;
        A.out = c->out.as<uint8_t>();
        A.cap = c->out.cap;
        if (serial_pass(c, A, r, st) != DMX_OK) return DMX_ERR_DEVICE;
    }
    end_timing(c, st);
    if (c->diag & DIAG_FB) dump_serial_cycles(r);
    *total_out = r.total;
    c->last_end = r.end_byte;
    c->stats.out_bytes = r.total;
    if (dev_out) *dev_out = A.out;
    return r.status;
}

// What follows the plan's passes (r: the last validation): the decoded stream's figures, or the
// chain repair, path 5 and the serial decoder.  out / cap: where the passes decoded to.
int inflate_finish(dmx_ctx* c, PlanRun& s, const InflateResult& r, const uint8_t* d_in, size_t n, uint8_t* fixed_out,
                   uint8_t* out, size_t cap, bool parallel_ok, size_t* total_out, uint8_t** dev_out, uint32_t iflags) {
    hipStream_t st = s.st;
    const uint64_t ncand = s.A.ncand;
    c->stats.segments = ncand;
    c->stats.in_bytes = n;
    if (r.status == 0) {
        end_timing(c, st);
        c->last_end = r.end_byte;
        c->stats.path = s.lead_mode == 4 ? 4 : s.lead_mode >= 2 ? 3 : s.lead_mode;
        c->stats.out_bytes = r.total;
        *total_out = r.total;
        if (dev_out) *dev_out = out;
        if (r.total > cap) return DMX_ERR_CAPACITY;
        if (c->seek_tap && s.lead_mode == 4) return seek_tap_uniform(c, s.A, r, st);
        return DMX_OK;
    }
    c->ev3_marked = false;  // (the paths below wait again: their end_timing records the end)
    if (s.lead_mode == 4 && parallel_ok && ncand > 1) {
        bool repaired = false;
        const int rc = chain_repair(s, fixed_out != nullptr, out, cap, total_out, dev_out, &repaired);
        if (rc != DMX_OK || repaired) return rc;
    }
    c->ev3_marked = false;
    if (c->inflate_pass == -1 || c->inflate_pass == 5) {
        bool handled = false;
        const int rc = inflate_fb_locked(c, d_in, n, fixed_out, cap, total_out, dev_out, st, &handled, iflags);
        if (handled) {
            end_timing(c, st);
            c->stats.path = 5;
            c->stats.in_bytes = n;
            c->stats.out_bytes = *total_out;
            return rc;
        }
    }
    return inflate_serial(c, s.A, n, fixed_out, cap, total_out, dev_out, st);
}

}  // namespace

int inflate_device_locked(dmx_ctx* c, const uint8_t* d_in, size_t n, uint8_t* fixed_out, size_t cap,
                          size_t* total_out, uint8_t** dev_out, hipStream_t st, uint32_t iflags) {
    // an asynchronous inflate still running uses the same scratch
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    begin_timing(c, st);
    *total_out = 0;
    if (n == 0) return DMX_ERR_OVERREAD;  // the reference throws (or faults) on empty input
    if (!c->scal.ensure(sizeof(Scal))) return DMX_ERR_NOMEM;
    const StreamWords w(d_in);

    Scal* const ds = c->scal.as<Scal>();

    // The speculative first pass (inflate_plan.h): into a caller's buffer whose size says the lane
    // decoder comes first, the marker list, the lane pass and its validation are launched for the
    // provisioned count before the count is known, and the call waits once.
    uint64_t ncap = 0;
    PassPlan splan{};
    bool spec = c->hres && spec_wanted(c->spec, fixed_out != nullptr, (iflags & DMX_IFLAG_PIECE) != 0,
                                       (c->diag & (DIAG_PHASES | DIAG_RECS)) != 0, c->inflate_pass, c->seg, cap);
    if (spec) {
        ncap = spec_provision(c->seg, cap, n);
        spec = cand_bufs(c, ncap);
        if (spec) splan = make_plan(c, n, ncap, true);
        spec = spec && splan.np > 0 && splan.pass[0][0] == 4;
    }

    // candidate segment starts
    uint64_t ntiles = 0, nmarkers = 0;
    const uint32_t* hl_zeroed = nullptr;
    if (const int rc = marker_scan(c, w, n, &ntiles, st, true, &hl_zeroed); rc != DMX_OK) return rc;
    bool vw_zeroed = true;
    if (spec) {
        if (marker_write(c, w, n, ntiles, ncap, st) != DMX_OK) return DMX_ERR_DEVICE;
        PlanRun s{c, st, inflate_args(c, w, n, ncap, fixed_out, cap, iflags), splan};
        s.A.ncand_dev = &ds->ncand;
        s.one_pass = true;
        s.vw_zeroed = true;
        s.hl_zeroed = hl_zeroed;
        InflateResult r{};
        if (const int rc = run_plan(s, r); rc != DMX_OK) return rc;
        vw_zeroed = false, hl_zeroed = nullptr;  // used up
        nmarkers = c->hres->nmarkers;
        const uint64_t ncand = nmarkers + 1;
        const PassPlan classic = ncand <= ncap ? make_plan(c, n, ncand, true) : PassPlan{};
        const SpecVerdict v = spec_decide(splan, classic, ncand, ncap, r.status, r.exotic);
        if (v != SpecVerdict::Discard) {
            // the pass stands as the classic plan's first: the rest of that plan, then as ever
            s.A.ncand = ncand;
            s.A.ncand_dev = nullptr;
            s.plan = classic;
            s.one_pass = false;
            if (v == SpecVerdict::Continue) {
                s.first = 1;
                if (const int rc = run_plan(s, r); rc != DMX_OK) return rc;
                s.first = 0;
            }
            return inflate_finish(c, s, r, d_in, n, fixed_out, fixed_out, cap, true, total_out, dev_out, iflags);
        }
        // discarded: today's flow from the marker list on (the count is known, the tile offsets stand)
    } else {
        if (c->hres) {
            HIPCHK(hipStreamSynchronize(st));
            nmarkers = c->hres->nmarkers;
        } else {
            HIPCHK(hipMemcpyAsync(&nmarkers, &ds->nmarkers, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    const uint64_t ncand = nmarkers + 1;
    if (!cand_bufs(c, ncand)) return DMX_ERR_NOMEM;
    if (marker_write(c, w, n, ntiles, ~0ull, st) != DMX_OK) return DMX_ERR_DEVICE;

    uint8_t* out = fixed_out;
    // The segment-parallel passes place candidate j at j * 32 KiB.  Every 00 00 FF FF inside
    // stored data is a candidate too, so a marker-dense stream can ask for more HBM than exists:
    // then the parallel plan is skipped and the serial decoder (sized by its count pass) runs.
    bool parallel_ok = true;
    if (!out) {
        size_t freeb = 0, totb = 0;
        if (hipMemGetInfo(&freeb, &totb) != hipSuccess) freeb = 0;
        const size_t want = ncand * (size_t)std::max<uint32_t>(kSegCap, c->seg);
        if ((want <= c->out.cap || want <= freeb / 2) && c->out.ensure(want)) {
            out = c->out.as<uint8_t>();
            cap = c->out.cap;
        } else {
            parallel_ok = false;
            if (!c->out.ensure(1)) return DMX_ERR_NOMEM;
            out = c->out.as<uint8_t>();
            cap = 0;
        }
    }
    PlanRun s{c, st, inflate_args(c, w, n, ncand, out, cap, iflags), PassPlan{}};
    s.A.dbg = phase_buf(c, ncand);
    s.plan = make_plan(c, n, ncand, parallel_ok);
    s.vw_zeroed = vw_zeroed;
    s.hl_zeroed = hl_zeroed;  // (make_plan may have moved the list: run_plan compares)
    InflateResult r{};
    if (const int rc = run_plan(s, r); rc != DMX_OK) return rc;
    return inflate_finish(c, s, r, d_in, n, fixed_out, out, cap, parallel_ok, total_out, dev_out, iflags);
}

// dmx_inflate_device_async: the lane path (path 4) of a libdmx-layout stream with no host
// synchronisation.  The candidate count stays on the device: the scratch is provisioned for
// cap / segment + 64 candidates (a libdmx stream has one per segment), the grids are sized for
// that many and every kernel stops at the device-side count.  No heavy route, no patch pass,
// no chain repair: any stream the lanes do not decode whole -- another layout, a declined
// segment, more candidates than provisioned, output beyond cap -- ends with status 1 in
// d_result[1], and the caller decodes it with dmx_inflate_device.
int inflate_device_async_locked(dmx_ctx* c, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap,
                                uint64_t* d_result, hipStream_t st, uint32_t iflags) {
    static const uint64_t fail[2] = {0, 1};
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    if (n == 0) {
        HIPCHK(hipMemcpyAsync(d_result, fail, 16, hipMemcpyHostToDevice, st));
        return DMX_OK;
    }
    if (!c->scal.ensure(sizeof(Scal))) return DMX_ERR_NOMEM;
    Scal* ds = c->scal.as<Scal>();
    const StreamWords w(d_in);
    const uint64_t ncap = cap / c->seg + 64;
    if (!cand_bufs(c, ncap) || !lane_bufs(c, ncap, n)) return DMX_ERR_NOMEM;
    uint64_t ntiles = 0;
    if (const int rc = marker_scan(c, w, n, &ntiles, st); rc != DMX_OK) return rc;
    HIPCHK(launch_async_prep(&ds->nmarkers, &ds->ncand, st));
    if (marker_write(c, w, n, ntiles, ncap, st) != DMX_OK) return DMX_ERR_DEVICE;
    InflateArgs A = inflate_args(c, w, n, ncap, d_out, cap, iflags);
    A.ncand_dev = &ds->ncand;
    A.mode = 4;
    A.slot = c->seg;
    if (lanes_pass(c, A, 0, 0, nullptr, st, nullptr, nullptr) != DMX_OK) return DMX_ERR_DEVICE;
    HIPCHK(launch_inflate_validate(A, &ds->vw, &ds->res, st));
    HIPCHK(launch_async_result(&ds->res, &ds->ncand, ncap, cap, d_result, st));
    HIPCHK(hipEventRecord(c->ev_inf, st));
    c->inf_pending = true;
    return DMX_OK;
}

}  // namespace dmx
