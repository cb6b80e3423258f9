// host_fb.cpp -- the host side of path 5, the block-parallel inflate of an arbitrary stream
// (inflate_blocks.hip): header scan, unit decode, the chain walk (FbPlan, inflate_plan.h),
// replay / window hand-off / resolve.  *handled = false sends the stream to the serial decoder
// (no chain from bit 0 to a BFINAL block, a unit that errors or runs out of token space, a copy
// from before the stream start): results and error codes are then the serial decoder's, i.e.
// the reference's.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "dmx_ctx.h"
#include "inflate_plan.h"

namespace dmx {
namespace {

// DMX_CFG_FB_SERIAL: path 5 decodes every unit with one wavefront (A/B reference for k_fb_pdecode)
bool fb_serial_only(const dmx_ctx* c) { return (c->flags & DMX_CFG_FB_SERIAL) != 0; }

// host-to-device copy through the context's pinned staging (see dmx_ctx::pin); the caller
// resets c->pin_off once the previous batch's copies are known complete
hipError_t pin_h2d(dmx_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st) {
    if (!bytes) return hipSuccess;
    constexpr size_t kPinCap = 1u << 20;
    if (!c->pin && hipHostMalloc(reinterpret_cast<void**>(&c->pin), kPinCap, hipHostMallocDefault) == hipSuccess)
        c->pin_cap = kPinCap;
    if (!c->pin || c->pin_off + bytes > c->pin_cap) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    uint8_t* h = c->pin + c->pin_off;
    std::memcpy(h, src, bytes);
    c->pin_off += (bytes + 255) & ~size_t(255);
    return hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, st);
}

// one call's state: the stream, the plan and the developer counters
struct FbRun {
    dmx_ctx* c;
    StreamWords in;
    size_t n;
    hipStream_t st;
    uint32_t iflags;
    FbPlan plan;
    bool debug;                        // DMX_FB_DEBUG: unit outcomes, chain breaks
    uint32_t* dstats = nullptr;        // DMX_FB_DEBUG: the decode counters
    const uint64_t* dcbit = nullptr;   // set once the regions' chunk entries exist
    // DMX_FB_HOSTTIME: host-side wall clock per phase (us)
    std::chrono::steady_clock::time_point ht[8];
    void hmark(int k) {
        if (c->diag & DIAG_FBT) ht[k] = std::chrono::steady_clock::now();
    }
};

// ---- developer dumps (DMX_FB_DEBUG, DMX_FB_HOSTTIME) ----

int dump_check(const FbRun& r, unsigned long long* cph, uint64_t nhits) {
    unsigned long long q[5];
    HIPCHK(hipMemcpyAsync(q, cph + 8, sizeof(q), hipMemcpyDeviceToHost, r.st));
    HIPCHK(hipStreamSynchronize(r.st));
    const unsigned long long w = q[4] ? q[4] : 1;
    std::fprintf(stderr, "dmx fb: k_fb_check %llu candidates, %llu waves: per wave refill %llu cycles, "
                 "steps %llu cycles, %llu steps, %.1f busy lanes per step\n", (unsigned long long)nhits, w,
                 q[0] / w, q[1] / w, q[2] / w, q[2] ? (double)q[3] / (double)q[2] : 0.0);
    return DMX_OK;
}

// the decode counters so far (cumulative over the first pass, the region units and the repair
// rounds; "longest" is the longest unit of each kind so far)
int dump_stats(const FbRun& r, const char* what, uint64_t Kn) {
    if (!r.dstats) return DMX_OK;
    uint32_t hs[16];
    unsigned long long ph[21];
    HIPCHK(hipMemcpyAsync(hs, r.dstats, 64, hipMemcpyDeviceToHost, r.st));
    HIPCHK(hipMemcpyAsync(ph, r.dstats + 16, sizeof(ph), hipMemcpyDeviceToHost, r.st));
    HIPCHK(hipStreamSynchronize(r.st));
    const uint64_t K = std::max<uint64_t>(Kn, 1);
    std::fprintf(stderr, "dmx fb [%s]: pdecode header cycles per unit: precode %llu, code lengths %llu, trees %llu, "
                 "tables %llu; longest unit: lane-parallel %llu, serial %llu, serial after a block %llu, weak %llu\n",
                 what, ph[10] / K, ph[11] / K, ph[12] / K, ph[13] / K, ph[14] >> 24, ph[15] >> 24, ph[16] >> 24,
                 ph[17] >> 24);
    std::fprintf(stderr, "dmx fb [%s]: longest lane-parallel unit: %llu settle rounds, %llu attempts; "
                 "settle re-decodes %llu cycles per unit\n",
                 what, (ph[14] >> 4) & 4095, ph[14] & 15, ph[20] / K);
    std::fprintf(stderr, "dmx fb [%s]: pdecode cycles per unit: stage %llu, header %llu, tables %llu, first pass %llu, "
                 "settle %llu (%.1f rounds, %.1f lane redos), recount %llu, scans %llu, words %llu\n",
                 what, ph[0] / K, ph[1] / K, ph[2] / K, ph[3] / K, ph[4] / K, (double)ph[8] / K, (double)ph[9] / K,
                 ph[5] / K, ph[6] / K, ph[7] / K);
    std::fprintf(stderr, "dmx fb [%s]: %llu units: %u lane-parallel, %u serial, %u serial after a parallel block, %u weak; "
                 "serial because: header %u, unsettled %u, no end of block %u, bad end %u, capacity %u, "
                 "stream-start copy %u\n",
                 what, (unsigned long long)Kn, hs[0], hs[1], hs[2], hs[3], hs[4], hs[5], hs[6], hs[7], hs[8], hs[9]);
    return DMX_OK;
}

void dump_regions(const FbPlan& p, const uint32_t* vis, const FbRegionUnits& ru) {
    for (uint64_t r = 0; r < ru.regions; r++) {
        const uint32_t rs = vis[p.nsb + r];
        std::fprintf(stderr, "dmx fb: region %llu: bits %llu..%llu, %llu super blocks, walk %s\n",
                     (unsigned long long)r, (unsigned long long)p.regs[r].E, (unsigned long long)p.regs[r].T,
                     (unsigned long long)p.regs[r].nsb,
                     rs == FB_REGION_END ? "end" : rs == FB_REGION_LINK ? "link" : "fail (cut there)");
    }
    if (!ru.ok && ru.token_space)  // (say so instead of a silent serial decode)
        std::fprintf(stderr, "dmx fb: region token space (%llu words) exhausted at unit %llu: "
                     "the serial decoder takes the stream\n",
                     (unsigned long long)p.rep_words, (unsigned long long)ru.unit);
}

void dump_chain_break(const FbPlan& p, const FbWalk& w) {
    const FbUnit& u = p.units[w.unit];
    std::fprintf(stderr, "dmx fb: chain breaks at unit %llu of %llu (%s): start %llu end %llu size %llu flags %u\n",
                 (unsigned long long)w.unit, (unsigned long long)p.Ku, w.why, (unsigned long long)u.start,
                 (unsigned long long)u.end, (unsigned long long)u.size, u.flags);
}

void dump_chain_error(const FbPlan& p, const FbWalk& w) {
    std::fprintf(stderr, "dmx fb: the chain meets a stream error at unit %llu (start %llu): %s\n",
                 (unsigned long long)w.unit, (unsigned long long)p.units[w.unit].start, dmx_strerror(w.err));
}

void dump_hosttime(const FbRun& r) {
    auto us = [&](int a, int b) { return std::chrono::duration<double, std::micro>(r.ht[b] - r.ht[a]).count(); };
    std::fprintf(stderr, "dmx fb: host us: scan+check+starts %.1f, unit setup %.1f, upload %.1f, pass-1 decode "
                 "(launch to records) %.1f, chain walk %.1f, chain upload + launches %.1f\n", us(0, 1), us(1, 2),
                 us(2, 3), us(3, 4), us(4, 5), us(5, 6));
}

// ---- the steps ----

// Header scan and check: the accepted unit starts in `hits`, sorted.  *fits = false: a scratch
// buffer did not fit (the serial decoder takes the stream).
int scan_hits(FbRun& r, std::vector<uint64_t>& hits, bool* fits) {
    dmx_ctx* c = r.c;
    hipStream_t st = r.st;
    Scal* ds = c->scal.as<Scal>();
    *fits = false;
    const uint64_t nc = fb_scan_chunks(r.n);
    if (!c->fbc.ensure(nc * 4) || !c->fbh.ensure(nc * fb_hits_per_chunk() * 8) || !c->fbo.ensure(scan_words(nc) * 8))
        return DMX_OK;
    HIPCHK(launch_fb_scan(r.in.words, r.in.misalign, r.n, c->fbc.as<uint32_t>(), c->fbh.as<uint64_t>(),
                          c->fbo.as<uint64_t>(), &ds->nmarkers, st));
    // The check appends the accepted starts to a host-mapped list, so one sync gives them (the
    // candidate count need not come back first); its grid is sized for the most the scan can
    // list.  Without that list (or when it overflows) the candidates come back in two steps.
    constexpr uint32_t kKeepCap = 1u << 20;
    if (!c->fbkeep_h) {
        void* h = nullptr;
        if (hipHostMalloc(&h, kKeepCap * 8ull, hipHostMallocMapped) == hipSuccess) {
            void* d = nullptr;
            if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
                c->fbkeep_h = static_cast<uint64_t*>(h);
                c->fbkeep_d = static_cast<uint64_t*>(d);
            } else {
                (void)hipHostFree(h);
            }
        }
    }
    const uint64_t max_hits = nc * (uint64_t)fb_hits_per_chunk();
    const bool one_sync = c->fbkeep_d && c->fbl.ensure(max_hits * 8);
    unsigned long long* cph = nullptr;  // DMX_FB_DEBUG: k_fb_check counters
    if (r.debug && c->fbph.ensure(256)) {
        cph = c->fbph.as<unsigned long long>();
        HIPCHK(hipMemsetAsync(cph, 0, 256, st));
    }
    uint64_t nhits = 0;
    bool have_hits = false;
    if (one_sync) {
        HIPCHK(hipMemsetAsync(&ds->fb_nkeep, 0, 4, st));
        HIPCHK(launch_fb_compact(r.in.words, r.in.misalign, r.n, c->fbc.as<uint32_t>(), c->fbo.as<uint64_t>(),
                                 c->fbh.as<uint64_t>(), nc, c->fbl.as<uint64_t>(), &ds->nmarkers, max_hits, cph,
                                 c->fbkeep_d, &ds->fb_nkeep, kKeepCap, st));
        uint32_t nkeep = 0;
        HIPCHK(hipMemcpyAsync(&nhits, &ds->nmarkers, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&nkeep, &ds->fb_nkeep, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (nkeep <= kKeepCap) {
            hits.assign(c->fbkeep_h, c->fbkeep_h + nkeep);
            std::sort(hits.begin(), hits.end(), [](uint64_t a, uint64_t b) {
                return (a & FB_STOP_MASK) < (b & FB_STOP_MASK);
            });
            have_hits = true;
        }
    } else {
        HIPCHK(hipMemcpyAsync(&nhits, &ds->nmarkers, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (nhits) {
            if (!c->fbl.ensure(nhits * 8)) return DMX_OK;
            HIPCHK(launch_fb_compact(r.in.words, r.in.misalign, r.n, c->fbc.as<uint32_t>(), c->fbo.as<uint64_t>(),
                                     c->fbh.as<uint64_t>(), nc, c->fbl.as<uint64_t>(), &ds->nmarkers, nhits, cph,
                                     nullptr, nullptr, 0, st));
        }
    }
    if (cph && dump_check(r, cph, nhits) != DMX_OK) return DMX_ERR_DEVICE;
    if (!have_hits && nhits) {  // the candidates with their reject marks
        hits.resize(nhits);
        HIPCHK(hipMemcpyAsync(hits.data(), c->fbl.p, nhits * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    *fits = true;
    return DMX_OK;
}

// the planned units [k0, k0 + cnt) to the device (each batch follows a stream sync) ...
int upload(FbRun& r, uint64_t k0, uint64_t cnt) {
    dmx_ctx* c = r.c;
    const FbPlan& p = r.plan;
    c->pin_off = 0;
    HIPCHK(pin_h2d(c, c->fbs.as<uint64_t>() + k0, &p.starts[k0], cnt * 8, r.st));
    HIPCHK(pin_h2d(c, c->fbstop.as<uint64_t>() + k0, &p.stops[k0], cnt * 8, r.st));
    HIPCHK(pin_h2d(c, c->fbt.as<uint64_t>() + k0, &p.tokoff[k0], (cnt + 1) * 8, r.st));
    HIPCHK(pin_h2d(c, c->fbvm.as<uint8_t>() + k0, &p.vmode[k0], cnt, r.st));
    HIPCHK(pin_h2d(c, c->fbvh.as<uint64_t>() + k0, &p.vhdr[k0], cnt * 8, r.st));
    HIPCHK(pin_h2d(c, c->fbucb.as<uint32_t>() + k0, &p.ucb[k0], cnt * 4, r.st));
    return DMX_OK;
}

// ... and their decode; the records come back into the plan
int decode(FbRun& r, uint64_t u0, uint64_t cnt) {
    dmx_ctx* c = r.c;
    HIPCHK(launch_fb_decode(r.in.words, r.in.misalign, r.n, c->fbs.as<uint64_t>(), c->fbstop.as<uint64_t>(),
                            c->fbvm.as<uint8_t>(), c->fbvh.as<uint64_t>(), r.plan.K, u0, cnt, c->fbt.as<uint64_t>(),
                            c->fbk.as<uint32_t>(), c->fbu.as<FbUnit>(), c->flags | r.iflags, !fb_serial_only(c),
                            r.dstats, r.dcbit, r.dcbit ? c->fbucb.as<uint32_t>() : nullptr, r.st));
    HIPCHK(hipMemcpyAsync(&r.plan.units[u0], c->fbu.as<FbUnit>() + u0, cnt * sizeof(FbUnit), hipMemcpyDeviceToHost,
                          r.st));
    HIPCHK(hipStreamSynchronize(r.st));
    return DMX_OK;
}

// The fixed-code regions the first pass found: the region map and walk on the device, then the
// region units.  *fits = false: the serial decoder takes the stream.
int regions(FbRun& r, bool* fits) {
    dmx_ctx* c = r.c;
    FbPlan& p = r.plan;
    hipStream_t st = r.st;
    *fits = false;
    p.select_regions();
    std::vector<uint32_t> vis;
    const uint64_t k0 = p.Ku, nreg = p.regs.size(), nsb = p.nsb;
    if (nreg) {
        const FbGeom& g = p.geom;
        if (!c->fbreg.ensure(nreg * 24 + nsb * 4) || !c->fbJ.ensure(nsb * (uint64_t)g.nodes * 4) ||
            !c->fbvis.ensure((nsb + nreg) * 4) || !c->fbJraw.ensure(nsb * (uint64_t)g.nodes * 4) ||
            !c->fbJsub.ensure(nsb * (uint64_t)g.nodes * 8) || !c->fbcbit.ensure(nsb * (uint64_t)g.entries * 8))
            return DMX_OK;
        std::vector<uint64_t> hreg(3 * nreg);
        std::vector<uint32_t> sbreg(nsb);
        for (uint64_t i = 0; i < nreg; i++) {
            hreg[3 * i] = p.regs[i].E;
            hreg[3 * i + 1] = p.regs[i].T;
            hreg[3 * i + 2] = p.regs[i].sb0;
            for (uint64_t j = 0; j < p.regs[i].nsb; j++) sbreg[p.regs[i].sb0 + j] = (uint32_t)i;
        }
        uint64_t* dreg = c->fbreg.as<uint64_t>();
        uint32_t* dsbr = reinterpret_cast<uint32_t*>(dreg + 3 * nreg);
        uint32_t* dvis = c->fbvis.as<uint32_t>();
        HIPCHK(hipMemcpyAsync(dreg, hreg.data(), nreg * 24, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dsbr, sbreg.data(), nsb * 4, hipMemcpyHostToDevice, st));
        HIPCHK(launch_fb_regions(r.in.words, r.in.misalign, r.n, dreg, (uint32_t)nreg, dsbr, nsb, c->fbJ.as<uint32_t>(),
                                 dvis, dvis + nsb, c->fbJraw.as<uint32_t>(), c->fbJsub.as<uint64_t>(),
                                 c->fbcbit.as<uint64_t>(), st));
        r.dcbit = c->fbcbit.as<uint64_t>();
        vis.resize(nsb + nreg);
        HIPCHK(hipMemcpyAsync(vis.data(), dvis, (nsb + nreg) * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    const FbRegionUnits ru = p.region_units(vis.data());
    if (r.debug) dump_regions(p, vis.data(), ru);
    if (!ru.ok) return DMX_OK;
    if (p.Ku > k0 && (upload(r, k0, p.Ku - k0) != DMX_OK || decode(r, k0, p.Ku - k0) != DMX_OK)) return DMX_ERR_DEVICE;
    if (nreg && r.debug && dump_stats(r, "region units", p.Ku) != DMX_OK) return DMX_ERR_DEVICE;
    *fits = true;
    return DMX_OK;
}

// The chain's units to the output: replay, window hand-off, resolve.  *ferr: a copy reached
// before the stream start (the serial decoder takes the stream).
int resolve(FbRun& r, const uint8_t* d_in, uint8_t* out, uint32_t* ferr) {
    dmx_ctx* c = r.c;
    const FbPlan& p = r.plan;
    hipStream_t st = r.st;
    Scal* ds = c->scal.as<Scal>();
    const uint64_t nch = p.chain.size();
    c->pin_off = 0;  // (the chain walk followed a stream sync)
    HIPCHK(pin_h2d(c, c->fbch.p, p.chain.data(), nch * 4, st));
    HIPCHK(pin_h2d(c, c->fbco.p, p.coffs.data(), nch * 8, st));
    HIPCHK(pin_h2d(c, c->fbcs.p, p.csizes.data(), nch * 8, st));
    HIPCHK(hipMemsetAsync(&ds->fb_err, 0, 4, st));
    // the parallel window hand-off when its scratch fits (nch * 128 KiB), else the serial one
    uint32_t *win = nullptr, *open = nullptr;
    const uint64_t went = fb_window_entries(nch);
    if (went && !fb_serial_only(c) && c->fbwin.ensure(went * 4) && c->fbopen.ensure(fb_window_rounds(nch) * 4)) {
        win = c->fbwin.as<uint32_t>();
        open = c->fbopen.as<uint32_t>();
    }
    unsigned long long* uph = nullptr;
    if (r.debug && c->fbph.ensure(256)) {
        uph = c->fbph.as<unsigned long long>();
        HIPCHK(hipMemsetAsync(uph, 0, 64, st));
    }
    HIPCHK(launch_fb_resolve(d_in, c->fbs.as<uint64_t>(), c->fbch.as<uint32_t>(), c->fbco.as<uint64_t>(),
                             c->fbcs.as<uint64_t>(), nch, c->fbt.as<uint64_t>(), c->fbk.as<uint32_t>(),
                             c->fbu.as<FbUnit>(), c->fbimg.as<uint16_t>(), p.total, out, &ds->fb_err, win, open,
                             !fb_serial_only(c), uph, st));
    if (uph) {
        unsigned long long ph[5];
        HIPCHK(hipMemcpyAsync(ph, uph, sizeof(ph), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        std::fprintf(stderr, "dmx fb: k_fb_units cycles per unit: batches %llu, expansion %llu, jumping %llu (%llu rounds "
                     "in all), write-out %llu\n", ph[0] / nch, ph[1] / nch, ph[2] / nch, ph[4], ph[3] / nch);
    }
    r.hmark(6);
    if (c->diag & DIAG_FBT) dump_hosttime(r);
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    HIPCHK(hipMemcpyAsync(ferr, &ds->fb_err, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DMX_OK;
}

}  // namespace

int inflate_fb_locked(dmx_ctx* c, const uint8_t* d_in, size_t n, uint8_t* fixed_out, size_t cap,
                      size_t* total_out, uint8_t** dev_out, hipStream_t st, bool* handled, uint32_t iflags) {
    *handled = false;
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    FbRun r{c, StreamWords(d_in), n, st, iflags,
            FbPlan(n, {fb_region_super_bits(), fb_region_chunk_bits(), fb_region_nodes(), fb_region_entries()}),
            (c->diag & DIAG_FB) != 0};
    FbPlan& p = r.plan;
    r.hmark(0);
    bool fits = false;
    {
        std::vector<uint64_t> hits;
        if (const int rc = scan_hits(r, hits, &fits); rc != DMX_OK || !fits) return rc;
        r.hmark(1);
        p.from_hits(hits.data(), hits.size());
    }
    p.budgets();
    const uint64_t Kcap = p.Kcap;
    if (!c->fbs.ensure(Kcap * 8) || !c->fbt.ensure((Kcap + 1) * 8) || !c->fbk.ensure((p.tokoff[p.K] + p.rep_words) * 4) ||
        !c->fbu.ensure(Kcap * sizeof(FbUnit)) || !c->fbstop.ensure(Kcap * 8) || !c->fbvm.ensure(Kcap) ||
        !c->fbvh.ensure(Kcap * 8) || !c->fbucb.ensure(Kcap * 4))
        return DMX_OK;
    r.hmark(2);
    if (upload(r, 0, p.K) != DMX_OK) return DMX_ERR_DEVICE;
    r.hmark(3);
    if (r.debug && c->fbopen.ensure(256)) {
        r.dstats = c->fbopen.as<uint32_t>();
        HIPCHK(hipMemsetAsync(r.dstats, 0, 256, st));
    }
    if (decode(r, 0, p.K) != DMX_OK) return DMX_ERR_DEVICE;
    r.hmark(4);
    if (dump_stats(r, "first pass", p.K) != DMX_OK) return DMX_ERR_DEVICE;
    if (const int rc = regions(r, &fits); rc != DMX_OK || !fits) return rc;
    // walk the chain; every round that finds breaks decodes their repair units and walks again
    for (int round = 0;; round++) {
        const FbWalk w = p.walk(round);
        if (w.kind == FbWalk::DONE) break;
        if (w.kind == FbWalk::DECLINE) {
            if (r.debug) dump_chain_break(p, w);
            return DMX_OK;
        }
        if (w.kind == FbWalk::STREAM_ERROR) {
            if (r.debug) dump_chain_error(p, w);
            *handled = true;
            *total_out = 0;
            c->stats.segments = p.chain.size();
            return w.err;
        }
        if (upload(r, w.k0, p.Ku - w.k0) != DMX_OK || decode(r, w.k0, p.Ku - w.k0) != DMX_OK) return DMX_ERR_DEVICE;
        if (r.debug) {
            std::fprintf(stderr, "dmx fb: repair round %d: %llu units\n", round, (unsigned long long)(p.Ku - w.k0));
            if (dump_stats(r, "after repair round", p.Ku) != DMX_OK) return DMX_ERR_DEVICE;
        }
    }
    // the path's own scratch first: when it does not fit, the stream still decodes on the
    // serial decoder, which needs only the output
    const uint64_t nch = p.chain.size(), total = p.total;
    if (!c->fbch.ensure(nch * 4) || !c->fbco.ensure(nch * 8) || !c->fbcs.ensure(nch * 8) ||
        !c->fbimg.ensure(total * 2 + 16))
        return DMX_OK;
    *handled = true;
    *total_out = total;
    uint8_t* out = fixed_out;
    if (!out) {
        if (!c->out.ensure(total ? total : 1)) return DMX_ERR_NOMEM;
        out = c->out.as<uint8_t>();
    } else if (total > cap) {
        return DMX_ERR_CAPACITY;
    }
    r.hmark(5);
    uint32_t ferr = 0;
    if (const int rc = resolve(r, d_in, out, &ferr); rc != DMX_OK) return rc;
    if (ferr) {
        *handled = false;
        *total_out = 0;
        return DMX_OK;
    }
    c->stats.segments = nch;
    c->last_end = (p.units[p.chain.back()].end + 7) / 8;
    if (c->seek_tap) {  // the index's checkpoints: the chain members that start at a block header
        c->seek_tap->cands.clear();
        for (uint64_t k = 0; k < nch; k++)
            if (p.expects(p.chain[k]) == FB_AT_HEADER)
                c->seek_tap->cands.push_back({p.units[p.chain[k]].start, p.coffs[k], false});
    }
    if (dev_out) *dev_out = out;
    return DMX_OK;
}

}  // namespace dmx
