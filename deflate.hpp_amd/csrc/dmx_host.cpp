// dmx_host.cpp -- host runtime and C-ABI of libdmx (see include/dmx.h): the context, the deflate
// side, the batch calls, the containers, the files, multi-GPU.  The inflate drivers are in
// host_inflate.cpp and host_fb.cpp; dmx_ctx.h holds what they share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <thread>
#include <cstdlib>
#include <vector>
#include <cstring>
#include <mutex>
#include <new>
#include <string>

#include "dmx_ctx.h"

using namespace dmx;

namespace dmx {

const Diag& diag_env() {  // first use (a dmx_create) reads the environment
    static const Diag d = [] {
        Diag r;
        if (std::getenv("DMX_DEBUG")) r.bits |= DIAG_DEBUG;
        if (const char* e = std::getenv("DMX_PHASES")) r.bits |= DIAG_PHASES, r.phases_path = e;
        if (const char* e = std::getenv("DMX_FB_DEBUG"); e && *e) r.bits |= DIAG_FB;
        if (const char* e = std::getenv("DMX_FB_HOSTTIME"); e && *e) r.bits |= DIAG_FBT;
        if (std::getenv("DMX_RECS")) r.bits |= DIAG_RECS;
        return r;
    }();
    return d;
}
void hipchk_report(const char* what, hipError_t e, const char* file, int line) {
    if (diag_env().bits & DIAG_DEBUG)
        std::fprintf(stderr, "dmx: %s failed (%s:%d): %s\n", what, file, line, hipGetErrorString(e));
}

uint64_t* phase_buf(dmx_ctx* c, uint64_t nidx) {
    if (!(c->diag & DIAG_PHASES)) return nullptr;
    if (!c->dbg.ensure(nidx * kPhaseSlots * 8)) return nullptr;
    (void)hipMemset(c->dbg.p, 0, nidx * kPhaseSlots * 8);
    return c->dbg.as<uint64_t>();
}
void phase_dump(dmx_ctx* c, const char* kernel, uint64_t nidx, hipStream_t st, uint64_t stride) {
    if (!(c->diag & DIAG_PHASES) || !c->dbg.p) return;
    const char* path = diag_env().phases_path.c_str();
    std::vector<uint64_t> h(nidx * kPhaseSlots);
    (void)hipStreamSynchronize(st);
    (void)hipMemcpy(h.data(), c->dbg.p, h.size() * 8, hipMemcpyDeviceToHost);
    double sum[kPhaseSlots] = {0}, xsum[kPhaseSlots] = {0};
    uint64_t xcnt[kPhaseSlots] = {0};
    uint64_t cnt[kPhaseSlots] = {0};
    const bool inf = std::string(kernel) == "inflate";
    for (uint64_t i = 0; i < nidx; i++) {
        const uint64_t* r = &h[i * kPhaseSlots];
        uint64_t prev = r[0];
        for (int k = 1; k < (inf ? 8 : 12); k++) {
            if (!r[k]) continue;
            sum[k] += (double)(r[k] - prev);
            cnt[k]++;
            prev = r[k];
        }
        if (inf) {  // slots 8..10: raw per-segment values (header cycles / settle and jump rounds)
            for (int k = 8; k < 16; k++) { xsum[k] += (double)r[k]; xcnt[k]++; }
        }
        if (!inf && r[12] && r[13] && r[3] && r[14]) {  // Huffman build sub-phases, match rounds
            sum[12] += (double)(r[12] - r[3]); cnt[12]++;
            sum[13] += (double)(r[13] - r[12]); cnt[13]++;
            sum[14] += (double)(r[14] - r[1]); cnt[14]++;
        }
    }
    FILE* f = std::fopen(path, "a");
    if (!f) return;
    std::fprintf(f, "%s %llu", kernel, (unsigned long long)nidx);
    for (int k = 1; k < kPhaseSlots; k++) std::fprintf(f, " p%d=%.0f", k, cnt[k] ? sum[k] / cnt[k] : 0.0);
    if (!inf) {  // timeline: mean cycles from slot 0 to every recorded slot (developer aid)
        for (int k = 1; k < kPhaseSlots; k++) {
            double a = 0;
            uint64_t m = 0;
            for (uint64_t i = 0; i < nidx; i++) {
                const uint64_t* r = &h[i * kPhaseSlots];
                if (r[k] && r[0] && r[k] >= r[0]) { a += (double)(r[k] - r[0]); m++; }
            }
            if (m) std::fprintf(f, " t%d=%.0f", k, a / m);
        }
        // Persistent workgroups (stride = the grid): what no phase counts, between a segment and
        // the workgroup's next one.  gap: from the token words' end (slot 11) to the next
        // segment's loaded image (its slot 1); gap0: from the segment's last stamp (slot 10) to
        // the next one's first (slot 0), the loop's closing barrier
        if (stride && stride < nidx) {
            double g = 0, g0 = 0;
            uint64_t m = 0;
            for (uint64_t i = 0; i + stride < nidx; i++) {
                const uint64_t *r = &h[i * kPhaseSlots], *q = &h[(i + stride) * kPhaseSlots];
                if (!r[11] || !r[10] || q[1] < r[11] || q[0] < r[10]) continue;
                g += (double)(q[1] - r[11]);
                g0 += (double)(q[0] - r[10]);
                m++;
            }
            if (m) std::fprintf(f, " gap=%.0f gap0=%.0f", g / m, g0 / m);
        }
    }
    if (inf)
        for (int k = 8; k < kPhaseSlots; k++) std::fprintf(f, " x%d=%.1f", k, xcnt[k] ? xsum[k] / xcnt[k] : 0.0);

    std::fprintf(f, "\n");
    std::fclose(f);
}

void begin_timing(dmx_ctx* c, hipStream_t st) {
    c->stats = dmx_stats{};
    c->ev3_marked = false;
    if (c->timing) (void)hipEventRecord(c->ev[0], st);
}
void mark_end(dmx_ctx* c, hipStream_t st) {
    if (!c->timing) return;
    (void)hipEventRecord(c->ev[3], st);
    c->ev3_marked = true;
}
void end_timing(dmx_ctx* c, hipStream_t st) {
    if (!c->timing) return;
    if (!c->ev3_marked) {  // (marked: recorded in front of the wait the caller has just done)
        (void)hipEventRecord(c->ev[3], st);
        (void)hipEventSynchronize(c->ev[3]);
    }
    c->ev3_marked = false;
    float a = 0, b = 0;
    (void)hipEventElapsedTime(&a, c->ev[0], c->ev[3]);
    (void)hipEventElapsedTime(&b, c->ev[1], c->ev[2]);
    (void)hipGetLastError();  // a failed query must not surface in the caller's next HIP call
    c->stats.ms_device_total = a;
    c->stats.ms_main_kernel = b;
}

}  // namespace dmx

namespace {

// The deflate's scratch for nseg segments, of which the front kernel sees nfront of fseg_bytes
// each, and the scratch half of its arguments.  false: out of device memory.
bool deflate_scratch(dmx_ctx* c, DeflateArgs& A, uint64_t nseg, uint64_t nfront, int level, uint32_t fseg_bytes) {
    const uint64_t ns = std::max<uint64_t>(1, nseg), nf = std::max<uint64_t>(1, nfront);
    A.nseg = nseg;
    A.level = level;
    A.slot_bytes = c->seg + 256;
    A.tok_stride = level >= 2 ? deflate_tok_stride(fseg_bytes) : 0u;
    if (!c->slots.ensure(ns * (size_t)A.slot_bytes) || !c->sizes.ensure(ns * 4) || !c->offs.ensure(scan_words(nseg) * 8) ||
        !c->dtok.ensure(std::max<uint64_t>(1, nfront * (uint64_t)A.tok_stride) * 4) || !c->dntok.ensure(nf * 4))
        return false;
    A.slots = c->slots.as<uint8_t>();
    A.tok = c->dtok.as<uint32_t>();
    A.ntok = c->dntok.as<uint32_t>();
    A.sizes = c->sizes.as<uint32_t>();
    A.offsets = c->offs.as<uint64_t>();
    return true;
}

// The chunk pipeline's side stream and events, made by the first call that takes the pipeline:
// non-blocking, at the device's lowest priority, so that the dispatcher places a front workgroup
// before the emission waves that fill what it leaves.
bool pipe_streams(dmx_ctx* c) {
    if (c->side) return true;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);  // (lo: the numerically greatest, the lowest priority)
    if (hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, lo) != hipSuccess) {
        c->side = nullptr;
        return false;
    }
    if (hipEventCreateWithFlags(&c->ev_chunk, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_side, hipEventDisableTiming) != hipSuccess) {
        if (c->ev_chunk) (void)hipEventDestroy(c->ev_chunk);
        (void)hipStreamDestroy(c->side);
        c->side = nullptr, c->ev_chunk = c->ev_side = nullptr;
        return false;
    }
    return true;
}

// d_total != nullptr: asynchronous (dmx_deflate_device_async): the length goes to that device
// word, nothing waits for the work.  Every deflate on a context waits for the previous one's work
// (ev_df), whatever streams they run on: the slots, sizes and token words are reused.
int deflate_device_locked(dmx_ctx* c, const uint8_t* d_in, size_t n, int level, uint32_t flags,
                          uint8_t* d_out, size_t cap, size_t* out_len, hipStream_t st,
                          uint64_t* d_total = nullptr) {
    if (level < 0 || level > 3) level = 1;  // reference switch has no default (deflate.hpp:699)
    const bool final_last = (flags & DMX_DEFLATE_NOT_FINAL) == 0;
    const bool async = d_total != nullptr;
    if (c->df_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_df, 0));
    if (!async) begin_timing(c, st);
    if (n == 0) {
        // empty input: one empty fixed-Huffman final block, as the reference's levels 1-3
        static const uint8_t empty_final[2] = {0x03, 0x00};
        static const uint64_t lens[2] = {0, 2};
        if (out_len) *out_len = final_last ? 2 : 0;
        if (async) {
            if (final_last && cap >= 2) HIPCHK(hipMemcpyAsync(d_out, empty_final, 2, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_total, &lens[final_last ? 1 : 0], 8, hipMemcpyHostToDevice, st));
            return DMX_OK;
        }
        if (!final_last) return DMX_OK;
        if (cap < 2) return DMX_ERR_CAPACITY;
        HIPCHK(hipMemcpyAsync(d_out, empty_final, 2, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        return DMX_OK;
    }
    const uint64_t nseg = (n + c->seg - 1) / c->seg;
    // the front kernel's segments: 64 KiB blocks are matched as two 32 KiB halves
    const uint32_t fseg_bytes = std::min<uint32_t>(c->seg, 32768);
    DeflateArgs A;
    if (!c->scal.ensure(sizeof(Scal)) || !deflate_scratch(c, A, nseg, (n + fseg_bytes - 1) / fseg_bytes, level, fseg_bytes))
        return DMX_ERR_NOMEM;
    A.in = d_in;
    A.n = n;
    A.final_last = final_last ? 1 : 0;
    A.total = async ? d_total : &c->scal.as<Scal>()->total;
    A.out = d_out;
    A.cap = cap;
    A.dbg = async ? nullptr : phase_buf(c, nseg);
    const bool tm = c->timing && !async;
    // the chunk pipeline (deflate_pipe.h): levels 2-3 of 32 KiB segments from two front grids'
    // worth of segments.  64 KiB blocks (measured 1.3 % slower with it) and the
    // asynchronous call (not measured) take it only when the knob asks for it.
    DeflatePipe P{0, nullptr, nullptr, nullptr};
    if (c->pipe.on && level >= 2 && !A.dbg &&
        (c->pipe.explicit_on ? c->seg >= 32768 : c->seg == 32768 && !async)) {
        P.chunk = pipe_chunk_segs(nseg, deflate_front_fit(c->seg), c->pipe.chunks, c->pipe.forced);
        if (P.chunk && !pipe_streams(c)) return DMX_ERR_DEVICE;
        P.side = c->side, P.ev_chunk = c->ev_chunk, P.ev_side = c->ev_side;
    }
    // the synchronous call reads the length from the host result block (k_scan_apply stores it
    // there too): no copy operation behind the work
    uint64_t* const total_host = (!async && c->hres) ? &c->hres_dev->total : nullptr;
    HIPCHK(launch_deflate(A, c->seg, st, tm ? c->ev[1] : nullptr, tm ? c->ev[2] : nullptr, false, nullptr, nullptr,
                          P.chunk ? &P : nullptr, total_host));
    HIPCHK(hipEventRecord(c->ev_df, st));
    c->df_pending = true;
    if (async) return DMX_OK;
    if (A.dbg) phase_dump(c, "deflate", nseg, st, c->seg == 65536 ? 0 : std::min<uint64_t>(nseg, deflate_front_fit(c->seg)));
    uint64_t total = 0;
    if (!total_host) HIPCHK(hipMemcpyAsync(&total, A.total, 8, hipMemcpyDeviceToHost, st));
    mark_end(c, st);
    HIPCHK(hipStreamSynchronize(st));
    if (total_host) total = c->hres->total;
    end_timing(c, st);
    c->stats.segments = nseg;
    c->stats.in_bytes = n;
    c->stats.out_bytes = total;
    *out_len = total;
    return total > cap ? DMX_ERR_CAPACITY : DMX_OK;
}

// ---- batched calls (dmx_deflate_batch_device / dmx_inflate_batch_device) ----------------------

// Batch deflate: one segment table over all buffers (DESIGN "Batched API"), uploaded with the
// per-buffer arrays in one copy; one front launch, one emit launch, one scan and k_compact_batch
// cover the batch, and the results come back in the call's only host synchronisation.
// A preset dictionary (d_dict, dict_len > 0; 32 KiB segments): at levels 2 and 3 the first
// segment of every buffer takes seg - Du bytes, Du = min(dict_len, kDeflateDictMax), and carries
// the dictionary's last Du bytes (DeflateBatchSeg); the later segments are ordinary -- the
// dictionary has left their window.  The segment count stays <= ceil(n / 16384), which
// dmx_deflate_bound allows for.  Levels 0 and 1 have no matcher: their table is the plain one.
// A framed call (fp != nullptr, dmx_deflate_batch_framed_device): the arrays describe the raw
// streams inside the frames; after the deflate, k_checksum_batch sums the plain inputs and
// k_frame_write adds headers and trailers and rewrites the results, before the one read-back.
struct FramePlan {
    uint32_t format;                // DMX_FRAME_*
    int level;                      // deflate: the level the header states
    bool verify;                    // inflate: DMX_BATCH_VERIFY
    const InflateBatchDesc* hdesc;  // deflate: count x {plain input, size, framed output, capacity}
};
int checksum_locked(dmx_ctx* c, bool crc, const uint8_t* d, size_t n, uint32_t init, uint32_t* out, hipStream_t st);

int deflate_batch_locked(dmx_ctx* c, const uint8_t* const* d_in, const size_t* n, size_t count, int level,
                         uint8_t* const* d_out, const size_t* cap, dmx_batch_result* res, hipStream_t st,
                         const uint8_t* d_dict = nullptr, size_t dict_len = 0, const FramePlan* fp = nullptr) {
    if (level < 0 || level > 3) level = 1;  // as deflate_device_locked
    const uint32_t seg = c->seg;
    const uint32_t du = level >= 2 ? (uint32_t)std::min<size_t>(dict_len, kDeflateDictMax) : 0u;
    if (du && seg != 32768) return DMX_ERR_ARG;
    const uint8_t* const dtail = du ? d_dict + (dict_len - du) : nullptr;
    const size_t seg0 = seg - du;  // bytes of a buffer's first segment
    uint64_t nseg = 0;
    for (size_t i = 0; i < count; i++) {
        if ((!d_in[i] && n[i]) || (!d_out[i] && cap[i])) return DMX_ERR_ARG;
        nseg += n[i] <= seg0 ? (n[i] ? 1 : 0) : 1 + (n[i] - seg0 + seg - 1) / seg;
    }
    // host image of the upload: segment table | first segment of each buffer | outputs | capacities
    const size_t off_first = nseg * sizeof(DeflateBatchSeg);
    const size_t off_out = off_first + (count + 1) * 8, off_cap = off_out + count * 8, bytes = off_cap + count * 8;
    std::vector<uint64_t> image;
    try {
        image.resize(bytes / 8);
    } catch (const std::bad_alloc&) {
        return DMX_ERR_NOMEM;
    }
    static_assert(sizeof(DeflateBatchSeg) == 40 && sizeof(void*) == 8, "the upload image is built from 8-byte words");
    uint8_t* const img = reinterpret_cast<uint8_t*>(image.data());
    DeflateBatchSeg* tab = reinterpret_cast<DeflateBatchSeg*>(img);
    uint64_t* first = reinterpret_cast<uint64_t*>(img + off_first);
    uint64_t s = 0;
    for (size_t i = 0; i < count; i++) {
        first[i] = s;
        for (size_t o = 0, len = seg0; o < n[i]; o += len, len = seg, s++) {
            const size_t rest = n[i] - o;
            tab[s].src = d_in[i] + o;
            tab[s].tail = rest;
            tab[s].nb = (uint32_t)std::min<size_t>(len, rest);
            tab[s].buf = (uint32_t)i | (rest <= len ? DF_BATCH_LAST : 0u);
            tab[s].dict = o == 0 ? dtail : nullptr;
            tab[s].dlen = o == 0 ? du : 0u;
        }
        reinterpret_cast<uint64_t*>(img + off_out)[i] = (uint64_t)(uintptr_t)d_out[i];
        reinterpret_cast<uint64_t*>(img + off_cap)[i] = cap[i];
    }
    first[count] = s;

    if (c->df_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_df, 0));
    begin_timing(c, st);
    DeflateArgs A;
    // results | (framed) the checksum kernel's ticket | one FrameHead per buffer
    const size_t res_bytes = count * sizeof(dmx_batch_result);
    if (!c->btab.ensure(bytes) || !c->bres.ensure(res_bytes + (fp ? 16 + count * sizeof(FrameHead) : 0)) ||
        (fp && !c->fdesc.ensure(count * sizeof(InflateBatchDesc))) || !deflate_scratch(c, A, nseg, nseg, level, seg))
        return DMX_ERR_NOMEM;
    HIPCHK(hipMemcpyAsync(c->btab.p, img, bytes, hipMemcpyHostToDevice, st));
    if (fp)
        HIPCHK(hipMemcpyAsync(c->fdesc.p, fp->hdesc, count * sizeof(InflateBatchDesc), hipMemcpyHostToDevice, st));
    uint8_t* const dimg = c->btab.as<uint8_t>();
    A.in = nullptr;
    A.n = 0;
    A.final_last = 1;
    A.total = c->offs.as<uint64_t>() + nseg;  // the scan's total follows the offsets (scan_words)
    A.out = nullptr;
    A.cap = 0;
    A.dbg = nullptr;
    A.btab = reinterpret_cast<const DeflateBatchSeg*>(dimg);
    A.bfirst = reinterpret_cast<const uint64_t*>(dimg + off_first);
    A.bout = reinterpret_cast<uint8_t* const*>(dimg + off_out);
    A.bcap = reinterpret_cast<const uint64_t*>(dimg + off_cap);
    A.bres = c->bres.as<dmx_batch_result>();
    A.nbuf = count;
    HIPCHK(launch_deflate(A, seg, st, c->timing ? c->ev[1] : nullptr, c->timing ? c->ev[2] : nullptr, du != 0));
    if (fp) {
        unsigned int* const d_ticket = reinterpret_cast<unsigned int*>(c->bres.as<uint8_t>() + res_bytes);
        FrameHead* const d_side = reinterpret_cast<FrameHead*>(c->bres.as<uint8_t>() + res_bytes + 16);
        HIPCHK(launch_checksum_batch(c->fdesc.as<InflateBatchDesc>(), nullptr, d_side, count,
                                     fp->format != DMX_FRAME_ZLIB, d_ticket, st));
        HIPCHK(launch_frame_write(c->fdesc.as<InflateBatchDesc>(), d_side, A.bres, count, fp->format, fp->level, st));
    }
    HIPCHK(hipEventRecord(c->ev_df, st));
    c->df_pending = true;
    HIPCHK(hipMemcpyAsync(res, c->bres.p, res_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    end_timing(c, st);
    c->stats.segments = nseg;
    for (size_t i = 0; i < count; i++) {
        c->stats.in_bytes += n[i];
        c->stats.out_bytes += res[i].bytes;
    }
    return DMX_OK;
}

// Streams above this many compressed bytes leave the batch kernel for the single-stream plan:
// one wavefront is the wrong tool for a long stream, which the segmented and block-parallel
// decoders spread over the whole device.  Measured (profiles/batch_probe.json): for
// ONE stream alone the single-stream plan wins at every probed size (64 KiB of text: 0.32 ms
// against 7.7 ms on one wavefront), so a latency crossover would lie below the smallest probe;
// but a routed stream costs ~0.3 ms of serial, host-driven time, and in a batch of many streams
// the batch kernel wins by throughput (4096 x 64 KiB: 32 ms against 1184 ms for the loop).  The
// threshold therefore only bounds how long one stream may hold the batch's tail: 1 MiB of
// compressed input is ~0.3 s on one wavefront.  A rule that weighs the batch's size is the
// follow-up.  (kBatchRouteBytes: dmx_internal.h, shared with the multi-member gzip call.)

// Batch inflate: k_inflate_batch decodes the streams it keeps, longest first; the routed ones
// follow through inflate_device_locked, one after another.
// A preset dictionary (d_dict, dict_len > 0): the batch kernel pre-fills every stream's window
// with its last min(dict_len, kInflateDictMax) bytes.  The single-stream plan knows no
// dictionary, so no stream is routed then, whatever its size.
int inflate_batch_locked(dmx_ctx* c, const uint8_t* const* d_in, const size_t* n, size_t count,
                         uint8_t* const* d_out, const size_t* cap, dmx_batch_result* res, uint32_t flags,
                         hipStream_t st, const uint8_t* d_dict = nullptr, size_t dict_len = 0,
                         const FramePlan* fp = nullptr) {
    std::vector<uint32_t> order, routed;
    std::vector<uint64_t> image, back;
    const size_t off_order = count * sizeof(InflateBatchDesc);
    const uint32_t dl = (uint32_t)std::min<size_t>(dict_len, kInflateDictMax);
    try {
        for (size_t i = 0; i < count; i++) {
            if ((!d_in[i] && n[i]) || (!d_out[i] && cap[i])) return DMX_ERR_ARG;
            const bool route = !dl && !(flags & DMX_BATCH_NO_ROUTE) && n[i] > kBatchRouteBytes && d_out[i];
            (route ? routed : order).push_back((uint32_t)i);
        }
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return n[a] > n[b]; });
        image.resize((off_order + order.size() * 4 + 7) / 8);
        if (fp) back.resize((count * (sizeof(dmx_batch_result) + sizeof(FrameHead)) + 32) / 8);
    } catch (const std::bad_alloc&) {
        return DMX_ERR_NOMEM;
    }
    static_assert(sizeof(InflateBatchDesc) == 32, "the upload image is built from 8-byte words");
    uint8_t* const img = reinterpret_cast<uint8_t*>(image.data());
    InflateBatchDesc* desc = reinterpret_cast<InflateBatchDesc*>(img);
    for (size_t i = 0; i < count; i++) desc[i] = InflateBatchDesc{d_in[i], n[i], d_out[i], cap[i]};
    if (!order.empty()) std::memcpy(img + off_order, order.data(), order.size() * 4);

    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    begin_timing(c, st);
    const size_t res_bytes = count * sizeof(dmx_batch_result);
    // results | the decoder's ticket | (framed) the checksum kernel's ticket | one FrameHead per buffer
    const size_t back_bytes = fp ? res_bytes + 32 + count * sizeof(FrameHead) : res_bytes;
    if (!c->btab.ensure(image.size() * 8) || !c->bres.ensure(back_bytes + 16)) return DMX_ERR_NOMEM;
    HIPCHK(hipMemcpyAsync(c->btab.p, img, image.size() * 8, hipMemcpyHostToDevice, st));
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    const uint32_t* const d_order = reinterpret_cast<const uint32_t*>(c->btab.as<uint8_t>() + off_order);
    unsigned int* const d_ticket = reinterpret_cast<unsigned int*>(c->bres.as<uint8_t>() + res_bytes);
    FrameHead* const d_side = reinterpret_cast<FrameHead*>(c->bres.as<uint8_t>() + res_bytes + 32);
    if (fp) {
        // a routed stream's result is not written on the device: status -1 keeps it out of the
        // checksum launch, and the host fills it in below
        HIPCHK(hipMemsetAsync(c->bres.p, 0xFF, res_bytes, st));
        HIPCHK(launch_frame_parse(c->btab.as<InflateBatchDesc>(), d_side, count, fp->format, st));
    }
    if (dl)
        HIPCHK(launch_inflate_batch_dict(c->btab.as<InflateBatchDesc>(), d_order, order.size(),
                                         c->bres.as<dmx_batch_result>(), d_ticket, c->flags,
                                         d_dict + (dict_len - dl), dl, st));
    else
        HIPCHK(launch_inflate_batch(c->btab.as<InflateBatchDesc>(), d_order, order.size(),
                                    c->bres.as<dmx_batch_result>(), d_ticket, c->flags, st));
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    if (fp) {
        if (fp->verify)
            HIPCHK(launch_checksum_batch(c->btab.as<InflateBatchDesc>(), c->bres.as<dmx_batch_result>(), d_side, count,
                                         fp->format != DMX_FRAME_ZLIB, d_ticket + 4, st));
        HIPCHK(launch_frame_verdict(d_side, c->bres.as<dmx_batch_result>(), count, fp->format, fp->verify, st));
    }
    HIPCHK(hipEventRecord(c->ev_inf, st));
    c->inf_pending = true;
    // (framed: the side array rides in the same copy, for the routed streams' headers and trailers)
    HIPCHK(hipMemcpyAsync(fp ? (void*)back.data() : (void*)res, c->bres.p, back_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    end_timing(c, st);
    if (fp) std::memcpy(res, back.data(), res_bytes);
    const FrameHead* const side =
        fp ? reinterpret_cast<const FrameHead*>(reinterpret_cast<const uint8_t*>(back.data()) + res_bytes + 32) : nullptr;
    const dmx_stats batch_stats = c->stats;
    for (const uint32_t i : routed) {  // (each call synchronises on its own)
        if (fp && side[i].status != DMX_OK) continue;  // a header error: k_frame_verdict reported it
        const size_t head = fp ? (size_t)side[i].head : 0;
        size_t len = 0;
        int rc = inflate_device_locked(c, d_in[i] + head, n[i] - head, d_out[i], cap[i], &len, nullptr, st);
        if (rc == DMX_ERR_NOMEM || rc == DMX_ERR_DEVICE) return rc;
        const uint32_t path = c->stats.path;
        if (fp && fp->verify && rc == DMX_OK) {  // the single-buffer launches: this stream synchronises anyway
            const bool gz = fp->format != DMX_FRAME_ZLIB;
            uint32_t ck = 0;
            const int rk = checksum_locked(c, gz, d_out[i], len, gz ? 0u : 1u, &ck, st);
            if (rk != DMX_OK) return rk;
            if ((gz && side[i].isize != (uint32_t)len) || ck != side[i].want) rc = DMX_ERR_CHECKSUM;
        }
        res[i].bytes = len;
        res[i].status = rc;
        res[i].path = path;
    }
    c->stats = batch_stats;
    c->stats.segments = count;
    for (size_t i = 0; i < count; i++) {
        c->stats.in_bytes += n[i];
        if (res[i].status == DMX_OK) c->stats.out_bytes += res[i].bytes;
    }
    return DMX_OK;
}

// ---- batches from device-resident descriptors (dmx_deflate_batch_async / dmx_inflate_batch_async)
// The pointer, size and capacity arrays stay on the device: batch_table.hip builds the segment
// table / the descriptors and the order list there, the batch kernels stop at device-side counts
// and write the caller's d_res themselves.  The host sizes grids and scratch from count, max_n
// and max_total alone; once the scratch is large enough a call only enqueues.  The tables live in
// buffers of their own (c->adf, c->ainf): the synchronous calls' c->btab / c->bres serve both
// directions and are safe only because those calls end synchronised.

// the deflate's table capacity for a shape (batch_table.h), at least 1
int async_deflate_capacity(const dmx_ctx* c, size_t count, size_t max_n, size_t max_total, uint32_t du,
                           uint64_t* cap) {
    if (bt_segments(max_n, c->seg, du) >= (uint64_t)DF_BATCH_LAST) return DMX_ERR_ARG;  // (a buffer's count is 32 bits)
    *cap = std::max<uint64_t>(1, bt_capacity(count, max_n, max_total, c->seg, du));
    return *cap < (uint64_t)DF_BATCH_LAST ? DMX_OK : DMX_ERR_NOMEM;  // (its slots alone would be 64 TiB)
}

struct AsyncSegTab {  // c->adf: table | bfirst (scan_words(count)) | counts | the segment count | flags
    DeflateBatchSeg* tab;
    uint64_t* bfirst;
    uint32_t* counts;
    uint64_t* nseg;
    uint8_t* flag;
};
bool async_deflate_scratch(dmx_ctx* c, DeflateArgs& A, AsyncSegTab& T, size_t count, uint64_t cap, int level) {
    const size_t off_first = cap * sizeof(DeflateBatchSeg), off_counts = off_first + scan_words(count) * 8;
    const size_t off_nseg = off_counts + (count * 4 + 7) / 8 * 8, off_flag = off_nseg + 8;
    if (!c->adf.ensure(off_flag + count) || !deflate_scratch(c, A, cap, cap, level, c->seg)) return false;
    uint8_t* const base = c->adf.as<uint8_t>();
    T.tab = reinterpret_cast<DeflateBatchSeg*>(base);
    T.bfirst = reinterpret_cast<uint64_t*>(base + off_first);
    T.counts = reinterpret_cast<uint32_t*>(base + off_counts);
    T.nseg = reinterpret_cast<uint64_t*>(base + off_nseg);
    T.flag = base + off_flag;
    return true;
}

int deflate_batch_async_locked(dmx_ctx* c, const uint8_t* const* d_in, const uint64_t* d_n, size_t count,
                               size_t max_n, size_t max_total, int level, const uint8_t* d_dict, size_t dict_len,
                               uint8_t* const* d_out, const uint64_t* d_cap, dmx_batch_result* d_res,
                               hipStream_t st) {
    if (level < 0 || level > 3) level = 1;  // as deflate_device_locked
    const uint32_t seg = c->seg;
    const uint32_t du = level >= 2 ? (uint32_t)std::min<size_t>(dict_len, kDeflateDictMax) : 0u;
    if (du && seg != 32768) return DMX_ERR_ARG;
    uint64_t cap = 0;
    if (const int rc = async_deflate_capacity(c, count, max_n, max_total, du, &cap); rc != DMX_OK) return rc;
    if (c->df_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_df, 0));
    DeflateArgs A;
    AsyncSegTab T;
    if (!async_deflate_scratch(c, A, T, count, cap, level)) return DMX_ERR_NOMEM;
    // the sizes past the device-side count stay zero: the scan runs over the capacity
    HIPCHK(hipMemsetAsync(A.sizes, 0, cap * 4, st));
    HIPCHK(launch_batch_segtab(d_in, d_n, count, max_n, cap, seg, du, du ? d_dict + (dict_len - du) : nullptr,
                               T.counts, T.bfirst, T.tab, T.flag, T.nseg, st));
    A.in = nullptr;
    A.n = 0;
    A.final_last = 1;
    A.total = c->offs.as<uint64_t>() + cap;  // the scan's total follows the offsets (scan_words)
    A.out = nullptr;
    A.cap = 0;
    A.dbg = nullptr;
    A.btab = T.tab;
    A.bfirst = T.bfirst;
    A.bout = d_out;
    A.bcap = d_cap;
    A.bres = d_res;
    A.nbuf = count;
    HIPCHK(launch_deflate(A, seg, st, nullptr, nullptr, du != 0, T.nseg, T.flag));
    HIPCHK(hipEventRecord(c->ev_df, st));
    c->df_pending = true;
    c->stats = dmx_stats{};
    c->stats.segments = cap;  // (the table's capacity: the count itself never reaches the host)
    return DMX_OK;
}

struct AsyncDescTab {  // c->ainf: descriptors | order | class histogram + cursors | list length | ticket
    InflateBatchDesc* desc;
    uint32_t* order;
    uint32_t* work;
    uint32_t* norder;
    unsigned int* ticket;
};
bool async_inflate_scratch(dmx_ctx* c, AsyncDescTab& T, size_t count) {
    const size_t off_order = count * sizeof(InflateBatchDesc), off_work = off_order + (count * 4 + 15) / 16 * 16;
    const size_t off_norder = off_work + 2 * kBatchClasses * 4, off_ticket = off_norder + 8;
    if (!c->ainf.ensure(off_ticket + 8)) return false;
    uint8_t* const base = c->ainf.as<uint8_t>();
    T.desc = reinterpret_cast<InflateBatchDesc*>(base);
    T.order = reinterpret_cast<uint32_t*>(base + off_order);
    T.work = reinterpret_cast<uint32_t*>(base + off_work);
    T.norder = reinterpret_cast<uint32_t*>(base + off_norder);
    T.ticket = reinterpret_cast<unsigned int*>(base + off_ticket);
    return true;
}

int inflate_batch_async_locked(dmx_ctx* c, const uint8_t* const* d_in, const uint64_t* d_n, size_t count,
                               size_t max_n, const uint8_t* d_dict, size_t dict_len, uint8_t* const* d_out,
                               const uint64_t* d_cap, dmx_batch_result* d_res, uint32_t flags, hipStream_t st) {
    const uint32_t dl = (uint32_t)std::min<size_t>(dict_len, kInflateDictMax);
    // (the routing rule of inflate_batch_locked; a stream it would route is deferred to the caller)
    const uint64_t route_bytes = !dl && !(flags & DMX_BATCH_NO_ROUTE) ? kBatchRouteBytes : 0;
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    AsyncDescTab T;
    if (!async_inflate_scratch(c, T, count)) return DMX_ERR_NOMEM;
    HIPCHK(launch_batch_desc(d_in, d_n, d_out, d_cap, count, max_n, route_bytes, T.desc, T.order, T.norder, T.work,
                             d_res, st));
    if (dl)
        HIPCHK(launch_inflate_batch_dict(T.desc, T.order, count, d_res, T.ticket, c->flags, d_dict + (dict_len - dl), dl,
                                         st, T.norder));
    else
        HIPCHK(launch_inflate_batch(T.desc, T.order, count, d_res, T.ticket, c->flags, st, T.norder));
    HIPCHK(hipEventRecord(c->ev_inf, st));
    c->inf_pending = true;
    c->stats = dmx_stats{};
    c->stats.segments = count;
    return DMX_OK;
}

// Adler-32 / CRC-32 of a device buffer, computed on the GPU (checksum.hip); the value is
// returned to the host (the call synchronizes the stream).
int checksum_locked(dmx_ctx* c, bool crc, const uint8_t* d, size_t n, uint32_t init, uint32_t* out,
                    hipStream_t st) {
    if (!c->ck.ensure(256 + checksum_scratch_bytes(n))) return DMX_ERR_NOMEM;
    uint32_t* d_res = c->ck.as<uint32_t>();
    void* scratch = c->ck.as<uint8_t>() + 256;
    if (crc) HIPCHK(launch_crc32_raw(d, n, scratch, d_res, st));
    else HIPCHK(launch_adler32(d, n, init, scratch, d_res, st));
    uint32_t v = 0;
    HIPCHK(hipMemcpyAsync(&v, d_res, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *out = crc ? crc32_finish(v, n, init) : v;
    return DMX_OK;
}

// zlib (RFC 1950) / gzip (RFC 1952) framing around libdmx's raw stream; the checksum of the
// input is computed on the GPU from the device copy the deflate reads.
int deflate_framed(dmx_ctx* c, bool gz, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap,
                   size_t* out_len) {
    const size_t head = gz ? 10 : 2, tail = gz ? 8 : 4;
    *out_len = 0;
    const size_t bound = dmx_deflate_bound(n);
    if (!c->in.ensure(n + 16) || !c->out.ensure(bound)) return DMX_ERR_NOMEM;
    if (n) HIPCHK(hipMemcpyAsync(c->in.p, in, n, hipMemcpyHostToDevice, c->stream));
    size_t total = 0;
    int rc = deflate_device_locked(c, c->in.as<uint8_t>(), n, level, 0, c->out.as<uint8_t>(), c->out.cap,
                                   &total, c->stream);
    if (rc != DMX_OK) return rc;
    uint32_t ck = 0;
    rc = checksum_locked(c, gz, c->in.as<uint8_t>(), n, gz ? 0u : 1u, &ck, c->stream);
    if (rc != DMX_OK) return rc;
    *out_len = head + total + tail;
    if (head + total + tail > cap) return DMX_ERR_CAPACITY;
    const int lv = (level < 0 || level > 3) ? 1 : level;
    if (gz) {
        const uint8_t h[10] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, (uint8_t)(lv == 3 ? 2 : lv <= 1 ? 4 : 0), 255};
        std::memcpy(out, h, 10);
    } else {
        const uint32_t flevel = lv <= 1 ? 0 : lv == 2 ? 1 : 3;  // RFC 1950 FLEVEL
        const uint32_t cmf = 0x78, flg0 = flevel << 6;
        const uint32_t flg = flg0 + (31 - (cmf * 256 + flg0) % 31) % 31;
        out[0] = (uint8_t)cmf;
        out[1] = (uint8_t)flg;
    }
    if (total) HIPCHK(hipMemcpyAsync(out + head, c->out.p, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    uint8_t* t = out + head + total;
    if (gz) {
        for (int b = 0; b < 4; b++) t[b] = (uint8_t)(ck >> (8 * b));
        for (int b = 0; b < 4; b++) t[4 + b] = (uint8_t)((uint64_t)n >> (8 * b));
    } else {
        for (int b = 0; b < 4; b++) t[b] = (uint8_t)(ck >> (24 - 8 * b));
    }
    return DMX_OK;
}

// Restores the calling thread's current HIP device on scope exit: an entry point switches to
// its context's device, and a caller driving several GPUs from one thread must not see its
// current device move.
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = prev == dev || hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// ---- n_gpus > 1: the host-buffer API over several devices ---------------------
// Deflate: contiguous segment-aligned shards, one per sub-context, each deflated NOT_FINAL except
// the last non-empty one; one host thread per shard (the pageable H2D / D2H copies of different
// devices then overlap), sizes first, then every shard's bytes straight to its offset in `out`.
// Segments are independent (the reference resets its window per chunk, deflate.hpp:689-697), so
// the bytes equal the one-device stream.
template <class F>
void run_parallel(size_t G, F&& f) {
    std::vector<std::thread> th;
    for (size_t g = 1; g < G; g++) th.emplace_back(f, g);
    f((size_t)0);
    for (auto& t : th) t.join();
}

int deflate_multi(dmx_ctx* c, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap,
                  size_t* out_len) {
    const size_t G = c->subs.size(), seg = c->seg;
    size_t per = (n + G - 1) / G;
    per = (per + seg - 1) / seg * seg;
    std::vector<size_t> b(G), e(G), len(G, 0);
    std::vector<int> rc(G, DMX_OK);
    size_t last = 0, used = 0;
    for (size_t g = 0; g < G; g++) {
        b[g] = std::min(n, g * per);
        e[g] = std::min(n, b[g] + per);
        if (e[g] > b[g]) last = g, used++;
    }
    run_parallel(G, [&](size_t g) {
        if (e[g] == b[g]) return;
        dmx_ctx* s = c->subs[g];
        std::lock_guard<std::mutex> lk(s->mu);
        DeviceGuard dg(s->device);
        const size_t m = e[g] - b[g];
        if (!dg.ok) rc[g] = DMX_ERR_DEVICE;
        else if (!s->in.ensure(m + 16) || !s->out.ensure(dmx_deflate_bound(m))) rc[g] = DMX_ERR_NOMEM;
        else if (hipMemcpyAsync(s->in.p, in + b[g], m, hipMemcpyHostToDevice, s->stream) != hipSuccess) rc[g] = DMX_ERR_DEVICE;
        else rc[g] = deflate_device_locked(s, s->in.as<uint8_t>(), m, level, g == last ? 0u : DMX_DEFLATE_NOT_FINAL,
                                           s->out.as<uint8_t>(), s->out.cap, &len[g], s->stream);
    });
    size_t total = 0;
    for (size_t g = 0; g < G; g++) {
        if (rc[g] != DMX_OK) return rc[g];
        total += len[g];
    }
    *out_len = total;
    if (total > cap) return DMX_ERR_CAPACITY;
    std::vector<size_t> off(G, 0);
    for (size_t g = 1; g < G; g++) off[g] = off[g - 1] + len[g - 1];
    run_parallel(G, [&](size_t g) {
        if (!len[g]) return;
        dmx_ctx* s = c->subs[g];
        DeviceGuard dg(s->device);
        if (hipMemcpyAsync(out + off[g], s->out.p, len[g], hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
            hipStreamSynchronize(s->stream) != hipSuccess)
            rc[g] = DMX_ERR_DEVICE;
    });
    for (size_t g = 0; g < G; g++)
        if (rc[g] != DMX_OK) return rc[g];
    c->stats = dmx_stats{};
    c->stats.in_bytes = n;
    c->stats.out_bytes = total;
    c->stats.shards = (uint32_t)used;
    return DMX_OK;
}

// Inflate: sub-context 0 indexes the candidate segment starts (the bytes after every 00 00 FF FF)
// and proves cuts near equal shares of them with a piece-mode decode of the segment there (it must
// end on another candidate: a marker inside stored data is no cut); every sub-context decodes its
// piece (closed with an empty final block; pieces after the first in piece mode, where a
// reference before the piece is an error), then the outputs land at their offsets: in `out`
// (at most cap bytes, *written) or in a malloc'd buffer (*alloc).  Returns 1 when the stream does
// not split (fewer than G proven cuts' worth of candidates, or a piece fails): the caller then
// decodes it on one device, so the result never depends on the split.
int inflate_multi(dmx_ctx* c, const uint8_t* in, size_t n, uint8_t* out, size_t cap, uint8_t** alloc,
                  size_t* written, size_t* total_out) {
    const size_t G = c->subs.size();
    dmx_ctx* s0 = c->subs[0];
    std::vector<uint64_t> starts;
    {
        DeviceGuard dg(s0->device);
        if (!dg.ok) return 1;
        {
            std::lock_guard<std::mutex> lk(s0->mu);
            if (!s0->in.ensure(n + 16) || hipMemcpyAsync(s0->in.p, in, n, hipMemcpyHostToDevice, s0->stream) != hipSuccess)
                return 1;
        }
        size_t cnt = 0;
        if (dmx_segment_starts_device(s0, s0->in.p, n, nullptr, 0, &cnt, nullptr) != DMX_OK || cnt + 1 < 2 * G) return 1;
        starts.resize(cnt);
        if (dmx_segment_starts_device(s0, s0->in.p, n, starts.data(), cnt, &cnt, nullptr) != DMX_OK) return 1;
        // cut candidates: up to 8 around each target, proven in one batched check
        std::vector<uint64_t> near;
        for (size_t r = 1; r < G; r++) {
            const size_t t = r * starts.size() / G;
            for (size_t j = (t >= 4 ? t - 4 : 0); j < std::min(starts.size(), t + 4); j++)
                if (starts[j] < n) near.push_back(starts[j]);
        }
        std::sort(near.begin(), near.end());
        near.erase(std::unique(near.begin(), near.end()), near.end());
        std::vector<uint64_t> ends(near.size());
        if (dmx_segment_check_device(s0, s0->in.p, n, near.data(), near.size(), ends.data(), nullptr) != DMX_OK) return 1;
        std::vector<uint64_t> ok;
        for (size_t i = 0; i < near.size(); i++)
            if (ends[i] != UINT64_MAX && ends[i] > near[i] &&
                (ends[i] == n || std::binary_search(starts.begin(), starts.end(), ends[i])))
                ok.push_back(near[i]);
        std::vector<uint64_t> cut{0};
        for (size_t r = 1; r < G; r++) {
            const uint64_t target = starts[r * starts.size() / G];
            uint64_t best = 0, bd = UINT64_MAX;
            for (uint64_t x : ok)
                if (x > cut.back() && (x > target ? x - target : target - x) < bd) best = x, bd = x > target ? x - target : target - x;
            if (!best) return 1;
            cut.push_back(best);
        }
        cut.push_back(n);
        starts = cut;
    }
    std::vector<size_t> len(G, 0);
    std::vector<int> rc(G, DMX_OK);
    std::vector<uint8_t*> dev(G, nullptr);
    run_parallel(G, [&](size_t g) {
        dmx_ctx* s = c->subs[g];
        std::lock_guard<std::mutex> lk(s->mu);
        DeviceGuard dg(s->device);
        const size_t a = starts[g], m = starts[g + 1] - a;
        static const uint8_t close[2] = {0x03, 0x00};  // an empty final block ends the piece
        const bool closes = g + 1 < G;
        if (!dg.ok || !s->in.ensure(m + 16) ||
            hipMemcpyAsync(s->in.p, in + a, m, hipMemcpyHostToDevice, s->stream) != hipSuccess ||
            (closes && hipMemcpyAsync(s->in.as<uint8_t>() + m, close, 2, hipMemcpyHostToDevice, s->stream) != hipSuccess)) {
            rc[g] = DMX_ERR_DEVICE;
            return;
        }
        s->last_end = 0;
        rc[g] = inflate_device_locked(s, s->in.as<uint8_t>(), m + (closes ? 2 : 0), nullptr, 0, &len[g], &dev[g],
                                      s->stream, g ? DMX_IFLAG_PIECE : 0u);
        // a piece must end at its appended empty final block: a BFINAL block before it (two
        // streams concatenated: the reference stops at the first) would drop the piece's rest
        if (rc[g] == DMX_OK && closes && s->last_end != m + 2) rc[g] = DMX_ERR_DATA;
    });
    for (size_t g = 0; g < G; g++)
        if (rc[g] != DMX_OK) return 1;
    size_t total = 0;
    std::vector<size_t> off(G, 0);
    for (size_t g = 0; g < G; g++) {
        off[g] = total;
        total += len[g];
    }
    uint8_t* dst = out;
    size_t lim = cap;
    if (alloc) {
        dst = static_cast<uint8_t*>(std::malloc(total ? total : 1));
        if (!dst) return DMX_ERR_NOMEM;
        lim = total;
    }
    run_parallel(G, [&](size_t g) {
        const size_t w = off[g] >= lim ? 0 : std::min(len[g], lim - off[g]);
        if (!w) return;
        dmx_ctx* s = c->subs[g];
        DeviceGuard dg(s->device);
        if (hipMemcpyAsync(dst + off[g], dev[g], w, hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
            hipStreamSynchronize(s->stream) != hipSuccess)
            rc[g] = DMX_ERR_DEVICE;
    });
    for (size_t g = 0; g < G; g++)
        if (rc[g] != DMX_OK) {
            if (alloc) std::free(dst);
            return DMX_ERR_DEVICE;
        }
    if (alloc) *alloc = dst;
    if (written) *written = std::min(total, lim);
    *total_out = total;
    c->stats = dmx_stats{};
    c->stats.in_bytes = n;
    c->stats.out_bytes = total;
    c->stats.path = 4;
    c->stats.shards = (uint32_t)G;
    return DMX_OK;
}

bool is_gfx950(int dev) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) return false;
    return std::strncmp(p.gcnArchName, "gfx950", 6) == 0;
}

}  // namespace

extern "C" {

void dmx_config_default(dmx_config* cfg) {
    cfg->device = -1;
    cfg->segment_bytes = 32768;
    cfg->flags = 0;
    cfg->n_gpus = 1;
    cfg->dev_inflate_pass = 0;
    cfg->dev_heavy_bytes = 0;
}

int dmx_create(dmx_ctx** out, const dmx_config* cfg) {
    if (!out) return DMX_ERR_ARG;
    *out = nullptr;
    dmx_config d;
    dmx_config_default(&d);
    if (!cfg) cfg = &d;
    if (cfg->segment_bytes != 16384 && cfg->segment_bytes != 32768 && cfg->segment_bytes != 65536) return DMX_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return DMX_ERR_DEVICE;
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return DMX_ERR_DEVICE;
    if (dev >= ndev || !is_gfx950(dev)) return DMX_ERR_DEVICE;
    // n_gpus: at most 8 shards per visible device (a stale or garbage value -- a caller built
    // against an older dmx_config -- would otherwise create contexts without bound)
    if (cfg->n_gpus > 8u * (uint32_t)ndev) return DMX_ERR_ARG;
    DeviceGuard dg(dev);
    if (!dg.ok) return DMX_ERR_DEVICE;
    dmx_ctx* c = new (std::nothrow) dmx_ctx();
    if (!c) return DMX_ERR_NOMEM;
    c->device = dev;
    c->seg = cfg->segment_bytes;
    c->flags = cfg->flags;
    c->inflate_pass = (int)cfg->dev_inflate_pass - 1;
    c->heavy_bytes = cfg->dev_heavy_bytes;
    c->diag = diag_env().bits;
    c->pipe = pipe_knob(std::getenv("DMX_DEFLATE_PIPE"));
    c->spec = spec_knob(std::getenv("DMX_INFLATE_SPEC"));
    if (hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c->ncu <= 0)
        c->ncu = 256;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return DMX_ERR_DEVICE;
    }
    for (auto& e : c->ev) (void)hipEventCreate(&e);
    // the host result block (dmx_ctx.h); without it the calls copy their results as before
    {
        void *h = nullptr, *d = nullptr;
        if (hipHostMalloc(&h, sizeof(HostRes), hipHostMallocMapped) == hipSuccess) {
            if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess && d) {
                std::memset(h, 0, sizeof(HostRes));
                c->hres = static_cast<HostRes*>(h);
                c->hres_dev = static_cast<HostRes*>(d);
            } else {
                (void)hipHostFree(h);
            }
        }
        (void)hipGetLastError();
    }
    if (hipEventCreateWithFlags(&c->ev_df, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_inf, hipEventDisableTiming) != hipSuccess) {
        dmx_destroy(c);
        return DMX_ERR_DEVICE;
    }
    if (cfg->n_gpus > 1) {  // one context per shard, round-robin over the visible devices
        dmx_config sc = *cfg;
        sc.n_gpus = 1;
        for (uint32_t i = 0; i < cfg->n_gpus; i++) {
            sc.device = (dev + (int)i) % ndev;
            dmx_ctx* s = nullptr;
            const int rc = is_gfx950(sc.device) ? dmx_create(&s, &sc) : DMX_ERR_DEVICE;
            if (rc != DMX_OK) {
                dmx_destroy(c);
                return rc;
            }
            c->subs.push_back(s);
        }
    }
    *out = c;
    return DMX_OK;
}

void dmx_destroy(dmx_ctx* c) {
    if (!c) return;
    for (dmx_ctx* s : c->subs) dmx_destroy(s);
    c->subs.clear();
    DeviceGuard dg(c->device);
    (void)hipStreamSynchronize(c->stream);
    // work enqueued on the callers' streams (the asynchronous calls) still uses the scratch
    if (c->df_pending && c->ev_df) (void)hipEventSynchronize(c->ev_df);
    if (c->inf_pending && c->ev_inf) (void)hipEventSynchronize(c->ev_inf);
    for (DevBuf* b : {&c->in, &c->out, &c->slots, &c->sizes, &c->offs, &c->scal, &c->cands,
                      &c->tiles, &c->tileoffs, &c->recs, &c->status, &c->dbg, &c->ltok,
                      &c->ltokoff, &c->lntok, &c->lcaps, &c->lheavy, &c->rtmp, &c->rchain, &c->fbc, &c->fbh, &c->fbo, &c->fbl,
                      &c->fbs, &c->fbt, &c->fbk, &c->fbu, &c->fbch, &c->fbco, &c->fbcs, &c->fbimg, &c->fbstop, &c->fbwin, &c->fbopen, &c->fbvm, &c->fbvh,
                      &c->fbreg, &c->fbJ, &c->fbvis, &c->fbph,
                      &c->ck, &c->btab, &c->bres, &c->adf, &c->ainf, &c->fdesc, &c->bgzs, &c->bgzc, &c->bgzd, &c->bgzt,
                      &c->seekd})
        b->release();
    for (auto& e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->ev_df) (void)hipEventDestroy(c->ev_df);
    if (c->ev_inf) (void)hipEventDestroy(c->ev_inf);
    if (c->side) {  // (its work ended before ev_df)
        (void)hipStreamSynchronize(c->side);
        (void)hipStreamDestroy(c->side);
        (void)hipEventDestroy(c->ev_chunk);
        (void)hipEventDestroy(c->ev_side);
    }
    if (c->fbkeep_h) (void)hipHostFree(c->fbkeep_h);
    if (c->hres) (void)hipHostFree(c->hres);
    if (c->pin) (void)hipHostFree(c->pin);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

static std::mutex g_default_mu;
static dmx_config g_default_cfg;
static bool g_default_set = false, g_default_made = false;

int dmx_set_default_config(const dmx_config* cfg) {
    if (!cfg) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(g_default_mu);
    if (g_default_made) return DMX_ERR_ARG;
    g_default_cfg = *cfg;
    g_default_set = true;
    return DMX_OK;
}

dmx_ctx* dmx_default_ctx(void) {
    static std::once_flag once;
    static dmx_ctx* ctx = nullptr;
    std::call_once(once, [] {
        std::lock_guard<std::mutex> g(g_default_mu);
        g_default_made = true;
        if (dmx_create(&ctx, g_default_set ? &g_default_cfg : nullptr) != DMX_OK) ctx = nullptr;
    });
    return ctx;
}

size_t dmx_deflate_bound(size_t n) { return n + 10 * ((n + 16383) / 16384) + 16; }

int dmx_deflate_device(dmx_ctx* c, const void* d_in, size_t n, int level, uint32_t flags,
                       void* d_out, size_t cap, size_t* out_len, void* stream) {
    if (!c || (!d_in && n) || !d_out || !out_len) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return deflate_device_locked(c, (const uint8_t*)d_in, n, level, flags, (uint8_t*)d_out, cap,
                                 out_len, st);
}

int dmx_deflate_device_async(dmx_ctx* c, const void* d_in, size_t n, int level, uint32_t flags,
                             void* d_out, size_t cap, uint64_t* d_out_len, void* stream) {
    if (!c || (!d_in && n) || !d_out || !d_out_len) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return deflate_device_locked(c, (const uint8_t*)d_in, n, level, flags, (uint8_t*)d_out, cap,
                                 nullptr, st, d_out_len);
}

int dmx_inflate_device(dmx_ctx* c, const void* d_in, size_t n, void* d_out, size_t cap,
                       size_t* out_len, void* stream) {
    if (!c || (!d_in && n) || !d_out || !out_len) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return inflate_device_locked(c, (const uint8_t*)d_in, n, (uint8_t*)d_out, cap, out_len,
                                 nullptr, st);
}

int dmx_inflate_device_async(dmx_ctx* c, const void* d_in, size_t n, void* d_out, size_t cap,
                             uint64_t* d_result, uint32_t flags, void* stream) {
    if (!c || (!d_in && n) || !d_out || !d_result || (flags & ~DMX_INFLATE_PIECE)) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return inflate_device_async_locked(c, (const uint8_t*)d_in, n, (uint8_t*)d_out, cap, d_result, st,
                                       (flags & DMX_INFLATE_PIECE) ? DMX_IFLAG_PIECE : 0u);
}

int dmx_inflate_piece_device(dmx_ctx* c, const void* d_in, size_t n, void* d_out, size_t cap,
                             size_t* out_len, void* stream) {
    if (!c || (!d_in && n) || !d_out || !out_len) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return inflate_device_locked(c, (const uint8_t*)d_in, n, (uint8_t*)d_out, cap, out_len, nullptr, st,
                                 DMX_IFLAG_PIECE);
}

// ---- batched API ---------------------------------------------------------------------------
// (a context with n_gpus > 1 runs the batch on its own, i.e. its first, device)
static bool batch_args_ok(const dmx_ctx* c, const void* in, const size_t* n, size_t count, const void* out,
                          const size_t* cap, const dmx_batch_result* res) {
    return c && count < (size_t)DF_BATCH_LAST && (count == 0 || (in && n && out && cap && res));
}

// (the plain calls are the dictionary calls with dict_len == 0)
int dmx_deflate_batch_dict_device(dmx_ctx* c, const void* const* d_in, const size_t* n, size_t count, int level,
                                  const void* d_dict, size_t dict_len, void* const* d_out, const size_t* cap,
                                  dmx_batch_result* res, void* stream) {
    if (!batch_args_ok(c, d_in, n, count, d_out, cap, res) || (dict_len && !d_dict)) return DMX_ERR_ARG;
    if (c->seg != 16384 && c->seg != 32768) return DMX_ERR_ARG;  // 64 KiB blocks pair front segments
    if (dict_len && c->seg != 32768) return DMX_ERR_ARG;  // the 16 KiB image has no room for one
    if (count == 0) return DMX_OK;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return deflate_batch_locked(c, reinterpret_cast<const uint8_t* const*>(d_in), n, count, level,
                                reinterpret_cast<uint8_t* const*>(d_out), cap, res, st,
                                static_cast<const uint8_t*>(d_dict), dict_len);
}

int dmx_deflate_batch_device(dmx_ctx* c, const void* const* d_in, const size_t* n, size_t count, int level,
                             void* const* d_out, const size_t* cap, dmx_batch_result* res, void* stream) {
    return dmx_deflate_batch_dict_device(c, d_in, n, count, level, nullptr, 0, d_out, cap, res, stream);
}

int dmx_inflate_batch_dict_device(dmx_ctx* c, const void* const* d_in, const size_t* n, size_t count,
                                  const void* d_dict, size_t dict_len, void* const* d_out, const size_t* cap,
                                  dmx_batch_result* res, uint32_t flags, void* stream) {
    if (!batch_args_ok(c, d_in, n, count, d_out, cap, res) || (flags & ~DMX_BATCH_NO_ROUTE) || (dict_len && !d_dict))
        return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return inflate_batch_locked(c, reinterpret_cast<const uint8_t* const*>(d_in), n, count,
                                reinterpret_cast<uint8_t* const*>(d_out), cap, res, flags, st,
                                static_cast<const uint8_t*>(d_dict), dict_len);
}

int dmx_inflate_batch_device(dmx_ctx* c, const void* const* d_in, const size_t* n, size_t count,
                             void* const* d_out, const size_t* cap, dmx_batch_result* res, uint32_t flags,
                             void* stream) {
    return dmx_inflate_batch_dict_device(c, d_in, n, count, nullptr, 0, d_out, cap, res, flags, stream);
}

// ---- batches from device-resident descriptor arrays -------------------------------------------
static bool batch_async_args_ok(const dmx_ctx* c, const void* in, const void* n, size_t count, const void* out,
                                const void* cap, const void* res) {
    return c && count < (size_t)DF_BATCH_LAST && (count == 0 || (in && n && out && cap && res));
}

int dmx_batch_reserve(dmx_ctx* c, size_t count, size_t max_n, size_t max_total, size_t dict_len) {
    if (!c || count >= (size_t)DF_BATCH_LAST) return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    AsyncDescTab D;
    if (!async_inflate_scratch(c, D, count)) return DMX_ERR_NOMEM;
    if (c->seg != 16384 && c->seg != 32768) return DMX_OK;  // no deflate side on 64 KiB contexts
    // the deflate side at its largest: level 3's token words; a dictionary only where one is taken
    const uint32_t du = c->seg == 32768 ? (uint32_t)std::min<size_t>(dict_len, kDeflateDictMax) : 0u;
    uint64_t cap = 0;
    if (const int rc = async_deflate_capacity(c, count, max_n, max_total, du, &cap); rc != DMX_OK) return rc;
    if (du) {  // (levels 0-1 ignore the dictionary: their capacity may be the larger one)
        uint64_t cap0 = 0;
        if (const int rc = async_deflate_capacity(c, count, max_n, max_total, 0, &cap0); rc != DMX_OK) return rc;
        cap = std::max(cap, cap0);
    }
    DeflateArgs A;
    AsyncSegTab T;
    return async_deflate_scratch(c, A, T, count, cap, 3) ? DMX_OK : DMX_ERR_NOMEM;
}

int dmx_deflate_batch_async(dmx_ctx* c, const void* const* d_in, const uint64_t* d_n, size_t count, size_t max_n,
                            size_t max_total, int level, const void* d_dict, size_t dict_len, void* const* d_out,
                            const uint64_t* d_cap, dmx_batch_result* d_res, void* stream) {
    if (!batch_async_args_ok(c, d_in, d_n, count, d_out, d_cap, d_res) || (dict_len && !d_dict)) return DMX_ERR_ARG;
    if (c->seg != 16384 && c->seg != 32768) return DMX_ERR_ARG;  // as dmx_deflate_batch_device
    if (dict_len && c->seg != 32768 && level >= 2 && level <= 3) return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return deflate_batch_async_locked(c, reinterpret_cast<const uint8_t* const*>(d_in), d_n, count, max_n, max_total,
                                      level, static_cast<const uint8_t*>(d_dict), dict_len,
                                      reinterpret_cast<uint8_t* const*>(d_out), d_cap, d_res, st);
}

int dmx_inflate_batch_async(dmx_ctx* c, const void* const* d_in, const uint64_t* d_n, size_t count, size_t max_n,
                            const void* d_dict, size_t dict_len, void* const* d_out, const uint64_t* d_cap,
                            dmx_batch_result* d_res, uint32_t flags, void* stream) {
    if (!batch_async_args_ok(c, d_in, d_n, count, d_out, d_cap, d_res) || (flags & ~DMX_BATCH_NO_ROUTE) ||
        (dict_len && !d_dict))
        return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return inflate_batch_async_locked(c, reinterpret_cast<const uint8_t* const*>(d_in), d_n, count, max_n,
                                      static_cast<const uint8_t*>(d_dict), dict_len,
                                      reinterpret_cast<uint8_t* const*>(d_out), d_cap, d_res, flags, st);
}

// Host buffers: the inputs are packed into one staging image at 16-byte aligned offsets and go up
// in one copy; the outputs come back in one copy of the packed output area and are handed out.
// ocap(i): the device bytes reserved for output i.  A preset dictionary (dict_len > 0) follows the
// inputs in the staging image and goes up in the same copy; run() gets its device address.
extern "C++" {
template <class OutCap, class Run>
static int batch_host(dmx_ctx* c, const uint8_t* const* in, const size_t* n, size_t count, uint8_t* const* out,
                      const size_t* cap, dmx_batch_result* res, const uint8_t* dict, size_t dict_len, OutCap ocap,
                      Run run) {
    for (size_t i = 0; i < count; i++)
        if ((!in[i] && n[i]) || (!out[i] && cap[i])) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    std::vector<size_t> ioff(count + 1), ooff(count + 1), dcap(count);
    std::vector<const uint8_t*> din(count);
    std::vector<uint8_t*> dout(count);
    std::vector<uint8_t> stage;
    size_t ti = 0, to = 0;
    for (size_t i = 0; i < count; i++) {
        ioff[i] = ti;
        ooff[i] = to;
        dcap[i] = ocap(i);
        ti += (n[i] + 15) & ~size_t(15);
        to += (dcap[i] + 15) & ~size_t(15);
    }
    const size_t doff = ti;
    ti += (dict_len + 15) & ~size_t(15);
    try {
        stage.resize(std::max(ti, to));
    } catch (const std::bad_alloc&) {
        return DMX_ERR_NOMEM;
    }
    if (!c->in.ensure(ti + 16) || !c->out.ensure(to + 16)) return DMX_ERR_NOMEM;
    for (size_t i = 0; i < count; i++) {
        if (n[i]) std::memcpy(stage.data() + ioff[i], in[i], n[i]);
        din[i] = c->in.as<uint8_t>() + ioff[i];
        dout[i] = c->out.as<uint8_t>() + ooff[i];
    }
    if (dict_len) std::memcpy(stage.data() + doff, dict, dict_len);
    if (ti) HIPCHK(hipMemcpyAsync(c->in.p, stage.data(), ti, hipMemcpyHostToDevice, c->stream));
    const int rc = run(din.data(), dout.data(), dcap.data(), dict_len ? c->in.as<uint8_t>() + doff : nullptr);
    if (rc != DMX_OK) return rc;
    if (to) HIPCHK(hipMemcpyAsync(stage.data(), c->out.p, to, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < count; i++) {
        // a result that fits the device area but not the caller's buffer
        if (res[i].status == DMX_OK && res[i].bytes > cap[i]) res[i].status = DMX_ERR_CAPACITY;
        const size_t w = std::min<size_t>({(size_t)res[i].bytes, cap[i], dcap[i]});
        // (DMX_ERR_CHECKSUM, framed calls only: the decoded bytes are handed out all the same)
        if (w && (res[i].status == DMX_OK || res[i].status == DMX_ERR_CAPACITY || res[i].status == DMX_ERR_CHECKSUM))
            std::memcpy(out[i], stage.data() + ooff[i], w);
    }
    return DMX_OK;
}
}  // extern "C++"

int dmx_deflate_batch_dict(dmx_ctx* c, const uint8_t* const* in, const size_t* n, size_t count, int level,
                           const uint8_t* dict, size_t dict_len, uint8_t* const* out, const size_t* cap,
                           dmx_batch_result* res) {
    if (!batch_args_ok(c, in, n, count, out, cap, res) || (dict_len && !dict)) return DMX_ERR_ARG;
    if (c->seg != 16384 && c->seg != 32768) return DMX_ERR_ARG;
    if (dict_len && c->seg != 32768) return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    return batch_host(c, in, n, count, out, cap, res, dict, dict_len,
                      [&](size_t i) { return std::min(cap[i], dmx_deflate_bound(n[i])); },
                      [&](const uint8_t* const* di, uint8_t* const* dou, const size_t* dc, const uint8_t* dd) {
                          return deflate_batch_locked(c, di, n, count, level, dou, dc, res, c->stream, dd, dict_len);
                      });
}

int dmx_deflate_batch(dmx_ctx* c, const uint8_t* const* in, const size_t* n, size_t count, int level,
                      uint8_t* const* out, const size_t* cap, dmx_batch_result* res) {
    return dmx_deflate_batch_dict(c, in, n, count, level, nullptr, 0, out, cap, res);
}

int dmx_inflate_batch_dict(dmx_ctx* c, const uint8_t* const* in, const size_t* n, size_t count, const uint8_t* dict,
                           size_t dict_len, uint8_t* const* out, const size_t* cap, dmx_batch_result* res,
                           uint32_t flags) {
    if (!batch_args_ok(c, in, n, count, out, cap, res) || (flags & ~DMX_BATCH_NO_ROUTE) || (dict_len && !dict))
        return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    return batch_host(c, in, n, count, out, cap, res, dict, dict_len, [&](size_t i) { return cap[i]; },
                      [&](const uint8_t* const* di, uint8_t* const* dou, const size_t* dc, const uint8_t* dd) {
                          return inflate_batch_locked(c, di, n, count, dou, dc, res, flags, c->stream, dd, dict_len);
                      });
}

int dmx_inflate_batch(dmx_ctx* c, const uint8_t* const* in, const size_t* n, size_t count, uint8_t* const* out,
                      const size_t* cap, dmx_batch_result* res, uint32_t flags) {
    return dmx_inflate_batch_dict(c, in, n, count, nullptr, 0, out, cap, res, flags);
}

// ---- framed batch calls: zlib / gzip / BGZF around the batch (frame_batch.hip) ---------------
size_t dmx_batch_framed_bound(uint32_t format, size_t n) {
    const uint32_t head = frame_head_bytes(format);
    return head ? dmx_deflate_bound(n) + head + frame_tail_bytes(format) : 0;
}

extern "C++" {
// The batch deflate writes each raw stream behind its header's place, into the capacity less
// header and trailer (clamped at 0); a BGZF buffer above the block size is given nothing to do
// and k_frame_write reports it.
static int deflate_batch_framed_locked(dmx_ctx* c, const uint8_t* const* d_in, const size_t* n, size_t count,
                                       int level, uint32_t format, uint8_t* const* d_out, const size_t* cap,
                                       dmx_batch_result* res, hipStream_t st) {
    const size_t frame = frame_head_bytes(format) + frame_tail_bytes(format);
    std::vector<InflateBatchDesc> desc;
    std::vector<size_t> rn, rcap;
    std::vector<uint8_t*> rout;
    try {
        desc.resize(count);
        rn.resize(count);
        rcap.resize(count);
        rout.resize(count);
    } catch (const std::bad_alloc&) {
        return DMX_ERR_NOMEM;
    }
    for (size_t i = 0; i < count; i++) {
        if ((!d_in[i] && n[i]) || (!d_out[i] && cap[i])) return DMX_ERR_ARG;
        const bool big = format == DMX_FRAME_BGZF && n[i] > kBgzfBlock;
        desc[i] = InflateBatchDesc{d_in[i], n[i], d_out[i], cap[i]};
        rn[i] = big ? 0 : n[i];
        rcap[i] = (big || cap[i] < frame) ? 0 : cap[i] - frame;
        rout[i] = rcap[i] ? d_out[i] + frame_head_bytes(format) : nullptr;
    }
    const FramePlan fp{format, level, false, desc.data()};
    return deflate_batch_locked(c, d_in, rn.data(), count, level, rout.data(), rcap.data(), res, st, nullptr, 0, &fp);
}
}  // extern "C++"

static bool frame_format_ok(uint32_t format) { return frame_head_bytes(format) != 0; }

int dmx_deflate_batch_framed_device(dmx_ctx* c, const void* const* d_in, const size_t* n, size_t count, int level,
                                    uint32_t format, void* const* d_out, const size_t* cap, dmx_batch_result* res,
                                    void* stream) {
    if (!batch_args_ok(c, d_in, n, count, d_out, cap, res) || !frame_format_ok(format)) return DMX_ERR_ARG;
    if (c->seg != 16384 && c->seg != 32768) return DMX_ERR_ARG;  // as dmx_deflate_batch_device
    if (count == 0) return DMX_OK;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return deflate_batch_framed_locked(c, reinterpret_cast<const uint8_t* const*>(d_in), n, count, level, format,
                                       reinterpret_cast<uint8_t* const*>(d_out), cap, res, st);
}

int dmx_inflate_batch_framed_device(dmx_ctx* c, const void* const* d_in, const size_t* n, size_t count,
                                    uint32_t format, void* const* d_out, const size_t* cap, dmx_batch_result* res,
                                    uint32_t flags, void* stream) {
    if (!batch_args_ok(c, d_in, n, count, d_out, cap, res) || !frame_format_ok(format) ||
        (flags & ~(DMX_BATCH_NO_ROUTE | DMX_BATCH_VERIFY)))
        return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const FramePlan fp{format, 0, (flags & DMX_BATCH_VERIFY) != 0, nullptr};
    return inflate_batch_locked(c, reinterpret_cast<const uint8_t* const*>(d_in), n, count,
                                reinterpret_cast<uint8_t* const*>(d_out), cap, res, flags & DMX_BATCH_NO_ROUTE, st,
                                nullptr, 0, &fp);
}

int dmx_deflate_batch_framed(dmx_ctx* c, const uint8_t* const* in, const size_t* n, size_t count, int level,
                             uint32_t format, uint8_t* const* out, const size_t* cap, dmx_batch_result* res) {
    if (!batch_args_ok(c, in, n, count, out, cap, res) || !frame_format_ok(format)) return DMX_ERR_ARG;
    if (c->seg != 16384 && c->seg != 32768) return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    return batch_host(c, in, n, count, out, cap, res, nullptr, 0,
                      [&](size_t i) { return std::min(cap[i], dmx_batch_framed_bound(format, n[i])); },
                      [&](const uint8_t* const* di, uint8_t* const* dou, const size_t* dc, const uint8_t*) {
                          return deflate_batch_framed_locked(c, di, n, count, level, format, dou, dc, res, c->stream);
                      });
}

int dmx_inflate_batch_framed(dmx_ctx* c, const uint8_t* const* in, const size_t* n, size_t count, uint32_t format,
                             uint8_t* const* out, const size_t* cap, dmx_batch_result* res, uint32_t flags) {
    if (!batch_args_ok(c, in, n, count, out, cap, res) || !frame_format_ok(format) ||
        (flags & ~(DMX_BATCH_NO_ROUTE | DMX_BATCH_VERIFY)))
        return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    const FramePlan fp{format, 0, (flags & DMX_BATCH_VERIFY) != 0, nullptr};
    return batch_host(c, in, n, count, out, cap, res, nullptr, 0, [&](size_t i) { return cap[i]; },
                      [&](const uint8_t* const* di, uint8_t* const* dou, const size_t* dc, const uint8_t*) {
                          return inflate_batch_locked(c, di, n, count, dou, dc, res, flags & DMX_BATCH_NO_ROUTE,
                                                      c->stream, nullptr, 0, &fp);
                      });
}

// ---- BGZF files on host buffers: one framed batch call each -----------------------------------
static const uint8_t kBgzfEof[kBgzfEofBytes] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                                                0x02, 0,    0x1b, 0,    0x03, 0, 0, 0, 0, 0,    0,    0, 0,    0};

size_t dmx_bgzf_bound(size_t n) {
    const size_t full = n / kBgzfBlock, rem = n % kBgzfBlock;
    return full * dmx_batch_framed_bound(DMX_FRAME_BGZF, kBgzfBlock) +
           (rem ? dmx_batch_framed_bound(DMX_FRAME_BGZF, rem) : 0) + kBgzfEofBytes;
}

int dmx_deflate_bgzf(dmx_ctx* c, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap, size_t* out_len) {
    if (!c) c = dmx_default_ctx();
    if (!c) return DMX_ERR_DEVICE;
    if ((!in && n) || !out_len || !out) return DMX_ERR_ARG;
    *out_len = 0;
    const size_t nblk = (n + kBgzfBlock - 1) / kBgzfBlock;
    const size_t slot = dmx_batch_framed_bound(DMX_FRAME_BGZF, kBgzfBlock);
    std::vector<const uint8_t*> ins;
    std::vector<uint8_t*> outs;
    std::vector<size_t> ns, caps;
    std::vector<dmx_batch_result> res;
    std::vector<uint8_t> members;  // one slot per member; concatenated into `out` below
    try {
        ins.resize(nblk);
        outs.resize(nblk);
        ns.resize(nblk);
        caps.resize(nblk);
        res.resize(nblk);
        members.resize(nblk * slot);
    } catch (const std::bad_alloc&) {
        return DMX_ERR_NOMEM;
    }
    for (size_t i = 0; i < nblk; i++) {
        ins[i] = in + i * kBgzfBlock;
        ns[i] = std::min<size_t>(kBgzfBlock, n - i * kBgzfBlock);
        outs[i] = members.data() + i * slot;
        caps[i] = slot;
    }
    const int rc = dmx_deflate_batch_framed(c, ins.data(), ns.data(), nblk, level, DMX_FRAME_BGZF, outs.data(),
                                            caps.data(), res.data());
    if (rc != DMX_OK) return rc;
    size_t total = kBgzfEofBytes;
    for (size_t i = 0; i < nblk; i++) {
        if (res[i].status != DMX_OK) return res[i].status;
        total += res[i].bytes;
    }
    *out_len = total;
    if (total > cap) return DMX_ERR_CAPACITY;
    uint8_t* o = out;
    for (size_t i = 0; i < nblk; i++) {
        std::memcpy(o, outs[i], res[i].bytes);
        o += res[i].bytes;
    }
    std::memcpy(o, kBgzfEof, kBgzfEofBytes);
    return DMX_OK;
}

int dmx_inflate_bgzf(dmx_ctx* c, const uint8_t* in, size_t n, uint32_t flags, uint8_t** out, size_t* len) {
    if (!c) c = dmx_default_ctx();
    if (!c) return DMX_ERR_DEVICE;
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

// ---- BGZF files in device memory (bgzf_chain.hip) ---------------------------------------------
extern "C++" {
static size_t up16(size_t b) { return (b + 15) & ~size_t(15); }

// The member chain of d_in[0, n), found on the device; two host synchronisations (the candidate
// count sizes the scratch; then the member count, the plain bytes and the chain status).
struct BgzfChain {
    uint64_t members = 0, total = 0;
    int status = DMX_OK;
    BgzfCand* rows = nullptr;     // device: members entries, chain order
    uint64_t* uoff = nullptr;     // device: their output offsets
    BgzfChainHead* head = nullptr;
};
static int bgzf_chain_locked(dmx_ctx* c, const uint8_t* d_in, size_t n, hipStream_t st, BgzfChain* ch) {
    if (!n) return DMX_OK;  // no member, DMX_OK
    const uint64_t nt = bgzf_tiles(d_in, n);
    const size_t off_offs = up16(nt * 4), off_head = off_offs + up16(scan_words(nt) * 8);
    if (!c->bgzt.ensure(off_head + 64)) return DMX_ERR_NOMEM;
    uint8_t* const tb = c->bgzt.as<uint8_t>();
    uint64_t* const tile_offs = reinterpret_cast<uint64_t*>(tb + off_offs);
    ch->head = reinterpret_cast<BgzfChainHead*>(tb + off_head);
    uint64_t* const d_ncand = reinterpret_cast<uint64_t*>(tb + off_head + 32);
    HIPCHK(launch_bgzf_count(d_in, n, reinterpret_cast<uint32_t*>(tb), tile_offs, d_ncand, st));
    uint64_t ncand = 0;
    HIPCHK(hipMemcpyAsync(&ncand, d_ncand, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ncand >= kBgzfNone) return DMX_ERR_NOMEM;  // (links are 32-bit candidate indices)
    const uint32_t levels = bgzf_levels(ncand);
    const size_t off_rows = up16(ncand * sizeof(BgzfCand)), off_J = off_rows * 2;
    const size_t off_isz = off_J + up16((size_t)levels * ncand * 4), off_uoff = off_isz + up16(ncand * 4);
    if (!c->bgzc.ensure(off_uoff + scan_words(ncand) * 8)) return DMX_ERR_NOMEM;
    uint8_t* const cb = c->bgzc.as<uint8_t>();
    ch->rows = reinterpret_cast<BgzfCand*>(cb + off_rows);
    ch->uoff = reinterpret_cast<uint64_t*>(cb + off_uoff);
    HIPCHK(launch_bgzf_chain(d_in, n, tile_offs, ncand, reinterpret_cast<BgzfCand*>(cb),
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

// The framed batch inflate over device-built arrays: desc / order hold `count` members (identity
// order, path 6 throughout: a member is at most 64 KiB), built by `build`.  One host
// synchronisation, the read-back of the file status.
struct BgzfBatch {
    InflateBatchDesc* desc;
    uint32_t* order;
};
template <class Build, class After>
static int bgzf_inflate_locked(dmx_ctx* c, uint8_t* base, size_t count, bool verify, hipStream_t st, Build build,
                               After after) {
    // (base: c->bgzd behind what the caller keeps there)  desc | order | results | tickets | side | key
    const size_t off_order = count * sizeof(InflateBatchDesc), off_res = off_order + up16(count * 4);
    const size_t off_ticket = off_res + count * sizeof(dmx_batch_result), off_side = off_ticket + 32;
    const size_t off_key = off_side + count * sizeof(FrameHead);
    InflateBatchDesc* const desc = reinterpret_cast<InflateBatchDesc*>(base);
    uint32_t* const order = reinterpret_cast<uint32_t*>(base + off_order);
    dmx_batch_result* const res = reinterpret_cast<dmx_batch_result*>(base + off_res);
    unsigned int* const ticket = reinterpret_cast<unsigned int*>(base + off_ticket);
    FrameHead* const side = reinterpret_cast<FrameHead*>(base + off_side);
    unsigned long long* const key = reinterpret_cast<unsigned long long*>(base + off_key);
    HIPCHK(hipMemsetAsync(res, 0xFF, off_ticket - off_res, st));
    HIPCHK(hipMemsetAsync(key, 0xFF, 8, st));
    HIPCHK(build(BgzfBatch{desc, order}));
    HIPCHK(launch_frame_parse(desc, side, count, DMX_FRAME_BGZF, st));
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    HIPCHK(launch_inflate_batch(desc, order, count, res, ticket, c->flags, st));
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    if (verify) HIPCHK(launch_checksum_batch(desc, res, side, count, true, ticket + 4, st));
    HIPCHK(launch_frame_verdict(side, res, count, DMX_FRAME_BGZF, verify, st));
    HIPCHK(launch_bgzf_status(res, desc, count, key, st));
    HIPCHK(after());
    HIPCHK(hipEventRecord(c->ev_inf, st));
    c->inf_pending = true;
    unsigned long long k = 0;
    HIPCHK(hipMemcpyAsync(&k, key, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    end_timing(c, st);
    c->stats.segments = count;
    c->stats.path = 6;
    return k == ~0ull ? DMX_OK : (int)(int32_t)(uint32_t)k;
}
static size_t bgzf_batch_bytes(size_t count) {
    return count * (sizeof(InflateBatchDesc) + sizeof(dmx_batch_result) + sizeof(FrameHead)) + up16(count * 4) + 48;
}
}  // extern "C++"

int dmx_deflate_bgzf_device(dmx_ctx* c, const void* d_in, size_t n, int level, void* d_out, size_t cap,
                            size_t* out_len, void* stream) {
    if (!c || (!d_in && n) || !out_len || (!d_out && cap)) return DMX_ERR_ARG;
    if (c->seg != 16384 && c->seg != 32768) return DMX_ERR_ARG;  // as dmx_deflate_batch_framed_device
    *out_len = 0;
    const size_t nblk = (n + kBgzfBlock - 1) / kBgzfBlock;
    if (nblk >= (size_t)DF_BATCH_LAST) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (!nblk) {  // the EOF member alone
        *out_len = kBgzfEofBytes;
        if (cap < kBgzfEofBytes) return DMX_ERR_CAPACITY;
        HIPCHK(hipMemcpyAsync(d_out, kBgzfEof, kBgzfEofBytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        return DMX_OK;
    }
    // member i into slot i, as dmx_deflate_bgzf does on the host
    const size_t slot = dmx_batch_framed_bound(DMX_FRAME_BGZF, kBgzfBlock);
    std::vector<const uint8_t*> ins;
    std::vector<uint8_t*> outs;
    std::vector<size_t> ns, caps;
    std::vector<dmx_batch_result> res;
    try {
        ins.resize(nblk);
        outs.resize(nblk);
        ns.resize(nblk);
        caps.assign(nblk, slot);
        res.resize(nblk);
    } catch (const std::bad_alloc&) {
        return DMX_ERR_NOMEM;
    }
    const size_t off_offs = up16(nblk * 4), off_key = off_offs + up16(scan_words(nblk) * 8);
    if (!c->bgzs.ensure(nblk * slot + 16) || !c->bgzc.ensure(off_key + 16 + sizeof(BgzfChainHead))) return DMX_ERR_NOMEM;
    for (size_t i = 0; i < nblk; i++) {
        ins[i] = static_cast<const uint8_t*>(d_in) + i * kBgzfBlock;
        ns[i] = std::min<size_t>(kBgzfBlock, n - i * kBgzfBlock);
        outs[i] = c->bgzs.as<uint8_t>() + i * slot;
    }
    const int rc = deflate_batch_framed_locked(c, ins.data(), ns.data(), nblk, level, DMX_FRAME_BGZF, outs.data(),
                                               caps.data(), res.data(), st);
    if (rc != DMX_OK) return rc;
    // the members back to back into d_out, the EOF member behind them; the results are still in
    // c->bres, where the batch left them
    uint8_t* const cb = c->bgzc.as<uint8_t>();
    unsigned long long* const key = reinterpret_cast<unsigned long long*>(cb + off_key);
    BgzfChainHead* const head = reinterpret_cast<BgzfChainHead*>(cb + off_key + 16);
    HIPCHK(hipMemsetAsync(key, 0xFF, 8, st));
    HIPCHK(launch_bgzf_pack(c->bgzs.as<uint8_t>(), slot, c->bres.as<dmx_batch_result>(), nblk,
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
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
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
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
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
    if (!c->bgzd.ensure(bgzf_batch_bytes(ch.members))) return DMX_ERR_NOMEM;
    const uint8_t* const in = static_cast<const uint8_t*>(d_in);
    uint8_t* const out = static_cast<uint8_t*>(d_out);
    rc = bgzf_inflate_locked(
        c, c->bgzd.as<uint8_t>(), ch.members, (flags & DMX_VERIFY) != 0, st,
        [&](const BgzfBatch& b) { return launch_bgzf_desc(in, ch.rows, ch.uoff, ch.members, out, b.desc, b.order, st); },
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
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const size_t idx_bytes = up16((count + 1) * sizeof(dmx_bgzf_entry));
    if (!c->bgzs.ensure(edge0 + edge1 + 16) || !c->bgzd.ensure(idx_bytes + bgzf_batch_bytes(count))) return DMX_ERR_NOMEM;
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    begin_timing(c, st);
    dmx_bgzf_entry* const d_idx = c->bgzd.as<dmx_bgzf_entry>();
    HIPCHK(hipMemcpyAsync(d_idx, index + k0, (count + 1) * sizeof(dmx_bgzf_entry), hipMemcpyHostToDevice, st));
    const uint8_t* const in = static_cast<const uint8_t*>(d_in);
    uint8_t* const out = static_cast<uint8_t*>(d_out);
    uint8_t* const edge = c->bgzs.as<uint8_t>();
    const int rc = bgzf_inflate_locked(
        c, c->bgzd.as<uint8_t>() + idx_bytes, count, (flags & DMX_VERIFY) != 0, st,
        [&](const BgzfBatch& b) {
            return launch_bgzf_range_desc(in, d_idx, count, u0, u1, out, edge, b.desc, b.order, st);
        },
        [&] { return launch_bgzf_range_copy(d_idx, count, u0, u1, edge, out, st); });
    c->stats.out_bytes = rc == DMX_OK ? len : 0;
    return rc;
}

// ---- multi-member gzip files (gzip_members.hip; the walk: gzip_members.h) ----------------------
extern "C++" {
// Developer switch, read per call and only with dmx_set_timing on: which phase
// dmx_stats.ms_main_kernel brackets -- DMX_GZM_MAIN=scan (candidate count, its host read and the
// candidate list), =measure (the measuring pass); anything else: the batch decode.
static int gzm_main_phase(const dmx_ctx* c) {
    if (!c->timing) return 2;
    const char* e = std::getenv("DMX_GZM_MAIN");
    return e && !std::strcmp(e, "scan") ? 0 : e && !std::strcmp(e, "measure") ? 1 : 2;
}

// The file d_in[0, n) -> out[0, cap).  Scratch: c->bgzt (tile counts and offsets, the small words),
// c->bgzc (candidates and records), c->bgzd (the gap list, then the batch's arrays) -- the BGZF
// device calls' buffers, which like this call end synchronised and wait for c->ev_inf.
static int gzip_members_locked(dmx_ctx* c, const uint8_t* in, size_t n, bool verify, uint8_t* out, size_t cap,
                               dmx_bgzf_entry* entries, size_t entry_cap, size_t* members, size_t* out_len,
                               hipStream_t st) {
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    begin_timing(c, st);
    const int phase = gzm_main_phase(c);
    // ---- candidates and their records ----
    const uint64_t nt = gzm_tiles(in, n);
    const size_t off_offs = up16(nt * 4), off_words = off_offs + up16(scan_words(nt) * 8);
    if (!c->bgzt.ensure(off_words + 128)) return DMX_ERR_NOMEM;
    uint8_t* const tb = c->bgzt.as<uint8_t>();
    uint64_t* const tile_offs = reinterpret_cast<uint64_t*>(tb + off_offs);
    // the small words: candidate count | gap flag | gap result (2) | measuring ticket | the batch's
    // tickets (decode, checksum) | the batch's key
    uint64_t* const d_ncand = reinterpret_cast<uint64_t*>(tb + off_words);
    unsigned long long* const d_flag = reinterpret_cast<unsigned long long*>(tb + off_words + 8);
    uint64_t* const d_gapres = reinterpret_cast<uint64_t*>(tb + off_words + 16);
    unsigned int* const d_mticket = reinterpret_cast<unsigned int*>(tb + off_words + 32);
    unsigned int* const d_ticket = reinterpret_cast<unsigned int*>(tb + off_words + 48);
    unsigned long long* const d_key = reinterpret_cast<unsigned long long*>(tb + off_words + 80);
    if (phase == 0) (void)hipEventRecord(c->ev[1], st);
    HIPCHK(launch_gzm_count(in, n, reinterpret_cast<uint32_t*>(tb), tile_offs, d_ncand, st));
    uint64_t ncand = 0;
    HIPCHK(hipMemcpyAsync(&ncand, d_ncand, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ncand >= 0xFFFFFFFFull) return DMX_ERR_NOMEM;  // (tickets and order entries are 32-bit)
    std::vector<GzmCand> hc;
    std::vector<GzmRec> hr;
    std::vector<GzmRow> rows;
    std::vector<GzmGap> gaps;
    std::vector<uint64_t> uoffs;   // rows[k]'s first plain byte
    std::vector<uint32_t> small;   // the rows the batch decodes (the others are long: decoded in the walk)
    try {
        hc.resize(ncand);
        hr.resize(ncand);
    } catch (const std::bad_alloc&) {
        return DMX_ERR_NOMEM;
    }
    const size_t off_recs = up16(ncand * sizeof(GzmCand));
    if (!c->bgzc.ensure(off_recs + ncand * sizeof(GzmRec) + 16)) return DMX_ERR_NOMEM;
    GzmCand* const d_cands = c->bgzc.as<GzmCand>();
    GzmRec* const d_recs = reinterpret_cast<GzmRec*>(c->bgzc.as<uint8_t>() + off_recs);
    HIPCHK(launch_gzm_write(in, n, tile_offs, d_cands, ncand, st));
    if (phase == 0) (void)hipEventRecord(c->ev[2], st);
    if (phase == 1) (void)hipEventRecord(c->ev[1], st);
    int occupancy = 0;
    HIPCHK(launch_gzm_measure(in, n, d_cands, ncand, d_recs, d_mticket, c->flags, kBatchRouteBytes, st, &occupancy));
    if (phase == 1) (void)hipEventRecord(c->ev[2], st);
    if (c->diag & DIAG_DEBUG)
        std::fprintf(stderr, "dmx: gzip members: %llu candidates, measuring pass at %d workgroups per CU\n",
                     (unsigned long long)ncand, occupancy);
    if (ncand) {
        HIPCHK(hipMemcpyAsync(hc.data(), d_cands, ncand * sizeof(GzmCand), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hr.data(), d_recs, ncand * sizeof(GzmRec), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    float phase_ms = 0;  // (read here: a long member's own call records these events anew)
    if (phase < 2 && ncand) {
        (void)hipEventElapsedTime(&phase_ms, c->ev[1], c->ev[2]);
        (void)hipGetLastError();
    }
    // ---- the chain: the host's walk, a long member decoded where the walk meets it ----
    uint64_t total = 0, from = 0;
    int tail = DMX_OK;  // what ended the chain early: the first failure that is not a batch member's
    bool bad_start = false;
    try {
        for (;;) {
            const GzmWalk w = gzm_walk(hc.data(), hr.data(), ncand, n, from, &rows, &gaps);
            for (size_t k = uoffs.size(); k < rows.size(); k++) {
                uoffs.push_back(total);
                small.push_back((uint32_t)k);
                total += rows[k].plain;
            }
            if (w.what == GZM_DONE) break;
            if (w.what == GZM_BAD_START) {
                bad_start = true;
                break;
            }
            if (w.what != GZM_LONG) {
                tail = w.what;
                break;
            }
            // a long member: the single-stream plan, straight into its place
            if (!out || total > cap) {
                tail = DMX_ERR_CAPACITY;  // (its size is not known)
                break;
            }
            const GzmCand lc = hc[w.k];
            const uint64_t s0 = lc.off + lc.head;
            GzmCut cut = gzm_first_cut(hc.data(), ncand, w.k, n, kBatchRouteBytes);
            size_t len = 0;
            int rc;
            for (;;) {
                rc = inflate_device_locked(c, in + s0, (size_t)(cut.end - s0), out + total, cap - total, &len, nullptr, st);
                if (rc == DMX_ERR_NOMEM || rc == DMX_ERR_DEVICE || rc == DMX_ERR_INTERNAL) return rc;
                // DMX_ERR_OVERREAD with more of the file behind the cut: a false candidate inside the member
                if (rc != DMX_ERR_OVERREAD || !gzm_next_cut(hc.data(), ncand, n, &cut)) break;
            }
            if (rc != DMX_OK) {
                tail = rc;
                break;
            }
            const uint64_t end = s0 + c->last_end;
            if (end > n || n - end < 8) {
                tail = DMX_ERR_OVERREAD;
                break;
            }
            if (verify) {
                uint8_t t8[8];
                uint32_t ck = 0;
                HIPCHK(hipMemcpyAsync(t8, in + end, 8, hipMemcpyDeviceToHost, st));
                const int rk = checksum_locked(c, true, out + total, len, 0u, &ck, st);  // (waits for the copy too)
                if (rk != DMX_OK) return rk;
                if (frame_le32(t8) != ck || frame_le32(t8 + 4) != (uint32_t)len) {
                    tail = DMX_ERR_CHECKSUM;
                    break;
                }
            }
            rows.push_back(GzmRow{lc.off, lc.head, end, len});
            uoffs.push_back(total);
            total += len;
            from = end + 8;
        }
    } catch (const std::bad_alloc&) {
        return DMX_ERR_NOMEM;
    }
    // ---- the spaces between the members: zeros, or the status of the header expected there ----
    if (bad_start || !gaps.empty()) {
        uint64_t longest = 0;
        for (const GzmGap& g : gaps) longest = std::max(longest, g.b - g.a);
        GzmGap* d_gaps = nullptr;
        if (!bad_start) {
            if (!c->bgzd.ensure(gaps.size() * sizeof(GzmGap))) return DMX_ERR_NOMEM;
            d_gaps = c->bgzd.as<GzmGap>();
            HIPCHK(hipMemcpyAsync(d_gaps, gaps.data(), gaps.size() * sizeof(GzmGap), hipMemcpyHostToDevice, st));
        }
        HIPCHK(launch_gzm_gaps(in, n, d_gaps, bad_start ? 0 : gaps.size(), longest, bad_start ? 0ull : ~0ull, d_flag,
                               d_gapres, st));
        uint64_t gr[2] = {~0ull, 0};
        HIPCHK(hipMemcpyAsync(gr, d_gapres, 16, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (gr[0] != ~0ull) {  // the members in front of it stay; it comes before whatever ended the walk
            while (!rows.empty() && rows.back().coff > gr[0]) {
                if (!small.empty() && small.back() == rows.size() - 1) small.pop_back();
                rows.pop_back();
                uoffs.pop_back();
            }
            total = rows.empty() ? 0 : uoffs.back() + rows.back().plain;
            tail = (int)(int64_t)gr[1];
        }
    }
    const size_t nrows = rows.size();
    if (members) *members = nrows;
    c->stats.in_bytes = n;
    c->stats.segments = nrows;
    c->stats.path = 6;
    if (tail != DMX_OK) {
        // Under DMX_VERIFY a member in front of the failure may fail its checksum, which then comes
        // first; that needs the members' bytes, so only where they fit.
        if (!verify || small.empty() || total > cap) return tail;
    } else {
        if (entries && entry_cap < nrows + 1) return DMX_ERR_CAPACITY;
        if (total > cap) {  // before any member within the measuring limit is decoded
            *out_len = (size_t)total;
            return DMX_ERR_CAPACITY;
        }
    }
    // ---- the members within the measuring limit: one framed batch inflate ----
    const size_t count = small.size();
    if (count) {
        std::vector<uint64_t> image;
        const size_t off_order = count * sizeof(InflateBatchDesc), off_res = off_order + up16(count * 4);
        const size_t off_side = off_res + count * sizeof(dmx_batch_result);
        try {
            image.resize(off_res / 8);
        } catch (const std::bad_alloc&) {
            return DMX_ERR_NOMEM;
        }
        InflateBatchDesc* const hd = reinterpret_cast<InflateBatchDesc*>(image.data());
        uint32_t* const ho = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(image.data()) + off_order);
        for (size_t i = 0; i < count; i++) {  // buffer i = the member with its header and trailer
            const GzmRow& r = rows[small[i]];
            hd[i] = InflateBatchDesc{in + r.coff, r.end + 8 - r.coff, out + uoffs[small[i]], r.plain};
            ho[i] = (uint32_t)i;
        }
        std::stable_sort(ho, ho + count, [&](uint32_t a, uint32_t b) { return hd[a].n > hd[b].n; });  // longest first
        if (!c->bgzd.ensure(off_side + count * sizeof(FrameHead))) return DMX_ERR_NOMEM;
        uint8_t* const base = c->bgzd.as<uint8_t>();
        InflateBatchDesc* const desc = reinterpret_cast<InflateBatchDesc*>(base);
        const uint32_t* const order = reinterpret_cast<const uint32_t*>(base + off_order);
        dmx_batch_result* const res = reinterpret_cast<dmx_batch_result*>(base + off_res);
        FrameHead* const side = reinterpret_cast<FrameHead*>(base + off_side);
        HIPCHK(hipMemcpyAsync(base, image.data(), off_res, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(res, 0xFF, count * sizeof(dmx_batch_result), st));
        HIPCHK(hipMemsetAsync(d_key, 0xFF, 8, st));
        HIPCHK(launch_frame_parse(desc, side, count, DMX_FRAME_GZIP, st));
        if (phase == 2 && c->timing) (void)hipEventRecord(c->ev[1], st);
        HIPCHK(launch_inflate_batch(desc, order, count, res, d_ticket, c->flags, st));
        if (phase == 2 && c->timing) (void)hipEventRecord(c->ev[2], st);
        if (verify) HIPCHK(launch_checksum_batch(desc, res, side, count, true, d_ticket + 4, st));
        HIPCHK(launch_frame_verdict(side, res, count, DMX_FRAME_GZIP, verify, st));
        HIPCHK(launch_gzm_status(res, desc, count, d_key, st));
        HIPCHK(hipEventRecord(c->ev_inf, st));
        c->inf_pending = true;
        unsigned long long key = 0;
        HIPCHK(hipMemcpyAsync(&key, d_key, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));  // (the image is a local: the upload has finished too)
        if (key != ~0ull) {
            if (members) *members = small[(size_t)(key >> 32)];
            end_timing(c, st);
            return (int)(int32_t)(uint32_t)key;
        }
    }
    end_timing(c, st);
    if (phase < 2) c->stats.ms_main_kernel = phase_ms;
    if (tail != DMX_OK) return tail;
    if (entries) {
        for (size_t k = 0; k < nrows; k++) entries[k] = dmx_bgzf_entry{rows[k].coff, uoffs[k]};
        entries[nrows] = dmx_bgzf_entry{n, total};
    }
    c->stats.out_bytes = total;
    *out_len = (size_t)total;
    return DMX_OK;
}
}  // extern "C++"

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
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return gzip_members_locked(c, static_cast<const uint8_t*>(d_in), n, (flags & DMX_VERIFY) != 0,
                               static_cast<uint8_t*>(d_out), cap, entries, entry_cap, members, out_len, st);
}

int dmx_inflate_gzip_members(dmx_ctx* c, const uint8_t* in, size_t n, uint32_t flags, uint8_t* out, size_t cap,
                             size_t* members, size_t* out_len) {
    if (!c || !out_len || (!in && n) || (!out && cap) || (flags & ~DMX_VERIFY)) return DMX_ERR_ARG;
    *out_len = 0;
    if (members) *members = 0;
    if (!n) return DMX_OK;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
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

// ---- seek index and ranged reads for unblocked streams ----------------------------------------
// (the decisions: seek_plan.h; the kernels: inflate_span.hip; the checkpoint hand-over: the
// context's seek_tap, which host_fb.cpp and host_inflate.cpp fill when it is set)
size_t dmx_seek_windows_bound(size_t cap, size_t spacing) {
    return spacing < DMX_SEEK_WINDOW ? 0 : (cap / spacing + 2) * (size_t)DMX_SEEK_WINDOW;
}

int dmx_inflate_index_device(dmx_ctx* c, const void* d_in, size_t n, void* d_out, size_t cap, size_t spacing,
                             dmx_seek_entry* entries, size_t entry_cap, void* d_windows, size_t windows_cap,
                             size_t* count, size_t* out_len, void* stream) {
    if (!c || (!d_in && n) || !d_out || !out_len || !count || spacing < DMX_SEEK_WINDOW ||
        (!entries && entry_cap) || (!d_windows && windows_cap))
        return DMX_ERR_ARG;
    *count = 0;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    SeekTap tap;
    c->seek_tap = &tap;
    const int rc = inflate_device_locked(c, (const uint8_t*)d_in, n, (uint8_t*)d_out, cap, out_len, nullptr, st);
    c->seek_tap = nullptr;
    if (rc != DMX_OK) return rc;
    const std::vector<dmx_seek_entry> sel = seek_select(tap.cands.data(), tap.cands.size(), spacing);
    *count = sel.size();
    if (entry_cap < sel.size() + 1 || windows_cap / DMX_SEEK_WINDOW < sel.size()) return DMX_ERR_CAPACITY;
    std::copy(sel.begin(), sel.end(), entries);
    entries[sel.size()] = dmx_seek_entry{8 * c->last_end, *out_len, 0, 0};
    std::vector<SeekSlot> slots;
    for (size_t k = 0; k < sel.size(); k++)
        if (!(sel[k].flags & DMX_SEEK_NOWINDOW)) slots.push_back({k, sel[k].uoffset});
    if (slots.empty()) return DMX_OK;
    if (!c->seekd.ensure(slots.size() * sizeof(SeekSlot))) return DMX_ERR_NOMEM;
    HIPCHK(hipMemcpyAsync(c->seekd.p, slots.data(), slots.size() * sizeof(SeekSlot), hipMemcpyHostToDevice, st));
    HIPCHK(launch_seek_gather((const uint8_t*)d_out, c->seekd.as<SeekSlot>(), slots.size(), (uint8_t*)d_windows, st));
    HIPCHK(hipStreamSynchronize(st));
    return DMX_OK;
}

int dmx_inflate_range_device(dmx_ctx* c, const void* d_in, size_t n, const dmx_seek_entry* entries, size_t count,
                             const void* d_windows, uint64_t uoffset, size_t len, void* d_out, void* stream) {
    if (!c || (!d_in && n) || !entries) return DMX_ERR_ARG;
    std::vector<SeekSpan> spans;
    if (const int rc = seek_range_plan(entries, count, n, uoffset, len, &spans); rc != DMX_OK) return rc;
    if (spans.empty()) return DMX_OK;
    if (!d_out || spans.size() > 0x7FFFFFFFull) return DMX_ERR_ARG;
    for (const SeekSpan& s : spans)
        if (s.window && !d_windows) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    // one upload: the head {ticket 0, key all ones}, then the spans; one launch; the key back
    const size_t bytes = sizeof(SeekSpanHead) + spans.size() * sizeof(SeekSpan);
    if (!c->seekd.ensure(bytes)) return DMX_ERR_NOMEM;
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    begin_timing(c, st);
    std::vector<uint8_t> up(bytes);
    const SeekSpanHead head{0, 0, ~0ull};
    std::memcpy(up.data(), &head, sizeof head);
    std::memcpy(up.data() + sizeof head, spans.data(), spans.size() * sizeof(SeekSpan));
    SeekSpanHead* const d_head = c->seekd.as<SeekSpanHead>();
    HIPCHK(hipMemcpyAsync(d_head, up.data(), bytes, hipMemcpyHostToDevice, st));
    const StreamWords w((const uint8_t*)d_in);
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    HIPCHK(launch_inflate_spans(w.words, w.misalign, n, reinterpret_cast<const SeekSpan*>(d_head + 1),
                                (uint32_t)spans.size(), (const uint8_t*)d_windows, (uint8_t*)d_out, d_head, c->flags,
                                st));
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    unsigned long long key = ~0ull;
    HIPCHK(hipMemcpyAsync(&key, &d_head->key, 8, hipMemcpyDeviceToHost, st));
    mark_end(c, st);
    HIPCHK(hipStreamSynchronize(st));
    end_timing(c, st);
    const int rc = key == ~0ull ? DMX_OK : (int)(int32_t)(uint32_t)key;
    c->stats.segments = spans.size();
    c->stats.in_bytes = n;
    c->stats.out_bytes = rc == DMX_OK ? len : 0;
    return rc;
}

int dmx_deflate(dmx_ctx* c, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap,
                size_t* out_len) {
    if (!c) c = dmx_default_ctx();
    if (!c) return DMX_ERR_DEVICE;
    if ((!in && n) || !out_len || (!out && cap)) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (c->subs.size() > 1 && n >= 2 * c->subs.size() * (size_t)c->seg)
        return deflate_multi(c, in, n, level, out, cap, out_len);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    const size_t bound = dmx_deflate_bound(n);
    if (!c->in.ensure(n + 16) || !c->out.ensure(bound)) return DMX_ERR_NOMEM;
    if (n) HIPCHK(hipMemcpyAsync(c->in.p, in, n, hipMemcpyHostToDevice, c->stream));
    size_t total = 0;
    int rc = deflate_device_locked(c, c->in.as<uint8_t>(), n, level, 0, c->out.as<uint8_t>(),
                                   c->out.cap, &total, c->stream);
    *out_len = total;
    if (rc != DMX_OK) return rc;
    if (total > cap) return DMX_ERR_CAPACITY;
    if (total) HIPCHK(hipMemcpyAsync(out, c->out.p, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return DMX_OK;
}

static int inflate_host(dmx_ctx* c, const uint8_t* in, size_t n, uint8_t** dev, size_t* total) {
    if (!c->in.ensure(n + 16)) return DMX_ERR_NOMEM;
    if (n) HIPCHK(hipMemcpyAsync(c->in.p, in, n, hipMemcpyHostToDevice, c->stream));
    return inflate_device_locked(c, c->in.as<uint8_t>(), n, nullptr, 0, total, dev, c->stream);
}

int dmx_inflate(dmx_ctx* c, const uint8_t* in, size_t n, uint8_t* out, size_t cap,
                size_t* written, size_t* total) {
    if (!c) c = dmx_default_ctx();
    if (!c) return DMX_ERR_DEVICE;
    if ((!in && n) || (!out && cap) || !written) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    uint8_t* dev = nullptr;
    size_t tot = 0;
    *written = 0;
    if (total) *total = 0;
    if (c->subs.size() > 1 && n >= 4 * c->subs.size() * (size_t)c->seg) {
        const int mr = inflate_multi(c, in, n, out, cap, nullptr, written, &tot);
        if (mr != 1) {
            if (total) *total = tot;
            return mr;
        }
    }
    int rc = inflate_host(c, in, n, &dev, &tot);
    if (rc != DMX_OK) return rc;
    const size_t w = tot < cap ? tot : cap;
    if (w) HIPCHK(hipMemcpyAsync(out, dev, w, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *written = w;
    if (total) *total = tot;
    return DMX_OK;
}

int dmx_inflate_alloc(dmx_ctx* c, const uint8_t* in, size_t n, uint8_t** out, size_t* len) {
    if (!c) c = dmx_default_ctx();
    if (!c) return DMX_ERR_DEVICE;
    if ((!in && n) || !out || !len) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    *out = nullptr;
    *len = 0;
    uint8_t* dev = nullptr;
    size_t tot = 0;
    if (c->subs.size() > 1 && n >= 4 * c->subs.size() * (size_t)c->seg) {
        const int mr = inflate_multi(c, in, n, nullptr, 0, out, nullptr, &tot);
        if (mr != 1) {
            if (mr == DMX_OK) *len = tot;
            return mr;
        }
    }
    int rc = inflate_host(c, in, n, &dev, &tot);
    if (rc != DMX_OK) return rc;
    uint8_t* h = static_cast<uint8_t*>(std::malloc(tot ? tot : 1));
    if (!h) return DMX_ERR_NOMEM;
    if (tot && hipMemcpyAsync(h, dev, tot, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
        std::free(h);
        return DMX_ERR_DEVICE;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
        std::free(h);
        return DMX_ERR_DEVICE;
    }
    *out = h;
    *len = tot;
    return DMX_OK;
}

// ---- segment index for multi-GPU inflate ------------------------------------
int dmx_segment_starts_device(dmx_ctx* c, const void* d_in, size_t n, uint64_t* starts, size_t cap,
                              size_t* count, void* stream) {
    if (!c || (!d_in && n) || !count || (!starts && cap)) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    *count = 0;
    if (n == 0) return DMX_OK;
    if (!c->scal.ensure(sizeof(Scal))) return DMX_ERR_NOMEM;
    Scal* ds = c->scal.as<Scal>();
    const StreamWords w(static_cast<const uint8_t*>(d_in));
    uint64_t ntiles = 0;
    if (const int rc = marker_scan(c, w, n, &ntiles, st); rc != DMX_OK) return rc;
    uint64_t nm = 0;
    HIPCHK(hipMemcpyAsync(&nm, &ds->nmarkers, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!c->cands.ensure((nm + 1) * 8)) return DMX_ERR_NOMEM;
    if (marker_write(c, w, n, ntiles, ~0ull, st) != DMX_OK) return DMX_ERR_DEVICE;
    // cands[0] is the stream start; markers follow
    const size_t k = std::min<size_t>(cap, nm);
    if (k) HIPCHK(hipMemcpyAsync(starts, c->cands.as<uint64_t>() + 1, k * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *count = nm;
    return DMX_OK;
}

int dmx_segment_check_device(dmx_ctx* c, const void* d_in, size_t n, const uint64_t* starts, size_t k,
                             uint64_t* ends, void* stream) {
    if (!c || (!d_in && n) || (k && (!starts || !ends))) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (k == 0) return DMX_OK;
    if (!c->cands.ensure(2 * k * 8)) return DMX_ERR_NOMEM;
    uint64_t* d_starts = c->cands.as<uint64_t>();
    uint64_t* d_ends = d_starts + k;
    HIPCHK(hipMemcpyAsync(d_starts, starts, k * 8, hipMemcpyHostToDevice, st));
    const uint8_t* in = static_cast<const uint8_t*>(d_in);
    InflateArgs A{};
    A.misalign = (uintptr_t)in & 3;
    A.in_words = reinterpret_cast<const uint32_t*>(in - A.misalign);
    A.n = n;
    A.flags = c->flags | DMX_IFLAG_PIECE;
    HIPCHK(launch_segment_check(A, d_starts, k, d_ends, st));
    HIPCHK(hipMemcpyAsync(ends, d_ends, k * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DMX_OK;
}

// ---- checksums and zlib / gzip containers ------------------------------
int dmx_adler32_device(dmx_ctx* c, const void* d, size_t n, uint32_t init, uint32_t* out, void* stream) {
    if (!c || (!d && n) || !out) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    return checksum_locked(c, false, (const uint8_t*)d, n, init, out, stream ? (hipStream_t)stream : c->stream);
}

int dmx_crc32_device(dmx_ctx* c, const void* d, size_t n, uint32_t init, uint32_t* out, void* stream) {
    if (!c || (!d && n) || !out) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    return checksum_locked(c, true, (const uint8_t*)d, n, init, out, stream ? (hipStream_t)stream : c->stream);
}

static int checksum_host(dmx_ctx* c, bool crc, const uint8_t* in, size_t n, uint32_t init, uint32_t* out) {
    if (!c) c = dmx_default_ctx();
    if (!c) return DMX_ERR_DEVICE;
    if ((!in && n) || !out) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    if (!c->in.ensure(n + 16)) return DMX_ERR_NOMEM;
    if (n) HIPCHK(hipMemcpyAsync(c->in.p, in, n, hipMemcpyHostToDevice, c->stream));
    return checksum_locked(c, crc, c->in.as<uint8_t>(), n, init, out, c->stream);
}

int dmx_adler32(dmx_ctx* c, const uint8_t* in, size_t n, uint32_t init, uint32_t* out) {
    return checksum_host(c, false, in, n, init, out);
}

int dmx_crc32(dmx_ctx* c, const uint8_t* in, size_t n, uint32_t init, uint32_t* out) {
    return checksum_host(c, true, in, n, init, out);
}

size_t dmx_framed_bound(size_t n) { return dmx_deflate_bound(n) + 18; }

static int deflate_framed_entry(dmx_ctx* c, bool gz, const uint8_t* in, size_t n, int level, uint8_t* out,
                                size_t cap, size_t* out_len) {
    if (!c) c = dmx_default_ctx();
    if (!c) return DMX_ERR_DEVICE;
    if ((!in && n) || !out_len || !out) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    return deflate_framed(c, gz, in, n, level, out, cap, out_len);
}

int dmx_deflate_zlib(dmx_ctx* c, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap,
                     size_t* out_len) {
    return deflate_framed_entry(c, false, in, n, level, out, cap, out_len);
}

int dmx_deflate_gzip(dmx_ctx* c, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap,
                     size_t* out_len) {
    return deflate_framed_entry(c, true, in, n, level, out, cap, out_len);
}

// Parses the container header, inflates the raw stream on the GPU and (DMX_VERIFY) checks the
// trailer against the GPU checksum of the decoded bytes.  The trailer is taken from the last
// 4 (zlib) / 8 (gzip) bytes of the input.
static int inflate_framed(dmx_ctx* c, bool gz, const uint8_t* in, size_t n, uint32_t flags, uint8_t** out,
                          size_t* len) {
    if (!c) c = dmx_default_ctx();
    if (!c) return DMX_ERR_DEVICE;
    if ((!in && n) || !out || !len) return DMX_ERR_ARG;
    *out = nullptr;
    *len = 0;
    // (container_parse.h: the parse the framed batch kernels run)
    const FrameHead fh = parse_frame(gz ? DMX_FRAME_GZIP : DMX_FRAME_ZLIB, in, n);
    if (fh.status != DMX_OK) return fh.status;
    const size_t head = (size_t)fh.head;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    uint8_t* dev = nullptr;
    size_t tot = 0;
    int rc = inflate_host(c, in + head, n - head, &dev, &tot);
    if (rc != DMX_OK) return rc;
    if (flags & DMX_VERIFY) {
        uint32_t ck = 0;
        rc = checksum_locked(c, gz, dev, tot, gz ? 0u : 1u, &ck, c->stream);
        if (rc != DMX_OK) return rc;
        if (gz && fh.isize != (uint32_t)tot) return DMX_ERR_CHECKSUM;
        if (ck != fh.want) return DMX_ERR_CHECKSUM;
    }
    uint8_t* h = static_cast<uint8_t*>(std::malloc(tot ? tot : 1));
    if (!h) return DMX_ERR_NOMEM;
    if (tot && hipMemcpyAsync(h, dev, tot, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
        std::free(h);
        return DMX_ERR_DEVICE;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
        std::free(h);
        return DMX_ERR_DEVICE;
    }
    *out = h;
    *len = tot;
    return DMX_OK;
}

int dmx_inflate_zlib(dmx_ctx* c, const uint8_t* in, size_t n, uint32_t flags, uint8_t** out, size_t* len) {
    return inflate_framed(c, false, in, n, flags, out, len);
}

int dmx_inflate_gzip(dmx_ctx* c, const uint8_t* in, size_t n, uint32_t flags, uint8_t** out, size_t* len) {
    return inflate_framed(c, true, in, n, flags, out, len);
}

// ---- file-path overloads with streaming I/O ----------------------------
namespace {

struct Pinned {
    void* p = nullptr;
    explicit Pinned(size_t n) {
        if (hipHostMalloc(&p, n ? n : 1, hipHostMallocDefault) != hipSuccess) p = nullptr;
    }
    ~Pinned() {
        if (p) (void)hipHostFree(p);
    }
    uint8_t* u8() const { return static_cast<uint8_t*>(p); }
};

struct File {
    FILE* f = nullptr;
    File(const char* path, const char* mode) : f(std::fopen(path, mode)) {}
    ~File() {
        if (f) std::fclose(f);
    }
};

// A reader thread fills two pinned buffers in turn from a file (chunk k into buffer k % 2);
// the consumer takes chunk k, and releases its buffer once the H2D copy from it has finished.
struct ChunkReader {
    FILE* f;
    size_t chunk, total, nchunks;
    uint8_t* buf[2];
    size_t len[2] = {0, 0};
    bool ready[2] = {false, false};
    bool failed = false, stop = false;
    std::mutex m;
    std::condition_variable cv;
    std::thread th;
    ChunkReader(FILE* f_, size_t total_, size_t chunk_, uint8_t* b0, uint8_t* b1)
        : f(f_), chunk(chunk_), total(total_), nchunks((total_ + chunk_ - 1) / chunk_), buf{b0, b1} {
        th = std::thread([this] { run(); });
    }
    ~ChunkReader() {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        cv.notify_all();
        th.join();
    }
    void run() {
        for (size_t k = 0; k < nchunks; k++) {
            const int b = (int)(k & 1);
            {
                std::unique_lock<std::mutex> g(m);
                cv.wait(g, [&] { return !ready[b] || stop; });
                if (stop) return;
            }
            const size_t want = std::min(chunk, total - k * chunk);
            const size_t got = std::fread(buf[b], 1, want, f);
            std::lock_guard<std::mutex> g(m);
            len[b] = want;
            ready[b] = true;
            if (got != want) failed = true;
            cv.notify_all();
        }
    }
    // waits for chunk k; returns its buffer and length (nullptr on a read error)
    uint8_t* take(size_t k, size_t* n) {
        const int b = (int)(k & 1);
        std::unique_lock<std::mutex> g(m);
        cv.wait(g, [&] { return ready[b] || failed; });
        if (failed) return nullptr;
        *n = len[b];
        return buf[b];
    }
    void release(size_t k) {
        std::lock_guard<std::mutex> g(m);
        ready[k & 1] = false;
        cv.notify_all();
    }
};

// A writer thread takes the compressed chunks in order: chunk k's D2H into pinned buffer
// k % 2 was recorded on an event by the producer; the writer waits for the event and writes
// the bytes, then frees the buffer for chunk k + 2.  The producer meanwhile compresses the
// next chunk, so the D2H and the file write of chunk k overlap the compression of k + 1.
struct ChunkWriter {
    FILE* f;
    uint8_t* buf[2];
    hipEvent_t ev[2];
    size_t len[2] = {0, 0};
    bool full[2] = {false, false};
    bool failed = false, stop = false;
    size_t next = 0, queued = 0;  // next chunk to write, chunks handed over
    std::mutex m;
    std::condition_variable cv;
    std::thread th;
    ChunkWriter(FILE* f_, uint8_t* b0, uint8_t* b1, hipEvent_t e0, hipEvent_t e1)
        : f(f_), buf{b0, b1}, ev{e0, e1} {
        th = std::thread([this] { run(); });
    }
    ~ChunkWriter() {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        cv.notify_all();
        th.join();
    }
    void run() {
        for (;;) {
            size_t k, n;
            {
                std::unique_lock<std::mutex> g(m);
                cv.wait(g, [&] { return full[next & 1] || stop; });
                if (!full[next & 1]) return;  // stop with nothing queued
                k = next;
                n = len[k & 1];
            }
            bool ok = hipEventSynchronize(ev[k & 1]) == hipSuccess;
            ok = ok && (n == 0 || std::fwrite(buf[k & 1], 1, n, f) == n);
            std::lock_guard<std::mutex> g(m);
            if (!ok) failed = true;
            full[k & 1] = false;
            next++;
            cv.notify_all();
        }
    }
    // waits until buffer k % 2 is free (chunk k - 2 written); false after a write error
    bool acquire(size_t k) {
        std::unique_lock<std::mutex> g(m);
        cv.wait(g, [&] { return !full[k & 1] || failed; });
        return !failed;
    }
    void hand_over(size_t k, size_t n) {
        std::lock_guard<std::mutex> g(m);
        len[k & 1] = n;
        full[k & 1] = true;
        queued = k + 1;
        cv.notify_all();
    }
    bool drain() {  // all handed-over chunks written
        std::unique_lock<std::mutex> g(m);
        cv.wait(g, [&] { return next == queued || failed; });
        return !failed;
    }
};

int64_t file_size(FILE* f) {
    if (std::fseek(f, 0, SEEK_END) != 0) return -1;
    const long long n = ftello(f);
    if (std::fseek(f, 0, SEEK_SET) != 0) return -1;
    return n;
}

constexpr size_t kFileChunk = 64ull << 20;  // bytes per streamed chunk (a multiple of 32 KiB)

}  // namespace

int dmx_deflate_file(dmx_ctx* c, const char* in_path, const char* out_path, int level, size_t* in_bytes,
                     size_t* out_bytes) {
    if (!c) c = dmx_default_ctx();
    if (!c) return DMX_ERR_DEVICE;
    if (!in_path || !out_path) return DMX_ERR_ARG;
    File fi(in_path, "rb");
    if (!fi.f) return DMX_ERR_ARG;
    const int64_t N = file_size(fi.f);
    if (N < 0) return DMX_ERR_ARG;
    File fo(out_path, "wb");
    if (!fo.f) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    const size_t K = kFileChunk;
    const size_t bound = dmx_deflate_bound(K);
    Pinned hin0(K), hin1(K), hout0(bound), hout1(bound);
    DevBuf din[2], dout[2];
    auto release_all = [&] {
        for (auto& d : din) d.release();
        for (auto& d : dout) d.release();
    };
    if (!hin0.p || !hin1.p || !hout0.p || !hout1.p || !din[0].ensure(K) || !din[1].ensure(K) ||
        !dout[0].ensure(bound) || !dout[1].ensure(bound)) {
        release_all();
        return DMX_ERR_NOMEM;
    }
    hipStream_t cs = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr}, evo[2] = {nullptr, nullptr};
    int rc = DMX_OK;
    if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) rc = DMX_ERR_DEVICE;
    for (auto* e : {&ev[0], &ev[1], &evo[0], &evo[1]})
        if (rc == DMX_OK && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) rc = DMX_ERR_DEVICE;
    size_t written = 0;
    if (rc == DMX_OK && N == 0) {  // empty file: one empty final block, as dmx_deflate
        size_t len = 0;
        rc = deflate_device_locked(c, nullptr, 0, level, 0, dout[0].as<uint8_t>(), bound, &len, c->stream);
        if (rc == DMX_OK && hipMemcpy(hout0.p, dout[0].p, len, hipMemcpyDeviceToHost) != hipSuccess) rc = DMX_ERR_DEVICE;
        if (rc == DMX_OK && std::fwrite(hout0.p, 1, len, fo.f) != len) rc = DMX_ERR_ARG;
        written = len;
    } else if (rc == DMX_OK) {
        ChunkReader rd(fi.f, (size_t)N, K, hin0.u8(), hin1.u8());
        ChunkWriter wr(fo.f, hout0.u8(), hout1.u8(), evo[0], evo[1]);
        const size_t nch = rd.nchunks;
        // copy chunk k + 1 in on the copy stream while chunk k compresses on the context stream
        auto h2d = [&](size_t k) -> int {
            size_t n = 0;
            uint8_t* h = rd.take(k, &n);
            if (!h) return DMX_ERR_ARG;
            if (hipMemcpyAsync(din[k & 1].p, h, n, hipMemcpyHostToDevice, cs) != hipSuccess) return DMX_ERR_DEVICE;
            if (hipEventRecord(ev[k & 1], cs) != hipSuccess) return DMX_ERR_DEVICE;
            return DMX_OK;
        };
        rc = h2d(0);
        for (size_t k = 0; k < nch && rc == DMX_OK; k++) {
            if (k + 1 < nch && (rc = h2d(k + 1)) != DMX_OK) break;
            if (hipStreamWaitEvent(c->stream, ev[k & 1], 0) != hipSuccess) { rc = DMX_ERR_DEVICE; break; }
            const size_t n = std::min(K, (size_t)N - k * K);
            size_t len = 0;
            // output buffers k % 2 are free once chunk k - 2 is written (its D2H is done then)
            if (!wr.acquire(k)) { rc = DMX_ERR_ARG; break; }
            rc = deflate_device_locked(c, din[k & 1].as<uint8_t>(), n, level, k + 1 < nch ? DMX_DEFLATE_NOT_FINAL : 0,
                                       dout[k & 1].as<uint8_t>(), bound, &len, c->stream);
            if (rc != DMX_OK) break;
            rd.release(k);  // the H2D of chunk k is complete (the deflate waited for it)
            // D2H on the copy stream (after the deflate, which synchronized), written by the
            // writer thread while chunk k + 1 compresses
            if ((len && hipMemcpyAsync(k & 1 ? hout1.p : hout0.p, dout[k & 1].p, len, hipMemcpyDeviceToHost, cs) != hipSuccess) ||
                hipEventRecord(evo[k & 1], cs) != hipSuccess) { rc = DMX_ERR_DEVICE; break; }
            wr.hand_over(k, len);
            written += len;
        }
        if (!wr.drain() && rc == DMX_OK) rc = DMX_ERR_ARG;
        (void)hipStreamSynchronize(cs);
    }
    for (auto* e : {ev[0], ev[1], evo[0], evo[1]})
        if (e) (void)hipEventDestroy(e);
    if (cs) (void)hipStreamDestroy(cs);
    release_all();
    if (in_bytes) *in_bytes = (size_t)N;
    if (out_bytes) *out_bytes = written;
    return rc;
}

int dmx_inflate_file(dmx_ctx* c, const char* in_path, const char* out_path, size_t* out_bytes) {
    if (!c) c = dmx_default_ctx();
    if (!c) return DMX_ERR_DEVICE;
    if (!in_path || !out_path) return DMX_ERR_ARG;
    if (out_bytes) *out_bytes = 0;
    File fi(in_path, "rb");
    if (!fi.f) return DMX_ERR_ARG;
    const int64_t C = file_size(fi.f);
    if (C < 0) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    const size_t K = kFileChunk;
    if (!c->in.ensure((size_t)C + 16)) return DMX_ERR_NOMEM;
    Pinned hb0(K), hb1(K);
    if (!hb0.p || !hb1.p) return DMX_ERR_NOMEM;
    int rc = DMX_OK;
    {   // stream the compressed file in: disk reads overlap the H2D copies of earlier chunks
        ChunkReader rd(fi.f, (size_t)C, K, hb0.u8(), hb1.u8());
        for (size_t k = 0; k < rd.nchunks && rc == DMX_OK; k++) {
            size_t n = 0;
            uint8_t* h = rd.take(k, &n);
            if (!h) { rc = DMX_ERR_ARG; break; }
            if (hipMemcpyAsync(c->in.as<uint8_t>() + k * K, h, n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                hipStreamSynchronize(c->stream) != hipSuccess) { rc = DMX_ERR_DEVICE; break; }
            rd.release(k);
        }
    }
    if (rc != DMX_OK) return rc;
    uint8_t* dev = nullptr;
    size_t tot = 0;
    rc = inflate_device_locked(c, c->in.as<uint8_t>(), (size_t)C, nullptr, 0, &tot, &dev, c->stream);
    if (rc != DMX_OK) return rc;
    File fo(out_path, "wb");
    if (!fo.f) return DMX_ERR_ARG;
    // stream the output back: the D2H of chunk k + 1 overlaps the file write of chunk k
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (auto& e : ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) rc = DMX_ERR_DEVICE;
    uint8_t* hb[2] = {hb0.u8(), hb1.u8()};
    const size_t nch = (tot + K - 1) / K;
    auto d2h = [&](size_t k) -> bool {
        const size_t n = std::min(K, tot - k * K);
        return hipMemcpyAsync(hb[k & 1], dev + k * K, n, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
               hipEventRecord(ev[k & 1], c->stream) == hipSuccess;
    };
    if (rc == DMX_OK && nch && !d2h(0)) rc = DMX_ERR_DEVICE;
    for (size_t k = 0; k < nch && rc == DMX_OK; k++) {
        if (hipEventSynchronize(ev[k & 1]) != hipSuccess) { rc = DMX_ERR_DEVICE; break; }
        if (k + 1 < nch && !d2h(k + 1)) { rc = DMX_ERR_DEVICE; break; }
        const size_t n = std::min(K, tot - k * K);
        if (std::fwrite(hb[k & 1], 1, n, fo.f) != n) rc = DMX_ERR_ARG;
    }
    (void)hipStreamSynchronize(c->stream);
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
    if (out_bytes && rc == DMX_OK) *out_bytes = tot;
    return rc;
}

void dmx_free(void* p) { std::free(p); }

const char* dmx_strerror(int code) {
    switch (code) {
        case DMX_OK: return "ok";
        case DMX_ERR_ARG: return "invalid argument";
        case DMX_ERR_NOMEM: return "out of memory";
        case DMX_ERR_DEVICE: return "HIP device error (no usable gfx950 device?)";
        case DMX_ERR_DATA: return "invalid deflate stream";
        case DMX_ERR_OVERREAD: return "Reading bits beyond the alloted buffer size!";
        case DMX_ERR_CAPACITY: return "output buffer too small";
        case DMX_ERR_INTERNAL: return "internal error";
        case DMX_ERR_CHECKSUM: return "container checksum or length mismatch";
        default: return "unknown error";
    }
}

int dmx_set_timing(dmx_ctx* c, int enable) {
    if (!c) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    c->timing = enable != 0;
    return DMX_OK;
}

int dmx_last_stats(dmx_ctx* c, dmx_stats* st) {
    if (!c || !st) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    *st = c->stats;
    return DMX_OK;
}

}  // extern "C"
