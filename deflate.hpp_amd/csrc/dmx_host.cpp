// dmx_host.cpp -- host runtime and C-ABI of libdmx (see include/dmx.h): the context, diagnostics
// and timing, the single-stream calls and checksums, the host zlib / gzip forms, the seek calls,
// the files, multi-GPU.  The batch calls are in host_batch.cpp, BGZF and multi-member gzip in
// host_members.cpp, the inflate drivers in host_inflate.cpp and host_fb.cpp; dmx_ctx.h holds
// what they share.
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

}  // namespace dmx

namespace {

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

// The host forms' deflate: `in` up into c->in, its raw stream into c->out, *total = its length
int deflate_host(dmx_ctx* c, const uint8_t* in, size_t n, int level, size_t* total) {
    if (!c->in.ensure(n + 16) || !c->out.ensure(dmx_deflate_bound(n))) return DMX_ERR_NOMEM;
    if (n) HIPCHK(hipMemcpyAsync(c->in.p, in, n, hipMemcpyHostToDevice, c->stream));
    return deflate_device_locked(c, c->in.as<uint8_t>(), n, level, 0, c->out.as<uint8_t>(), c->out.cap, total, c->stream);
}

// zlib (RFC 1950) / gzip (RFC 1952) framing around libdmx's raw stream; the checksum of the
// input is computed on the GPU from the device copy the deflate reads.  (container_parse.h: the
// header and trailer the framed batch kernels write)
int deflate_framed(dmx_ctx* c, bool gz, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap,
                   size_t* out_len) {
    if (!c && !(c = dmx_default_ctx())) return DMX_ERR_DEVICE;
    if ((!in && n) || !out_len || !out) return DMX_ERR_ARG;
    DMX_ENTER(g, c);
    const uint32_t format = gz ? DMX_FRAME_GZIP : DMX_FRAME_ZLIB;
    const size_t head = frame_head_bytes(format), tail = frame_tail_bytes(format);
    *out_len = 0;
    size_t total = 0;
    int rc = deflate_host(c, in, n, level, &total);
    if (rc != DMX_OK) return rc;
    uint32_t ck = 0;
    rc = checksum_locked(c, gz, c->in.as<uint8_t>(), n, gz ? 0u : 1u, &ck, c->stream);
    if (rc != DMX_OK) return rc;
    *out_len = head + total + tail;
    if (head + total + tail > cap) return DMX_ERR_CAPACITY;
    frame_write_head(format, level, 0, out);
    if (total) HIPCHK(hipMemcpyAsync(out + head, c->out.p, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    frame_write_tail(format, ck, n, out + head + total);
    return DMX_OK;
}

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
    DMX_ENTER(g, c, stream);
    return deflate_device_locked(c, (const uint8_t*)d_in, n, level, flags, (uint8_t*)d_out, cap,
                                 out_len, g.st);
}

int dmx_deflate_device_async(dmx_ctx* c, const void* d_in, size_t n, int level, uint32_t flags,
                             void* d_out, size_t cap, uint64_t* d_out_len, void* stream) {
    if (!c || (!d_in && n) || !d_out || !d_out_len) return DMX_ERR_ARG;
    DMX_ENTER(g, c, stream);
    return deflate_device_locked(c, (const uint8_t*)d_in, n, level, flags, (uint8_t*)d_out, cap,
                                 nullptr, g.st, d_out_len);
}

int dmx_inflate_device(dmx_ctx* c, const void* d_in, size_t n, void* d_out, size_t cap,
                       size_t* out_len, void* stream) {
    if (!c || (!d_in && n) || !d_out || !out_len) return DMX_ERR_ARG;
    DMX_ENTER(g, c, stream);
    return inflate_device_locked(c, (const uint8_t*)d_in, n, (uint8_t*)d_out, cap, out_len,
                                 nullptr, g.st);
}

int dmx_inflate_device_async(dmx_ctx* c, const void* d_in, size_t n, void* d_out, size_t cap,
                             uint64_t* d_result, uint32_t flags, void* stream) {
    if (!c || (!d_in && n) || !d_out || !d_result || (flags & ~DMX_INFLATE_PIECE)) return DMX_ERR_ARG;
    DMX_ENTER(g, c, stream);
    return inflate_device_async_locked(c, (const uint8_t*)d_in, n, (uint8_t*)d_out, cap, d_result, g.st,
                                       (flags & DMX_INFLATE_PIECE) ? DMX_IFLAG_PIECE : 0u);
}

int dmx_inflate_piece_device(dmx_ctx* c, const void* d_in, size_t n, void* d_out, size_t cap,
                             size_t* out_len, void* stream) {
    if (!c || (!d_in && n) || !d_out || !out_len) return DMX_ERR_ARG;
    DMX_ENTER(g, c, stream);
    return inflate_device_locked(c, (const uint8_t*)d_in, n, (uint8_t*)d_out, cap, out_len, nullptr, g.st,
                                 DMX_IFLAG_PIECE);
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
    DMX_ENTER(g, c, stream);
    const hipStream_t st = g.st;
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
    DMX_ENTER(g, c, stream);
    const hipStream_t st = g.st;
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
    if (!c && !(c = dmx_default_ctx())) return DMX_ERR_DEVICE;
    if ((!in && n) || !out_len || (!out && cap)) return DMX_ERR_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (c->subs.size() > 1 && n >= 2 * c->subs.size() * (size_t)c->seg)
        return deflate_multi(c, in, n, level, out, cap, out_len);
    DeviceGuard dg(c->device);
    if (!dg.ok) return DMX_ERR_DEVICE;
    size_t total = 0;
    const int rc = deflate_host(c, in, n, level, &total);
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

// the decoded bytes (c->stream's work) into a malloc'd host buffer, which dmx_free releases
static int inflate_to_malloc(dmx_ctx* c, const uint8_t* dev, size_t tot, uint8_t** out, size_t* len) {
    uint8_t* h = static_cast<uint8_t*>(std::malloc(tot ? tot : 1));
    if (!h) return DMX_ERR_NOMEM;
    if ((tot && hipMemcpyAsync(h, dev, tot, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        std::free(h);
        return DMX_ERR_DEVICE;
    }
    *out = h;
    *len = tot;
    return DMX_OK;
}

int dmx_inflate(dmx_ctx* c, const uint8_t* in, size_t n, uint8_t* out, size_t cap,
                size_t* written, size_t* total) {
    if (!c && !(c = dmx_default_ctx())) return DMX_ERR_DEVICE;
    if ((!in && n) || (!out && cap) || !written) return DMX_ERR_ARG;
    DMX_ENTER(g, c);
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
    if (!c && !(c = dmx_default_ctx())) return DMX_ERR_DEVICE;
    if ((!in && n) || !out || !len) return DMX_ERR_ARG;
    DMX_ENTER(g, c);
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
    return inflate_to_malloc(c, dev, tot, out, len);
}

// ---- segment index for multi-GPU inflate ------------------------------------
int dmx_segment_starts_device(dmx_ctx* c, const void* d_in, size_t n, uint64_t* starts, size_t cap,
                              size_t* count, void* stream) {
    if (!c || (!d_in && n) || !count || (!starts && cap)) return DMX_ERR_ARG;
    DMX_ENTER(g, c, stream);
    const hipStream_t st = g.st;
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
    DMX_ENTER(g, c, stream);
    const hipStream_t st = g.st;
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
    DMX_ENTER(g, c, stream);
    return checksum_locked(c, false, (const uint8_t*)d, n, init, out, g.st);
}

int dmx_crc32_device(dmx_ctx* c, const void* d, size_t n, uint32_t init, uint32_t* out, void* stream) {
    if (!c || (!d && n) || !out) return DMX_ERR_ARG;
    DMX_ENTER(g, c, stream);
    return checksum_locked(c, true, (const uint8_t*)d, n, init, out, g.st);
}

static int checksum_host(dmx_ctx* c, bool crc, const uint8_t* in, size_t n, uint32_t init, uint32_t* out) {
    if (!c && !(c = dmx_default_ctx())) return DMX_ERR_DEVICE;
    if ((!in && n) || !out) return DMX_ERR_ARG;
    DMX_ENTER(g, c);
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

int dmx_deflate_zlib(dmx_ctx* c, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap,
                     size_t* out_len) {
    return deflate_framed(c, false, in, n, level, out, cap, out_len);
}

int dmx_deflate_gzip(dmx_ctx* c, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap,
                     size_t* out_len) {
    return deflate_framed(c, true, in, n, level, out, cap, out_len);
}

// Parses the container header, inflates the raw stream on the GPU and (DMX_VERIFY) checks the
// trailer against the GPU checksum of the decoded bytes.  The trailer is taken from the last
// 4 (zlib) / 8 (gzip) bytes of the input.
static int inflate_framed(dmx_ctx* c, bool gz, const uint8_t* in, size_t n, uint32_t flags, uint8_t** out,
                          size_t* len) {
    if (!c && !(c = dmx_default_ctx())) return DMX_ERR_DEVICE;
    if ((!in && n) || !out || !len) return DMX_ERR_ARG;
    *out = nullptr;
    *len = 0;
    // (container_parse.h: the parse the framed batch kernels run)
    const FrameHead fh = parse_frame(gz ? DMX_FRAME_GZIP : DMX_FRAME_ZLIB, in, n);
    if (fh.status != DMX_OK) return fh.status;
    const size_t head = (size_t)fh.head;
    DMX_ENTER(g, c);
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
    return inflate_to_malloc(c, dev, tot, out, len);
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
    if (!c && !(c = dmx_default_ctx())) return DMX_ERR_DEVICE;
    if (!in_path || !out_path) return DMX_ERR_ARG;
    File fi(in_path, "rb");
    if (!fi.f) return DMX_ERR_ARG;
    const int64_t N = file_size(fi.f);
    if (N < 0) return DMX_ERR_ARG;
    File fo(out_path, "wb");
    if (!fo.f) return DMX_ERR_ARG;
    DMX_ENTER(g, c);
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
    if (!c && !(c = dmx_default_ctx())) return DMX_ERR_DEVICE;
    if (!in_path || !out_path) return DMX_ERR_ARG;
    if (out_bytes) *out_bytes = 0;
    File fi(in_path, "rb");
    if (!fi.f) return DMX_ERR_ARG;
    const int64_t C = file_size(fi.f);
    if (C < 0) return DMX_ERR_ARG;
    DMX_ENTER(g, c);
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
