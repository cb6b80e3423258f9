// host_batch.cpp -- the batch calls of libdmx (see include/dmx.h): many independent buffers per
// call, from host arrays (dmx_*_batch_device), from device-resident arrays (dmx_*_batch_async),
// from host buffers (dmx_*_batch), with preset dictionaries and with zlib / gzip / BGZF framing.
// dmx_ctx.h declares the drivers that host_members.cpp builds the BGZF files on.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "dmx_ctx.h"

using namespace dmx;

namespace dmx {

// one buffer of a batch: a null pointer only with nothing to read / no room to write
static bool buf_ok(const void* in, size_t n, const void* out, size_t cap) { return (in || !n) && (out || !cap); }

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
int deflate_batch_locked(dmx_ctx* c, const uint8_t* const* d_in, const size_t* n, size_t count, int level,
                         uint8_t* const* d_out, const size_t* cap, dmx_batch_result* res, hipStream_t st,
                         const uint8_t* d_dict, size_t dict_len, const FramePlan* fp) {
    if (level < 0 || level > 3) level = 1;  // as deflate_device_locked
    const uint32_t seg = c->seg;
    const uint32_t du = level >= 2 ? (uint32_t)std::min<size_t>(dict_len, kDeflateDictMax) : 0u;
    if (du && seg != 32768) return DMX_ERR_ARG;
    const uint8_t* const dtail = du ? d_dict + (dict_len - du) : nullptr;
    const size_t seg0 = seg - du;  // bytes of a buffer's first segment
    uint64_t nseg = 0;
    for (size_t i = 0; i < count; i++) {
        if (!buf_ok(d_in[i], n[i], d_out[i], cap[i])) return DMX_ERR_ARG;
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
    DeflateArgs A{};  // (no single stream: in, n, out, cap and dbg stay null)
    // results | (framed) the checksum kernel's ticket | one FrameHead per buffer
    const size_t res_bytes = count * sizeof(dmx_batch_result);
    if (!c->btab.ensure(bytes) || !c->bres.ensure(res_bytes + (fp ? 16 + count * sizeof(FrameHead) : 0)) ||
        (fp && !c->fdesc.ensure(count * sizeof(InflateBatchDesc))) || !deflate_scratch(c, A, nseg, nseg, level, seg))
        return DMX_ERR_NOMEM;
    HIPCHK(hipMemcpyAsync(c->btab.p, img, bytes, hipMemcpyHostToDevice, st));
    if (fp)
        HIPCHK(hipMemcpyAsync(c->fdesc.p, fp->hdesc, count * sizeof(InflateBatchDesc), hipMemcpyHostToDevice, st));
    uint8_t* const dimg = c->btab.as<uint8_t>();
    A.final_last = 1;
    A.total = c->offs.as<uint64_t>() + nseg;  // the scan's total follows the offsets (scan_words)
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
                         hipStream_t st, const uint8_t* d_dict, size_t dict_len, const FramePlan* fp) {
    std::vector<uint32_t> order, routed;
    std::vector<uint64_t> image, back;
    const size_t off_order = count * sizeof(InflateBatchDesc);
    const uint32_t dl = (uint32_t)std::min<size_t>(dict_len, kInflateDictMax);
    try {
        for (size_t i = 0; i < count; i++) {
            if (!buf_ok(d_in[i], n[i], d_out[i], cap[i])) return DMX_ERR_ARG;
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
    InflateBatchDesc* const d_desc = c->btab.as<InflateBatchDesc>();
    const uint32_t* const d_order = reinterpret_cast<const uint32_t*>(c->btab.as<uint8_t>() + off_order);
    dmx_batch_result* const d_res = c->bres.as<dmx_batch_result>();
    unsigned int* const d_ticket = reinterpret_cast<unsigned int*>(c->bres.as<uint8_t>() + res_bytes);
    FrameHead* const d_side = reinterpret_cast<FrameHead*>(c->bres.as<uint8_t>() + res_bytes + 32);
    if (fp) {
        // a routed stream's result is not written on the device: status -1 keeps it out of the
        // checksum launch, and the host fills it in below
        HIPCHK(hipMemsetAsync(d_res, 0xFF, res_bytes, st));
        HIPCHK(launch_frame_parse(d_desc, d_side, count, fp->format, st));
    }
    if (dl)
        HIPCHK(launch_inflate_batch_dict(d_desc, d_order, order.size(), d_res, d_ticket, c->flags,
                                         d_dict + (dict_len - dl), dl, st));
    else
        HIPCHK(launch_inflate_batch(d_desc, d_order, order.size(), d_res, d_ticket, c->flags, st));
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    if (fp) {
        if (fp->verify)
            HIPCHK(launch_checksum_batch(d_desc, d_res, d_side, count, fp->format != DMX_FRAME_ZLIB, d_ticket + 4, st));
        HIPCHK(launch_frame_verdict(d_side, d_res, count, fp->format, fp->verify, st));
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

// The batch deflate writes each raw stream behind its header's place, into the capacity less
// header and trailer (clamped at 0); a BGZF buffer above the block size is given nothing to do
// and k_frame_write reports it.
int deflate_batch_framed_locked(dmx_ctx* c, const uint8_t* const* d_in, const size_t* n, size_t count, int level,
                                uint32_t format, uint8_t* const* d_out, const size_t* cap, dmx_batch_result* res,
                                hipStream_t st) {
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
        if (!buf_ok(d_in[i], n[i], d_out[i], cap[i])) return DMX_ERR_ARG;
        const bool big = format == DMX_FRAME_BGZF && n[i] > kBgzfBlock;
        desc[i] = InflateBatchDesc{d_in[i], n[i], d_out[i], cap[i]};
        rn[i] = big ? 0 : n[i];
        rcap[i] = (big || cap[i] < frame) ? 0 : cap[i] - frame;
        rout[i] = rcap[i] ? d_out[i] + frame_head_bytes(format) : nullptr;
    }
    const FramePlan fp{format, level, false, desc.data()};
    return deflate_batch_locked(c, d_in, rn.data(), count, level, rout.data(), rcap.data(), res, st, nullptr, 0, &fp);
}

}  // namespace dmx

namespace {

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
    DeflateArgs A{};  // (no single stream: in, n, out, cap and dbg stay null)
    AsyncSegTab T;
    if (!async_deflate_scratch(c, A, T, count, cap, level)) return DMX_ERR_NOMEM;
    // the sizes past the device-side count stay zero: the scan runs over the capacity
    HIPCHK(hipMemsetAsync(A.sizes, 0, cap * 4, st));
    HIPCHK(launch_batch_segtab(d_in, d_n, count, max_n, cap, seg, du, du ? d_dict + (dict_len - du) : nullptr,
                               T.counts, T.bfirst, T.tab, T.flag, T.nseg, st));
    A.final_last = 1;
    A.total = c->offs.as<uint64_t>() + cap;  // the scan's total follows the offsets (scan_words)
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
    const size_t off_order = count * sizeof(InflateBatchDesc), off_work = off_order + up16(count * 4);
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

// (a context with n_gpus > 1 runs the batch on its own, i.e. its first, device)
// the arrays: host arrays of the synchronous calls, device arrays of the asynchronous ones
bool batch_args_ok(const dmx_ctx* c, const void* in, const void* n, size_t count, const void* out, const void* cap,
                   const void* res) {
    return c && count < (size_t)DF_BATCH_LAST && (count == 0 || (in && n && out && cap && res));
}

bool frame_format_ok(uint32_t format) { return frame_head_bytes(format) != 0; }

// Host buffers: the inputs are packed into one staging image at 16-byte aligned offsets and go up
// in one copy; the outputs come back in one copy of the packed output area and are handed out.
// ocap(i): the device bytes reserved for output i.  A preset dictionary (dict_len > 0) follows the
// inputs in the staging image and goes up in the same copy; run() gets its device address.
template <class OutCap, class Run>
int batch_host(dmx_ctx* c, const uint8_t* const* in, const size_t* n, size_t count, uint8_t* const* out,
               const size_t* cap, dmx_batch_result* res, const uint8_t* dict, size_t dict_len, OutCap ocap, Run run) {
    for (size_t i = 0; i < count; i++)
        if (!buf_ok(in[i], n[i], out[i], cap[i])) return DMX_ERR_ARG;
    DMX_ENTER(g, c);
    std::vector<size_t> ioff(count + 1), ooff(count + 1), dcap(count);
    std::vector<const uint8_t*> din(count);
    std::vector<uint8_t*> dout(count);
    std::vector<uint8_t> stage;
    size_t ti = 0, to = 0;
    for (size_t i = 0; i < count; i++) {
        ioff[i] = ti;
        ooff[i] = to;
        dcap[i] = ocap(i);
        ti += up16(n[i]);
        to += up16(dcap[i]);
    }
    const size_t doff = ti;
    ti += up16(dict_len);
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

}  // namespace

extern "C" {

// ---- batched API ---------------------------------------------------------------------------
// (the plain calls are the dictionary calls with dict_len == 0)
int dmx_deflate_batch_dict_device(dmx_ctx* c, const void* const* d_in, const size_t* n, size_t count, int level,
                                  const void* d_dict, size_t dict_len, void* const* d_out, const size_t* cap,
                                  dmx_batch_result* res, void* stream) {
    if (!batch_args_ok(c, d_in, n, count, d_out, cap, res) || (dict_len && !d_dict)) return DMX_ERR_ARG;
    if (!has_batch_deflate(c)) return DMX_ERR_ARG;
    if (dict_len && c->seg != 32768) return DMX_ERR_ARG;  // the 16 KiB image has no room for one
    if (count == 0) return DMX_OK;
    DMX_ENTER(g, c, stream);
    return deflate_batch_locked(c, reinterpret_cast<const uint8_t* const*>(d_in), n, count, level,
                                reinterpret_cast<uint8_t* const*>(d_out), cap, res, g.st,
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
    DMX_ENTER(g, c, stream);
    return inflate_batch_locked(c, reinterpret_cast<const uint8_t* const*>(d_in), n, count,
                                reinterpret_cast<uint8_t* const*>(d_out), cap, res, flags, g.st,
                                static_cast<const uint8_t*>(d_dict), dict_len);
}

int dmx_inflate_batch_device(dmx_ctx* c, const void* const* d_in, const size_t* n, size_t count,
                             void* const* d_out, const size_t* cap, dmx_batch_result* res, uint32_t flags,
                             void* stream) {
    return dmx_inflate_batch_dict_device(c, d_in, n, count, nullptr, 0, d_out, cap, res, flags, stream);
}

// ---- batches from device-resident descriptor arrays -------------------------------------------
int dmx_batch_reserve(dmx_ctx* c, size_t count, size_t max_n, size_t max_total, size_t dict_len) {
    if (!c || count >= (size_t)DF_BATCH_LAST) return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    DMX_ENTER(g, c);
    AsyncDescTab D;
    if (!async_inflate_scratch(c, D, count)) return DMX_ERR_NOMEM;
    if (!has_batch_deflate(c)) return DMX_OK;  // no deflate side on 64 KiB contexts
    // the deflate side at its largest: level 3's token words; a dictionary only where one is taken
    const uint32_t du = c->seg == 32768 ? (uint32_t)std::min<size_t>(dict_len, kDeflateDictMax) : 0u;
    uint64_t cap = 0;
    if (const int rc = async_deflate_capacity(c, count, max_n, max_total, du, &cap); rc != DMX_OK) return rc;
    if (du) {  // (levels 0-1 ignore the dictionary: their capacity may be the larger one)
        uint64_t cap0 = 0;
        if (const int rc = async_deflate_capacity(c, count, max_n, max_total, 0, &cap0); rc != DMX_OK) return rc;
        cap = std::max(cap, cap0);
    }
    DeflateArgs A{};  // (no single stream: in, n, out, cap and dbg stay null)
    AsyncSegTab T;
    return async_deflate_scratch(c, A, T, count, cap, 3) ? DMX_OK : DMX_ERR_NOMEM;
}

int dmx_deflate_batch_async(dmx_ctx* c, const void* const* d_in, const uint64_t* d_n, size_t count, size_t max_n,
                            size_t max_total, int level, const void* d_dict, size_t dict_len, void* const* d_out,
                            const uint64_t* d_cap, dmx_batch_result* d_res, void* stream) {
    if (!batch_args_ok(c, d_in, d_n, count, d_out, d_cap, d_res) || (dict_len && !d_dict)) return DMX_ERR_ARG;
    if (!has_batch_deflate(c)) return DMX_ERR_ARG;
    if (dict_len && c->seg != 32768 && level >= 2 && level <= 3) return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    DMX_ENTER(g, c, stream);
    return deflate_batch_async_locked(c, reinterpret_cast<const uint8_t* const*>(d_in), d_n, count, max_n, max_total,
                                      level, static_cast<const uint8_t*>(d_dict), dict_len,
                                      reinterpret_cast<uint8_t* const*>(d_out), d_cap, d_res, g.st);
}

int dmx_inflate_batch_async(dmx_ctx* c, const void* const* d_in, const uint64_t* d_n, size_t count, size_t max_n,
                            const void* d_dict, size_t dict_len, void* const* d_out, const uint64_t* d_cap,
                            dmx_batch_result* d_res, uint32_t flags, void* stream) {
    if (!batch_args_ok(c, d_in, d_n, count, d_out, d_cap, d_res) || (flags & ~DMX_BATCH_NO_ROUTE) ||
        (dict_len && !d_dict))
        return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    DMX_ENTER(g, c, stream);
    return inflate_batch_async_locked(c, reinterpret_cast<const uint8_t* const*>(d_in), d_n, count, max_n,
                                      static_cast<const uint8_t*>(d_dict), dict_len,
                                      reinterpret_cast<uint8_t* const*>(d_out), d_cap, d_res, flags, g.st);
}

// ---- host buffers (batch_host) -------------------------------------------------------------------
int dmx_deflate_batch_dict(dmx_ctx* c, const uint8_t* const* in, const size_t* n, size_t count, int level,
                           const uint8_t* dict, size_t dict_len, uint8_t* const* out, const size_t* cap,
                           dmx_batch_result* res) {
    if (!batch_args_ok(c, in, n, count, out, cap, res) || (dict_len && !dict)) return DMX_ERR_ARG;
    if (!has_batch_deflate(c)) return DMX_ERR_ARG;
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

int dmx_deflate_batch_framed_device(dmx_ctx* c, const void* const* d_in, const size_t* n, size_t count, int level,
                                    uint32_t format, void* const* d_out, const size_t* cap, dmx_batch_result* res,
                                    void* stream) {
    if (!batch_args_ok(c, d_in, n, count, d_out, cap, res) || !frame_format_ok(format)) return DMX_ERR_ARG;
    if (!has_batch_deflate(c)) return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    DMX_ENTER(g, c, stream);
    return deflate_batch_framed_locked(c, reinterpret_cast<const uint8_t* const*>(d_in), n, count, level, format,
                                       reinterpret_cast<uint8_t* const*>(d_out), cap, res, g.st);
}

int dmx_inflate_batch_framed_device(dmx_ctx* c, const void* const* d_in, const size_t* n, size_t count,
                                    uint32_t format, void* const* d_out, const size_t* cap, dmx_batch_result* res,
                                    uint32_t flags, void* stream) {
    if (!batch_args_ok(c, d_in, n, count, d_out, cap, res) || !frame_format_ok(format) ||
        (flags & ~(DMX_BATCH_NO_ROUTE | DMX_BATCH_VERIFY)))
        return DMX_ERR_ARG;
    if (count == 0) return DMX_OK;
    DMX_ENTER(g, c, stream);
    const FramePlan fp{format, 0, (flags & DMX_BATCH_VERIFY) != 0, nullptr};
    return inflate_batch_locked(c, reinterpret_cast<const uint8_t* const*>(d_in), n, count,
                                reinterpret_cast<uint8_t* const*>(d_out), cap, res, flags & DMX_BATCH_NO_ROUTE, g.st,
                                nullptr, 0, &fp);
}

int dmx_deflate_batch_framed(dmx_ctx* c, const uint8_t* const* in, const size_t* n, size_t count, int level,
                             uint32_t format, uint8_t* const* out, const size_t* cap, dmx_batch_result* res) {
    if (!batch_args_ok(c, in, n, count, out, cap, res) || !frame_format_ok(format)) return DMX_ERR_ARG;
    if (!has_batch_deflate(c)) return DMX_ERR_ARG;
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

}  // extern "C"
