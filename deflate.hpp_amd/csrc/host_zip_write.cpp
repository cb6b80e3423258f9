// host_zip_write.cpp -- writing ZIP archives (see include/dmx.h): the method 8 entries compressed
// by one batch deflate into context scratch slots, the CRC-32 of every plain input by one checksum
// launch, then the layout and the pack launch of zip_write.hip, which moves every payload byte to
// its final place and writes the records.  The format and the steps: zip_write.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "dmx_ctx.h"

using namespace dmx;

namespace {

// the payload bound of one entry: what the batch deflate may write, or the plain bytes
size_t payload_bound(const dmx_zip_source& s) { return s.method == 8 ? dmx_deflate_bound((size_t)s.n) : (size_t)s.n; }

// the argument errors of both forms, before any device work
bool zip_write_args_ok(const dmx_ctx* c, const dmx_zip_source* src, size_t count, uint32_t flags, const void* comment,
                       size_t comment_len, const void* out, size_t cap, const size_t* out_len) {
    if (!c || !out_len || (!src && count) || (!out && cap) || (flags & ~DMX_ZIP_FORCE64)) return false;
    if (comment_len > 65535 || (!comment && comment_len) || count >= (size_t)DF_BATCH_LAST) return false;
    for (size_t k = 0; k < count; k++) {
        if ((!src[k].data && src[k].n) || !src[k].name) return false;
        if (zipw_check_source(src[k].name_len, src[k].method) != DMX_OK) return false;
    }
    return has_batch_deflate(c);  // as every batch deflate call
}

// The work tables for `count` entries at `base` (16-byte aligned; null: for `bytes` alone):
//   csize | local_off | record halves | central bytes | three scans | totals | key | ticket |
//   side | head | rows        (head and rows adjoin: they come back in one copy)
struct ZipwTab {
    uint64_t *csize, *loff;
    uint32_t *lo, *hi, *cbytes;
    uint64_t *off_lo, *off_hi, *coff, *totals;
    unsigned long long* key;
    unsigned int* ticket;
    FrameHead* side;
    ZipwHead* head;
    dmx_zip_entry* rows;
    size_t bytes;
};
ZipwTab zipw_tab(uint8_t* base, size_t count) {
    const size_t off_loff = count * 8, off_lo = off_loff + count * 8, off_hi = off_lo + up16(count * 4);
    const size_t off_cb = off_hi + up16(count * 4), off_slo = off_cb + up16(count * 4);
    const size_t sw = up16((size_t)scan_words(count) * 8);
    const size_t off_shi = off_slo + sw, off_sc = off_shi + sw, off_tot = off_sc + sw;
    const size_t off_key = off_tot + 32, off_ticket = off_key + 16, off_side = off_ticket + 16;
    const size_t off_head = off_side + count * sizeof(FrameHead), off_rows = off_head + sizeof(ZipwHead);
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    return ZipwTab{reinterpret_cast<uint64_t*>(b),
                   reinterpret_cast<uint64_t*>(b + off_loff),
                   reinterpret_cast<uint32_t*>(b + off_lo),
                   reinterpret_cast<uint32_t*>(b + off_hi),
                   reinterpret_cast<uint32_t*>(b + off_cb),
                   reinterpret_cast<uint64_t*>(b + off_slo),
                   reinterpret_cast<uint64_t*>(b + off_shi),
                   reinterpret_cast<uint64_t*>(b + off_sc),
                   reinterpret_cast<uint64_t*>(b + off_tot),
                   reinterpret_cast<unsigned long long*>(b + off_key),
                   reinterpret_cast<unsigned int*>(b + off_ticket),
                   reinterpret_cast<FrameHead*>(b + off_side),
                   reinterpret_cast<ZipwHead*>(b + off_head),
                   reinterpret_cast<dmx_zip_entry*>(b + off_rows),
                   off_rows + count * sizeof(dmx_zip_entry)};
}

// The archive of src[0, count) (data: DEVICE pointers) into d_out; the arguments are checked.
// Scratch: c->bgzs (the deflate slots), c->bgzd (the upload image), c->bgzc (the work tables) --
// the BGZF device calls' buffers, which like this call end synchronised.  Host synchronisations:
// the batch deflate's read-back (none without a method 8 entry) and one more, the read-back of
// the head and the written table.  count == 0: one, behind the copy of the end record.
int zip_write_locked(dmx_ctx* c, const dmx_zip_source* src, size_t count, int level, bool force64,
                     const uint8_t* comment, size_t comment_len, uint8_t* d_out, size_t cap, dmx_zip_entry* entries,
                     size_t* out_len, hipStream_t st) try {
    if (!count) {  // the end record and the comment alone
        uint8_t end[kZip64Bytes + 22];
        const size_t rec = zipw_write_end(end, 0, 0, 0, nullptr, (uint32_t)comment_len, force64);
        *out_len = rec + comment_len;
        if (*out_len > cap) return DMX_ERR_CAPACITY;
        if (c->df_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_df, 0));
        HIPCHK(hipMemcpyAsync(d_out, end, rec, hipMemcpyHostToDevice, st));
        if (comment_len) HIPCHK(hipMemcpyAsync(d_out + rec, comment, comment_len, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        return DMX_OK;
    }
    // the upload image: sources | descriptors | chunk-bound prefix sums | name blob | comment
    size_t names = 0, slots = 0, ndef = 0;
    for (size_t k = 0; k < count; k++) {
        names += src[k].name_len;
        if (src[k].method == 8) {
            slots += up16(payload_bound(src[k]));
            ndef++;
        }
    }
    const size_t off_desc = count * sizeof(ZipwSrc), off_first = off_desc + count * sizeof(InflateBatchDesc);
    const size_t off_names = off_first + (count + 1) * 8, off_comment = off_names + up16(names);
    const size_t image_bytes = off_comment + up16(comment_len);
    std::vector<uint64_t> image((image_bytes + 7) / 8);
    std::vector<const uint8_t*> dins(ndef);
    std::vector<uint8_t*> douts(ndef);
    std::vector<size_t> dns(ndef), dcaps(ndef);
    std::vector<dmx_batch_result> dres(ndef);
    if (!c->bgzs.ensure(slots + 16) || !c->bgzd.ensure(image_bytes + 16) || !c->bgzc.ensure(zipw_tab(nullptr, count).bytes))
        return DMX_ERR_NOMEM;
    static_assert(sizeof(InflateBatchDesc) == 32, "the upload image is built from 8-byte words");
    uint8_t* const img = reinterpret_cast<uint8_t*>(image.data());
    ZipwSrc* const hs = reinterpret_cast<ZipwSrc*>(img);
    InflateBatchDesc* const hd = reinterpret_cast<InflateBatchDesc*>(img + off_desc);
    uint64_t* const first = reinterpret_cast<uint64_t*>(img + off_first);
    uint64_t uoff = 0, chunks = 0;
    size_t at_name = 0, at_slot = 0, j = 0;
    for (size_t k = 0; k < count; k++) {
        const dmx_zip_source& s = src[k];
        const uint8_t* const name = reinterpret_cast<const uint8_t*>(s.name);
        const size_t bound = payload_bound(s);
        uint8_t* payload = const_cast<uint8_t*>(static_cast<const uint8_t*>(s.data));
        hs[k] = ZipwSrc{at_name, uoff, s.dostime ? s.dostime : kZipwDosTime, (uint32_t)j, (uint16_t)s.name_len,
                        s.method, (uint16_t)zipw_flags(name, s.name_len), 0};
        if (s.method == 8) {
            payload = c->bgzs.as<uint8_t>() + at_slot;
            dins[j] = static_cast<const uint8_t*>(s.data);
            dns[j] = (size_t)s.n;
            douts[j] = payload;
            dcaps[j] = bound;
            at_slot += up16(bound);
            j++;
        }
        hd[k] = InflateBatchDesc{static_cast<const uint8_t*>(s.data), s.n, payload, bound};
        std::memcpy(img + off_names + at_name, name, s.name_len);
        at_name += s.name_len;
        first[k] = chunks;
        chunks += zipw_chunk_bound(bound, kZipwChunk);
        uoff += s.n;
    }
    first[count] = chunks;
    if (chunks >= 0x7FFFFFFFull) return DMX_ERR_ARG;  // (the pack's grid: 128 TiB of payload)
    if (comment_len) std::memcpy(img + off_comment, comment, comment_len);

    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    if (c->df_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_df, 0));
    uint8_t* const dimg = c->bgzd.as<uint8_t>();
    HIPCHK(hipMemcpyAsync(dimg, img, image_bytes, hipMemcpyHostToDevice, st));
    dmx_stats deflate_stats{};
    if (ndef) {
        const int rc = deflate_batch_locked(c, dins.data(), dns.data(), ndef, level, douts.data(), dcaps.data(),
                                            dres.data(), st);
        if (rc != DMX_OK) return rc;
        deflate_stats = c->stats;
    }
    // CRC, layout and pack; the deflate's results are still in c->bres, where the batch left them
    begin_timing(c, st);
    const ZipwTab T = zipw_tab(c->bgzc.as<uint8_t>(), count);
    const ZipwSrc* const d_src = reinterpret_cast<const ZipwSrc*>(dimg);
    const InflateBatchDesc* const d_desc = reinterpret_cast<const InflateBatchDesc*>(dimg + off_desc);
    HIPCHK(hipMemsetAsync(T.key, 0xFF, 8, st));
    HIPCHK(launch_zipw_layout(d_src, d_desc, c->bres.as<dmx_batch_result>(), count, force64, T.csize, T.lo, T.hi,
                              T.off_lo, T.off_hi, T.loff, T.cbytes, T.coff, T.totals, T.key, st));
    HIPCHK(launch_checksum_batch(d_desc, nullptr, T.side, count, true, T.ticket, st));
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    HIPCHK(launch_zipw_pack(d_src, d_desc, T.side, dimg + off_names, dimg + off_comment, (uint32_t)comment_len,
                            reinterpret_cast<const uint64_t*>(dimg + off_first), count, chunks, T.csize, T.loff,
                            T.coff, T.totals, T.key, force64, d_out, cap, T.head, T.rows, st));
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    HIPCHK(hipEventRecord(c->ev_df, st));
    c->df_pending = true;
    // (the rows are read only where the status is DMX_OK)
    std::vector<uint64_t> back((sizeof(ZipwHead) + (entries ? count * sizeof(dmx_zip_entry) : 0)) / 8);
    HIPCHK(hipMemcpyAsync(back.data(), T.head, back.size() * 8, hipMemcpyDeviceToHost, st));
    mark_end(c, st);
    HIPCHK(hipStreamSynchronize(st));
    end_timing(c, st);
    ZipwHead h;
    std::memcpy(&h, back.data(), sizeof(h));
    // ms_main_kernel: the pack launch; ms_device_total: the batch deflate's plus CRC, layout and pack
    c->stats.ms_device_total += deflate_stats.ms_device_total;
    c->stats.segments = count;
    c->stats.in_bytes = uoff;
    c->stats.out_bytes = h.status == DMX_OK ? h.bytes : 0;
    if (h.status == DMX_OK || h.status == DMX_ERR_CAPACITY) *out_len = (size_t)h.bytes;
    if (h.status == DMX_OK && entries) std::memcpy(entries, back.data() + sizeof(ZipwHead) / 8, count * sizeof(dmx_zip_entry));
    return h.status;
} catch (const std::bad_alloc&) {
    return DMX_ERR_NOMEM;
}

}  // namespace

extern "C" {

size_t dmx_zip_bound(const dmx_zip_source* src, size_t count, size_t comment_len, uint32_t flags) {
    const bool force64 = (flags & DMX_ZIP_FORCE64) != 0;
    uint64_t local = 0, central = 0;
    for (size_t k = 0; k < count; k++) {
        const uint64_t bound = payload_bound(src[k]);
        central += zipw_central_bytes(src[k].name_len, src[k].n, bound, local, force64);
        local += zipw_local_bytes(src[k].name_len, src[k].n, bound, force64) + bound;
    }
    return (size_t)(local + central + zipw_end_bytes(count, central, local, comment_len, force64));
}

int dmx_zip_write_device(dmx_ctx* c, const dmx_zip_source* src, size_t count, int level, uint32_t flags,
                         const void* comment, size_t comment_len, void* d_out, size_t cap, dmx_zip_entry* entries,
                         size_t* out_len, void* stream) {
    if (!zip_write_args_ok(c, src, count, flags, comment, comment_len, d_out, cap, out_len)) return DMX_ERR_ARG;
    *out_len = 0;
    DMX_ENTER(g, c, stream);
    return zip_write_locked(c, src, count, level, (flags & DMX_ZIP_FORCE64) != 0, static_cast<const uint8_t*>(comment),
                            comment_len, static_cast<uint8_t*>(d_out), cap, entries, out_len, g.st);
}

// host buffers: the plain inputs staged in c->in with one copy, the archive built in c->out and
// copied back with one copy (nothing else in this call uses either)
int dmx_zip_write(dmx_ctx* c, const dmx_zip_source* src, size_t count, int level, uint32_t flags, const void* comment,
                  size_t comment_len, uint8_t* out, size_t cap, dmx_zip_entry* entries, size_t* out_len) try {
    if (!zip_write_args_ok(c, src, count, flags, comment, comment_len, out, cap, out_len)) return DMX_ERR_ARG;
    *out_len = 0;
    DMX_ENTER(g, c);
    const size_t dcap = std::min(cap, dmx_zip_bound(src, count, comment_len, flags));  // (no archive is longer)
    std::vector<dmx_zip_source> dsrc(src, src + count);
    size_t total = 0;
    for (size_t k = 0; k < count; k++) total += up16((size_t)src[k].n);
    std::vector<uint8_t> stage(total);
    if (!c->in.ensure(total + 16) || !c->out.ensure(dcap + 16)) return DMX_ERR_NOMEM;
    size_t at = 0;
    for (size_t k = 0; k < count; k++) {
        if (src[k].n) std::memcpy(stage.data() + at, src[k].data, (size_t)src[k].n);
        dsrc[k].data = c->in.as<uint8_t>() + at;
        at += up16((size_t)src[k].n);
    }
    if (total) HIPCHK(hipMemcpyAsync(c->in.p, stage.data(), total, hipMemcpyHostToDevice, c->stream));
    const int rc = zip_write_locked(c, dsrc.data(), count, level, (flags & DMX_ZIP_FORCE64) != 0,
                                    static_cast<const uint8_t*>(comment), comment_len, c->out.as<uint8_t>(), dcap,
                                    entries, out_len, c->stream);
    if (rc != DMX_OK || !*out_len) return rc;
    HIPCHK(hipMemcpyAsync(out, c->out.p, *out_len, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return DMX_OK;
} catch (const std::bad_alloc&) {
    return DMX_ERR_NOMEM;
}

}  // extern "C"
