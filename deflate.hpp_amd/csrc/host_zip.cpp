// host_zip.cpp -- ZIP archives (see include/dmx.h): the directory read on the device
// (zip_dir.hip), the entries extracted by one batch inflate, one copy launch and one checksum
// launch, the entries above the batch calls' routing threshold by the single-stream plan.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "dmx_ctx.h"

using namespace dmx;

namespace {

// The directory of d_in[0, n), n >= 22, read on the device.  Scratch: c->bgzt (the head, the
// candidate scan's tile counts and offsets), c->bgzc (candidates, jump tables, the entry table and
// its scans) -- the BGZF device calls' buffers, which like these calls end synchronised and wait
// for c->ev_inf.  Three host synchronisations: the end record; the candidate count; the status, the
// plain bytes and, where `entries` holds h.count of them, the entries.
struct ZipIndex {
    ZipHead h{};                      // status: the archive's
    dmx_zip_entry* d_ents = nullptr;  // device: h.count entries, directory order
    bool copied = false;              // the entries were copied to the caller's array
};
int zip_index_locked(dmx_ctx* c, const uint8_t* in, size_t n, dmx_zip_entry* entries, size_t entry_cap, hipStream_t st,
                     ZipIndex* X) {
    // (a directory is shorter than the archive: the tile arrays are sized before its extent is known)
    ScanScratch S;
    if (!S.carve(c, scan_tiles(nullptr, n + 16), sizeof(ZipHead))) return DMX_ERR_NOMEM;
    ZipHead* const d_head = reinterpret_cast<ZipHead*>(S.words);
    HIPCHK(launch_zip_tail(in, n, d_head, st));
    ZipHead& h = X->h;
    HIPCHK(hipMemcpyAsync(&h, d_head, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h.status != DMX_OK) return DMX_OK;
    if (!h.dir_size) {  // no record: the count must say so
        if (h.count) h.status = DMX_ERR_DATA;
        return DMX_OK;
    }
    // (links are 32-bit candidate indices)
    const int rc = S.count(launch_zip_count(in, h, S.counts, S.offs, S.d_ncand, st), kBgzfNone, st);
    if (rc != DMX_OK) return rc;
    const uint64_t ncand = S.ncand;
    if (!ncand || h.count > ncand) {               // (a chain is no longer than the candidate list)
        h.status = DMX_ERR_DATA;
        return DMX_OK;
    }
    const uint32_t levels = bgzf_levels(ncand);
    const size_t cnt = (size_t)h.count;
    const size_t off_J = up16(ncand * sizeof(BgzfCand)), off_ents = off_J + up16((size_t)levels * ncand * 4);
    const size_t off_lo = off_ents + cnt * sizeof(dmx_zip_entry), off_hi = off_lo + up16(cnt * 4);
    const size_t off_slo = off_hi + up16(cnt * 4), off_shi = off_slo + scan_words(cnt) * 8;
    const size_t off_tot = off_shi + scan_words(cnt) * 8;
    if (!c->bgzc.ensure(off_tot + 16 + 64)) return DMX_ERR_NOMEM;
    uint8_t* const cb = c->bgzc.as<uint8_t>();
    X->d_ents = reinterpret_cast<dmx_zip_entry*>(cb + off_ents);
    ZipHead* const d_head2 = reinterpret_cast<ZipHead*>(cb + off_tot + 16);
    HIPCHK(launch_zip_chain(in, n, h, S.offs, ncand, reinterpret_cast<BgzfCand*>(cb),
                            reinterpret_cast<uint32_t*>(cb + off_J), X->d_ents, reinterpret_cast<uint32_t*>(cb + off_lo),
                            reinterpret_cast<uint32_t*>(cb + off_hi), reinterpret_cast<uint64_t*>(cb + off_slo),
                            reinterpret_cast<uint64_t*>(cb + off_shi), reinterpret_cast<uint64_t*>(cb + off_tot),
                            d_head2, st));
    HIPCHK(hipMemcpyAsync(&h, d_head2, sizeof(h), hipMemcpyDeviceToHost, st));
    if (entries && entry_cap >= cnt) {  // (read only where the status is DMX_OK)
        HIPCHK(hipMemcpyAsync(entries, X->d_ents, cnt * sizeof(dmx_zip_entry), hipMemcpyDeviceToHost, st));
        X->copied = true;
    }
    HIPCHK(hipStreamSynchronize(st));
    return DMX_OK;
}

// The extraction's scratch for `count` entries at `base` (16-byte aligned; null: for `bytes` alone):
//   entries (an uploaded selection) | desc | results | side | kind | order | class work | tickets
struct ZipTab {
    dmx_zip_entry* ents;
    InflateBatchDesc* desc;
    dmx_batch_result* res;
    FrameHead* side;
    uint32_t *kind, *order, *work;
    unsigned int* ticket;
    size_t bytes;
};
ZipTab zip_tab(uint8_t* base, size_t count) {
    const size_t off_desc = count * sizeof(dmx_zip_entry), off_res = off_desc + count * sizeof(InflateBatchDesc);
    const size_t off_side = off_res + count * sizeof(dmx_batch_result), off_kind = off_side + count * sizeof(FrameHead);
    const size_t off_order = off_kind + up16(count * 4), off_work = off_order + up16(count * 4);
    const size_t off_ticket = off_work + 2 * kBatchClasses * 4;
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    return ZipTab{reinterpret_cast<dmx_zip_entry*>(b),
                  reinterpret_cast<InflateBatchDesc*>(b + off_desc),
                  reinterpret_cast<dmx_batch_result*>(b + off_res),
                  reinterpret_cast<FrameHead*>(b + off_side),
                  reinterpret_cast<uint32_t*>(b + off_kind),
                  reinterpret_cast<uint32_t*>(b + off_order),
                  reinterpret_cast<uint32_t*>(b + off_work),
                  reinterpret_cast<unsigned int*>(b + off_ticket),
                  off_ticket + 32};
}

// Extracts ents[0, count), count > 0: h_ents on the host and the same table on the device (d_ents;
// null: h_ents is uploaded), uoffset = each entry's slot in out, which the caller has checked to
// lie inside the output.  res: `count` results on the host.  One host synchronisation, the
// read-back of res; the entries above kBatchRouteBytes follow, one after another.
int zip_extract_locked(dmx_ctx* c, const uint8_t* in, size_t n, const dmx_zip_entry* h_ents,
                       const dmx_zip_entry* d_ents, size_t count, bool verify, uint8_t* out, dmx_batch_result* res,
                       hipStream_t st) {
    if (count >= (size_t)DF_BATCH_LAST) return DMX_ERR_NOMEM;  // (as dmx_inflate_bgzf_device)
    size_t nbatch = 0, ncopy = 0;
    std::vector<uint32_t> big;
    for (size_t k = 0; k < count; k++) {  // the kernels' own rule: host and device agree on every entry
        int st_k;
        const uint32_t job = zip_job(h_ents[k], n, kBatchRouteBytes, &st_k);
        nbatch += job == ZIP_JOB_BATCH;
        ncopy += job == ZIP_JOB_COPY;
        if (job >= ZIP_JOB_INFLATE) big.push_back((uint32_t)k);
    }
    if (!c->bgzd.ensure(zip_tab(nullptr, count).bytes)) return DMX_ERR_NOMEM;
    const ZipTab T = zip_tab(c->bgzd.as<uint8_t>(), count);
    if (!d_ents) {
        HIPCHK(hipMemcpyAsync(T.ents, h_ents, count * sizeof(dmx_zip_entry), hipMemcpyHostToDevice, st));
        d_ents = T.ents;
    }
    HIPCHK(launch_zip_jobs(d_ents, count, in, n, out, kBatchRouteBytes, T.desc, T.res, T.side, T.kind, T.order, T.work,
                           st));
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    if (nbatch) HIPCHK(launch_inflate_batch(T.desc, T.order, nbatch, T.res, T.ticket, c->flags, st));
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    if (ncopy) HIPCHK(launch_zip_copy(T.desc, T.kind, count, T.res, st));
    if (verify && nbatch + ncopy) HIPCHK(launch_checksum_batch(T.desc, T.res, T.side, count, true, T.ticket + 4, st));
    HIPCHK(launch_zip_verdict(d_ents, T.kind, T.side, count, verify, T.res, st));
    HIPCHK(hipEventRecord(c->ev_inf, st));
    c->inf_pending = true;
    HIPCHK(hipMemcpyAsync(res, T.res, count * sizeof(dmx_batch_result), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    end_timing(c, st);
    const dmx_stats batch_stats = c->stats;
    bool unsynced = false;
    for (const uint32_t k : big) {  // (each decode synchronises on its own)
        const dmx_zip_entry& e = h_ents[k];
        uint8_t* const dst = out + e.uoffset;
        size_t len = 0;
        uint32_t path = 0;
        int rc = DMX_OK;
        if (e.method == 8) {
            rc = inflate_device_locked(c, in + e.data_off, (size_t)e.csize, dst, (size_t)e.usize, &len, nullptr, st);
            if (rc == DMX_ERR_NOMEM || rc == DMX_ERR_DEVICE || rc == DMX_ERR_INTERNAL) return rc;
            path = c->stats.path;
        } else {
            HIPCHK(hipMemcpyAsync(dst, in + e.data_off, (size_t)e.csize, hipMemcpyDeviceToDevice, st));
            len = (size_t)e.csize;
            unsynced = true;
        }
        uint32_t ck = 0;
        if (verify && rc == DMX_OK && len == e.usize) {
            const int rk = checksum_locked(c, true, dst, len, 0u, &ck, st);
            if (rk != DMX_OK) return rk;
            unsynced = false;
        }
        res[k] = dmx_batch_result{len, zip_verdict(rc, len, e, verify, ck), path};
    }
    if (!big.empty()) {
        HIPCHK(hipEventRecord(c->ev_inf, st));
        if (unsynced) HIPCHK(hipStreamSynchronize(st));
    }
    c->stats = batch_stats;
    c->stats.segments = count;
    c->stats.in_bytes = n;
    c->stats.path = 6;
    for (size_t k = 0; k < count; k++)
        if (res[k].status == DMX_OK) c->stats.out_bytes += res[k].bytes;
    return DMX_OK;
}

int zip_index_call(dmx_ctx* c, const uint8_t* in, size_t n, dmx_zip_entry* entries, size_t entry_cap, size_t* count,
                   uint64_t* plain_bytes, hipStream_t st) {
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    begin_timing(c, st);
    if (c->timing) (void)hipEventRecord(c->ev[1], st);
    ZipIndex X;
    const int rc = zip_index_locked(c, in, n, entries, entry_cap, st, &X);
    if (rc != DMX_OK) return rc;
    if (c->timing) (void)hipEventRecord(c->ev[2], st);
    HIPCHK(hipEventRecord(c->ev_inf, st));
    c->inf_pending = true;
    end_timing(c, st);
    c->stats.in_bytes = n;
    if (X.h.status != DMX_OK) return X.h.status;
    c->stats.segments = X.h.count;
    if (count) *count = (size_t)X.h.count;
    if (plain_bytes) *plain_bytes = X.h.total;
    if (entries && !X.copied && X.h.count) return DMX_ERR_CAPACITY;
    return DMX_OK;
}

int zip_inflate_call(dmx_ctx* c, const uint8_t* in, size_t n, bool verify, uint8_t* out, size_t cap,
                     dmx_zip_entry* entries, size_t entry_cap, size_t* count, size_t* out_len, hipStream_t st) try {
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(st, c->ev_inf, 0));
    begin_timing(c, st);
    ZipIndex X;
    const int rc = zip_index_locked(c, in, n, entries, entry_cap, st, &X);
    if (rc != DMX_OK) return rc;
    HIPCHK(hipEventRecord(c->ev_inf, st));
    c->inf_pending = true;
    c->stats.in_bytes = n;
    if (X.h.status != DMX_OK) return X.h.status;
    const size_t cnt = (size_t)X.h.count;
    if (count) *count = cnt;
    if (cnt && !X.copied) return DMX_ERR_CAPACITY;
    if (X.h.total > cap) {  // before any entry is decoded
        *out_len = (size_t)X.h.total;
        return DMX_ERR_CAPACITY;
    }
    *out_len = (size_t)X.h.total;
    if (!cnt) {
        end_timing(c, st);
        return DMX_OK;
    }
    std::vector<dmx_batch_result> res(cnt);
    const int re = zip_extract_locked(c, in, n, entries, X.d_ents, cnt, verify, out, res.data(), st);
    if (re != DMX_OK) {
        *out_len = 0;
        return re;
    }
    for (size_t k = 0; k < cnt; k++) {
        entries[k].status = res[k].status;
        entries[k].path = res[k].path;
    }
    return DMX_OK;
} catch (const std::bad_alloc&) {
    return DMX_ERR_NOMEM;
}

}  // namespace

extern "C" {

int dmx_zip_index_device(dmx_ctx* c, const void* d_in, size_t n, dmx_zip_entry* entries, size_t entry_cap,
                         size_t* count, uint64_t* plain_bytes, void* stream) {
    if (!c || (!d_in && n)) return DMX_ERR_ARG;
    if (count) *count = 0;
    if (plain_bytes) *plain_bytes = 0;
    if (n < 22) return DMX_ERR_DATA;  // no room for an end record
    DMX_ENTER(g, c, stream);
    return zip_index_call(c, static_cast<const uint8_t*>(d_in), n, entries, entry_cap, count, plain_bytes, g.st);
}

int dmx_zip_extract_device(dmx_ctx* c, const void* d_in, size_t n, const dmx_zip_entry* entries, size_t count,
                           const size_t* sel, size_t nsel, uint32_t flags, void* d_out, size_t cap,
                           dmx_batch_result* res, size_t* out_len, void* stream) try {
    if (!c || (!d_in && n) || !out_len || (!d_out && cap) || (flags & ~DMX_VERIFY)) return DMX_ERR_ARG;
    *out_len = 0;
    if (!sel) nsel = count;
    if (nsel && (!entries || !res)) return DMX_ERR_ARG;
    // the selection with its layout: uoffset becomes the entry's slot
    std::vector<dmx_zip_entry> picked(nsel);
    uint64_t total = 0;
    for (size_t i = 0; i < nsel; i++) {
        const size_t k = sel ? sel[i] : i;
        if (k >= count) return DMX_ERR_ARG;
        picked[i] = entries[k];
        picked[i].uoffset = total;
        if (picked[i].usize > (1ull << 63) - total) return DMX_ERR_DATA;
        total += picked[i].usize;
    }
    *out_len = (size_t)total;
    if (total > cap) return DMX_ERR_CAPACITY;  // before any entry is decoded
    if (!nsel) return DMX_OK;
    DMX_ENTER(g, c, stream);
    if (c->inf_pending) HIPCHK(hipStreamWaitEvent(g.st, c->ev_inf, 0));
    begin_timing(c, g.st);
    const int rc = zip_extract_locked(c, static_cast<const uint8_t*>(d_in), n, picked.data(), nullptr, nsel,
                                      (flags & DMX_VERIFY) != 0, static_cast<uint8_t*>(d_out), res, g.st);
    if (rc != DMX_OK) *out_len = 0;
    return rc;
} catch (const std::bad_alloc&) {
    return DMX_ERR_NOMEM;
}

int dmx_inflate_zip_device(dmx_ctx* c, const void* d_in, size_t n, uint32_t flags, void* d_out, size_t cap,
                           dmx_zip_entry* entries, size_t entry_cap, size_t* count, size_t* out_len, void* stream) {
    if (!c || (!d_in && n) || !out_len || (!d_out && cap) || (!entries && entry_cap) || (flags & ~DMX_VERIFY))
        return DMX_ERR_ARG;
    *out_len = 0;
    if (count) *count = 0;
    if (n < 22) return DMX_ERR_DATA;
    DMX_ENTER(g, c, stream);
    return zip_inflate_call(c, static_cast<const uint8_t*>(d_in), n, (flags & DMX_VERIFY) != 0,
                            static_cast<uint8_t*>(d_out), cap, entries, entry_cap, count, out_len, g.st);
}

// ---- host buffers: the archive staged in context scratch (nothing else in these calls uses it) ----
int dmx_zip_index(dmx_ctx* c, const uint8_t* in, size_t n, dmx_zip_entry* entries, size_t entry_cap, size_t* count,
                  uint64_t* plain_bytes) {
    if (!c || (!in && n)) return DMX_ERR_ARG;
    if (count) *count = 0;
    if (plain_bytes) *plain_bytes = 0;
    if (n < 22) return DMX_ERR_DATA;
    DMX_ENTER(g, c);
    if (!c->bgzs.ensure(n + 16)) return DMX_ERR_NOMEM;
    HIPCHK(hipMemcpyAsync(c->bgzs.p, in, n, hipMemcpyHostToDevice, c->stream));
    return zip_index_call(c, c->bgzs.as<uint8_t>(), n, entries, entry_cap, count, plain_bytes, c->stream);
}

int dmx_inflate_zip(dmx_ctx* c, const uint8_t* in, size_t n, uint32_t flags, uint8_t* out, size_t cap,
                    dmx_zip_entry* entries, size_t entry_cap, size_t* count, size_t* out_len) {
    if (!c || (!in && n) || !out_len || (!out && cap) || (!entries && entry_cap) || (flags & ~DMX_VERIFY))
        return DMX_ERR_ARG;
    *out_len = 0;
    if (count) *count = 0;
    if (n < 22) return DMX_ERR_DATA;
    DMX_ENTER(g, c);
    const size_t off_out = up16(n + 16);
    if (!c->bgzs.ensure(off_out + cap + 16)) return DMX_ERR_NOMEM;
    uint8_t* const d_in = c->bgzs.as<uint8_t>();
    uint8_t* const d_out = cap ? d_in + off_out : nullptr;
    HIPCHK(hipMemcpyAsync(d_in, in, n, hipMemcpyHostToDevice, c->stream));
    const int rc = zip_inflate_call(c, d_in, n, (flags & DMX_VERIFY) != 0, d_out, cap, entries, entry_cap, count,
                                    out_len, c->stream);
    if (rc != DMX_OK || !*out_len) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out, *out_len, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return DMX_OK;
}

}  // extern "C"
