// zip_dir.hip -- ZIP archives in device memory (gfx950): the end record found by one workgroup,
// the central directory walked in parallel, the entry table, and for the extraction the batch
// inflate's descriptors, the stored entries' copy and the per-entry verdict.
//
// The steps are zip_dir.h's (plain C++, run serially by tests/cpp/zip_dir_test.cpp); the chain is
// bgzf_chain.hip's sequence over central records instead of BGZF members:
//   k_zip_tail                  the highest valid end record position in the last 65557 bytes
//                               (one workgroup, an LDS maximum), then one thread reads the ZIP64
//                               records and writes the head
//   k_scan_count / k_scan_list  cand_scan.h's scan over ZipScan: every offset of the directory
//                               region that starts with 50 4b 01 02 is tested with zip_cd_candidate
//   launch_chain_links          bgzf_chain.hip's: successor = the candidate at off + size; level k
//                               -> level k + 1
//   k_zip_head                  one thread: the chain from the region's first byte must end at its
//                               end after as many records as the end record states
//   k_zip_entries               one thread per entry: rank lookup, the record's fields, the local
//                               header; the halves of usize for the two scans
//   launch_scan_u32 (twice)     uoffset = the exclusive prefix sum of usize
//   k_zip_finish                uoffset into the entries; the plain bytes (at most 2^63)
// and for an extraction over a table of entries whose uoffset is the entry's slot:
//   k_zip_jobs / k_zip_order    desc[k] = {in + data_off, csize, out + slot, usize}, the result of
//                               an entry that is not extracted, and the batch decoder's order list,
//                               longest class first (batch_table.h's classes)
//   k_zip_copy                  one workgroup per stored entry: 16-byte stores to the aligned
//                               body of the destination from two aligned loads of the source,
//                               byte heads and tails
//   k_zip_verdict               size and CRC-32 against the directory's (zip_verdict)
// False signatures inside names, extras and comments take part in the links and the doubling, but
// only what is reachable from the candidate at the directory's first byte is counted or ranked.
//
// Every store is a plain vector store.  No byte outside [in, in + n) is read but for the 16-byte
// aligned loads that share their line with a byte of the archive: the scan's staging (cand_scan.h)
// and k_zip_copy's source lines.
#include "zip_dir.h"
#include "cand_scan.h"

namespace dmx {

constexpr uint32_t ZD_NT = 256;
constexpr uint32_t ZD_TAIL_NT = 1024;

// ---- the end record -----------------------------------------------------------------------------
__global__ __launch_bounds__(ZD_TAIL_NT) void k_zip_tail(const uint8_t* in, uint64_t n, ZipHead* head) {
    __shared__ unsigned long long best;  // the highest valid position + 1
    const uint32_t t = threadIdx.x;
    if (t == 0) best = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (uint64_t p = zip_tail_start(n) + t; p + 22 <= n; p += ZD_TAIL_NT)
        if (in[p] == 0x50 && zip_eocd_at(in, n, p)) mine = p + 1;  // (positions rise: the last hit is the highest)
    if (mine) atomicMax(&best, mine);
    __syncthreads();
    if (t == 0) {
        ZipHead h{};
        h.status = best ? zip_read_end(in, n, best - 1, &h) : DMX_ERR_DATA;
        *head = h;
    }
}

// ---- the candidate scan over the directory region [d0, d1) and the chain -----------------------
// the scan's format (cand_scan.h): a central record that lies inside the region
struct ZipScan {
    const uint8_t* in;
    uint64_t d0, d1;
    using Cand = BgzfCand;
    static constexpr uint32_t kMinBytes = 46;
    __device__ bool magic(uint32_t word) const { return word == kZipSigCentral; }
    __device__ bool candidate(uint64_t off, BgzfCand* c) const { return zip_cd_candidate(in, d0, d1, d0 + off, c); }
};

__global__ void k_zip_head(const BgzfCand* cands, uint64_t ncand, const uint32_t* J, uint32_t levels, ZipHead h,
                           ZipHead* head) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t entries = 0;
    h.status = zip_chain_status(cands, ncand, J, levels, h, &entries);
    h.total = 0;
    *head = h;
}

// count = the end record's (<= ncand); behind a broken chain nothing is parsed
__global__ __launch_bounds__(ZD_NT) void k_zip_entries(const uint8_t* in, uint64_t n, uint64_t base, uint64_t count,
                                                       const BgzfCand* cands, uint64_t ncand, const uint32_t* J,
                                                       uint32_t levels, const ZipHead* head, ::dmx_zip_entry* ents,
                                                       uint32_t* lo, uint32_t* hi) {
    const uint64_t r = (uint64_t)blockIdx.x * ZD_NT + threadIdx.x;
    if (r >= count) return;
    if (head->status != DMX_OK) {
        lo[r] = 0;
        hi[r] = 0;
        return;
    }
    ::dmx_zip_entry e;
    zip_entry(in, n, base, cands[bgzf_rank_lookup(J, ncand, levels, r)], &e);
    ents[r] = e;
    lo[r] = (uint32_t)e.usize;
    hi[r] = (uint32_t)(e.usize >> 32);
}

__global__ __launch_bounds__(ZD_NT) void k_zip_finish(::dmx_zip_entry* ents, uint64_t count, const uint64_t* off_lo,
                                                      const uint64_t* off_hi, const uint64_t* totals, ZipHead* head) {
    const uint64_t r = (uint64_t)blockIdx.x * ZD_NT + threadIdx.x;
    if (head->status != DMX_OK) return;
    if (r < count) ents[r].uoffset = off_lo[r] + (off_hi[r] << 32);  // (wraps only where zip_total fails)
    if (r == 0) {
        uint64_t total = 0;
        if (zip_total(totals[0], totals[1], &total)) head->total = total;
        else head->status = DMX_ERR_DATA;
    }
}

// ---- extraction -----------------------------------------------------------------------------
// ents[k].uoffset is entry k's slot in out.  hist: kBatchClasses words, zero at the launch.
__global__ __launch_bounds__(ZD_NT) void k_zip_jobs(const ::dmx_zip_entry* ents, uint64_t count, const uint8_t* in,
                                                    uint64_t n, uint8_t* out, uint64_t route_bytes,
                                                    InflateBatchDesc* desc, ::dmx_batch_result* res, FrameHead* side,
                                                    uint32_t* kind, uint32_t* hist) {
    __shared__ uint32_t h[kBatchClasses];
    if (threadIdx.x < kBatchClasses) h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * ZD_NT + threadIdx.x;
    if (k < count) {
        const ::dmx_zip_entry e = ents[k];
        int st;
        const uint32_t job = zip_job(e, n, route_bytes, &st);
        InflateBatchDesc d;
        d.in = job == ZIP_JOB_NONE ? in : in + e.data_off;
        d.n = job == ZIP_JOB_NONE ? 0 : e.csize;
        d.out = out + e.uoffset;
        d.cap = job == ZIP_JOB_NONE ? 0 : e.usize;
        desc[k] = d;
        ::dmx_batch_result r;
        r.bytes = 0;
        // (a job of the host's is kept out of the checksum launch by a status that is not DMX_OK;
        // the decoder and the copy kernel write their entries' results)
        r.status = job == ZIP_JOB_NONE ? st : job >= ZIP_JOB_INFLATE ? DMX_BATCH_DEFERRED : DMX_ERR_INTERNAL;
        r.path = 0;
        res[k] = r;
        side[k] = FrameHead{};
        kind[k] = job;
        if (job == ZIP_JOB_BATCH) atomicAdd(&h[bt_class(d.n)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kBatchClasses && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// cursor: kBatchClasses words, zero at the launch (k_bt_order's scatter, over the job kinds)
__global__ __launch_bounds__(ZD_NT) void k_zip_order(const InflateBatchDesc* desc, const uint32_t* kind, uint64_t count,
                                                     const uint32_t* hist, uint32_t* cursor, uint32_t* order) {
    const uint64_t i = (uint64_t)blockIdx.x * ZD_NT + threadIdx.x;
    const bool keep = i < count && kind[i] == ZIP_JOB_BATCH;
    (void)bt_order_scatter(keep, keep ? bt_class(desc[i].n) : 0u, (uint32_t)i, hist, cursor, order);
}

// Workgroup k copies stored entry k: desc[k].n bytes from desc[k].in to desc[k].out, any alignment
// of either.  The destination's aligned body gets 16-byte stores; where the source is not aligned
// with it, each comes from the two aligned 16-byte lines that hold its bytes -- both share a byte
// with the entry -- shifted by the misalignment, which is the same for the whole entry.
__global__ __launch_bounds__(ZD_NT) void k_zip_copy(const InflateBatchDesc* desc, const uint32_t* kind,
                                                    ::dmx_batch_result* res) {
    const uint64_t k = blockIdx.x;
    if (kind[k] != ZIP_JOB_COPY) return;
    const InflateBatchDesc d = desc[k];
    const uint32_t t = threadIdx.x;
    const uint8_t* const src = d.in;
    uint8_t* const dst = d.out;
    const uint64_t len = d.n;
    const uint64_t to16 = (16 - ((uintptr_t)dst & 15)) & 15;
    const uint64_t lead = len < to16 ? len : to16;
    const uint64_t body = (len - lead) & ~15ull;
    if (t < lead) dst[t] = src[t];
    const uint32_t m = (uint32_t)((uintptr_t)(src + lead) & 15);
    if (m == 0) {
        for (uint64_t p = lead + 16ull * t; p < lead + body; p += 16 * ZD_NT)
            *reinterpret_cast<uint4*>(dst + p) = *reinterpret_cast<const uint4*>(src + p);
    } else {
        const uint8_t* const sa = src + lead - m;  // 16-byte aligned
        const uint32_t q = m >> 2, r = m & 3;
        for (uint64_t p = 16ull * t; p < body; p += 16 * ZD_NT) {
            const uint4 a = *reinterpret_cast<const uint4*>(sa + p);
            const uint4 b = *reinterpret_cast<const uint4*>(sa + p + 16);  // (holds byte lead + p + 16 - m < len)
            const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t o[4];
#define ZD_TAKE(Q)                                                                        \
    _Pragma("unroll") for (int j = 0; j < 4; j++) o[j] = __builtin_amdgcn_alignbyte(w[Q + j + 1], w[Q + j], r)
            if (q == 0) ZD_TAKE(0);
            else if (q == 1) ZD_TAKE(1);
            else if (q == 2) ZD_TAKE(2);
            else ZD_TAKE(3);
#undef ZD_TAKE
            *reinterpret_cast<uint4*>(dst + lead + p) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
    for (uint64_t p = lead + body + t; p < len; p += ZD_NT) dst[p] = src[p];
    if (t == 0) {
        ::dmx_batch_result r;
        r.bytes = len;
        r.status = DMX_OK;
        r.path = 0;
        res[k] = r;
    }
}

// side[k].ck: launch_checksum_batch's CRC-32 of the output (verify)
__global__ __launch_bounds__(ZD_NT) void k_zip_verdict(const ::dmx_zip_entry* ents, const uint32_t* kind,
                                                       const FrameHead* side, uint64_t count, int verify,
                                                       ::dmx_batch_result* res) {
    const uint64_t k = (uint64_t)blockIdx.x * ZD_NT + threadIdx.x;
    if (k >= count) return;
    const uint32_t job = kind[k];
    if (job != ZIP_JOB_BATCH && job != ZIP_JOB_COPY) return;
    res[k].status = zip_verdict(res[k].status, res[k].bytes, ents[k], verify != 0, side[k].ck);
}

// ---- launches -----------------------------------------------------------------------------------
static uint32_t zd_grid(uint64_t count) { return (uint32_t)((count + ZD_NT - 1) / ZD_NT); }

hipError_t launch_zip_tail(const uint8_t* in, uint64_t n, ZipHead* head, hipStream_t st) {
    hipLaunchKernelGGL(k_zip_tail, dim3(1), dim3(ZD_TAIL_NT), 0, st, in, n, head);
    return hipGetLastError();
}

hipError_t launch_zip_count(const uint8_t* in, const ZipHead& h, uint32_t* tile_counts, uint64_t* tile_offs,
                            uint64_t* ncand, hipStream_t st) {
    if (!h.dir_size) return hipErrorInvalidValue;
    return launch_scan_count(ZipScan{in, h.dir_off, h.dir_off + h.dir_size}, in + h.dir_off, h.dir_size, tile_counts,
                             tile_offs, ncand, st);
}

hipError_t launch_zip_chain(const uint8_t* in, uint64_t n, const ZipHead& h, const uint64_t* tile_offs, uint64_t ncand,
                            BgzfCand* cands, uint32_t* J, ::dmx_zip_entry* ents, uint32_t* lo, uint32_t* hi,
                            uint64_t* off_lo, uint64_t* off_hi, uint64_t* totals, ZipHead* head, hipStream_t st) {
    if (!ncand || h.count > ncand) return hipErrorInvalidValue;
    const uint64_t d1 = h.dir_off + h.dir_size;
    const uint32_t levels = bgzf_levels(ncand);
    hipError_t e = launch_scan_list(ZipScan{in, h.dir_off, d1}, in + h.dir_off, h.dir_size, tile_offs, cands, ncand, st);
    if (e != hipSuccess) return e;
    e = launch_chain_links(cands, ncand, d1, J, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_zip_head, dim3(1), dim3(64), 0, st, cands, ncand, J, levels, h, head);
    if (h.count)
        hipLaunchKernelGGL(k_zip_entries, dim3(zd_grid(h.count)), dim3(ZD_NT), 0, st, in, n, h.base, h.count, cands,
                           ncand, J, levels, head, ents, lo, hi);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (count == 0: the scans of nothing write the totals 0)
    e = launch_scan_u32(lo, off_lo, h.count, totals, st);
    if (e != hipSuccess) return e;
    e = launch_scan_u32(hi, off_hi, h.count, totals + 1, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_zip_finish, dim3(h.count ? zd_grid(h.count) : 1), dim3(ZD_NT), 0, st, ents, h.count, off_lo,
                       off_hi, totals, head);
    return hipGetLastError();
}

hipError_t launch_zip_jobs(const ::dmx_zip_entry* ents, uint64_t count, const uint8_t* in, uint64_t n, uint8_t* out,
                           uint64_t route_bytes, InflateBatchDesc* desc, ::dmx_batch_result* res, FrameHead* side,
                           uint32_t* kind, uint32_t* order, uint32_t* work, hipStream_t st) {
    if (!count) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(work, 0, 2 * kBatchClasses * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_zip_jobs, dim3(zd_grid(count)), dim3(ZD_NT), 0, st, ents, count, in, n, out, route_bytes, desc,
                       res, side, kind, work);
    hipLaunchKernelGGL(k_zip_order, dim3(zd_grid(count)), dim3(ZD_NT), 0, st, desc, kind, count, work,
                       work + kBatchClasses, order);
    return hipGetLastError();
}

hipError_t launch_zip_copy(const InflateBatchDesc* desc, const uint32_t* kind, uint64_t count,
                           ::dmx_batch_result* res, hipStream_t st) {
    hipLaunchKernelGGL(k_zip_copy, dim3((uint32_t)count), dim3(ZD_NT), 0, st, desc, kind, res);
    return hipGetLastError();
}

hipError_t launch_zip_verdict(const ::dmx_zip_entry* ents, const uint32_t* kind, const FrameHead* side, uint64_t count,
                              bool verify, ::dmx_batch_result* res, hipStream_t st) {
    hipLaunchKernelGGL(k_zip_verdict, dim3(zd_grid(count)), dim3(ZD_NT), 0, st, ents, kind, side, count,
                       verify ? 1 : 0, res);
    return hipGetLastError();
}

}  // namespace dmx
