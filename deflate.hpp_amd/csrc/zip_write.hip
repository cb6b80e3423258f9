// zip_write.hip -- ZIP archives written in device memory (gfx950): the entries' sizes behind the
// batch deflate, the layout, and one launch that moves every payload byte to its final place and
// writes the local headers, the central directory, the end records and the written table.
//
// The records and the steps are zip_write.h's (plain C++, run serially by
// tests/cpp/zip_write_test.cpp):
//   k_zipw_sizes               one thread per entry: csize from the batch deflate's result (method
//                              8) or the plain size (method 0), the halves of the local record's
//                              bytes for the two scans; a failed deflate folds k << 32 | status
//                              into the key (k_bgzf_sizes' rule)
//   launch_scan_u32 (twice)    local_off = the exclusive prefix sum of the local records
//   k_zipw_central             one thread per entry: local_off from the halves (k_zip_finish's
//                              join), the central record's bytes, which depend on it
//   launch_scan_u32            the central records' offsets in the directory
//   k_zipw_pack                workgroup w < first[count]: its entry by binary search over the
//                              host's chunk bounds, its chunk of the payload copied; chunk 0 of an
//                              entry also writes the local header (wave 0), the central record and
//                              the table's row (wave 1).  The last workgroup writes the end
//                              records, the comment and the head {archive bytes, status}.
// If any entry failed, or the archive does not fit cap, nothing is written to out (k_bgzf_pack's
// rule): the status is the first failing entry's, or DMX_ERR_CAPACITY with the size needed.
//
// The copy is k_zip_copy's, per chunk: 16-byte stores to the destination's aligned body, each
// from the two aligned 16-byte source lines that hold its bytes, shifted by the misalignment; byte
// heads and tails.  Interior chunks start 16-byte aligned in the destination, so only an entry's
// first and last chunk have a head or a tail.  Every store is a plain vector store.  No byte
// outside a payload's source [src, src + csize) is read but for the aligned loads that share
// their line with one of its bytes; no byte outside out[0, archive bytes) is written.
#include "zip_write.h"
#include "dmx_internal.h"

namespace dmx {

constexpr uint32_t ZW_NT = 256;

__global__ __launch_bounds__(ZW_NT) void k_zipw_sizes(const ZipwSrc* src, const InflateBatchDesc* desc,
                                                      const ::dmx_batch_result* res, uint64_t count, int force64,
                                                      uint64_t* csize, uint32_t* lo, uint32_t* hi,
                                                      unsigned long long* key) {
    const uint64_t k = (uint64_t)blockIdx.x * ZW_NT + threadIdx.x;
    if (k >= count) return;
    const ZipwSrc s = src[k];
    const uint64_t n = desc[k].n;
    uint64_t cs;
    const int st = zipw_csize(s, n, res, &cs);
    if (st != DMX_OK) atomicMin(key, (unsigned long long)((k << 32) | (uint32_t)st));
    const uint64_t rec = zipw_local_bytes(s.name_len, n, cs, force64 != 0) + cs;
    csize[k] = cs;
    lo[k] = (uint32_t)rec;
    hi[k] = (uint32_t)(rec >> 32);
}

__global__ __launch_bounds__(ZW_NT) void k_zipw_central(const ZipwSrc* src, const InflateBatchDesc* desc,
                                                        const uint64_t* csize, const uint64_t* off_lo,
                                                        const uint64_t* off_hi, uint64_t count, int force64,
                                                        uint64_t* loff, uint32_t* cbytes) {
    const uint64_t k = (uint64_t)blockIdx.x * ZW_NT + threadIdx.x;
    if (k >= count) return;
    const uint64_t off = off_lo[k] + (off_hi[k] << 32);
    loff[k] = off;
    cbytes[k] = zipw_central_bytes(src[k].name_len, desc[k].n, csize[k], off, force64 != 0);
}

// len bytes from src to dst, any alignment of either, by the whole workgroup
__device__ __forceinline__ void zw_copy(const uint8_t* src, uint8_t* dst, uint64_t len, uint32_t t) {
    const uint64_t to16 = (16 - ((uintptr_t)dst & 15)) & 15;
    const uint64_t lead = len < to16 ? len : to16;
    const uint64_t body = (len - lead) & ~15ull;
    if (t < lead) dst[t] = src[t];
    const uint32_t m = (uint32_t)((uintptr_t)(src + lead) & 15);
    if (m == 0) {
        for (uint64_t p = lead + 16ull * t; p < lead + body; p += 16 * ZW_NT)
            *reinterpret_cast<uint4*>(dst + p) = *reinterpret_cast<const uint4*>(src + p);
    } else {
        const uint8_t* const sa = src + lead - m;  // 16-byte aligned
        const uint32_t q = m >> 2, r = m & 3;
        for (uint64_t p = 16ull * t; p < body; p += 16 * ZW_NT) {
            const uint4 a = *reinterpret_cast<const uint4*>(sa + p);       // (holds byte lead + p)
            const uint4 b = *reinterpret_cast<const uint4*>(sa + p + 16);  // (holds byte lead + p + 16 - m < len)
            const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t o[4];
#define ZW_TAKE(Q)                                                                        \
    _Pragma("unroll") for (int j = 0; j < 4; j++) o[j] = __builtin_amdgcn_alignbyte(w[Q + j + 1], w[Q + j], r)
            if (q == 0) ZW_TAKE(0);
            else if (q == 1) ZW_TAKE(1);
            else if (q == 2) ZW_TAKE(2);
            else ZW_TAKE(3);
#undef ZW_TAKE
            *reinterpret_cast<uint4*>(dst + lead + p) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
    for (uint64_t p = lead + body + t; p < len; p += ZW_NT) dst[p] = src[p];
}

// desc[k] = {plain input, n, payload source, (unused)}; side[k].ck: the plain input's CRC-32;
// first: the prefix sum of the chunk bounds, nchunks = first[count]; totals: the three scans'.
__global__ __launch_bounds__(ZW_NT) void k_zipw_pack(const ZipwSrc* src, const InflateBatchDesc* desc,
                                                     const FrameHead* side, const uint8_t* names,
                                                     const uint8_t* comment, uint32_t comment_len,
                                                     const uint64_t* first, uint64_t count, uint64_t nchunks,
                                                     const uint64_t* csize, const uint64_t* loff, const uint64_t* coff,
                                                     const uint64_t* totals, const unsigned long long* key,
                                                     int force64, uint8_t* out, uint64_t cap, ZipwHead* head,
                                                     ::dmx_zip_entry* rows) {
    const uint32_t t = threadIdx.x;
    const uint64_t w = blockIdx.x;
    const bool f64 = force64 != 0;
    const ZipwHead h = zipw_layout(count, totals[0] + (totals[1] << 32), totals[2], comment_len, f64, *key, cap);
    if (w == nchunks && t == 0) *head = h;
    if (h.status != DMX_OK) return;
    if (w == nchunks) {
        uint8_t* const end = out + h.cd_off + h.cd_size;
        const uint32_t at = zipw_end_bytes(count, h.cd_size, h.cd_off, 0, f64);
        if (t == 0) (void)zipw_write_end(end, count, h.cd_size, h.cd_off, nullptr, comment_len, f64);
        for (uint32_t i = t; i < comment_len; i += ZW_NT) end[at + i] = comment[i];
        return;
    }
    const uint64_t k = zipw_find(first, count, w), j = w - first[k];
    const ZipwSrc s = src[k];
    const uint64_t n = desc[k].n, cs = csize[k], lo = loff[k];
    uint8_t* const dst = out + lo + zipw_local_bytes(s.name_len, n, cs, f64);
    if (j == 0 && (t == 0 || t == 64)) {
        ZipwEntry e;
        e.name = names + s.name_off;
        e.name_len = s.name_len;
        e.method = s.method;
        e.gpflags = s.gpflags;
        e.dostime = s.dostime;
        e.crc = side[k].ck;
        e.usize = n;
        e.csize = cs;
        if (t == 0) {
            (void)zipw_write_local(out + lo, e, f64);
        } else {
            const uint64_t central = h.cd_off + coff[k];
            (void)zipw_write_central(out + central, e, lo, f64);
            zipw_row(e, lo, central, s.uoffset, f64, &rows[k]);
        }
    }
    uint64_t b0, b1;
    if (!zipw_chunk(cs, (uint32_t)((uintptr_t)dst & 15), kZipwChunk, j, &b0, &b1)) return;
    zw_copy(desc[k].out + b0, dst + b0, b1 - b0, t);
}

// ---- launches -----------------------------------------------------------------------------------
static uint32_t zw_grid(uint64_t count) { return (uint32_t)((count + ZW_NT - 1) / ZW_NT); }

hipError_t launch_zipw_layout(const ZipwSrc* src, const InflateBatchDesc* desc, const ::dmx_batch_result* res,
                              uint64_t count, bool force64, uint64_t* csize, uint32_t* lo, uint32_t* hi,
                              uint64_t* off_lo, uint64_t* off_hi, uint64_t* loff, uint32_t* cbytes, uint64_t* coff,
                              uint64_t* totals, unsigned long long* key, hipStream_t st) {
    if (!count) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_zipw_sizes, dim3(zw_grid(count)), dim3(ZW_NT), 0, st, src, desc, res, count, force64 ? 1 : 0,
                       csize, lo, hi, key);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_scan_u32(lo, off_lo, count, totals, st);
    if (e != hipSuccess) return e;
    e = launch_scan_u32(hi, off_hi, count, totals + 1, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_zipw_central, dim3(zw_grid(count)), dim3(ZW_NT), 0, st, src, desc, csize, off_lo, off_hi,
                       count, force64 ? 1 : 0, loff, cbytes);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_u32(cbytes, coff, count, totals + 2, st);
}

hipError_t launch_zipw_pack(const ZipwSrc* src, const InflateBatchDesc* desc, const FrameHead* side,
                            const uint8_t* names, const uint8_t* comment, uint32_t comment_len, const uint64_t* first,
                            uint64_t count, uint64_t nchunks, const uint64_t* csize, const uint64_t* loff,
                            const uint64_t* coff, const uint64_t* totals, const unsigned long long* key, bool force64,
                            uint8_t* out, uint64_t cap, ZipwHead* head, ::dmx_zip_entry* rows, hipStream_t st) {
    if (!count || nchunks >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_zipw_pack, dim3((uint32_t)nchunks + 1), dim3(ZW_NT), 0, st, src, desc, side, names, comment,
                       comment_len, first, count, nchunks, csize, loff, coff, totals, key, force64 ? 1 : 0, out, cap,
                       head, rows);
    return hipGetLastError();
}

}  // namespace dmx
