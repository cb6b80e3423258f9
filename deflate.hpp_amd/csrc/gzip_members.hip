// gzip_members.hip -- multi-member gzip files in device memory (dmx_inflate_gzip_members_device,
// gfx950): where the members are, found without their extents being given.
//
// RFC 1952 2.2: a gzip file is a series of members.  Member k + 1 starts where member k's DEFLATE
// stream and trailer end, and nothing in a header says where that is -- only a decode does.  So:
//   k_scan_count / k_scan_list  cand_scan.h's scan over GzmScan: every offset p of the file is
//                               tested: 1f 8b 08 and a header that parses with 8 bytes left behind
//                               it (gzip_head_len, container_parse.h) is a CANDIDATE {p, header
//                               length}.
//   k_gzm_measure               one wavefront per candidate on a persistent grid: inflate_blocks
//                               over the candidate's stream with a sink that only counts, over a
//                               window of at most `limit` bytes -> GzmRec {end, plain bytes,
//                               status, cut}.  False candidates (the three bytes inside a payload,
//                               a .gz file inside a stored block) are measured like true ones;
//                               the host's walk (gzip_members.cpp) never looks at those that lie
//                               inside a member.
//   k_gzm_gaps / k_gzm_gap_status   the bytes between a trailer and the next member must be zeros:
//                               the least offset of a non-zero byte in a list of ranges, and the
//                               header status (gzip_head_len) at that offset.
// The decode itself is the framed batch inflate's (frame_batch.hip, inflate_batch.hip), over
// descriptors built from the walk.
//
// The measuring kernel keeps no output: no 32 KiB ring in LDS and no store to HBM but its record.
// Its LDS is the input ring and the code tables, about 8 KiB against the batch decoder's 40 KiB.
// It is a translation unit of its own (inflate_batch.hip:126-130: a second instantiation in one
// unit stops the decoder's helpers from being inlined).
//
// Every store is a plain vector store; there is no inline assembly.  No byte at or beyond in + n
// is read, but for the aligned loads that share their 4- or 16-byte line with a byte of the file
// (the scan's staging, cand_scan.h, and the batch decoder's input ring).
#include "inflate_common.h"
#include "cand_scan.h"

namespace dmx {

constexpr uint32_t GM_NT = 256;

// the candidate scan's format (cand_scan.h): 1f 8b 08 and a header that gzip_head_len accepts
struct GzmScan {
    const uint8_t* in;
    uint64_t n;
    using Cand = GzmCand;
    static constexpr uint32_t kMinBytes = 18;
    __device__ bool magic(uint32_t word) const { return (word & 0xFFFFFFu) == 0x088B1Fu; }
    __device__ bool candidate(uint64_t off, GzmCand* c) const {
        c->off = off;
        return gzip_head_len(in + off, n - off, &c->head) == DMX_OK;
    }
};

// ---- the measuring pass -------------------------------------------------------------------------
constexpr uint32_t GM_RW = 512, GM_RC = 128;  // input ring words, words per slide (the batch decoder's)
using MeasureIn = RingInT<GM_RW, GM_RC>;

// The sink interface of the batch decoder's BatchSink (full, literal, copy, stored, pos) with the
// position alone: what BatchSink would have counted, byte for byte.  A distance beyond the stream
// start copies nothing and counts nothing, as there (inflate_batch.hip, the reference's rule).
struct CountSink {
    uint64_t pos;
    uint32_t err;
    __device__ bool full() const { return false; }
    __device__ bool literal(uint32_t) {
        pos++;
        return true;
    }
    __device__ bool copy(uint32_t L, uint32_t dist) {
        if (L == 0 || dist == 0) return true;
        if (dist > pos) return true;
        pos += L;
        return true;
    }
    template <class BR>
    __device__ bool stored(const BR&, uint64_t, uint32_t len) {
        pos += len;
        return true;
    }
};

// Candidate k's stream is [off + head, n); the decode sees at most `limit` bytes of it.
__global__ __launch_bounds__(IF_NT) void k_gzm_measure(const uint8_t* in, uint64_t n, const GzmCand* cands,
                                                       uint64_t ncand, GzmRec* recs, unsigned int* ticket,
                                                       uint32_t flags, uint64_t limit) {
    __shared__ uint32_t inring[GM_RW];
    __shared__ Tables T;
    for (;;) {
        uint32_t k = 0;
        if (threadIdx.x == 0) k = atomicAdd(ticket, 1u);
        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        if (k >= ncand) break;
        const GzmCand c = cands[k];
        GzmRec r;
        r.end = 0;
        r.plain = 0;
        r.status = DMX_ERR_OVERREAD;
        r.cut = 0;
        r.pad_ = 0;
        const uint64_t s0 = c.off + c.head;
        if (s0 < n) {  // (a candidate has 8 bytes behind its header)
            const uint64_t avail = n - s0;
            const uint64_t win = avail < limit ? avail : limit;
            if (threadIdx.x == 0) T.fixed_loaded = 0;
            wave_sync();
            const uint8_t* const sp = in + s0;
            const uint64_t misalign = reinterpret_cast<uintptr_t>(sp) & 3;
            MeasureIn br;
            br.init(reinterpret_cast<const uint32_t*>(sp - misalign), misalign, win, inring);
            br.seek(misalign * 8);
            CountSink sk{0, 0};
            uint64_t end_byte = 0;
            bool fin = false;
            const uint32_t err = inflate_blocks(br, T, sk, (flags & DMX_CFG_RFC_STRICT) != 0, false, &end_byte, &fin);
            if (err == 0) {
                r.end = s0 + (end_byte - misalign);
                r.plain = sk.pos;
                r.status = DMX_OK;
            } else if (err & SEGF_OVERREAD) {
                r.cut = win < avail ? 1u : 0u;
            } else {
                r.status = DMX_ERR_DATA;
            }
        }
        if (threadIdx.x == 0) recs[k] = r;
        wave_sync();  // the next candidate reuses the ring and the tables
    }
}

// ---- the gap check ------------------------------------------------------------------------------
constexpr uint32_t GM_GAP_CHUNK = GM_NT * 64;  // bytes of a range one workgroup looks at per step

// *flag (preset to all ones) = the least file offset of a non-zero byte in the ranges; the ranges
// are in file order, so this is also the least index of a range that holds one.  blockIdx.x strides
// over the ranges, blockIdx.y over a range's chunks.
__global__ __launch_bounds__(GM_NT) void k_gzm_gaps(const uint8_t* in, uint64_t n, const GzmGap* gaps, uint64_t ngaps,
                                                    unsigned long long* flag) {
    for (uint64_t g = blockIdx.x; g < ngaps; g += gridDim.x) {
        const GzmGap r = gaps[g];
        const uint64_t b = r.b < n ? r.b : n;
        for (uint64_t c0 = r.a + (uint64_t)blockIdx.y * GM_GAP_CHUNK; c0 < b; c0 += (uint64_t)gridDim.y * GM_GAP_CHUNK) {
            const uint64_t c1 = c0 + GM_GAP_CHUNK < b ? c0 + GM_GAP_CHUNK : b;
            for (uint64_t q = c0 + threadIdx.x; q < c1; q += GM_NT) {
                if (in[q]) {  // (a thread's offsets rise: its first hit is its least)
                    atomicMin(flag, (unsigned long long)q);
                    break;
                }
            }
        }
    }
}

// res[0] = the offset (forced != all ones: `forced` itself, the header expected at the file's
// start), res[1] = the status of a header there; {all ones, DMX_OK} when every range is zeros
__global__ void k_gzm_gap_status(const uint8_t* in, uint64_t n, const unsigned long long* flag, uint64_t forced,
                                 uint64_t* res) {
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t q = forced != ~0ull ? forced : (uint64_t)*flag;
    int st = DMX_OK;
    if (q != ~0ull) {
        uint64_t head;
        st = q < n ? gzip_head_len(in + q, n - q, &head) : DMX_ERR_OVERREAD;
        if (st == DMX_OK) st = DMX_ERR_DATA;  // (a header that parses would have been a candidate)
    }
    res[0] = q;
    res[1] = (uint64_t)(int64_t)st;
}

// ---- launches -----------------------------------------------------------------------------------
uint32_t gzm_tile_bytes() { return kScanTile; }

hipError_t launch_gzm_count(const uint8_t* in, uint64_t n, uint32_t* tile_counts, uint64_t* tile_offs,
                            uint64_t* ncand, hipStream_t st) {
    return launch_scan_count(GzmScan{in, n}, in, n, tile_counts, tile_offs, ncand, st);
}

hipError_t launch_gzm_write(const uint8_t* in, uint64_t n, const uint64_t* tile_offs, GzmCand* cands,
                            uint64_t ncand, hipStream_t st) {
    return launch_scan_list(GzmScan{in, n}, in, n, tile_offs, cands, ncand, st);
}

hipError_t launch_gzm_measure(const uint8_t* in, uint64_t n, const GzmCand* cands, uint64_t ncand, GzmRec* recs,
                              unsigned int* ticket, uint32_t flags, uint64_t limit, hipStream_t st, int* occupancy) {
    int dev = 0, ncu = 0, per = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_gzm_measure, IF_NT, 0);
    if (occupancy) *occupancy = per;
    if (!ncand) return hipSuccess;
    const uint64_t fit = (uint64_t)max(ncu, 1) * (uint64_t)max(per, 1);
    const uint32_t grid = (uint32_t)(ncand < fit ? ncand : fit);
    const hipError_t e = hipMemsetAsync(ticket, 0, sizeof(unsigned int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gzm_measure, dim3(grid), dim3(IF_NT), 0, st, in, n, cands, ncand, recs, ticket, flags, limit);
    return hipGetLastError();
}

hipError_t launch_gzm_gaps(const uint8_t* in, uint64_t n, const GzmGap* gaps, uint64_t ngaps, uint64_t longest,
                           uint64_t forced, unsigned long long* flag, uint64_t* res, hipStream_t st) {
    hipError_t e = hipMemsetAsync(flag, 0xFF, 8, st);
    if (e != hipSuccess) return e;
    if (ngaps && forced == ~0ull) {
        const uint64_t chunks = (longest + GM_GAP_CHUNK - 1) / GM_GAP_CHUNK;
        const dim3 grid((uint32_t)(ngaps < 4096 ? ngaps : 4096), (uint32_t)(chunks < 1 ? 1 : chunks < 1024 ? chunks : 1024));
        hipLaunchKernelGGL(k_gzm_gaps, grid, dim3(GM_NT), 0, st, in, n, gaps, ngaps, flag);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_gzm_gap_status, dim3(1), dim3(64), 0, st, in, n, flag, forced, res);
    return hipGetLastError();
}

}  // namespace dmx
