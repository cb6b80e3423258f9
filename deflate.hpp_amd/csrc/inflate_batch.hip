// inflate_batch.hip -- k_inflate_batch: many independent streams per launch, ONE WAVEFRONT PER
// STREAM (dmx_inflate_batch_device, dmx_batch_result.path 6).
//
// Each stream is decoded by the exact decoder inflate_blocks (realDecompress, inflate.hpp:
// 277-322, with the reference's lenient cases and error semantics) exactly as k_inflate_serial
// decodes one stream per process -- but a 64-thread workgroup here keeps under 40 KiB of LDS,
// so four decoders share a CU where the serial kernel's 64 KiB output ring fits two:
//     output ring   32768 B   the 32 KiB window; flushed to HBM by the whole wave in pieces
//     input ring     2048 B   RingInT<512, 128>: every bit read is an LDS read
//     Tables         ~5.6 KB  code tables of the block being decoded
// The grid is persistent (at most four workgroups per CU): a workgroup draws the next position
// of `order` from a device ticket until none is left; the host lists the streams longest
// first, so a long stream starts early and does not form the tail.
#include "inflate_common.h"

namespace dmx {

constexpr uint32_t BT_RING = 32768;       // output ring bytes = the DEFLATE window
constexpr uint32_t BT_FLUSH = 16384;      // unflushed bytes that trigger a flush
constexpr uint32_t BT_RW = 512, BT_RC = 128;  // input ring words, words per slide
using BatchIn = RingInT<BT_RW, BT_RC>;

// Output sink of one stream, modelled on the serial path's FlushSink with a ring of exactly the
// window size.  Byte k of the output lives at ring[k % 32768] until byte k + 32768 is written,
// so before a write every byte it replaces must already be in HBM: pos + L - flushed <= 32768.
// A literal or a copy adds at most 258 bytes and grown() flushes at 16384 unflushed bytes, so
// the bound holds with room to spare; a stored block flushes first and writes its bytes to HBM
// itself.  The window is intact: a copy reads bytes [pos - dist, pos), dist <= 32768, none of
// which a write at or after pos has replaced -- at dist = 32768 lane i reads and writes the same
// slot (read first), and for dist just below it the slot lane i reads is written by a later lane
// of the same wave-wide store, which executes after the wave-wide load.
// Bytes past `cap` are counted, not written; a distance beyond the stream start copies nothing,
// as in the reference (inflate.hpp:268-270).
// A preset dictionary (dmx_inflate_batch_dict_device) is history before byte 0: the wave fills
// the ring with its last dl <= 32768 bytes before decoding (batch_prefill), dictionary byte j at
// slot (j - dl) mod 32768, i.e. where output byte j - dl would lie.  pos still starts at 0 and
// the invariant above is unchanged -- the slots behind pos hold real history instead of stale
// bytes -- and the stream start moves back by dl: only a distance beyond pos + dl copies nothing.
// The dictionary itself is never flushed (flushed starts at 0, like pos).
template <bool DICT>
struct BatchHistory {  // DICT: dictionary bytes in the ring before byte 0
    uint32_t dl;
    __device__ uint32_t before() const { return dl; }
};
template <>
struct BatchHistory<false> {  // (the plain sink carries no such member)
    __device__ uint32_t before() const { return 0; }
};
template <bool DICT>
struct BatchSink : BatchHistory<DICT> {
    uint8_t* ring;     // BT_RING bytes of LDS
    uint64_t pos;      // output bytes so far
    uint64_t flushed;  // bytes [0, min(flushed, cap)) are in `out`
    uint8_t* out;
    uint64_t cap;
    uint32_t err;
    __device__ bool full() const { return false; }
    __device__ void flush() {  // [flushed, pos) ring -> out
        const uint64_t hi = pos < cap ? pos : cap;
        wave_sync();
        for (uint64_t i = flushed + lane_id(); i < hi; i += 64) out[i] = ring[i & (BT_RING - 1)];
        flushed = pos;
    }
    __device__ void grown() {
        if (pos - flushed >= BT_FLUSH) flush();
    }
    __device__ bool literal(uint32_t b) {
        if (lane_id() == 0) ring[pos & (BT_RING - 1)] = (uint8_t)b;
        pos++;
        grown();
        return true;
    }
    __device__ bool copy(uint32_t L, uint32_t dist) {
        if (L == 0 || dist == 0) return true;
        if (dist > pos + this->before()) return true;  // reference: nothing to copy (inflate.hpp:268-270)
        wave_sync();
        const uint32_t lane = lane_id();
        const uint64_t src = pos - dist;  // (before byte 0: wraps, and 2^64 is a multiple of the ring)
        if (dist >= L || dist >= 64) {  // each group of 64 reads only bytes written before it
            for (uint32_t i = lane; i < L; i += 64) {
                ring[(pos + i) & (BT_RING - 1)] = ring[(src + i) & (BT_RING - 1)];
                wave_sync();
            }
        } else {  // periodic: byte i repeats byte i mod dist
            for (uint32_t i = lane; i < L; i += 64)
                ring[(pos + i) & (BT_RING - 1)] = ring[(src + i % dist) & (BT_RING - 1)];
        }
        wave_sync();
        pos += L;
        grown();
        return true;
    }
    // a stored block of up to 65535 bytes: bytes i and i + 32768 share a ring slot and a lane
    // (32768 % 64 == 0), so the later byte is the one that stays
    template <class BR>
    __device__ bool stored(const BR& br, uint64_t b0, uint32_t len) {
        flush();
        wave_sync();
        for (uint32_t i = lane_id(); i < len; i += 64) {
            const uint8_t v = br.byte_at(b0 + i);
            ring[(pos + i) & (BT_RING - 1)] = v;
            if (pos + i < cap) out[pos + i] = v;
        }
        wave_sync();
        pos += len;
        flushed = pos;
        return true;
    }
};

// the dictionary's dl bytes into the ring slots [32768 - dl, 32768): 16 B per lane where the
// source allows it (ring slot and source address congruent mod 16), bytes at the ends
__device__ __forceinline__ void batch_prefill(uint8_t* ring, const uint8_t* dict, uint32_t dl) {
    const uint32_t lane = lane_id();
    uint8_t* const dst = ring + (BT_RING - dl);
    uint32_t head = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dict) & 15)) & 15u;
    if (((BT_RING - dl + head) & 15u) != 0 || head > dl) head = dl;  // not congruent: bytes throughout
    for (uint32_t i = lane; i < head; i += 64) dst[i] = dict[i];
    const uint32_t nvec = (dl - head) / 16;
    const uint4* const s4 = reinterpret_cast<const uint4*>(dict + head);
    uint4* const d4 = reinterpret_cast<uint4*>(dst + head);
    for (uint32_t i = lane; i < nvec; i += 64) d4[i] = s4[i];
    for (uint32_t i = head + 16 * nvec + lane; i < dl; i += 64) dst[i] = dict[i];
}

// DICT: the streams were made with a preset dictionary (dict / dl, 0 < dl <= 32768).  Each
// instantiation is compiled in a translation unit of its own (inflate_batch_dict.hip includes
// this file with DMX_BATCH_DICT set): with both in one unit the decoder's helper functions have
// two callers, are no longer inlined, and the plain kernel goes from 123 VGPRs and no scratch
// to 162 VGPRs and 12 bytes of scratch.
// norder_dev (dmx_inflate_batch_async): the order list's length on the device, at most norder --
// which is then the capacity the grid was sized for; nullptr: norder is the length.
template <bool DICT>
__global__ __launch_bounds__(IF_NT) void k_inflate_batch(const InflateBatchDesc* desc, const uint32_t* order,
                                                         uint64_t norder, ::dmx_batch_result* res,
                                                         unsigned int* ticket, uint32_t flags,
                                                         const uint8_t* dict, uint32_t dl,
                                                         const uint32_t* norder_dev) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[BT_RING];
    __shared__ uint32_t inring[BT_RW];
    __shared__ Tables T;
    if (norder_dev) {
        const uint64_t d = *norder_dev;
        norder = d < norder ? d : norder;
    }
    for (;;) {
        uint32_t k = 0;
        if (threadIdx.x == 0) k = atomicAdd(ticket, 1u);
        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        if (k >= norder) break;
        const uint32_t idx = order[k];
        const InflateBatchDesc d = desc[idx];
        ::dmx_batch_result r;
        r.bytes = 0;
        r.status = DMX_ERR_OVERREAD;  // an empty input: the reference throws
        r.path = 6;
        if (d.n != 0) {
            if (threadIdx.x == 0) T.fixed_loaded = 0;
            wave_sync();
            const uint64_t misalign = reinterpret_cast<uintptr_t>(d.in) & 3;
            BatchIn br;
            br.init(reinterpret_cast<const uint32_t*>(d.in - misalign), misalign, d.n, inring);
            br.seek(misalign * 8);
            BatchSink<DICT> sk{{}, ring, 0, 0, d.out, d.cap, 0};
            if constexpr (DICT) {
                sk.dl = dl;
                batch_prefill(ring, dict, dl);  // (copy()'s wave_sync orders it before the reads)
            }
            uint64_t end_byte = 0;
            bool fin = false;
            const uint32_t err = inflate_blocks(br, T, sk, (flags & DMX_CFG_RFC_STRICT) != 0, false, &end_byte, &fin);
            sk.flush();
            if (err == 0) {
                r.bytes = sk.pos;
                r.status = sk.pos > d.cap ? DMX_ERR_CAPACITY : DMX_OK;
            } else {
                r.status = (err & SEGF_OVERREAD) ? DMX_ERR_OVERREAD : DMX_ERR_DATA;
            }
        }
        if (threadIdx.x == 0) res[idx] = r;
        wave_sync();  // the next stream reuses the rings and tables
    }
}

#ifndef DMX_BATCH_DICT
#define DMX_BATCH_DICT 0
#endif
#if DMX_BATCH_DICT
hipError_t launch_inflate_batch_dict(const InflateBatchDesc* desc, const uint32_t* order, uint64_t norder,
                                     ::dmx_batch_result* res, unsigned int* ticket, uint32_t flags,
                                     const uint8_t* dict, uint32_t dl, hipStream_t st,
                                     const uint32_t* norder_dev) {
    if (!dict || dl == 0 || dl > kInflateDictMax) return hipErrorInvalidValue;
#else
hipError_t launch_inflate_batch(const InflateBatchDesc* desc, const uint32_t* order, uint64_t norder,
                                ::dmx_batch_result* res, unsigned int* ticket, uint32_t flags, hipStream_t st,
                                const uint32_t* norder_dev) {
    const uint8_t* const dict = nullptr;
    const uint32_t dl = 0;
#endif
    constexpr bool DICT = DMX_BATCH_DICT != 0;
    if (!norder) return hipSuccess;
    int dev = 0, ncu = 0, per = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_inflate_batch<DICT>, IF_NT, 0);
    const uint64_t fit = (uint64_t)max(ncu, 1) * (uint64_t)max(per, 1);
    const uint32_t grid = (uint32_t)(norder < fit ? norder : fit);
    const hipError_t e = hipMemsetAsync(ticket, 0, sizeof(unsigned int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_inflate_batch<DICT>, dim3(grid), dim3(IF_NT), 0, st, desc, order, norder, res, ticket, flags,
                       dict, dl, norder_dev);
    return hipGetLastError();
}

}  // namespace dmx
