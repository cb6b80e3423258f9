// inflate_span.hip -- the seek index's kernels (dmx_inflate_index_device, dmx_inflate_range_device).
//
// k_inflate_spans: the ranged read.  ONE WAVEFRONT PER SPAN: each span of the plan (SeekSpan,
// seek_plan.h) starts at a block header's bit behind its own 32 KiB window, decodes `limit` plain
// bytes with the exact decoder's pieces (fast_header, decode_huffman; the reference's lenient cases
// and error semantics, as inflate_blocks) and stops.  The shape is k_inflate_batch's: a persistent
// grid (at most four workgroups per CU) that draws spans from a device ticket, and under 40 KiB of
// LDS per 64-thread workgroup:
//     output ring   32768 B   exactly the window; prefilled from the span's window slot
//     input ring     2048 B   RingInT<512, 128>: every bit read is an LDS read
//     Tables         ~5.6 KB  code tables of the block being decoded
// It has a translation unit of its own: a second caller of the decode helpers in inflate_batch.hip
// would cost that kernel registers (see there).
//
// k_seek_gather: the window store.  Slot k of the index gets the 32768 plain bytes before entry
// k's uoffset, out of the decoded output.
#include "inflate_common.h"

namespace dmx {

constexpr uint32_t SP_RING = 32768;       // output ring bytes = the DEFLATE window
constexpr uint32_t SP_FLUSH = 16384;      // unflushed bytes that trigger a flush
constexpr uint32_t SP_RW = 512, SP_RC = 128;  // input ring words, words per slide
using SpanIn = RingInT<SP_RW, SP_RC>;
static_assert(SP_RING == DMX_SEEK_WINDOW, "the ring is the window");

// Output sink of one span, BatchSink's ring discipline with a byte count.  Byte k of the span
// lives at ring[k % 32768] until byte k + 32768 is written, so before a write every byte it
// replaces that belongs to the caller must be in HBM: pos + L - flushed <= 32768.  A literal or a
// copy adds at most 258 bytes and grown() flushes at 16384 unflushed bytes; clipping a copy at
// `limit` only shortens it, so the bound holds.  The window is history before byte 0: its byte j
// (of wl = 32768) sits at slot j, where span byte j - 32768 would lie; pos starts at 0 and only a
// distance beyond pos + wl copies nothing (the stream-start rule, inflate.hpp:268-270, moved back
// by the window).  The window is never flushed, and neither are the span's first `skip` bytes:
// flush() writes positions [skip, pos) only, byte p to out[p - skip]; pos never passes limit.
struct SpanSink {
    uint8_t* ring;     // SP_RING bytes of LDS
    uint64_t pos;      // span bytes so far
    uint64_t flushed;  // bytes [skip, flushed) are in `out`
    uint64_t limit;    // the span's byte count
    uint64_t skip;     // leading bytes that are decoded, not written
    uint8_t* out;      // destination of byte `skip`
    uint32_t wl;       // window bytes in the ring before byte 0: 0 or 32768
    uint32_t err;
    __device__ bool full() const { return pos >= limit; }
    __device__ void flush() {  // [max(flushed, skip), pos) ring -> out
        const uint64_t lo = flushed > skip ? flushed : skip;
        wave_sync();
        for (uint64_t i = lo + lane_id(); i < pos; i += 64) out[i - skip] = ring[i & (SP_RING - 1)];
        flushed = pos;
    }
    __device__ void grown() {
        if (pos - flushed >= SP_FLUSH) flush();
    }
    __device__ bool literal(uint32_t b) {  // (decode_huffman asks full() before every token)
        if (lane_id() == 0) ring[pos & (SP_RING - 1)] = (uint8_t)b;
        pos++;
        grown();
        return true;
    }
    __device__ bool copy(uint32_t L, uint32_t dist) {
        if (L == 0 || dist == 0) return true;
        if (dist > pos + wl) return true;  // reference: nothing to copy (inflate.hpp:268-270)
        if (L > limit - pos) L = (uint32_t)(limit - pos);  // the span ends inside this copy
        wave_sync();
        const uint32_t lane = lane_id();
        const uint64_t src = pos - dist;  // (before byte 0: wraps, and 2^64 is a multiple of the ring)
        if (dist >= L || dist >= 64) {  // each group of 64 reads only bytes written before it
            for (uint32_t i = lane; i < L; i += 64) {
                ring[(pos + i) & (SP_RING - 1)] = ring[(src + i) & (SP_RING - 1)];
                wave_sync();
            }
        } else {  // periodic: byte i repeats byte i mod dist
            for (uint32_t i = lane; i < L; i += 64)
                ring[(pos + i) & (SP_RING - 1)] = ring[(src + i % dist) & (SP_RING - 1)];
        }
        wave_sync();
        pos += L;
        grown();
        return true;
    }
    // a stored block's first len bytes (the caller clips len at limit - pos): bytes i and i + 32768
    // share a ring slot and a lane (32768 % 64 == 0), so the later byte is the one that stays
    template <class BR>
    __device__ bool stored(const BR& br, uint64_t b0, uint32_t len) {
        flush();
        wave_sync();
        for (uint32_t i = lane_id(); i < len; i += 64) {
            const uint8_t v = br.byte_at(b0 + i);
            ring[(pos + i) & (SP_RING - 1)] = v;
            if (pos + i >= skip) out[pos + i - skip] = v;
        }
        wave_sync();
        pos += len;
        flushed = pos;
        return true;
    }
};

// the window slot's 32768 bytes into the ring: 16 B per lane when the slot is 16-byte aligned
__device__ __forceinline__ void span_prefill(uint8_t* ring, const uint8_t* win) {
    const uint32_t lane = lane_id();
    if ((reinterpret_cast<uintptr_t>(win) & 15) == 0) {
        const uint4* const s4 = reinterpret_cast<const uint4*>(win);
        uint4* const d4 = reinterpret_cast<uint4*>(ring);
        for (uint32_t i = lane; i < SP_RING / 16; i += 64) d4[i] = s4[i];
    } else {
        for (uint32_t i = lane; i < SP_RING; i += 64) ring[i] = win[i];
    }
}

// inflate_blocks (realDecompress, inflate.hpp:277-322) with a byte count: success as soon as the
// sink is full -- asked before each block header, and inside decode_huffman before each token --
// and SEGF_ERR_DATA when the BFINAL block ends before that (the index is not this stream's).
// A stored block is clipped to the bytes the span still needs.
template <class BR>
__device__ uint32_t span_blocks(BR& br, Tables& T, SpanSink& sk, bool rfc) {
    for (;;) {
        if (sk.full()) return 0;
        br.ensure(3);
        const uint32_t bfinal = br.bits(1);
        const uint32_t btype = br.bits(2);
        if (br.over()) return SEGF_OVERREAD;
        uint32_t err = 0;
        if (btype == 0) {
            br.align();
            br.ensure(32);
            const uint32_t len = br.bits(16);
            br.bits(16);  // NLEN is not checked (inflate.hpp:296-303)
            if (br.over()) return SEGF_OVERREAD;
            const uint64_t b0 = br.abspos() >> 3;
            const uint64_t room = sk.limit - sk.pos;
            const uint32_t take = len < room ? len : (uint32_t)room;
            if (b0 + take > br.end_bytes) return SEGF_OVERREAD;
            sk.stored(br, b0, take);
            if (sk.full()) return 0;
            br.seek(br.abspos() + 8ull * len);
            wave_sync();
        } else if (btype == 1) {
            if (!T.fixed_loaded) {
                load_fixed(T);
                T.fixed_loaded = 1;
            }
            err = decode_huffman(br, T, sk);
        } else if (btype == 2) {
            T.fixed_loaded = 0;
            uint64_t hp = br.abspos();
            err = fast_header(reader_words(br), &hp, br.end_bits, T, rfc, true);
            if (err) return err;
            br.seek(hp);
            err = decode_huffman(br, T, sk);
        }  // btype 3: no-op block (inflate.hpp:292 has no case 3)
        if (err == SEGF_SOFT) return 0;  // full inside the block
        if (err) return err;
        if (bfinal) return sk.full() ? 0 : SEGF_ERR_DATA;
    }
}

// head->key (preset to all ones by the upload): min over the failing spans of
// index << 32 | (uint32_t)status -- the first failing span's status
__global__ __launch_bounds__(IF_NT) void k_inflate_spans(const uint32_t* in_words, uint64_t misalign, uint64_t n,
                                                         const SeekSpan* spans, uint32_t nspans,
                                                         const uint8_t* windows, uint8_t* out, SeekSpanHead* head,
                                                         uint32_t flags) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[SP_RING];
    __shared__ uint32_t inring[SP_RW];
    __shared__ Tables T;
    for (;;) {
        uint32_t k = 0;
        if (threadIdx.x == 0) k = atomicAdd(&head->ticket, 1u);
        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        if (k >= nspans) break;
        const SeekSpan d = spans[k];
        if (threadIdx.x == 0) T.fixed_loaded = 0;
        SpanSink sk{ring, 0, 0, d.limit, d.skip, out + d.out_off, d.window ? SP_RING : 0u, 0};
        if (sk.wl) span_prefill(ring, windows + d.slot * (uint64_t)SP_RING);
        wave_sync();
        SpanIn br;
        br.init(in_words, misalign, n, inring);
        br.seek(misalign * 8 + d.bit);
        const uint32_t err = span_blocks(br, T, sk, (flags & DMX_CFG_RFC_STRICT) != 0);
        sk.flush();
        if (err && threadIdx.x == 0) {
            const int32_t status = (err & SEGF_OVERREAD) ? DMX_ERR_OVERREAD : DMX_ERR_DATA;
            atomicMin(&head->key, ((unsigned long long)k << 32) | (uint32_t)status);
        }
        wave_sync();  // the next span reuses the rings and tables
    }
}

hipError_t launch_inflate_spans(const uint32_t* in_words, uint64_t misalign, uint64_t n, const SeekSpan* spans,
                                uint32_t nspans, const uint8_t* windows, uint8_t* out, SeekSpanHead* head,
                                uint32_t flags, hipStream_t st) {
    if (!nspans) return hipSuccess;
    int dev = 0, ncu = 0, per = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_inflate_spans, IF_NT, 0);
    const uint64_t fit = (uint64_t)max(ncu, 1) * (uint64_t)max(per, 1);
    const uint32_t grid = (uint32_t)(nspans < fit ? nspans : fit);
    hipLaunchKernelGGL(k_inflate_spans, dim3(grid), dim3(IF_NT), 0, st, in_words, misalign, n, spans, nspans, windows,
                       out, head, flags);
    return hipGetLastError();
}

// Window slot list[b].slot = out[list[b].uoffset - 32768, list[b].uoffset).  Four workgroups of
// 256 threads per slot, 8 KiB each.  A block header falls on any byte, so the source is rarely
// aligned: when the slot is 16-byte aligned a lane builds each 16-byte store from the five aligned
// words that hold its bytes (the words at both ends lie in words the output buffer owns a byte
// of); a slot that is not goes byte by byte.
constexpr uint32_t SG_PART = 8192;
__global__ __launch_bounds__(256) void k_seek_gather(const uint8_t* out, const SeekSlot* list, uint8_t* windows) {
    const SeekSlot s = list[blockIdx.x];
    const uint64_t part = (uint64_t)blockIdx.y * SG_PART;
    const uint8_t* const src = out + (s.uoffset - SP_RING) + part;
    uint8_t* const dst = windows + s.slot * (uint64_t)SP_RING + part;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3);
        const uint32_t* const sw = reinterpret_cast<const uint32_t*>(src - a);
        uint4* const d4 = reinterpret_cast<uint4*>(dst);
        for (uint32_t v = threadIdx.x; v < SG_PART / 16; v += 256) {
            const uint32_t* const p = sw + 4 * v;
            const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3], w4 = a ? p[4] : 0u;
            const uint32_t sh = 8 * a;
            d4[v] = make_uint4(__builtin_amdgcn_alignbit(w1, w0, sh), __builtin_amdgcn_alignbit(w2, w1, sh),
                               __builtin_amdgcn_alignbit(w3, w2, sh), __builtin_amdgcn_alignbit(w4, w3, sh));
        }
    } else {
        for (uint32_t i = threadIdx.x; i < SG_PART; i += 256) dst[i] = src[i];
    }
}

hipError_t launch_seek_gather(const uint8_t* out, const SeekSlot* list, uint64_t nlist, uint8_t* windows,
                              hipStream_t st) {
    if (!nlist) return hipSuccess;
    hipLaunchKernelGGL(k_seek_gather, dim3((uint32_t)nlist, SP_RING / SG_PART), dim3(256), 0, st, out, list, windows);
    return hipGetLastError();
}

}  // namespace dmx
