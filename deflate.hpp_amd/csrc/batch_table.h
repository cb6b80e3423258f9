// batch_table.h -- the tables of a batch call built from device-resident descriptor arrays
// (dmx_deflate_batch_async / dmx_inflate_batch_async): the steps the kernels of batch_table.hip
// run, one call per "thread".  Plain C++, no HIP (DMX_HD as in container_parse.h):
// tests/cpp/batch_table_test.cpp runs the same calls serially and compares with the host loops of
// the synchronous batch calls.
//
// Deflate: the segment table of deflate_batch_locked -- a buffer's first segment holds seg - du
// bytes (du: the dictionary bytes it carries, 0 without one), the later ones seg.
//   1. count   one call per buffer: its segments; 0 and a flag for n > max_n (bt_count)
//   2. scan    bfirst[0 .. count] = the exclusive prefix sum of the counts (launch_scan_u32)
//   3. fill    one call per table slot below the capacity: its buffer by binary search in
//              bfirst, then the entry (bt_fill); a buffer whose segments do not all lie below
//              the capacity gets none
//   4. close   one call per buffer: the flag of a buffer that does not fit, and -- from exactly
//              one buffer -- the segment count the kernels work on, clipped at the first buffer
//              that does not fit (bt_close)
// Inflate: the streams the batch kernel keeps, listed longest class first (class = floor(log2 n)):
// a histogram of the classes, the classes' first positions, a scatter (bt_mark, bt_class,
// bt_class_starts; under hipcc also the scatter's one device form, bt_order_scatter, which
// k_bt_order and the ZIP extraction's k_zip_order call).
#pragma once
#include <stdint.h>

#include "container_parse.h"  // DMX_HD

namespace dmx {

// One segment of a batch: `nb` bytes at `src`; `tail` bytes are readable from src to the end of
// its buffer (a word read may not run into a neighbour's allocation).
// A preset dictionary (dmx_deflate_batch_dict_device): the first segment of every buffer carries
// the last dlen <= kDeflateDictMax dictionary bytes at dict; the front kernel matches in the image
// [dictionary bytes | the segment's nb bytes], dlen + nb <= the segment size, and emits tokens
// for the segment's own bytes only.  dlen == 0: an ordinary segment.
struct DeflateBatchSeg {
    const uint8_t* src;
    uint64_t tail;
    uint32_t nb;     // <= the context's segment size
    uint32_t buf;    // buffer index | DF_BATCH_LAST on the last segment of its buffer (BFINAL)
    const uint8_t* dict;
    uint64_t dlen;
};
constexpr uint32_t DF_BATCH_LAST = 1u << 31;

struct InflateBatchDesc {
    const uint8_t* in;
    uint64_t n;
    uint8_t* out;
    uint64_t cap;
};

// ---- deflate ----------------------------------------------------------------------------------
// segments of an n-byte buffer (the rule of deflate_batch_locked)
DMX_HD inline uint64_t bt_segments(uint64_t n, uint32_t seg, uint32_t du) {
    const uint64_t seg0 = seg - du;
    return n <= seg0 ? (n ? 1u : 0u) : 1 + (n - seg0 + seg - 1) / seg;
}

DMX_HD inline uint64_t bt_sat_mul(uint64_t a, uint64_t b) { return (b && a > ~0ull / b) ? ~0ull : a * b; }
DMX_HD inline uint64_t bt_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// The table's capacity: min(count * K, ceil(max_total / seg) + count), K = the segments of a
// max_n-byte buffer; max_total == 0: unknown, taken as count * max_n.  (Saturates at 2^64 - 1.)
DMX_HD inline uint64_t bt_capacity(uint64_t count, uint64_t max_n, uint64_t max_total, uint32_t seg, uint32_t du) {
    const uint64_t by_n = bt_sat_mul(count, bt_segments(max_n, seg, du));
    const uint64_t total = max_total ? max_total : bt_sat_mul(count, max_n);
    const uint64_t by_total = bt_sat_add(total / seg + (total % seg ? 1 : 0), count);
    return by_n < by_total ? by_n : by_total;
}

// step 1 (buffer i): its segment count; *flag = 1 and no segments when n > max_n, else 0.
// (The caller bounds max_n so that the count fits 32 bits.)
DMX_HD inline uint32_t bt_count(uint64_t n, uint64_t max_n, uint32_t seg, uint32_t du, uint8_t* flag) {
    const bool over = n > max_n;
    *flag = over ? 1 : 0;
    return over ? 0u : (uint32_t)bt_segments(n, seg, du);
}

// The buffer of table slot s: the b < count with bfirst[b] <= s < bfirst[b + 1] -- among equal
// entries (buffers without segments) the last one.  s < bfirst[count].
DMX_HD inline uint64_t bt_find(const uint64_t* bfirst, uint64_t count, uint64_t s) {
    uint64_t lo = 1, hi = count;  // the first j in [1, count] with bfirst[j] > s
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (bfirst[mid] > s) hi = mid;
        else lo = mid + 1;
    }
    return lo - 1;
}

// step 3 (slot s < cap): false when no segment lies there or its buffer does not fit the
// capacity; else *e = the entry the host loop of deflate_batch_locked writes.  n[b] <= max_n for
// the buffer found (a larger one has no slots).  dtail: the dictionary's last du bytes.
DMX_HD inline bool bt_fill(uint64_t s, const uint64_t* bfirst, uint64_t count, uint64_t cap,
                           const uint8_t* const* in, const uint64_t* n, uint32_t seg, uint32_t du,
                           const uint8_t* dtail, DeflateBatchSeg* e) {
    if (s >= bfirst[count]) return false;
    const uint64_t b = bt_find(bfirst, count, s);
    if (bfirst[b + 1] > cap) return false;
    const uint64_t k = s - bfirst[b], seg0 = seg - du;
    const uint64_t o = k ? seg0 + (k - 1) * seg : 0, len = k ? seg : seg0;
    const uint64_t rest = n[b] - o;
    e->src = in[b] + o;
    e->tail = rest;
    e->nb = (uint32_t)(len < rest ? len : rest);
    e->buf = (uint32_t)b | (rest <= len ? DF_BATCH_LAST : 0u);
    e->dict = o ? nullptr : dtail;  // (the host loop's test: o == 0)
    e->dlen = o ? 0u : du;
    return true;
}

// step 4 (buffer b): sets flag[b] when the buffer's segments do not all lie below cap (the
// flag of step 1 stays); true for exactly one b of a batch, with *nseg = the segments of the
// buffers before the first that does not fit (all of them when every buffer fits).
DMX_HD inline bool bt_close(uint64_t b, const uint64_t* bfirst, uint64_t count, uint64_t cap, uint8_t* flag,
                            uint64_t* nseg) {
    const bool over = bfirst[b + 1] > cap;
    if (over) flag[b] = 1;
    if (over && bfirst[b] <= cap) {  // the first one: its predecessor ends at bfirst[b] <= cap
        *nseg = bfirst[b];
        return true;
    }
    if (!over && b + 1 == count) {
        *nseg = bfirst[count];
        return true;
    }
    return false;
}

// ---- inflate ----------------------------------------------------------------------------------
enum : uint32_t { BT_KEEP = 0, BT_OVER = 1, BT_DEFER = 2 };
constexpr uint32_t kBatchClasses = 64;

// What becomes of stream i: over max_n (DMX_ERR_ARG), deferred to the single-stream plan (route:
// the call routes; route_bytes: the threshold of the synchronous call, which leaves a stream
// without an output buffer on the batch kernel), or kept.
DMX_HD inline uint32_t bt_mark(uint64_t n, uint64_t max_n, bool route, uint64_t route_bytes, bool has_out) {
    if (n > max_n) return BT_OVER;
    return route && n > route_bytes && has_out ? BT_DEFER : BT_KEEP;
}

// floor(log2 n); 0 for n == 0
DMX_HD inline uint32_t bt_class(uint64_t n) {
    uint32_t c = 0;
    while (n >>= 1) c++;
    return c;
}

// start[c] = the kept streams of the classes above c (the longest class comes first); returns
// the number of kept streams
DMX_HD inline uint32_t bt_class_starts(const uint32_t* hist, uint32_t* start) {
    uint32_t run = 0;
    for (uint32_t c = kBatchClasses; c-- > 0;) {
        start[c] = run;
        run += hist[c];
    }
    return run;
}

#if defined(__HIPCC__)
// The order list's scatter (k_bt_order, zip_dir.hip's k_zip_order), called by every thread of a
// workgroup of at least kBatchClasses threads: stream i of class cls goes into the list where
// `keep`.  The classes' first positions (every workgroup scans the 64 counts of hist itself), the
// stream's rank among the workgroup's of its class, the workgroup's range of each class claimed
// from cursor (kBatchClasses words, zero at the launch).  Thread 0 returns the kept streams of
// the whole launch.
__device__ __forceinline__ uint32_t bt_order_scatter(bool keep, uint32_t cls, uint32_t i, const uint32_t* hist,
                                                     uint32_t* cursor, uint32_t* order) {
    __shared__ uint32_t start[kBatchClasses];  // the class's first position in the order list
    __shared__ uint32_t h[kBatchClasses];      // this workgroup's streams per class, then their base
    uint32_t kept = 0;
    if (threadIdx.x < kBatchClasses) h[threadIdx.x] = 0;
    if (threadIdx.x == 0) kept = bt_class_starts(hist, start);
    __syncthreads();
    uint32_t rank = 0;
    if (keep) rank = atomicAdd(&h[cls], 1u);
    __syncthreads();
    if (threadIdx.x < kBatchClasses) {
        const uint32_t mine = h[threadIdx.x];
        h[threadIdx.x] = mine ? atomicAdd(&cursor[threadIdx.x], mine) : 0u;
    }
    __syncthreads();
    if (keep) order[start[cls] + h[cls] + rank] = i;
    return kept;
}
#endif

}  // namespace dmx
