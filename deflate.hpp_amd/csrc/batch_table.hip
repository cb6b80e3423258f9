// batch_table.hip -- the batch calls' tables built on the GPU from device-resident descriptor
// arrays (dmx_deflate_batch_async, dmx_inflate_batch_async): the host never reads a pointer, a
// size or a capacity.  The steps are the plain C++ of batch_table.h (shared with the CPU test);
// the kernels here only spread them over threads.
//
//   k_bt_count    one lane per buffer: its segment count and its over-max_n flag
//   (launch_scan_u32: bfirst = the exclusive prefix sum of the counts)
//   k_bt_fill     one thread per table slot below the capacity: the DeflateBatchSeg; and one thread
//                 per buffer: the does-not-fit flag and, from one of them, the device-side segment
//                 count
//   k_bt_desc     one lane per stream: its InflateBatchDesc, the result of a stream that is not
//                 decoded here, the class histogram (LDS per workgroup, then one atomic per class)
//   k_bt_order    the scatter of the kept streams into the order list (bt_order_scatter,
//                 batch_table.h, which the ZIP extraction's k_zip_order calls too)
// Counts and flags are written with ordinary (vector) stores from one lane.
#include "dmx_internal.h"

namespace dmx {

constexpr uint32_t BT_NT = 256;
static uint32_t bt_grid(uint64_t n) { return (uint32_t)((n + BT_NT - 1) / BT_NT); }

__global__ __launch_bounds__(BT_NT) void k_bt_count(const uint64_t* n, uint64_t count, uint64_t max_n, uint32_t seg,
                                                    uint32_t du, uint32_t* counts, uint8_t* flag) {
    const uint64_t i = (uint64_t)blockIdx.x * BT_NT + threadIdx.x;
    if (i >= count) return;
    uint8_t f;
    counts[i] = bt_count(n[i], max_n, seg, du, &f);
    flag[i] = f;
}

__global__ __launch_bounds__(BT_NT) void k_bt_fill(const uint8_t* const* in, const uint64_t* n, uint64_t count,
                                                   uint64_t cap, uint32_t seg, uint32_t du, const uint8_t* dtail,
                                                   const uint64_t* bfirst, DeflateBatchSeg* tab, uint8_t* flag,
                                                   uint64_t* nseg) {
    const uint64_t t = (uint64_t)blockIdx.x * BT_NT + threadIdx.x;
    if (t < cap) {
        DeflateBatchSeg e;
        if (bt_fill(t, bfirst, count, cap, in, n, seg, du, dtail, &e)) tab[t] = e;
    }
    if (t < count) {
        uint64_t ns;
        if (bt_close(t, bfirst, count, cap, flag, &ns)) *nseg = ns;
    }
}

__global__ __launch_bounds__(BT_NT) void k_bt_desc(const uint8_t* const* in, const uint64_t* n, uint8_t* const* out,
                                                   const uint64_t* cap, uint64_t count, uint64_t max_n,
                                                   uint64_t route_bytes, InflateBatchDesc* desc, uint32_t* hist,
                                                   ::dmx_batch_result* res) {
    __shared__ uint32_t h[kBatchClasses];
    if (threadIdx.x < kBatchClasses) h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * BT_NT + threadIdx.x;
    if (i < count) {
        InflateBatchDesc d;
        d.in = in[i];
        d.n = n[i];
        d.out = out[i];
        d.cap = cap[i];
        desc[i] = d;
        const uint32_t m = bt_mark(d.n, max_n, route_bytes != 0, route_bytes, d.out != nullptr);
        if (m == BT_KEEP) {
            atomicAdd(&h[bt_class(d.n)], 1u);
        } else {
            ::dmx_batch_result r;
            r.bytes = 0;
            r.status = m == BT_OVER ? DMX_ERR_ARG : DMX_BATCH_DEFERRED;
            r.path = 0;
            res[i] = r;
        }
    }
    __syncthreads();
    if (threadIdx.x < kBatchClasses && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// cursor: kBatchClasses words, zero at the launch
__global__ __launch_bounds__(BT_NT) void k_bt_order(const InflateBatchDesc* desc, uint64_t count, uint64_t max_n,
                                                    uint64_t route_bytes, const uint32_t* hist, uint32_t* cursor,
                                                    uint32_t* order, uint32_t* norder) {
    const uint64_t i = (uint64_t)blockIdx.x * BT_NT + threadIdx.x;
    bool keep = false;
    uint32_t cls = 0;
    if (i < count) {
        const InflateBatchDesc d = desc[i];
        keep = bt_mark(d.n, max_n, route_bytes != 0, route_bytes, d.out != nullptr) == BT_KEEP;
        cls = bt_class(d.n);
    }
    const uint32_t kept = bt_order_scatter(keep, cls, (uint32_t)i, hist, cursor, order);
    if (blockIdx.x == 0 && threadIdx.x == 0) *norder = kept;
}

hipError_t launch_batch_segtab(const uint8_t* const* in, const uint64_t* n, uint64_t count, uint64_t max_n,
                               uint64_t cap, uint32_t seg, uint32_t du, const uint8_t* dtail, uint32_t* counts,
                               uint64_t* bfirst, DeflateBatchSeg* tab, uint8_t* flag, uint64_t* nseg,
                               hipStream_t st) {
    if (!count || !cap) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bt_count, dim3(bt_grid(count)), dim3(BT_NT), 0, st, n, count, max_n, seg, du, counts, flag);
    const hipError_t e = launch_scan_u32(counts, bfirst, count, bfirst + count, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bt_fill, dim3(bt_grid(cap > count ? cap : count)), dim3(BT_NT), 0, st, in, n, count, cap, seg,
                       du, dtail, bfirst, tab, flag, nseg);
    return hipGetLastError();
}

hipError_t launch_batch_desc(const uint8_t* const* in, const uint64_t* n, uint8_t* const* out, const uint64_t* cap,
                             uint64_t count, uint64_t max_n, uint64_t route_bytes, InflateBatchDesc* desc,
                             uint32_t* order, uint32_t* norder, uint32_t* work, ::dmx_batch_result* res,
                             hipStream_t st) {
    if (!count) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(work, 0, 2 * kBatchClasses * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bt_desc, dim3(bt_grid(count)), dim3(BT_NT), 0, st, in, n, out, cap, count, max_n, route_bytes,
                       desc, work, res);
    hipLaunchKernelGGL(k_bt_order, dim3(bt_grid(count)), dim3(BT_NT), 0, st, desc, count, max_n, route_bytes, work,
                       work + kBatchClasses, order, norder);
    return hipGetLastError();
}

}  // namespace dmx
