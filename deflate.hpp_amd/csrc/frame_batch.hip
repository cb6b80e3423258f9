// frame_batch.hip -- the frame / unframe kernels of the framed batch calls
// (dmx_deflate_batch_framed_device, dmx_inflate_batch_framed_device; gfx950).
//
// The batch deflate and inflate kernels are not touched: they see raw RFC 1951 streams.  These
// kernels sit around them, one thread per buffer:
//   k_frame_parse    (inflate, before)  header -> side[k]; desc[k] narrowed to the raw stream
//   k_frame_verdict  (inflate, after)   header errors and trailer verdicts -> res[k]
//   k_frame_write    (deflate, after)   header, trailer and the framed res[k]
// The header parse and the writers are container_parse.h's, the code the CPU test runs.  The
// checksums come from k_checksum_batch (checksum.hip) in side[k].ck.  Every store is a plain
// byte or struct store.
#include "dmx_device.h"
#include "dmx_internal.h"

namespace dmx {

constexpr uint32_t FR_NT = 256;

__global__ __launch_bounds__(FR_NT) void k_frame_parse(InflateBatchDesc* desc, FrameHead* side, uint64_t count,
                                                       uint32_t format) {
    const uint64_t k = (uint64_t)blockIdx.x * FR_NT + threadIdx.x;
    if (k >= count) return;
    const InflateBatchDesc d = desc[k];
    const FrameHead h = parse_frame(format, d.in, d.n);
    side[k] = h;
    if (h.status == DMX_OK) {
        desc[k].in = d.in + h.head;
        desc[k].n = d.n - h.head;  // the trailer stays in the extent, as in dmx_inflate_zlib / _gzip
    } else {
        desc[k].n = 0;  // nothing to decode; k_frame_verdict reports the header's status
    }
}

__global__ __launch_bounds__(FR_NT) void k_frame_verdict(const FrameHead* side, ::dmx_batch_result* res,
                                                         uint64_t count, uint32_t format, int verify) {
    const uint64_t k = (uint64_t)blockIdx.x * FR_NT + threadIdx.x;
    if (k >= count) return;
    const FrameHead h = side[k];
    if (h.status != DMX_OK) {
        ::dmx_batch_result r;
        r.bytes = 0;
        r.status = h.status;
        r.path = 6;
        res[k] = r;
        return;
    }
    if (!verify || res[k].status != DMX_OK) return;  // (DMX_ERR_CAPACITY: the output is incomplete)
    const bool gz = format != DMX_FRAME_ZLIB;
    if ((gz && h.isize != (uint32_t)res[k].bytes) || h.ck != h.want) res[k].status = DMX_ERR_CHECKSUM;
}

__global__ __launch_bounds__(FR_NT) void k_frame_write(const InflateBatchDesc* desc, const FrameHead* side,
                                                       ::dmx_batch_result* res, uint64_t count, uint32_t format,
                                                       int level) {
    const uint64_t k = (uint64_t)blockIdx.x * FR_NT + threadIdx.x;
    if (k >= count) return;
    const InflateBatchDesc d = desc[k];
    ::dmx_batch_result r;
    r.path = 0;
    if (format == DMX_FRAME_BGZF && d.n > kBgzfBlock) {  // (the host gave the batch deflate nothing to do)
        r.bytes = 0;
        r.status = DMX_ERR_ARG;
        res[k] = r;
        return;
    }
    // the raw size is exact even when the raw stream did not fit its reduced capacity
    const uint64_t head = frame_head_bytes(format), tail = frame_tail_bytes(format);
    const uint64_t raw = res[k].bytes;
    r.bytes = head + raw + tail;
    r.status = r.bytes > d.cap ? DMX_ERR_CAPACITY : DMX_OK;
    if (r.status == DMX_OK) {
        frame_write_head(format, level, (uint32_t)r.bytes, d.out);
        frame_write_tail(format, side[k].ck, d.n, d.out + head + raw);
    }
    res[k] = r;
}

static uint32_t fr_grid(uint64_t count) { return (uint32_t)((count + FR_NT - 1) / FR_NT); }

hipError_t launch_frame_parse(InflateBatchDesc* desc, FrameHead* side, uint64_t count, uint32_t format,
                              hipStream_t st) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_frame_parse, dim3(fr_grid(count)), dim3(FR_NT), 0, st, desc, side, count, format);
    return hipGetLastError();
}

hipError_t launch_frame_verdict(const FrameHead* side, ::dmx_batch_result* res, uint64_t count, uint32_t format,
                                bool verify, hipStream_t st) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_frame_verdict, dim3(fr_grid(count)), dim3(FR_NT), 0, st, side, res, count, format,
                       verify ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_frame_write(const InflateBatchDesc* desc, const FrameHead* side, ::dmx_batch_result* res,
                              uint64_t count, uint32_t format, int level, hipStream_t st) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_frame_write, dim3(fr_grid(count)), dim3(FR_NT), 0, st, desc, side, res, count, format,
                       level);
    return hipGetLastError();
}

}  // namespace dmx
