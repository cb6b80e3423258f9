// dmx_ctx.h -- the context and the small pieces the host translation units share (dmx_host.cpp:
// context, single-stream calls, checksums, host zlib / gzip forms, seek calls, files, multi-GPU;
// host_batch.cpp: the batch calls, synchronous, asynchronous and framed; host_members.cpp: BGZF
// files and multi-member gzip; host_inflate.cpp: the segmented inflate plan, the async path, the
// serial fallback; host_fb.cpp: path 5).
//
// A context owns one HIP device, one non-blocking stream and grow-only device scratch
// (segment slots, size/offset arrays, candidate lists, look-back words).  Every entry point
// locks the context, so a context may be shared between threads; the default context is
// created once per process (std::call_once) on the caller's current device.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/dmx.h"
#include "dmx_internal.h"
#include "cand_scan.h"
#include "inflate_plan.h"

namespace dmx {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool ensure(size_t bytes) {
        if (bytes <= cap) return true;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 8 + 4096;
        if (hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            return false;
        }
        cap = want;
        return true;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// The synchronous calls' results, in pinned host memory mapped into the device: the kernels
// that produce these words store them here too, and the host reads them after the call's one
// hipStreamSynchronize -- no copy operation.  (The device-side copies in Scal stay: kernels read them.)
struct HostRes {
    uint64_t total;     // deflate: the stream's length (k_scan_apply)
    uint64_t nmarkers;  // inflate: the marker scan's total (k_scan_apply)
    InflateResult res;  // inflate: the last validation (k_inflate_validate)
};

}  // namespace dmx

struct dmx_ctx {
    using DevBuf = dmx::DevBuf;
    int device = 0;
    uint32_t seg = 32768;
    uint32_t flags = 0;
    int inflate_pass = -1;     // dmx_config.dev_inflate_pass - 1: forced pass, -1 = the plan
    uint32_t heavy_bytes = 0;  // dmx_config.dev_heavy_bytes
    uint32_t diag = 0;         // DIAG_* bits, read once from the environment at dmx_create
    hipStream_t stream = nullptr;
    std::mutex mu;
    DevBuf in, out, slots, sizes, offs, scal, cands, tiles, tileoffs, recs, status, dbg;
    DevBuf dtok, dntok;                  // deflate: the front kernel's token words and counts
    DevBuf rtmp, rchain;                 // chain repair: scratch output, chain / offsets / sizes
    DevBuf ltok, ltokoff, lntok, lcaps, lsplit;  // lane decoder token lists (mode 4), 64 KiB halves
    DevBuf lheavy;                       // heavy-candidate list for the workgroup decoder (mode 6)
    int ncu = 256;                       // compute units, read at dmx_create (mode 6 grid, lane resolve)
    // block-parallel path (path 5): scan counts / hits / offsets, hit list, unit starts, token
    // offsets and words, unit records, chain (unit index, offset, size), 16-bit image
    DevBuf fbc, fbh, fbo, fbl, fbs, fbt, fbk, fbu, fbch, fbco, fbcs, fbimg, fbstop, fbwin, fbopen;
    DevBuf fbvm, fbvh;  // per-unit start mode and code state (region and repair units)
    DevBuf fbph;  // DMX_FB_DEBUG: k_fb_units phase cycles
    // path 5: the accepted unit starts, written by k_fb_check straight into host memory
    uint64_t* fbkeep_h = nullptr;
    uint64_t* fbkeep_d = nullptr;
    // path 5: pinned staging of host-to-device uploads (a copy from pageable memory goes through
    // the driver's own staging); reused per batch -- a stream sync separates the batches
    uint8_t* pin = nullptr;
    size_t pin_cap = 0, pin_off = 0;
    DevBuf fbreg, fbJ, fbvis;  // fixed-code regions: {E, T, first super block} + super-block regions, jumps, visits
    DevBuf fbJraw, fbJsub, fbcbit, fbucb;  // regions: chunk maps, sub-chunk entries, chunk entries, unit chunk
    DevBuf ck;  // checksum scratch (checksum.hip) + the 4-byte result at its start
    DevBuf btab, bres;  // batch calls: the uploaded tables / descriptors; the results + the ticket
    DevBuf adf, ainf;   // dmx_*_batch_async: the tables built on the device (deflate; inflate)
    DevBuf fdesc;       // framed batch deflate: {plain input, size, framed output, capacity} per buffer
    // BGZF files in device memory: the deflate's member slots / the ranged read's edge members;
    // the chain scratch (tile counts, candidates, jump tables, member table); descriptors + results
    // (bgzt: the candidate scan's tile counts and offsets, which outlive the sizing of bgzc)
    DevBuf bgzs, bgzc, bgzd, bgzt;
    // seek index: the ranged read's head + spans, or the window gather's slot list; and, for the
    // one call that asks for an index (dmx_inflate_index_device, null otherwise), where the path
    // that decodes the stream lists its checkpoints
    DevBuf seekd;
    dmx::SeekTap* seek_tap = nullptr;
    dmx::HostRes* hres = nullptr;      // host address (nullptr: not available, results are copied)
    dmx::HostRes* hres_dev = nullptr;  // the same block as the device sees it
    dmx::SpecKnob spec = dmx::SpecKnob::On;  // DMX_INFLATE_SPEC, read at dmx_create
    bool timing = false;
    bool ev3_marked = false;  // ev[3] is recorded already, in front of the call's last wait (mark_end)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_df = nullptr;          // end of the last deflate's work (its scratch is reused)
    hipEvent_t ev_inf = nullptr;         // end of the last asynchronous inflate's work
    bool inf_pending = false;
    bool df_pending = false;
    // the deflate's chunk pipeline: the knob (DMX_DEFLATE_PIPE, read at dmx_create) and, from the
    // first call that takes it, the side stream of the emission kernels and its two events
    dmx::PipeKnob pipe{};
    hipStream_t side = nullptr;
    hipEvent_t ev_chunk = nullptr, ev_side = nullptr;
    dmx_stats stats{};
    uint64_t last_end = 0;               // the last inflate: stream byte just past its final block
    std::vector<dmx_ctx*> subs;          // n_gpus > 1: one context per shard / piece
};

namespace dmx {

// Diagnostics (never steer results): read from the environment once, at dmx_create.
//   DMX_DEBUG=1       names the failing HIP call on stderr (process-wide)
//   DMX_PHASES=<file> per-phase s_memtime timelines of the segmented kernels
//   DMX_FB_DEBUG=1    block-parallel path: unit outcomes and chain breaks on stderr
//   DMX_FB_HOSTTIME=1 block-parallel path: host wall clock per phase on stderr
//   DMX_RECS=1        segmented inflate: per-candidate outcome of each pass on stderr
// A developer switch of its own, read at every dmx_create (deflate_pipe.h: pipe_knob):
//   DMX_DEFLATE_PIPE=0|1|<chunks>|s<segments>  the deflate's chunk pipeline
//   DMX_INFLATE_SPEC=0|1|force  the synchronous inflate's speculative first pass (inflate_plan.h)
// and one read at every dmx_inflate_gzip_members call while dmx_set_timing is on:
//   DMX_GZM_MAIN=scan|measure  the phase dmx_stats.ms_main_kernel brackets there (else: the batch decode)
enum : uint32_t { DIAG_PHASES = 1, DIAG_FB = 2, DIAG_RECS = 4, DIAG_DEBUG = 8, DIAG_FBT = 16 };
struct Diag {
    uint32_t bits = 0;
    std::string phases_path;
};
const Diag& diag_env();  // first use (a dmx_create) reads the environment
void hipchk_report(const char* what, hipError_t e, const char* file, int line);
#define HIPCHK(x)                                          \
    do {                                                   \
        const hipError_t e_ = (x);                         \
        if (e_ != hipSuccess) {                            \
            hipchk_report(#x, e_, __FILE_NAME__, __LINE__); \
            return DMX_ERR_DEVICE;                         \
        }                                                  \
    } while (0)

struct Scal {  // small device-side scalars, one allocation
    uint64_t total;
    uint64_t nmarkers;
    uint32_t ticket;
    uint32_t fb_err;  // block-parallel path: a copy reached before the stream start
    uint32_t fb_nkeep;  // block-parallel path: accepted unit starts (k_fb_check)
    uint64_t ncand;     // dmx_inflate_device_async: the candidate count, on the device
    InflateResult res;
    ValidateWords vw;
};

// DMX_PHASES=<file>: kernels record s_memtime per phase and segment; the host appends one line
// "<kernel> <nsegs> <mean cycles of phase k - phase k-1 ...>" per call (developer profiling).
uint64_t* phase_buf(dmx_ctx* c, uint64_t nidx);
// stride (deflate): the front kernel's grid, for the interval between a workgroup's segments
void phase_dump(dmx_ctx* c, const char* kernel, uint64_t nidx, hipStream_t st, uint64_t stride = 0);

void begin_timing(dmx_ctx* c, hipStream_t st);
// mark_end in front of the call's last hipStreamSynchronize records the end event there, so that
// end_timing behind it reads the times without a wait of its own
void mark_end(dmx_ctx* c, hipStream_t st);
void end_timing(dmx_ctx* c, hipStream_t st);

// the stream seen as aligned words (the kernels read 4-byte words at or below its start)
struct StreamWords {
    const uint32_t* words;
    uint64_t misalign;
    explicit StreamWords(const uint8_t* d_in)
        : words(reinterpret_cast<const uint32_t*>(d_in - ((uintptr_t)d_in & 3))), misalign((uintptr_t)d_in & 3) {}
};

// What dmx_host.cpp, host_batch.cpp and host_members.cpp share among themselves.  Hidden: these
// names stay out of the library's dynamic symbol table.
#pragma GCC visibility push(hidden)

// Restores the calling thread's current HIP device on scope exit: an entry point switches to
// its context's device, and a caller driving several GPUs from one thread must not see its
// current device move.
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = prev == dev || hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// An entry point's prologue, behind its argument checks: locks the context, switches to its
// device and resolves the caller's stream (null: the context's own).  DMX_ENTER(g, c[, stream])
// declares the guard g and returns DMX_ERR_DEVICE where the switch failed, as HIPCHK does.
struct CallGuard {
    std::lock_guard<std::mutex> lock;
    DeviceGuard dev;
    const bool ok;
    const hipStream_t st;
    explicit CallGuard(dmx_ctx* c, void* stream = nullptr)
        : lock(c->mu), dev(c->device), ok(dev.ok), st(stream ? (hipStream_t)stream : c->stream) {}
};
#define DMX_ENTER(g, ...)   \
    CallGuard g(__VA_ARGS__); \
    if (!g.ok) return DMX_ERR_DEVICE

inline size_t up16(size_t b) { return (b + 15) & ~size_t(15); }
// the batch deflate knows 16 and 32 KiB segments (64 KiB blocks pair front segments)
inline bool has_batch_deflate(const dmx_ctx* c) { return c->seg == 16384 || c->seg == 32768; }

// The candidate scans' scratch in c->bgzt (cand_scan.h; BGZF, multi-member gzip, ZIP):
//   tile counts | tile offsets | the candidate count | `extra` bytes of the caller's small words
// carve sizes it for `tiles` tiles; count takes the result of the launch_*_count over counts, offs
// and d_ncand, reads the count back -- one host synchronisation -- and refuses `limit` candidates
// or more with DMX_ERR_NOMEM (candidate indices are 32-bit).
struct ScanScratch {
    uint32_t* counts = nullptr;
    uint64_t* offs = nullptr;
    uint64_t* d_ncand = nullptr;
    uint8_t* words = nullptr;
    uint64_t ncand = 0;
    bool carve(dmx_ctx* c, uint64_t tiles, size_t extra) {
        const size_t off_offs = up16(tiles * 4), off_ncand = off_offs + up16(scan_words(tiles) * 8);
        if (!c->bgzt.ensure(off_ncand + 16 + extra)) return false;
        uint8_t* const tb = c->bgzt.as<uint8_t>();
        counts = reinterpret_cast<uint32_t*>(tb);
        offs = reinterpret_cast<uint64_t*>(tb + off_offs);
        d_ncand = reinterpret_cast<uint64_t*>(tb + off_ncand);
        words = tb + off_ncand + 16;
        return true;
    }
    int count(hipError_t launched, uint64_t limit, hipStream_t st) {
        HIPCHK(launched);
        HIPCHK(hipMemcpyAsync(&ncand, d_ncand, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return ncand >= limit ? DMX_ERR_NOMEM : DMX_OK;
    }
};

// dmx_host.cpp
// The deflate's scratch for nseg segments, of which the front kernel sees nfront of fseg_bytes
// each, and the scratch half of its arguments.  false: out of device memory.
bool deflate_scratch(dmx_ctx* c, DeflateArgs& A, uint64_t nseg, uint64_t nfront, int level, uint32_t fseg_bytes);
// Adler-32 / CRC-32 of a device buffer, computed on the GPU (checksum.hip); the value is
// returned to the host (the call synchronizes the stream).
int checksum_locked(dmx_ctx* c, bool crc, const uint8_t* d, size_t n, uint32_t init, uint32_t* out, hipStream_t st);

// host_batch.cpp
// A framed batch call (dmx_*_batch_framed_device; the BGZF calls of host_members.cpp)
struct FramePlan {
    uint32_t format;                // DMX_FRAME_*
    int level;                      // deflate: the level the header states
    bool verify;                    // inflate: DMX_BATCH_VERIFY
    const InflateBatchDesc* hdesc;  // deflate: count x {plain input, size, framed output, capacity}
};
int deflate_batch_locked(dmx_ctx* c, const uint8_t* const* d_in, const size_t* n, size_t count, int level,
                         uint8_t* const* d_out, const size_t* cap, dmx_batch_result* res, hipStream_t st,
                         const uint8_t* d_dict = nullptr, size_t dict_len = 0, const FramePlan* fp = nullptr);
int inflate_batch_locked(dmx_ctx* c, const uint8_t* const* d_in, const size_t* n, size_t count,
                         uint8_t* const* d_out, const size_t* cap, dmx_batch_result* res, uint32_t flags,
                         hipStream_t st, const uint8_t* d_dict = nullptr, size_t dict_len = 0,
                         const FramePlan* fp = nullptr);
int deflate_batch_framed_locked(dmx_ctx* c, const uint8_t* const* d_in, const size_t* n, size_t count, int level,
                                uint32_t format, uint8_t* const* d_out, const size_t* cap, dmx_batch_result* res,
                                hipStream_t st);

#pragma GCC visibility pop

// host_inflate.cpp
// candidate segment starts: counts the markers per tile and scans the counts (Scal::nmarkers
// receives the total, nothing waits); then marker_write lists bit 0 and the markers in c->cands
// sync_call: the synchronous inflate's -- the count kernel zeroes the validation words and the
// heavy list's counters (*hl_zeroed: the list was there to zero), the total goes to the host
// block too and the candidate count to Scal::ncand
int marker_scan(dmx_ctx* c, const StreamWords& w, size_t n, uint64_t* ntiles, hipStream_t st, bool sync_call = false,
                const uint32_t** hl_zeroed = nullptr);
int marker_write(dmx_ctx* c, const StreamWords& w, size_t n, uint64_t ntiles, uint64_t cand_cap, hipStream_t st);
// Shared inflate driver.  fixed_out != nullptr: decode into the caller's device buffer of
// `cap` bytes.  Otherwise decode into c->out, grown as needed (*dev_out receives it).
// iflags: DMX_IFLAG_PIECE for one piece of a larger stream (dmx_inflate_piece_device).
int inflate_device_locked(dmx_ctx* c, const uint8_t* d_in, size_t n, uint8_t* fixed_out, size_t cap,
                          size_t* total_out, uint8_t** dev_out, hipStream_t st, uint32_t iflags = 0);
int inflate_device_async_locked(dmx_ctx* c, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap,
                                uint64_t* d_result, hipStream_t st, uint32_t iflags);
// host_fb.cpp
int inflate_fb_locked(dmx_ctx* c, const uint8_t* d_in, size_t n, uint8_t* fixed_out, size_t cap,
                      size_t* total_out, uint8_t** dev_out, hipStream_t st, bool* handled, uint32_t iflags);

}  // namespace dmx
