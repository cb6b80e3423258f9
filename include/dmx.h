/* dmx.h -- C-ABI of the MI355X-native DEFLATE/INFLATE engine (libdmx.so).
 *
 * This is the drop-in boundary for HyperBitGore/deflate.hpp's hot path.  The reference has no
 * C ABI of its own (header-only static methods); each entry point below states the reference
 * interface it replaces (file:line under the reference's include/).  include/deflate.hpp and
 * include/inflate.hpp re-expose the reference's class API on top of these functions, and
 * INTEGRATION.md shows the ctypes / C++ bindings a caller adds.
 *
 * Plain pointers and sizes only; no torch or HIP types in any signature (streams are passed as
 * an opaque void* that is a hipStream_t).  All functions are thread-safe per context; the
 * default context (dmx_default_ctx) is created lazily under a once-flag.
 */
#ifndef DMX_H
#define DMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------------- */
#define DMX_OK 0
#define DMX_ERR_ARG (-1)      /* bad argument (null pointer, unsupported option)              */
#define DMX_ERR_NOMEM (-2)    /* host or device allocation failed                               */
#define DMX_ERR_DEVICE (-3)   /* HIP runtime error or no usable gfx950 device                   */
#define DMX_ERR_DATA (-4)     /* stream cannot be decoded (no Huffman code matches, bad table) */
#define DMX_ERR_OVERREAD (-5) /* stream ends before its final block: the reference throws
                                 "Reading bits beyond the alloted buffer size!"
                                 (inflate.hpp:81-82, 97-99, 106-108)                          */
#define DMX_ERR_CAPACITY (-6) /* caller's output buffer too small (device API only)           */
#define DMX_ERR_INTERNAL (-7)
#define DMX_ERR_CHECKSUM (-8) /* zlib Adler-32 / gzip CRC-32 or ISIZE mismatch (DMX_VERIFY)      */

/* ---- context --------------------------------------------------------------------------- */
typedef struct dmx_ctx dmx_ctx;

typedef struct dmx_config {
    int device;             /* HIP device ordinal, -1 = the calling thread's current device  */
    uint32_t segment_bytes; /* independent deflate segment: 16384, 32768 (default) or 65536.
                               32768 mirrors the reference's per-chunk LZ77 reset
                               (deflate.hpp:689-697).  65536 (SURVEY 8(d) config C4's
                               64 KiB blocks): one DEFLATE block per 64 KiB of input, its
                               two 32 KiB halves matched independently under one Huffman
                               code; inflate then places 64 KiB per segment.  Inflate takes
                               any stream with any setting; the lane decoder's slot follows
                               this size.                                                      */
    uint32_t flags;         /* DMX_CFG_*                                                        */
    uint32_t n_gpus;        /* 0 or 1: one device.  N > 1: the host-buffer API (dmx_deflate,
                               dmx_inflate, dmx_inflate_alloc, hence deflate::compress and
                               inflate::decompress) splits each large call over N devices,
                               `device`, device + 1, ... (mod the visible count: fewer GPUs than N
                               run several shards each; more than 8 per visible GPU is
                               DMX_ERR_ARG).  Deflate: contiguous segment-aligned
                               shards, NOT_FINAL except the last -- segments are independent
                               (deflate.hpp:689-697), so the bytes equal the one-device stream.
                               Inflate: cuts at segment starts proven by a piece-mode decode
                               (dmx_segment_check_device), one piece per device, the outputs
                               concatenated; a stream that does not split decodes on one.
                               The split assumes the stream's first BFINAL block lies in its
                               last piece (every stream libdmx, zlib or the reference writes);
                               bytes after an early BFINAL that still decode as marker-delimited
                               segments would be inflated too, where one device stops.          */
    /* developer controls for A/B runs; dmx_config_default sets both to 0 = the product plan */
    uint32_t dev_inflate_pass; /* k + 1 forces inflate pass k of the segmented plan
                                  (0 wave, 1 workgroup, 2 look-back, 4 lanes, 5 block-parallel,
                                  7 the serial decoder alone) */
    uint32_t dev_heavy_bytes;  /* lane decoder: candidates spanning more compressed bytes go to
                                  the workgroup decoder; 0 = the built-in 2048 and CU rule      */
} dmx_config;

/* Inflate code-length RLE per RFC 1951 (repeat may span HLIT/HDIST, code 16 repeats the
 * previous length) instead of the reference's behaviour (SURVEY A-11/A-12, inflate.hpp:166-224).
 * Default off: output is bit-exact to the reference. */
#define DMX_CFG_RFC_STRICT 1u
/* Developer A/B: the block-parallel path decodes every unit with one wavefront. */
#define DMX_CFG_FB_SERIAL 2u

void dmx_config_default(dmx_config* cfg);
int dmx_create(dmx_ctx** ctx, const dmx_config* cfg);
void dmx_destroy(dmx_ctx* ctx);
/* process-wide context (never destroyed), created on first use with the config set by
 * dmx_set_default_config, else the default config on the current device.  This is the context
 * include/deflate.hpp and include/inflate.hpp use: a caller of the reference's class API turns
 * on the whole node with one call, e.g. cfg.n_gpus = 8, before its first compress. */
dmx_ctx* dmx_default_ctx(void);
/* DMX_ERR_ARG once the default context exists (the config is read at its creation). */
int dmx_set_default_config(const dmx_config* cfg);

/* ---- host-buffer API (what include/deflate.hpp / inflate.hpp call) ---------------------- */

/* Upper bound of dmx_deflate's output for n input bytes, any segment size / level. */
size_t dmx_deflate_bound(size_t n);

/* Replaces deflate::compress(char*, size_t, int)             deflate.hpp:779-796
 *          deflate::compress(std::vector<uint8_t>&, int)      deflate.hpp:798-815
 * Raw DEFLATE (RFC 1951, no zlib/gzip wrapper).  level 0 = stored, 1 = Huffman only,
 * 2 = fast (greedy hash), 3 = slow (lazy, deeper search); any other value behaves like 1,
 * as the reference's switch without default does (deflate.hpp:699-717).  Output is a valid
 * stream the reference inflate::decompress round-trips exactly (the reference's own levels
 * 2/3 are not; SURVEY A-1..A-3).  *out_len receives the stream length. */
int dmx_deflate(dmx_ctx* ctx, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap,
                size_t* out_len);

/* Replaces inflate::decompress(void*, size_t, void*, size_t)   inflate.hpp:338-350
 * Decodes the whole stream, copies min(total, cap) bytes to out.  *written = bytes copied
 * (the reference's return value), *total = full decoded size (may be NULL). */
int dmx_inflate(dmx_ctx* ctx, const uint8_t* in, size_t n, uint8_t* out, size_t cap,
                size_t* written, size_t* total);

/* Replaces inflate::decompress(void*, size_t)                  inflate.hpp:363-374
 *          inflate::decompress(std::vector<uint8_t>)           inflate.hpp:376-387
 * *out is allocated by the library; release it with dmx_free. */
int dmx_inflate_alloc(dmx_ctx* ctx, const uint8_t* in, size_t n, uint8_t** out, size_t* len);

void dmx_free(void* p);

/* Replaces deflate::compress(std::string, std::string, int)      deflate.hpp:755-777
 *          inflate::decompress(std::string, std::string)          inflate.hpp:390-408
 * Streaming file I/O in 64 MiB chunks.  Deflate: a reader thread fills two pinned buffers,
 * the H2D of chunk k + 1 and the D2H + file write of chunk k - 1 (a writer thread) overlap the
 * compression of chunk k; each chunk is a NOT_FINAL shard, the last one final, so the file is
 * one stream; device memory is bounded (2 x 64 MiB in, 2 x bound out).  Inflate: the
 * compressed file streams into HBM (disk reads overlapping the H2D copies), decodes as one
 * stream, and the D2H of each output chunk overlaps the file write of the previous one; it
 * holds the whole compressed file and the whole output in HBM (plus the decoder's scratch),
 * so files beyond the device's memory are not supported.  Unlike the reference (correct only
 * for files <= 32 KiB, SURVEY A-8) any size that fits works.  Sizes are reported through the
 * optional out-parameters. */
int dmx_deflate_file(dmx_ctx* ctx, const char* in_path, const char* out_path, int level,
                     size_t* in_bytes, size_t* out_bytes);
int dmx_inflate_file(dmx_ctx* ctx, const char* in_path, const char* out_path, size_t* out_bytes);
const char* dmx_strerror(int code);

/* ---- device-resident API (HBM in, HBM out; used by bench.py and multi-GPU sharding) ------ */

/* Do not set BFINAL on the last block: the output is one shard of a larger stream and ends
 * byte-aligned on an empty stored block, so shards concatenate with plain byte copies. */
#define DMX_DEFLATE_NOT_FINAL 1u

/* d_in/d_out are device pointers on the context's device; stream is a hipStream_t or NULL for
 * the context's own stream.  Returns DMX_ERR_CAPACITY if cap < the produced size.
 * Host synchronisations: 1 (the length, which the scan kernel stores into host-mapped memory:
 * no copy operation follows the work). */
int dmx_deflate_device(dmx_ctx* ctx, const void* d_in, size_t n, int level, uint32_t flags,
                       void* d_out, size_t cap, size_t* out_len, void* stream);

/* The same without a host synchronisation: every step is enqueued on `stream` and the stream
 * length lands in *d_out_len (8 bytes of DEVICE memory) when the work completes; the call
 * returns once it is enqueued (graph-capturable, and a multi-GPU caller can keep every device
 * busy from one thread).  A length above cap means the output did not fit: only the segments
 * that fit were written.  Calls on one context are ordered even across streams (the context's
 * scratch is reused). */
int dmx_deflate_device_async(dmx_ctx* ctx, const void* d_in, size_t n, int level, uint32_t flags,
                             void* d_out, size_t cap, uint64_t* d_out_len, void* stream);

/* Device-resident inflate.  Returns DMX_ERR_CAPACITY (and the needed size in *out_len) when
 * the decoded stream does not fit in cap.
 * Host synchronisations: 1 for a stream in libdmx's segment layout that the lane decoder takes
 * whole, when cap / segment_bytes exceeds 2048 and the stream has more than 2048 and at most
 * cap / segment_bytes + 64 segments -- the first pass is launched before the host knows the
 * segment count, and the count and the pass's validation come back together (DMX_INFLATE_SPEC=0
 * in the environment at dmx_create turns that off).  Otherwise 2 (segment count; validation),
 * plus one per further pass of the plan and those of the chain repair, path 5 or the serial
 * decoder where a stream needs them. */
int dmx_inflate_device(dmx_ctx* ctx, const void* d_in, size_t n, void* d_out, size_t cap,
                       size_t* out_len, void* stream);

/* Device-resident inflate without any host synchronisation, for streams in libdmx's segment
 * layout (its own deflate output, or any stream of independent marker-delimited segments of at
 * most segment_bytes each): every step is enqueued on `stream` and the call returns at once
 * (graph-capturable; a multi-GPU caller keeps every device busy from one thread).  When the
 * work completes, d_result (16 bytes of DEVICE memory) holds {decoded bytes, status}: status 0
 * = decoded into d_out; status 1 = this fast path does not take the stream (another layout, a
 * segment it declines, more segments than cap / segment_bytes + 64, output beyond cap) and
 * nothing is promised about d_out -- decode it with dmx_inflate_device, which takes any stream.
 * flags: DMX_INFLATE_PIECE for one piece of a larger stream (a back-reference before the piece
 * is an error, as in dmx_inflate_piece_device).  Calls on one context are ordered even across
 * streams.  Replaces nothing in the reference (whose inflate is synchronous, inflate.hpp:
 * 338-408); it is the asynchronous form of the same decode (multi-GPU pieces). */
#define DMX_INFLATE_PIECE 1u
int dmx_inflate_device_async(dmx_ctx* ctx, const void* d_in, size_t n, void* d_out, size_t cap,
                             uint64_t* d_result, uint32_t flags, void* stream);

/* Byte offsets just past every "00 00 FF FF" (empty stored block) in a device-resident stream:
 * the candidate segment starts of libdmx's layout, in order (at most cap written, *count = all).
 * Multi-GPU inflate splits a stream at these (deflate.hpp_amd/shard.py scatter_inflate); a
 * false candidate inside stored data makes the piece before it fail to decode, and the caller
 * then decodes the stream whole. */
int dmx_segment_starts_device(dmx_ctx* ctx, const void* d_in, size_t n, uint64_t* starts, size_t cap,
                              size_t* count, void* stream);

/* One piece of a larger stream cut at a segment start (multi-GPU inflate, shard.py): exactly
 * dmx_inflate_device, except that a back-reference reaching before the piece's first byte is
 * DMX_ERR_DATA.  At a stream's true start the reference copies nothing for such a distance
 * (inflate.hpp:268-270) and dmx_inflate_device does the same; inside a stream whose window
 * carries across the cut (zlib's sync flush) that rule would drop bytes without an error. */
int dmx_inflate_piece_device(dmx_ctx* ctx, const void* d_in, size_t n, void* d_out, size_t cap,
                             size_t* out_len, void* stream);

/* Cut-point check for multi-GPU inflate: for each of k candidate starts (host array, stream
 * byte offsets, e.g. from dmx_segment_starts_device) the one segment beginning there is decoded
 * by the exact decoder in piece mode; ends[i] (host array) = the byte just past its closing
 * empty stored block "00 00 FF FF" (or past its BFINAL block), or UINT64_MAX when it does not
 * decode (a "00 00 FF FF" inside stored data, more than 32 KiB of output, a reference before
 * the start).  A start whose segment ends on a marker is a block boundary the decoder reaches
 * with an empty window; shard.py cuts only there. */
int dmx_segment_check_device(dmx_ctx* ctx, const void* d_in, size_t n, const uint64_t* starts, size_t k,
                             uint64_t* ends, void* stream);

/* ---- batched API: many independent buffers per call (not in the reference) ----------------
 * Every entry point above takes one buffer and pays a fixed cost per call (kernel launches,
 * host synchronisations).  These take `count` independent buffers and cover all of them with
 * one set of launches.
 *
 * Return value: the call as a whole -- DMX_ERR_ARG (null context or array, unsupported
 * option), DMX_ERR_NOMEM or DMX_ERR_DEVICE.  A bad stream or a short cap[i] is reported only in
 * res[i] and never disturbs its neighbours; count == 0 is DMX_OK.
 *
 * Deflate: stream i is exactly the bytes dmx_deflate_device(ctx, d_in[i], n[i], level, 0, ...)
 * writes: a complete stream with BFINAL (an empty input gives 03 00); dmx_deflate_bound(n[i])
 * bounds it.  When cap[i] is too small, status = DMX_ERR_CAPACITY, bytes = the size that was
 * needed, and nothing is written past d_out[i] + cap[i].  Contexts with segment_bytes of 16 or
 * 32 KiB are supported; a context with segment_bytes = 65536 returns DMX_ERR_ARG (its emit
 * stage codes front segments 2s and 2s + 1 as one block, a pairing that does not survive buffer
 * boundaries).
 *
 * Inflate: the per-stream result equals dmx_inflate_device on that stream alone -- any RFC 1951
 * stream, the reference's lenient cases and the A-11/A-12 quirks included (DMX_CFG_RFC_STRICT of
 * the context is honoured), and the same codes: DMX_ERR_OVERREAD for n[i] == 0 or a truncated
 * stream, DMX_ERR_DATA, DMX_ERR_CAPACITY.  With DMX_ERR_CAPACITY from the batch decoder, bytes
 * = the full decoded size and the first cap[i] bytes are written.  One wavefront decodes one
 * stream; streams with n[i] above a built-in threshold go through the single-stream plan
 * instead, one after another (their `path` tells), unless DMX_BATCH_NO_ROUTE is set.
 *
 * Both calls take the context mutex, are ordered against the context's other deflate / inflate
 * work like their single-buffer siblings, and end with one host synchronisation, the read-back
 * of res (routed inflate streams add the single-stream plan's own).  A context with n_gpus > 1
 * runs the batch on its first device. */
typedef struct dmx_batch_result {
    uint64_t bytes;   /* produced bytes; on DMX_ERR_CAPACITY the size that was needed */
    int32_t status;   /* DMX_OK or DMX_ERR_* for this buffer alone */
    uint32_t path;    /* inflate: 6 = batch decoder (one wavefront per stream), else the
                         dmx_stats.path value of the single-stream plan it was routed to;
                         deflate: 0 */
} dmx_batch_result;

/* device-resident: HOST arrays of DEVICE pointers / sizes, `count` entries each */
int dmx_deflate_batch_device(dmx_ctx* ctx, const void* const* d_in, const size_t* n, size_t count,
                             int level, void* const* d_out, const size_t* cap,
                             dmx_batch_result* res, void* stream);
#define DMX_BATCH_NO_ROUTE 1u /* developer A/B: decode every stream on the batch kernel */
int dmx_inflate_batch_device(dmx_ctx* ctx, const void* const* d_in, const size_t* n, size_t count,
                             void* const* d_out, const size_t* cap, dmx_batch_result* res,
                             uint32_t flags, void* stream);
/* host buffers: the same with host pointers (one staged H2D, one D2H) */
int dmx_deflate_batch(dmx_ctx* ctx, const uint8_t* const* in, const size_t* n, size_t count, int level,
                      uint8_t* const* out, const size_t* cap, dmx_batch_result* res);
int dmx_inflate_batch(dmx_ctx* ctx, const uint8_t* const* in, const size_t* n, size_t count,
                      uint8_t* const* out, const size_t* cap, dmx_batch_result* res, uint32_t flags);

/* ---- preset dictionary for the batched calls (zlib's deflateSetDictionary /
 * inflateSetDictionary on raw RFC 1951 streams; not in the reference) -------------------------
 * Small buffers start with an empty window; a dictionary of typical content gives every buffer of
 * the batch history to refer to.  One dictionary per call, shared by all its buffers.  Semantics
 * are zlib's: a stream made with dictionary d decodes exactly when the decoder's window holds the
 * last <= 32768 bytes of d before the stream's first output byte -- libdmx's streams decode with
 * zlib.decompressobj(-15, zdict=d), and zlib's compressobj(level, DEFLATED, -15, zdict=d) streams
 * decode here given d.  No framing carries the dictionary: both sides must be given the same one.
 *
 * dict_len == 0 (a null dictionary is allowed then) is the plain batch call, byte for byte and
 * result for result.  dict_len > 0 with a null dictionary is DMX_ERR_ARG.  Return value and
 * res[i] follow the rules of the batch calls above.
 *
 * Deflate uses the last min(dict_len, 16384) bytes (Du) at levels 2 and 3: the first segment of a
 * buffer then holds 32768 - Du of its bytes (the dictionary shares the matcher's 32 KiB image),
 * the later segments are ordinary, and dmx_deflate_bound(n[i]) still bounds the stream.  Levels 0
 * and 1 have no matcher and ignore the dictionary; their streams are the plain ones and decode
 * with or without it.  Only contexts with segment_bytes = 32768 take a dictionary: any other
 * returns DMX_ERR_ARG when dict_len > 0.
 *
 * Inflate uses the last min(dict_len, 32768) bytes, with any context.  A distance that reaches
 * before the dictionary copies nothing (the stream-start rule of dmx_inflate, moved back by the
 * dictionary).  With dict_len > 0 every stream is decoded by the batch decoder (path 6) whatever
 * its size -- the single-stream plan has no dictionary support -- and DMX_BATCH_NO_ROUTE is
 * accepted and changes nothing.  A wrong dictionary is not detected: the stream decodes to other
 * bytes or ends in DMX_ERR_DATA, as with zlib's raw streams.
 *
 * d_dict: a device pointer with any alignment.  The host forms stage the dictionary with the
 * batch's one H2D copy. */
int dmx_deflate_batch_dict_device(dmx_ctx* ctx, const void* const* d_in, const size_t* n, size_t count,
                                  int level, const void* d_dict, size_t dict_len, void* const* d_out,
                                  const size_t* cap, dmx_batch_result* res, void* stream);
int dmx_inflate_batch_dict_device(dmx_ctx* ctx, const void* const* d_in, const size_t* n, size_t count,
                                  const void* d_dict, size_t dict_len, void* const* d_out,
                                  const size_t* cap, dmx_batch_result* res, uint32_t flags, void* stream);
int dmx_deflate_batch_dict(dmx_ctx* ctx, const uint8_t* const* in, const size_t* n, size_t count, int level,
                           const uint8_t* dict, size_t dict_len, uint8_t* const* out, const size_t* cap,
                           dmx_batch_result* res);
int dmx_inflate_batch_dict(dmx_ctx* ctx, const uint8_t* const* in, const size_t* n, size_t count,
                           const uint8_t* dict, size_t dict_len, uint8_t* const* out, const size_t* cap,
                           dmx_batch_result* res, uint32_t flags);

/* ---- asynchronous batches: device-resident descriptors, no host synchronisation -------------
 * The batch calls above read their pointer / size / capacity arrays on the host and end with a
 * host synchronisation.  These take the five arrays (d_in, d_n, d_out, d_cap, d_res; `count`
 * entries each) in DEVICE memory.  The kernels read them when the work runs, not when the call is
 * made, so they may be written by work queued earlier on `stream` -- a previous kernel's sizes,
 * the bytes of another call's d_res, a ragged tensor -- and results land in d_res on the device.
 *
 * count, max_n, max_total, level, dict_len and flags are host values: they size grids and
 * scratch.  The call takes the context mutex, enqueues everything on `stream` and returns.  When
 * the context's scratch is already large enough -- after a dmx_batch_reserve of at least this
 * shape, or an earlier call of at least this shape -- it makes no host synchronisation, no host
 * read of device memory and no allocation; otherwise it grows the scratch first (which may
 * allocate and synchronise), as the synchronous calls do.
 *
 * Return value: the call as a whole.  DMX_ERR_ARG: a null context, a null array with count > 0,
 * count > 2^31 - 1, a 64 KiB context on the deflate side, dict_len > 0 with a null d_dict, a
 * dictionary at levels 2-3 on a context that is not 32 KiB, an unknown flag, or a max_n beyond
 * 2^31 segments.  DMX_ERR_NOMEM also when the shape's segment table would pass 2^31 - 1 entries
 * (give max_total then).  count == 0 is DMX_OK with nothing enqueued.  The pointers in d_in /
 * d_out are not checked: entry i must be valid for n[i] / cap[i] bytes (the synchronous calls
 * refuse a null pointer with a non-zero size; these cannot see it).
 *
 * Calls on one context are ordered against its other deflate and inflate work, whatever streams
 * they run on, like dmx_deflate_device_async / dmx_inflate_device_async.  dmx_destroy waits for
 * enqueued work.  dmx_last_stats after one of these calls reports `segments` only (deflate: the
 * segment table's capacity; inflate: count) -- the host never learns the byte counts -- and
 * dmx_set_timing does not apply.  A context with n_gpus > 1 runs the call on its first device.
 *
 * Deflate.  max_n bounds every n[i]; max_total bounds their sum (0 = unknown, taken as count *
 * max_n).  For every buffer with n[i] <= max_n, d_out[i] and d_res[i] are byte for byte what
 * dmx_deflate_batch_dict_device writes for the same arrays: the same stream, 03 00 for n[i] == 0,
 * DMX_ERR_CAPACITY with the needed size and nothing written past cap[i].  A buffer with n[i] >
 * max_n gets status DMX_ERR_ARG, bytes 0, nothing written to d_out[i], and does not disturb its
 * neighbours.  The segment table holds min(count * K, ceil(max_total / S) + count) entries, S =
 * the context's segment_bytes, K = the segments of a max_n-byte buffer (first segment S - Du,
 * later ones S; Du as in the dictionary calls above).  If the actual segments exceed that, the
 * buffers from the first one that does not fit onward get DMX_ERR_ARG as above, and the buffers
 * before it are complete and correct.  (With a dictionary a buffer has ceil((n[i] + Du) / S)
 * segments: a max_total of sum(n[i]) + count * Du always fits.)
 *
 * Inflate.  For every stream the batch decoder takes, d_out[i] and d_res[i] equal
 * dmx_inflate_batch_dict_device(..., DMX_BATCH_NO_ROUTE)'s -- all error codes, DMX_CFG_RFC_STRICT
 * and path = 6 included.  A stream with n[i] > max_n gets DMX_ERR_ARG.  Without
 * DMX_BATCH_NO_ROUTE and without a dictionary, a stream above the synchronous call's routing
 * threshold is not decoded (the single-stream plan it would be routed to is host-driven): its
 * result is status DMX_BATCH_DEFERRED, bytes 0, path 0, d_out[i] is untouched, and the caller
 * decodes it with dmx_inflate_device -- the convention of dmx_inflate_device_async's status 1.
 * With DMX_BATCH_NO_ROUTE, or with a dictionary, every stream stays on the batch decoder.
 *
 * Graph capture of these calls has not been tested. */
#define DMX_BATCH_DEFERRED 1   /* per-buffer status of the async inflate: not decoded here, see above */

/* grow the context's scratch for async batches of this shape (may allocate and synchronise) */
int dmx_batch_reserve(dmx_ctx* ctx, size_t count, size_t max_n, size_t max_total, size_t dict_len);

int dmx_deflate_batch_async(dmx_ctx* ctx, const void* const* d_in, const uint64_t* d_n, size_t count,
                            size_t max_n, size_t max_total, int level, const void* d_dict, size_t dict_len,
                            void* const* d_out, const uint64_t* d_cap, dmx_batch_result* d_res, void* stream);
int dmx_inflate_batch_async(dmx_ctx* ctx, const void* const* d_in, const uint64_t* d_n, size_t count,
                            size_t max_n, const void* d_dict, size_t dict_len, void* const* d_out,
                            const uint64_t* d_cap, dmx_batch_result* d_res, uint32_t flags, void* stream);

/* ---- checksums and containers (not in the reference) -------------------
 * The reference's decompressZlib (inflate.hpp:326-361) skips the 2-byte header and ignores the
 * Adler-32 (SURVEY A-9); inflate.hpp's decompressZlib keeps exactly that.  These entry points
 * add what a zlib/gzip user needs on top: framing on the deflate side and a verified inflate,
 * with Adler-32 / CRC-32 computed block-parallel on the GPU (checksum.hip). */

/* zlib's adler32(init, buf, n) / crc32(init, buf, n) of a device buffer (init 1 / 0 to start). */
int dmx_adler32_device(dmx_ctx* ctx, const void* d, size_t n, uint32_t init, uint32_t* out, void* stream);
int dmx_crc32_device(dmx_ctx* ctx, const void* d, size_t n, uint32_t init, uint32_t* out, void* stream);
/* the same for a host buffer (copied to the device first) */
int dmx_adler32(dmx_ctx* ctx, const uint8_t* in, size_t n, uint32_t init, uint32_t* out);
int dmx_crc32(dmx_ctx* ctx, const uint8_t* in, size_t n, uint32_t init, uint32_t* out);

/* Upper bound of a zlib- or gzip-framed stream for n input bytes. */
size_t dmx_framed_bound(size_t n);
/* RFC 1950 zlib stream (CMF 0x78, FLEVEL from the level, Adler-32 trailer) / RFC 1952 gzip
 * member (no name, MTIME 0, OS 255, CRC-32 + ISIZE trailer) around dmx_deflate's raw stream. */
int dmx_deflate_zlib(dmx_ctx* ctx, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap,
                     size_t* out_len);
int dmx_deflate_gzip(dmx_ctx* ctx, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap,
                     size_t* out_len);

/* Check the container trailer against the decoded bytes (DMX_ERR_CHECKSUM on mismatch). */
#define DMX_VERIFY 1u
/* Inflate of a zlib stream (header checked; a container with FDICT set is DMX_ERR_DATA -- the
 * preset-dictionary calls dmx_inflate_batch_dict* take raw streams, not this framing) / a
 * single-member gzip stream (FEXTRA, FNAME, FCOMMENT, FHCRC skipped); the trailer is the last
 * 4 / 8 input bytes.  *out is allocated by the library (dmx_free). */
int dmx_inflate_zlib(dmx_ctx* ctx, const uint8_t* in, size_t n, uint32_t flags, uint8_t** out, size_t* len);
int dmx_inflate_gzip(dmx_ctx* ctx, const uint8_t* in, size_t n, uint32_t flags, uint8_t** out, size_t* len);

/* ---- framed batch calls: zlib / gzip / BGZF around the batched API (not in the reference) ----
 * The batch calls above speak raw RFC 1951; the container calls above take one buffer per call.
 * These frame and un-frame `count` buffers with one set of launches: the batch deflate / inflate
 * unchanged, one launch that computes every buffer's Adler-32 / CRC-32 on the GPU (lengths read
 * from device memory), and small kernels that write the headers and trailers or parse them and
 * apply the verdicts.  Argument conventions, return value, res[i] and the one host
 * synchronisation (plus the routed streams' own) are those of dmx_deflate_batch_device /
 * dmx_inflate_batch_device.  An unknown format or flag is DMX_ERR_ARG.
 *
 * Deflate.  ZLIB / GZIP: buffer i's output is byte for byte what dmx_deflate_zlib /
 * dmx_deflate_gzip writes for it alone on the same context (empty buffers, every level).  BGZF:
 * one gzip member 1f 8b 08 04, MTIME 0, XFL and OS as dmx_deflate_gzip, XLEN 6, 42 43 02 00,
 * BSIZE (member size - 1), the raw stream of dmx_deflate_device, CRC-32, ISIZE; a buffer with
 * n[i] > 65280 gets res[i].status = DMX_ERR_ARG (65280 = htslib's block size; with
 * dmx_deflate_bound(65280) + 26 = 65362 <= 65536 BSIZE always fits).  dmx_batch_framed_bound(format,
 * n[i]) bounds output i.  A short cap[i]: DMX_ERR_CAPACITY, bytes = the framed size needed, nothing
 * written past d_out[i] + cap[i].  A context with segment_bytes = 65536 returns DMX_ERR_ARG.
 *
 * Inflate.  res[i] has the status and bytes dmx_inflate_zlib / dmx_inflate_gzip report for buffer
 * i alone (DMX_BATCH_VERIFY = their DMX_VERIFY): n[i] < 6 / < 18 is DMX_ERR_OVERREAD, a bad
 * header or zlib's FDICT DMX_ERR_DATA; FEXTRA, FNAME, FCOMMENT, FHCRC are skipped; the trailer is
 * the last 4 / 8 bytes of buffer i, so the caller gives each member's extent (one member per
 * buffer).  GZIP accepts BGZF members; BGZF also requires the BC subfield with BSIZE + 1 == n[i]
 * (DMX_ERR_DATA otherwise).  DMX_ERR_CHECKSUM (Adler-32, CRC-32 or ISIZE mismatch under
 * DMX_BATCH_VERIFY): the decoded bytes are in d_out[i] and bytes is their count.
 * DMX_ERR_CAPACITY is the plain batch's -- the first cap[i] bytes, bytes = the full size -- and
 * carries no checksum verdict.  A header error has bytes = 0.  Streams are routed by n[i] as in
 * the plain batch (DMX_BATCH_NO_ROUTE honoured) with the same framing and verification.
 *
 * Not covered: preset dictionaries, files (BGZF files: the dmx_*_bgzf* calls below; a gzip file of
 * several members whose extents are not known: dmx_inflate_gzip_members below), graph capture. */
#define DMX_FRAME_ZLIB 1u   /* RFC 1950 */
#define DMX_FRAME_GZIP 2u   /* RFC 1952, one member per buffer */
#define DMX_FRAME_BGZF 3u   /* gzip member whose FEXTRA holds the BC subfield (BSIZE = member size - 1) */
#define DMX_BATCH_VERIFY 2u /* inflate: check each trailer on the GPU */

/* dmx_deflate_bound(n) + 6 / 18 / 26 for ZLIB / GZIP / BGZF; 0 for an unknown format */
size_t dmx_batch_framed_bound(uint32_t format, size_t n);

int dmx_deflate_batch_framed_device(dmx_ctx* ctx, const void* const* d_in, const size_t* n, size_t count,
                                    int level, uint32_t format, void* const* d_out, const size_t* cap,
                                    dmx_batch_result* res, void* stream);
int dmx_inflate_batch_framed_device(dmx_ctx* ctx, const void* const* d_in, const size_t* n, size_t count,
                                    uint32_t format, void* const* d_out, const size_t* cap,
                                    dmx_batch_result* res, uint32_t flags, void* stream);
/* host buffers */
int dmx_deflate_batch_framed(dmx_ctx* ctx, const uint8_t* const* in, const size_t* n, size_t count, int level,
                             uint32_t format, uint8_t* const* out, const size_t* cap, dmx_batch_result* res);
int dmx_inflate_batch_framed(dmx_ctx* ctx, const uint8_t* const* in, const size_t* n, size_t count,
                             uint32_t format, uint8_t* const* out, const size_t* cap, dmx_batch_result* res,
                             uint32_t flags);

/* BGZF files (the blocked gzip of BAM, VCF, tabix) on host buffers, one framed batch call each.
 * Deflate: members of 65280 input bytes plus the 28-byte empty EOF member (n == 0: that member
 * alone); dmx_bgzf_bound(n) bounds the file; DMX_ERR_CAPACITY sets *out_len to the size needed.
 * Inflate: the member chain is walked on the host by BSIZE, the outputs are laid out by the prefix
 * sum of the members' ISIZE and decoded by one batch call; *out is allocated by the library
 * (dmx_free); flags: DMX_VERIFY.  An empty member (the EOF block) contributes nothing and may be
 * absent.  Errors are the first failing member's, with nothing allocated: DMX_ERR_DATA (bad magic,
 * no BC subfield), DMX_ERR_OVERREAD (the chain runs past n), DMX_ERR_CHECKSUM (a decoded size
 * other than ISIZE, with or without DMX_VERIFY -- the layout rests on it; a CRC-32 mismatch under
 * DMX_VERIFY). */
size_t dmx_bgzf_bound(size_t n);
int dmx_deflate_bgzf(dmx_ctx* ctx, const uint8_t* in, size_t n, int level, uint8_t* out, size_t cap,
                     size_t* out_len);
int dmx_inflate_bgzf(dmx_ctx* ctx, const uint8_t* in, size_t n, uint32_t flags, uint8_t** out, size_t* len);

/* BGZF files in device memory: the same files and results with DEVICE pointers (any alignment),
 * plus the index and the ranged read that BGZF is blocked for.  The member chain is found on the
 * device (candidate scan, links, pointer doubling from offset 0): the host does no per-member work
 * for it.  The calls take the context mutex, are ordered against the context's other deflate /
 * inflate work like their siblings, run on `stream` (NULL: the context's stream) and return after
 * their last host synchronisation.  A null context is DMX_ERR_ARG; a context with n_gpus > 1 runs
 * them on its first device.
 *
 * dmx_deflate_bgzf_device: the file dmx_deflate_bgzf writes for the same bytes, level and context,
 * byte for byte, at d_out; *out_len = its size.  cap below that: DMX_ERR_CAPACITY, *out_len = the
 * size needed, nothing written.  A context with segment_bytes = 65536 returns DMX_ERR_ARG.  Host
 * synchronisations: 2 (the framed batch's results; the file size and status).
 *
 * dmx_bgzf_index_device: the chain walk alone, nothing is decoded and each trailer's ISIZE is
 * trusted.  *members and *plain_bytes (either may be NULL) are set; with entries != NULL,
 * members + 1 entries are written to HOST memory: entry k = member k's start in the file and in
 * the plain bytes, the last one the sentinel {n, plain_bytes}.  entry_cap < members + 1 with
 * entries != NULL: DMX_ERR_CAPACITY with *members set.  The chain's errors are dmx_inflate_bgzf's:
 * DMX_ERR_DATA / DMX_ERR_OVERREAD at the member where the walk from offset 0 stops; n == 0 is
 * DMX_OK with no member.  Host synchronisations: 3 (candidate count; member count, plain bytes and
 * status; the entries) -- 2 without entries.
 *
 * dmx_inflate_bgzf_device: result and bytes of dmx_inflate_bgzf, at d_out; *out_len = the plain
 * bytes.  plain bytes > cap: DMX_ERR_CAPACITY, *out_len = the size needed, nothing is decoded or
 * written (the check precedes every member).  flags: DMX_VERIFY or 0.  On any other error
 * *out_len = 0 and d_out may hold partial output.  Host synchronisations: 3 (candidate count;
 * member count, plain bytes and chain status; the file status).
 *
 * dmx_inflate_bgzf_range_device: bytes [uoffset, uoffset + len) of the plain file, given the
 * index (HOST memory, members + 1 entries as dmx_bgzf_index_device writes them).  Only the members
 * that overlap the range are decoded: whole members straight into d_out, the at most two edge
 * members into context scratch, from which their slice is copied.  Exactly len bytes are written.
 * uoffset + len beyond index[members].uoffset, index[members].coffset beyond n or an index that
 * is not monotone: DMX_ERR_ARG.  len == 0: DMX_OK, nothing launched.  Verification (DMX_VERIFY)
 * and the ISIZE rule cover the touched members only.  Host synchronisations: 1.
 *
 * Not covered: preset dictionaries, graph capture; the host forms above do not go through these
 * calls yet.  (Multi-member gzip without BSIZE: dmx_inflate_gzip_members below.) */
typedef struct dmx_bgzf_entry {
    uint64_t coffset; /* the member's first byte in the BGZF file   */
    uint64_t uoffset; /* its first byte in the plain (inflated) file */
} dmx_bgzf_entry;
int dmx_deflate_bgzf_device(dmx_ctx* ctx, const void* d_in, size_t n, int level, void* d_out, size_t cap,
                            size_t* out_len, void* stream);
int dmx_bgzf_index_device(dmx_ctx* ctx, const void* d_in, size_t n, dmx_bgzf_entry* entries, size_t entry_cap,
                          size_t* members, uint64_t* plain_bytes, void* stream);
int dmx_inflate_bgzf_device(dmx_ctx* ctx, const void* d_in, size_t n, uint32_t flags, void* d_out, size_t cap,
                            size_t* out_len, void* stream);
int dmx_inflate_bgzf_range_device(dmx_ctx* ctx, const void* d_in, size_t n, const dmx_bgzf_entry* index,
                                  size_t members, uint64_t uoffset, size_t len, uint32_t flags, void* d_out,
                                  void* stream);

/* ---- multi-member gzip files (RFC 1952 2.2; not in the reference) --------------------------------
 * A gzip FILE is a series of members back to back: `cat a.gz b.gz`, a log that gzip appended to, a
 * WARC archive with one member per record, a .gz padded with zeros to a block size.
 * dmx_inflate_gzip and DMX_FRAME_GZIP take one member whose extent the caller knows; these calls take
 * the file.  Python's gzip.decompress is the model: a member must start at offset 0; behind each
 * member's 8-byte trailer zero bytes are skipped, then the file ends or the next header begins.
 * Header checks are dmx_inflate_gzip's (magic, CM = 8; FEXTRA, FNAME, FCOMMENT, FHCRC skipped).
 *
 * Nothing in a header says where a member ends, so the device finds out: every offset where
 * 1f 8b 08 starts a header that parses is a candidate, every candidate's stream is measured by one
 * wavefront that decodes it without keeping the bytes (over at most 1 MiB of input, the batch
 * calls' routing threshold), the host walks the chain over those records, and the members on it
 * are decoded by one framed batch inflate -- each small member is decoded twice.  A member whose
 * stream is longer than the measuring limit goes to the single-stream plan of dmx_inflate_device
 * instead, one call each, decoded once unless the bytes 1f 8b 08 of a false candidate lie in it
 * behind the limit (then once more per such candidate).
 *
 * dmx_inflate_gzip_members_device: DEVICE pointers, any alignment.  The members' plain bytes are
 * written back to back at d_out, *out_len = their sum, *members (may be NULL) = the members.  With
 * entries != NULL, members + 1 entries are written to HOST memory, the table dmx_bgzf_index_device
 * writes: entry k = {member k's first header byte, the plain bytes before it}, the last one the
 * sentinel {n, *out_len}.  (Padding may follow a member, so an entry does not give the member's end:
 * no ranged read goes through this table.)  flags: DMX_VERIFY or 0.
 *   n == 0: DMX_OK, no member, no bytes.
 *   DMX_ERR_ARG: a null context or out_len, d_in == NULL with n > 0, d_out == NULL with cap > 0, an
 *     unknown flag -- checked before any device work.
 *   The status is the first failing member's, in file order.  Where a header is expected at offset
 *     p (0, or the first non-zero byte behind a trailer) with r bytes left: DMX_ERR_DATA when
 *     in[p] != 1f, or r >= 2 and in[p + 1] != 8b, or r >= 3 and in[p + 2] != 8; DMX_ERR_OVERREAD
 *     when the header, or the header plus an 8-byte trailer, does not fit in r.  Then
 *     DMX_ERR_OVERREAD when the member's stream or trailer runs past n, DMX_ERR_DATA on a stream
 *     that cannot be decoded, and under DMX_VERIFY DMX_ERR_CHECKSUM on a CRC-32 mismatch or an
 *     ISIZE that is not the member's plain size mod 2^32.  Decoding keeps the context's leniency
 *     (DMX_CFG_RFC_STRICT honoured), as the batch decoder does.  On these errors *out_len = 0,
 *     *members = the members in front of the failure, and d_out may hold partial output.
 *   DMX_ERR_CAPACITY:
 *     entry_cap < members + 1 with entries != NULL: *members set, *out_len = 0, d_out unspecified.
 *     The output does not fit cap and every member is within the measuring limit: *out_len = the
 *       exact size needed, nothing is written (the check precedes the decode).
 *     A member beyond the measuring limit does not fit what is left of cap: *out_len = 0 (its size
 *       is not known); earlier bytes of d_out are unspecified.  (Where long members fit and later
 *       small ones do not, *out_len is the exact size and the long members' bytes are in d_out.)
 *   Nothing is written outside [d_out, d_out + cap) and nothing is read outside [d_in, d_in + n),
 *   but for the aligned loads that share a 16-byte line with a byte of the file.
 * Host synchronisations: the candidate count; the candidates' records; the gap check, when bytes
 * lie between or behind members; the batch's status; and per long member those of
 * dmx_inflate_device plus, under DMX_VERIFY, its checksum.
 *
 * dmx_inflate_gzip_members: host buffers, the same statuses; the file is staged with one copy to
 * the device, the device form runs there, the bytes are copied back.
 *
 * The calls take the context mutex, are ordered against the context's other deflate / inflate work
 * like dmx_inflate_bgzf_device, run on `stream` (NULL: the context's stream; the host form always
 * there) and return after their last host synchronisation.  A context with n_gpus > 1 runs them on
 * its first device.
 *
 * Not covered: ranged reads through the table, writing multi-member files (BGZF does that), preset
 * dictionaries, graph capture. */
int dmx_inflate_gzip_members_device(dmx_ctx* ctx, const void* d_in, size_t n, uint32_t flags, void* d_out,
                                    size_t cap, dmx_bgzf_entry* entries, size_t entry_cap, size_t* members,
                                    size_t* out_len, void* stream);
int dmx_inflate_gzip_members(dmx_ctx* ctx, const uint8_t* in, size_t n, uint32_t flags, uint8_t* out, size_t cap,
                             size_t* members, size_t* out_len);

/* ---- ZIP archives (PKWARE APPNOTE, ZIP64 included; not in the reference) ---------------------------
 * A ZIP archive is many independent raw RFC 1951 streams (method 8) and stored byte runs (method 0)
 * plus a central directory that states every entry's extent, plain size and CRC-32: .npz files,
 * torch.save checkpoints, wheels, jars, docx / xlsx, zipped dataset shards.  Nothing has to be
 * discovered and nothing is decoded twice.  Python's zipfile is the model for what parses.
 *
 * The directory is read on the device.  One workgroup searches the last 65557 bytes for the end
 * record: the highest p where 50 4b 05 06 stands and p + 22 + comment length <= n.  Where the ZIP64
 * locator (50 4b 06 07) stands at p - 20 and the ZIP64 end record (50 4b 06 06) directly in front of
 * it, that record gives the entry count, the directory's size and its offset.  Bytes in front of the
 * archive (a self-extractor's stub) shift every stated offset by base = end record position -
 * directory size - directory offset, less 76 with the ZIP64 records, as zipfile does.  The central
 * directory is a chain of variable-length records (46 bytes plus name, extra and comment); it is
 * walked like the BGZF member chain: every offset of the directory region where 50 4b 01 02 starts a
 * record that fits the region is a candidate, a candidate links to the one that starts where it
 * ends, pointer doubling from the candidate at the region's first byte ranks the records.  A false
 * signature inside a name, an extra field or a comment is never counted.  The walk must end exactly
 * at the region's end after as many records as the end record states (zipfile ignores the count;
 * these calls do not: 0xFFFF without a ZIP64 record is a count of 65535).  One thread per record
 * then decodes its fields -- a ZIP64 extra 0x0001 supplies usize, csize and the local header's
 * offset, in that order, for exactly the fields that read 0xFFFFFFFF -- and reads the local header
 * for the data offset.  Sizes and CRC always come from the central directory, never from the local
 * header, so a data descriptor (flag bit 3) needs nothing.  The local header's name is not compared
 * with the central one.
 *
 * Per-entry status (dmx_zip_entry.status; never the return value):
 *   DMX_ERR_ARG       flag bit 0 (encrypted), or a method other than 0 and 8
 *   DMX_ERR_DATA      no 50 4b 03 04 at base + local header offset; a stored entry with
 *                     csize != usize; a corrupt extra field
 *   DMX_ERR_OVERREAD  the local header, or data_off + csize, passes n
 *
 * dmx_zip_index_device: the directory only, nothing is decoded.  DEVICE pointer d_in, any alignment.
 * *count and *plain_bytes (either may be NULL) are set; with entries != NULL, *count entries are
 * written to HOST memory in directory order.
 *   DMX_ERR_ARG: a null context, d_in == NULL with n > 0 -- checked before any device work.
 *   DMX_ERR_DATA: n < 22 (n == 0 included), no end record, a disk number other than 0 or more than
 *     one disk, a negative base, a chain that does not start at the directory's first byte or does
 *     not end at its end, a count that differs from the end record's, more than 2^63 plain bytes.
 *   DMX_ERR_NOMEM: a directory of 2^32 - 2 candidates or more (links are 32-bit), or no memory.
 *   DMX_ERR_CAPACITY: entry_cap < *count with entries != NULL; *count and *plain_bytes are set.
 * Host synchronisations: 3 (the end record; the candidate count; status, plain bytes and the
 * entries) -- 1 for an archive without entries.
 *
 * dmx_zip_extract_device: the entries sel[0 .. nsel) of `entries` (HOST arrays; sel == NULL: all
 * `count` entries in order, nsel is ignored) into d_out.  Duplicates are allowed, each with its own
 * slot; an index >= count is DMX_ERR_ARG.  The layout is the exclusive prefix sum of usize in
 * selection order; a failing entry still owns its slot, whose bytes are unspecified.  res: a HOST
 * array of one dmx_batch_result per selected entry (bytes = usize on DMX_OK; path = 6 for the batch
 * decoder, the single-stream plan's path for a deflated entry above the batch calls' routing
 * threshold of 1 MiB compressed, 0 for a stored entry).  A bad entry never disturbs its neighbours.
 * *out_len = the layout's size.  flags: DMX_VERIFY or 0.
 *   The sum of usize above cap: DMX_ERR_CAPACITY, *out_len = the size needed, nothing is written
 *     (the check precedes every decode); a sum beyond 2^63: DMX_ERR_DATA.
 *   The entries are the caller's and so untrusted again: an entry whose status is not DMX_OK keeps
 *     it, flags and method are classified again, data_off + csize > n is that entry's
 *     DMX_ERR_OVERREAD.  No entry causes a read outside [d_in, d_in + n) -- but for the aligned loads
 *     that share a 16-byte line with a byte of the archive -- or a write outside its slot.
 *   A decoded size other than usize, or a stream that does not fit its slot, is that entry's
 *     DMX_ERR_CHECKSUM with or without DMX_VERIFY: the layout rests on usize (the BGZF ISIZE rule).
 *     Under DMX_VERIFY a CRC-32 of the output that differs from the directory's is
 *     DMX_ERR_CHECKSUM too.  Stream errors are the batch decoder's (DMX_ERR_DATA, DMX_ERR_OVERREAD).
 * Host synchronisations: 1, the read-back of res (nsel == 0: none); every entry above the routing
 * threshold adds those of dmx_inflate_device (deflated) or none (stored: one device-to-device copy)
 * plus, under DMX_VERIFY, its checksum's.
 *
 * dmx_inflate_zip_device: index plus extract-all in one call; the descriptors are built from the
 * table the index left on the device.  entries (HOST memory, entry_cap of them; required) receive
 * *count entries with status and path as the extraction left them.  The return value covers the
 * archive (the index's errors; DMX_ERR_CAPACITY for entry_cap < *count, *count set, or for plain
 * bytes > cap, *out_len = the size needed, nothing decoded); per-entry failures are in
 * entries[k].status only.  Host synchronisations: the index's 3 plus the extraction's.
 *
 * dmx_zip_index / dmx_inflate_zip: the same on host buffers; the archive is staged with one copy to
 * the device, the device form runs there, the bytes are copied back with one copy.
 *
 * The calls take the context mutex, are ordered against the context's other deflate / inflate work
 * like dmx_inflate_bgzf_device, run on `stream` (NULL: the context's stream; the host forms always
 * there) and return after their last host synchronisation.  A context with n_gpus > 1 runs them on
 * its first device.
 *
 * Not covered: encryption, methods other than 0 and 8, multi-disk archives, a ZIP64 end record
 * with extensible data (it is looked for directly in front of its locator), comparing local with
 * central names, graph capture.  (Writing archives: the dmx_zip_write calls below.) */
typedef struct dmx_zip_entry {      /* 64 bytes */
    uint64_t name_off;   /* the name's first byte in the archive (inside the central directory) */
    uint64_t data_off;   /* the entry's first data byte */
    uint64_t csize, usize;
    uint64_t uoffset;    /* its first byte in a full extraction: prefix sum of usize */
    uint32_t crc;
    uint32_t dostime;    /* time | date << 16 */
    uint16_t name_len, method, gpflags, reserved;
    int32_t  status;     /* DMX_OK, or why this entry cannot be extracted */
    uint32_t path;       /* after extraction: 6, the single-stream path, 0 for stored */
} dmx_zip_entry;
int dmx_zip_index_device(dmx_ctx* ctx, const void* d_in, size_t n, dmx_zip_entry* entries, size_t entry_cap,
                         size_t* count, uint64_t* plain_bytes, void* stream);
int dmx_zip_extract_device(dmx_ctx* ctx, const void* d_in, size_t n, const dmx_zip_entry* entries, size_t count,
                           const size_t* sel, size_t nsel, uint32_t flags, void* d_out, size_t cap,
                           dmx_batch_result* res, size_t* out_len, void* stream);
int dmx_inflate_zip_device(dmx_ctx* ctx, const void* d_in, size_t n, uint32_t flags, void* d_out, size_t cap,
                           dmx_zip_entry* entries, size_t entry_cap, size_t* count, size_t* out_len, void* stream);
int dmx_zip_index(dmx_ctx* ctx, const uint8_t* in, size_t n, dmx_zip_entry* entries, size_t entry_cap,
                  size_t* count, uint64_t* plain_bytes);
int dmx_inflate_zip(dmx_ctx* ctx, const uint8_t* in, size_t n, uint32_t flags, uint8_t* out, size_t cap,
                    dmx_zip_entry* entries, size_t entry_cap, size_t* count, size_t* out_len);

/* ---- ZIP archives: writing (not in the reference) ------------------------------------------------
 * The inverse of the calls above for buffers that already sit in device memory: .npz files,
 * checkpoints, zipped dataset shards.  Entry k is written with method 8 (its payload is exactly the
 * raw stream dmx_deflate_batch_device writes for that buffer at that level) or method 0 (stored).
 * Sizes and CRC-32 are known before a header is written, so flag bit 3 is never set and there is no
 * data descriptor; flag bit 11 (UTF-8) is set iff the name holds a byte above 127.  The layout, in
 * archive order: per entry the local header (30 bytes, the name, and a ZIP64 extra 0x0001 of 16
 * bytes {usize, csize} when DMX_ZIP_FORCE64 is given or either size is >= 0xFFFFFFFF: both 32-bit
 * fields then read 0xFFFFFFFF and "version needed" is 45, else 20) and the payload; the central
 * directory (46 bytes and the name per entry, the extra 0x0001 with usize and csize under the same
 * rule, then the local header's offset when DMX_ZIP_FORCE64 is given or it is >= 0xFFFFFFFF;
 * external attributes 0x10 for a name that ends in '/', else 0); the ZIP64 end record (56 bytes)
 * and its locator (20 bytes) when DMX_ZIP_FORCE64 is given, or there are 65535 entries or more, or
 * the directory's size or offset is >= 0xFFFFFFFF -- the classic record then reads 0xFFFF, 0xFFFF,
 * 0xFFFFFFFF and 0xFFFFFFFF; the 22-byte end record and the archive comment.  The archive is a
 * pure function of the arguments: dostime 0 is written as 1980-01-01 00:00:00 (0x00210000).
 * Python's zipfile reads it (testzip() is None); without entries and without a comment it is the
 * 22 bytes zipfile writes.
 *
 * dmx_zip_bound: the archive's size with every deflated payload at dmx_deflate_bound of its n (no
 *   device work, no checks); an archive of these sources is never longer.
 * dmx_zip_write_device: src is a HOST array; data are DEVICE pointers of any alignment, d_out a
 *   DEVICE pointer of any alignment.  One upload carries the sources, the names and the comment;
 *   one batch deflate compresses the method 8 entries into context scratch; one checksum launch
 *   gives every plain input's CRC-32; the layout is two prefix sums on the device; one launch then
 *   moves every payload byte once, from its scratch slot or the caller's plain input to its final
 *   place -- in chunks of 64 KiB, so one large entry spreads over the device -- and writes the
 *   records.  *out_len = the archive's bytes.  entries (HOST memory, `count` rows, may be NULL)
 *   receive the table dmx_zip_index_device reads back from the written archive (status 0, path 0).
 *     DMX_ERR_ARG, before any device work and with nothing written: a null context, src == NULL
 *       with count > 0, out_len == NULL, d_out == NULL with cap > 0, data == NULL with n > 0, a
 *       method other than 0 and 8, name == NULL, name_len 0 or above 65535, a comment above 65535
 *       bytes or NULL with comment_len > 0, flags other than DMX_ZIP_FORCE64, 2^31 entries or
 *       more, a context whose segment_bytes is 65536 (as every batch deflate call).
 *     DMX_ERR_CAPACITY: the archive does not fit cap; *out_len = the size needed, nothing is
 *       written to d_out.  A deflate that fails returns its status, nothing is written either.
 *   Host synchronisations: 2 -- the batch deflate's read-back (none when no entry is method 8) and
 *   the read-back of the status, the size and the table.  count == 0: 1.
 * dmx_zip_write: the same on host buffers (data: HOST pointers): the plain inputs are staged with
 *   one copy to the device, the device form runs there, the archive is copied back with one copy.
 *
 * The calls take the context mutex, are ordered against the context's other deflate / inflate work
 * like dmx_deflate_bgzf_device, run on `stream` (NULL: the context's stream; the host form always
 * there) and return after their last host synchronisation.
 *
 * Not covered: falling back to method 0 when deflate does not shrink an entry, entry comments and
 * extras other than 0x0001, encryption, appending to an existing archive, graph capture. */
typedef struct dmx_zip_source {   /* one entry to write; HOST array; 40 bytes */
    const void* data;     /* DEVICE pointer (device form) / host pointer (host form); may be NULL when n == 0 */
    uint64_t    n;
    const char* name;     /* HOST bytes, not NUL-terminated */
    uint32_t    name_len; /* 1..65535, above that DMX_ERR_ARG */
    uint16_t    method;   /* 0 stored, 8 deflated */
    uint16_t    reserved; /* 0 */
    uint32_t    dostime;  /* time | date << 16; 0 means 1980-01-01 00:00:00 (0x00210000) */
} dmx_zip_source;
#define DMX_ZIP_FORCE64 1u  /* ZIP64 extras and end records whatever the sizes */
size_t dmx_zip_bound(const dmx_zip_source* src, size_t count, size_t comment_len, uint32_t flags);
int dmx_zip_write_device(dmx_ctx* ctx, const dmx_zip_source* src, size_t count, int level, uint32_t flags,
                         const void* comment, size_t comment_len, void* d_out, size_t cap, dmx_zip_entry* entries,
                         size_t* out_len, void* stream);
int dmx_zip_write(dmx_ctx* ctx, const dmx_zip_source* src, size_t count, int level, uint32_t flags,
                  const void* comment, size_t comment_len, uint8_t* out, size_t cap, dmx_zip_entry* entries,
                  size_t* out_len);

/* ---- seek index and ranged reads for unblocked streams (zran's idea; not in the reference) -----
 * BGZF is blocked for random access; an ordinary zlib / gzip / pigz stream and libdmx's own output
 * are not.  These calls build a zran-style index while a stream is decoded once -- checkpoints at
 * block headers, each with the 32 KiB of plain bytes before it -- and then read any range by
 * decoding only from the checkpoint before it.  Raw RFC 1951 streams: the caller passes the
 * stream inside a zlib or gzip file, and every `bit` is relative to that pointer.  The calls take
 * the context mutex, are ordered against the context's other deflate / inflate work like their
 * siblings, run on `stream` (NULL: the context's stream) and return after their last host
 * synchronisation.  A null context is DMX_ERR_ARG.
 *
 * dmx_inflate_index_device: dmx_inflate_device plus the index.  Bytes, *out_len, error codes and
 * the DMX_ERR_CAPACITY behaviour are dmx_inflate_device's; no index is promised on error (*count =
 * 0).  spacing: the least number of plain bytes between two checkpoints; below 32768 is
 * DMX_ERR_ARG.  *count = the checkpoints; count + 1 entries are written to HOST memory, entry 0 =
 * {0, 0, 0, DMX_SEEK_NOWINDOW} always, the last one the sentinel {8 * the stream's end byte, plain
 * bytes, 0, 0}.  entry_cap < count + 1 or windows_cap < count * 32768: DMX_ERR_CAPACITY with *count
 * set; the decoded bytes in d_out are valid.  Window slot k is d_windows + k * 32768 (device
 * memory, any alignment; 16-byte aligned is faster) and holds plain bytes [uoffset - 32768,
 * uoffset) for the entries without DMX_SEEK_NOWINDOW; the other slots are not written.
 * dmx_seek_windows_bound(cap, spacing) = (cap / spacing + 2) * 32768 bounds count * 32768 for any
 * stream of at most cap plain bytes: 12.5 % of cap at a spacing of 256 KiB.
 * Where the checkpoints come from: the block-parallel decoder (dmx_stats.path 5; zlib's, pigz's,
 * libdeflate's streams) gives the block headers its units start at; the lane decoder (path 4,
 * libdmx's own streams) gives the segment starts, all DMX_SEEK_NOWINDOW.  Of those, one is kept
 * when it is at least `spacing` plain bytes past the last kept one.  Every other path (the serial
 * decoder, the workgroup decoders) gives count = 1, entry 0 alone: correct but degenerate -- a
 * ranged read then decodes from the stream's start.  So does a stream that is one huge block:
 * there are no checkpoints inside a block.
 * Host synchronisations: those of dmx_inflate_device, plus 1 when window slots are written (the
 * gather kernel's completion) and 1 on path 4's uniform layout (the segment records).
 *
 * dmx_inflate_range_device: exactly plain bytes [uoffset, uoffset + len) at d_out (any alignment;
 * nothing is written past d_out + len), given the index (HOST memory, count + 1 entries as above)
 * and its windows.  Entry k covers [uoffset_k, uoffset_{k+1}); one wavefront per touched entry
 * starts at its bit behind its window and stops after its byte count, all in one launch.
 * len == 0: DMX_OK, nothing launched.  DMX_ERR_ARG: uoffset + len beyond the sentinel's uoffset,
 * the sentinel's bit beyond 8 * n, entries not strictly increasing in uoffset (the sentinel may
 * equal the last entry), an entry without DMX_SEEK_NOWINDOW whose window is not 32768.  Every entry
 * is looked at on every call (count steps on the host); only the uoffset order and the windows are
 * validated.  The entries' `bit` values are not: one that is not a block header of this stream, or
 * lies beyond 8 * n, ends in the decoded status of the span that starts there (DMX_ERR_DATA or
 * DMX_ERR_OVERREAD), never in a read outside [d_in, d_in + n) or a write outside [d_out, d_out +
 * len).  Otherwise the status is the first failing entry's: DMX_ERR_OVERREAD when it runs past n, DMX_ERR_DATA on an
 * undecodable code or when the final block ends before the byte count (the index does not belong
 * to the stream); d_out may then hold partial output.  DMX_CFG_RFC_STRICT and the lenient cases are
 * those of the batch decoder; a distance that reaches before the window copies nothing.
 * Host synchronisations: 1.  dmx_last_stats after it: segments = the spans decoded, in_bytes = n,
 * out_bytes = len (0 on error), path = 0 (no single-stream path ran).
 *
 * Not covered: checkpoints inside a block, containers, checksums of ranges, host-buffer forms,
 * graph capture, streams whose plain bytes do not fit the device. */
#define DMX_SEEK_WINDOW   32768u
#define DMX_SEEK_NOWINDOW 1u   /* entry flag: nothing before this point is referenced (libdmx segment start, or offset 0) */
typedef struct dmx_seek_entry {
    uint64_t bit;      /* stream bit of a block header (BFINAL bit), relative to d_in */
    uint64_t uoffset;  /* plain bytes before it */
    uint32_t window;   /* valid bytes in this entry's window slot: 0 or 32768 */
    uint32_t flags;    /* DMX_SEEK_* */
} dmx_seek_entry;      /* 24 bytes */

size_t dmx_seek_windows_bound(size_t cap, size_t spacing);   /* (cap / spacing + 2) * 32768; 0 for spacing < 32768 */

int dmx_inflate_index_device(dmx_ctx* ctx, const void* d_in, size_t n, void* d_out, size_t cap,
                             size_t spacing, dmx_seek_entry* entries, size_t entry_cap,
                             void* d_windows, size_t windows_cap,
                             size_t* count, size_t* out_len, void* stream);

int dmx_inflate_range_device(dmx_ctx* ctx, const void* d_in, size_t n,
                             const dmx_seek_entry* entries, size_t count,
                             const void* d_windows, uint64_t uoffset, size_t len,
                             void* d_out, void* stream);

/* ---- instrumentation -------------------------------------------------------------------- */
typedef struct dmx_stats {
    double ms_main_kernel;  /* HIP-event time of the dominant kernel of the last call       */
    double ms_device_total; /* HIP-event time of all device work of the last call          */
    uint64_t segments;      /* segments (deflate) / candidate segments (inflate)            */
    uint64_t in_bytes;
    uint64_t out_bytes;
    uint32_t path;          /* inflate: 0 = segment-parallel (speculative offsets),
                               1 = segment-parallel (look-back offsets), 2 = serial path,
                               3 = workgroup-per-segment decoder (32 KiB slots),
                               4 = lane decoder + wave resolve (the default for libdmx
                                   streams: one lane decodes a segment's tokens, one
                                   wavefront rebuilds its bytes; dense segments of streams
                                   with few of them go to the workgroup decoder instead),
                               5 = block-parallel decoder for streams without segment
                                   markers (zlib's, libdeflate's, the reference's own):
                                   header scan, one wavefront per unit of blocks, window
                                   hand-off,
                               6 = batch decoder, one wavefront per stream (reported in
                                   dmx_batch_result.path only; dmx_stats.path never holds it) */
    uint32_t shards;        /* host-buffer API with n_gpus > 1: the pieces the call was split
                               into (0 or 1: one device)                                       */
} dmx_stats;

/* Enable (1) / disable (0) per-call HIP-event timing on a context (off by default). */
int dmx_set_timing(dmx_ctx* ctx, int enable);
int dmx_last_stats(dmx_ctx* ctx, dmx_stats* st);

/* ---- synthetic corpora, bytes [offset, offset + n) --------------- */
#define DMX_CORPUS_ZEROS 0
#define DMX_CORPUS_REPEAT 1
#define DMX_CORPUS_RANDOM 2
#define DMX_CORPUS_TEXT 3
#define DMX_CORPUS_MIXED 4
#define DMX_CORPUS_BMP 5
int dmx_corpus_generate(int kind, uint64_t offset, size_t n, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* DMX_H */
