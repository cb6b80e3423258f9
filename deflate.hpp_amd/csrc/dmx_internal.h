// dmx_internal.h -- kernel launch interfaces shared by the host runtime and the .hip files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dmx.h"
#include "container_parse.h"  // FrameHead, parse_frame (plain C++, shared with the CPU test)
#include "bgzf_chain.h"       // BgzfCand and the chain steps (plain C++, shared with the CPU test)
#include "batch_table.h"      // the batch tables' records and build steps (plain C++, shared with the CPU test)
#include "deflate_pipe.h"     // the chunk pipeline's chunk arithmetic (plain C++, shared with the CPU test)
#include "inflate_records.h"  // SegRecord, FbUnit, SEGF_*, FB_* (plain C++, shared with inflate_plan)
#include "seek_plan.h"        // SeekSpan, SeekSpanHead, SeekSlot and the seek planners (plain C++, shared with the CPU test)
#include "gzip_members.h"     // GzmCand, GzmRec and the member walk (plain C++, shared with the CPU test)
#include "zip_dir.h"          // ZipHead and the ZIP directory's steps (plain C++, shared with the CPU test)
#include "zip_write.h"        // ZipwSrc, ZipwHead and the ZIP writer's records and steps (plain C++, shared with the CPU test)

namespace dmx {

// (DeflateBatchSeg, DF_BATCH_LAST and InflateBatchDesc: batch_table.h)
constexpr uint32_t kDeflateDictMax = 16384;  // dictionary bytes the deflate side uses (the last ones)
constexpr uint32_t kInflateDictMax = 32768;  // ... and the inflate side: the DEFLATE window
// Compressed bytes above which one wavefront is the wrong tool for a stream: the batch inflate
// routes such a stream to the single-stream plan (host_batch.cpp, where the measurements behind the
// number are), and the multi-member gzip call measures a member over at most this many bytes.
constexpr size_t kBatchRouteBytes = 1u << 20;

struct DeflateArgs {
    const uint8_t* in;
    uint64_t n;
    uint64_t nseg;
    int level;
    int final_last;       // set BFINAL on the last segment
    uint8_t* slots;       // nseg * slot_bytes scratch: each segment's bitstream
    uint32_t slot_bytes;
    uint32_t* tok;        // nseg * tok_stride words: the front kernel's token words (levels 2-3)
    uint32_t tok_stride;  // words per segment (a multiple of 4), deflate_tok_stride(segment bytes)
    uint32_t* ntok;       // nseg token word counts
    uint32_t* sizes;      // nseg
    uint64_t* offsets;    // nseg
    uint64_t* total;      // 1
    uint8_t* out;
    uint64_t cap;
    uint64_t* dbg;        // optional per-block phase timestamps (DMX_PHASES), else nullptr
    // batch (dmx_deflate_batch_device): the segments come from a table that spans several
    // buffers instead of from in / n; nullptr otherwise
    const DeflateBatchSeg* btab = nullptr;  // nseg entries
    const uint64_t* bfirst = nullptr;     // nbuf + 1: first segment of each buffer (bfirst[nbuf] = nseg)
    uint8_t* const* bout = nullptr;       // nbuf output pointers
    const uint64_t* bcap = nullptr;       // nbuf capacities
    ::dmx_batch_result* bres = nullptr;  // nbuf results, written by k_compact_batch
    uint64_t nbuf = 0;
};
// What the batch kernels take (the BATCH instantiations and k_compact_batch): DeflateArgs and,
// for dmx_deflate_batch_async, the segment count on the device (<= nseg, which is then the
// table's capacity the grids are sized for; nullptr: nseg is the count) and the buffers that get
// DMX_ERR_ARG and no output (nullptr: none).  A type of its own: the single-stream kernels'
// argument block, and with it their code, stays as it is.
struct DeflateBatchArgs : DeflateArgs {
    const uint64_t* nseg_dev = nullptr;
    const uint8_t* bflag = nullptr;
};
// What the chunk pipeline's kernels take: DeflateArgs and the chunk's segment range (front
// segments for the front kernel, emission segments for the emission kernel).  nseg stays the
// call's segment count: the last segment of the stream is still seg + 1 == nseg.
struct DeflatePipeArgs : DeflateArgs {
    uint64_t seg_first = 0, seg_end = 0;
};
// The chunk pipeline of one call (deflate_pipe.h): chunks of `chunk` segments, the front kernel
// on the caller's stream, each chunk's emission on `side` behind `ev_chunk` (the last chunk's on
// the caller's stream), and the caller's stream behind the side stream's emissions through `ev_side`.
struct DeflatePipe {
    uint64_t chunk;
    hipStream_t side;
    hipEvent_t ev_chunk, ev_side;
};

// Token words per segment of the front kernel: a literal word covers 1-3 input bytes, a match
// word at least 3, so at most seg / 2 words (one literal between every two 3-byte matches), plus
// one partial literal word per thread's token range (1024 threads).  The remaining 224 words are
// slack that nothing writes; they stay so that the token buffers' addresses and sizes do not move.
constexpr uint32_t deflate_tok_stride(uint32_t seg) { return seg / 2 + 1248; }
static_assert(deflate_tok_stride(32768) == 17632 && deflate_tok_stride(16384) == 9440,
              "the token buffers' layout is fixed");

// dict: the batch's segment table carries a preset dictionary (32 KiB segments, levels 2-3)
// nseg_dev / bflag: a batch's device-side segment count and flagged buffers (DeflateBatchArgs);
// the caller has zeroed A.sizes[0 .. A.nseg) then
// pipe: the chunk pipeline (single stream, levels 2-3, 32 or 64 KiB segments, no DMX_PHASES)
hipError_t launch_deflate(const DeflateArgs& A, uint32_t seg_bytes, hipStream_t st, hipEvent_t ev0,
                          hipEvent_t ev1, bool dict = false, const uint64_t* nseg_dev = nullptr,
                          const uint8_t* bflag = nullptr, const DeflatePipe* pipe = nullptr,
                          uint64_t* total_host = nullptr);
// the front kernel's persistent workgroups that fit the GPU at once: workgroup b takes the
// segments b, b + grid, ... with grid = min(segments, this)
uint64_t deflate_front_fit(uint32_t seg_bytes);

// InflateArgs::flags bit (internal): the stream is a piece of a larger stream (multi-GPU
// scatter): a back-reference before its first byte is an error, not the stream-start no-op.
constexpr uint32_t DMX_IFLAG_PIECE = 1u << 31;

struct InflateArgs {
    const uint32_t* in_words;  // 4-byte aligned base at or below the stream start
    uint64_t misalign;         // stream start = in_words bytes + misalign
    uint64_t n;                // stream bytes
    const uint64_t* cands;     // candidate segment starts (bytes, relative to stream)
    uint64_t ncand;
    uint8_t* out;
    uint64_t cap;
    SegRecord* recs;
    unsigned long long* status;  // ncand look-back words (zeroed)
    unsigned int* ticket;        // zeroed
    uint32_t flags;              // DMX_CFG_RFC_STRICT, DMX_IFLAG_PIECE
    uint32_t mode;               // 0 = speculative uniform segment sizes, 1 = decoupled look-back,
                                 // 2 = k_inflate_pj (segment j at j * slot),
                                 // 3 = k_inflate_segments redoing only SEGF_EXOTIC candidates
                                 //     of a mode-2 / mode-4 pass, at the same slots,
                                 // 4 = k_inflate_lanes + k_inflate_resolve (segment j at j * slot),
                                 // 6 = k_inflate_pj_list patching the heavy candidates of mode 4
    uint32_t slot;               // mode 2: segment bytes (16384 or 32768)
    uint64_t* dbg;               // optional per-segment phase timestamps (DMX_PHASES)
    // dmx_inflate_device_async: the candidate count lives on the device (<= ncand, which is then
    // the capacity the grids are sized for); nullptr: ncand is the count
    const uint64_t* ncand_dev = nullptr;
};
// the candidate count a kernel works on
__device__ __forceinline__ uint64_t cand_count(const InflateArgs& A) {
    return A.ncand_dev ? (*A.ncand_dev < A.ncand ? *A.ncand_dev : A.ncand) : A.ncand;
}

constexpr int kPhaseSlots = 16;
#define DMX_PHASE(dbg, idx, slot)                                                   \
    do {                                                                            \
        if ((dbg) && threadIdx.x == 0) (dbg)[(idx) * kPhaseSlots + (slot)] = __builtin_amdgcn_s_memtime(); \
    } while (0)

// result of validation / serial decode, copied to the host
struct InflateResult {
    uint64_t total;   // decoded bytes
    int32_t status;   // fast path: 0 ok, 1 re-run with look-back, 2 serial; serial: 0 / DMX_ERR_*
    uint32_t fin_index;
    uint64_t exotic;  // candidates flagged SEGF_EXOTIC by the pass
    uint64_t end_byte;  // status 0: the stream byte just past the final block (relative to the stream)
    uint64_t cycles[12];  // serial decoder (DMX_FB_DEBUG): s_memtime per phase -- decode, walk,
                         // offsets, literals + copies, flush + refill, steps
};

// zero_w / zero_hl (each or nullptr): validation words and the heavy list's two counters that
// block 0 zeroes, for the kernels that follow in the same call
struct ValidateWords;
hipError_t launch_marker_count(const uint32_t* in_words, uint64_t misalign, uint64_t n,
                               uint32_t* tile_counts, uint64_t ntiles, hipStream_t st,
                               ValidateWords* zero_w = nullptr, uint32_t* zero_hl = nullptr);
// cands holds cand_cap entries: candidates past them are not written (the async inflate sizes
// its scratch before the count is known)
hipError_t launch_marker_write(const uint32_t* in_words, uint64_t misalign, uint64_t n,
                               const uint64_t* tile_offs, uint64_t ntiles, uint64_t* cands,
                               uint64_t cand_cap, hipStream_t st);
// dmx_inflate_device_async: *ncand = min(nmarkers + 1, ...) on the device; the result words
// {decoded bytes, status} from the validation (status 0: decoded; 1: needs the general path)
hipError_t launch_async_prep(const uint64_t* nmarkers, uint64_t* ncand, hipStream_t st);
hipError_t launch_async_result(const InflateResult* res, const uint64_t* ncand, uint64_t cand_cap, uint64_t cap,
                               uint64_t* d_result, hipStream_t st);
uint64_t marker_tiles(uint64_t n, uint64_t misalign);
// exclusive scan of n values into offs (64-bit) and *total; offs must hold scan_words(n)
// entries (the block sums of the multi-workgroup scan follow the n offsets)
uint64_t scan_words(uint64_t n);
// total_host: host-mapped memory that receives the total too (the host reads it after its wait);
// count_dev: a device word that receives total + 1 (a marker scan's candidate count)
hipError_t launch_scan_u32(const uint32_t* v, uint64_t* offs, uint64_t n, uint64_t* total,
                           hipStream_t st, uint64_t* total_host = nullptr, uint64_t* count_dev = nullptr);
hipError_t launch_inflate_segments(const InflateArgs& A, hipStream_t st, hipEvent_t ev0,
                                   hipEvent_t ev1);
// workgroup-per-segment decoder (lane-parallel Huffman decode + pointer-jumping LZ77);
// segment j lands at j * 32768 (mode 2)
hipError_t launch_inflate_pj(const InflateArgs& A, uint32_t seg, hipStream_t st, hipEvent_t ev0,
                             hipEvent_t ev1);
// lane-per-segment Huffman decode (k_inflate_lanes) + wave-per-segment LZ77 resolve
// (k_inflate_resolve); segment j lands at j * A.slot (mode 4).  tok holds
// min(ncand * 16404, 8 * n + 20 * ncand) words; tokoff ncand + 1, ntok / caps ncand entries.
// heavy != 0: when at most `limit` candidates span more than `heavy` bytes (counted on the
// device into hl[1]), those are declined and listed in hl (hl[0] = count, the indices from
// hl[2] on; ncand + 2 words) for launch_inflate_pj_list.  hl_zeroed: hl[0..1] are zero already
// (launch_marker_count), no fill is launched.
// split: ncand words when A.slot is 64 KiB (the halves' split), else unused; ncu: the device's
// compute units (the grid of the one-wave resolve)
hipError_t launch_inflate_lanes(const InflateArgs& A, uint32_t* tok, uint64_t* tokoff,
                                uint32_t* ntok, uint32_t* caps, uint32_t heavy, uint32_t limit,
                                uint32_t* hl, uint32_t* split, int ncu, hipStream_t st, hipEvent_t ev0,
                                hipEvent_t ev1, bool hl_zeroed = false);
// mode 6: the workgroup decoder over the candidates listed in hl, `grid` persistent workgroups
hipError_t launch_inflate_pj_list(const InflateArgs& A, uint32_t seg, const uint32_t* hl, uint32_t grid,
                                  hipStream_t st, hipEvent_t ev1);
// validation scratch: five device words, zeroed by the launch (zeroed: an earlier kernel of the
// call has done that, launch_marker_count); res_host: host-mapped memory that receives the
// result too, or nullptr
struct ValidateWords {
    unsigned long long kmin, bmin, umin, xmin, xcnt;
};
hipError_t launch_inflate_validate(const InflateArgs& A, ValidateWords* W, InflateResult* res,
                                   hipStream_t st, bool zeroed = false, InflateResult* res_host = nullptr);

// block-parallel inflate of arbitrary streams (inflate_blocks.hip, path 5; FbUnit and the unit
// stops and code states: inflate_records.h)
uint64_t fb_scan_chunks(uint64_t n);
uint32_t fb_hits_per_chunk();
// header scan of every bit offset: counts[nchunks], hits[nchunks * fb_hits_per_chunk()],
// offs = exclusive scan of counts, *nhits = total
hipError_t launch_fb_scan(const uint32_t* in_words, uint64_t misalign, uint64_t n,
                          uint32_t* counts, uint64_t* hits, uint64_t* offs, uint64_t* nhits,
                          hipStream_t st);
// compacts the scan's candidates into one sorted list of count entries and runs the full header
// test on them (k_fb_check): a candidate that fails it gets FB_HIT_REJECT.  *pcount: the
// candidates (device), max_count: the most there can be (sizes the grids).  keep (host memory
// mapped into the device, or nullptr): the accepted starts, unordered, *nkeep of them (entries
// past keep_cap dropped).  ph: DMX_FB_DEBUG counters (or nullptr)
hipError_t launch_fb_compact(const uint32_t* in_words, uint64_t misalign, uint64_t n, const uint32_t* counts,
                             const uint64_t* offs, const uint64_t* hits, uint64_t nchunks, uint64_t* list,
                             const uint64_t* pcount, uint64_t max_count, unsigned long long* ph, uint64_t* keep,
                             uint32_t* nkeep, uint32_t keep_cap, hipStream_t st);
// hits carry bit 62 for a stored-block header; stops[u] = the next dynamic-header start after u
// units [u0, u0 + count) of the nunits listed; vmode / vhdr as above
// fixed-code regions (k_fb_smap + k_fb_swalk): reg = nreg x {E, T, first super block}, sbreg =
// the region of each of the nsb super blocks, J = nsb * fb_region_nodes() words, visit = nsb
// words (the node the path enters each super block at, ~0 = none: region chunk << 6 | f << 5 |
// offset, chunks of fb_region_chunk_bits()), rstat = nreg words (FB_REGION_END / _LINK / other)
uint64_t fb_region_super_bits();
uint64_t fb_region_chunk_bits();
uint32_t fb_region_nodes();
// Jraw (nsb * fb_region_nodes() words): the chunk maps before pointer jumping; cbit: the stream
// bit where the true path enters each chunk and sub-chunk (~0: not entered), k_fb_schunks
hipError_t launch_fb_regions(const uint32_t* in_words, uint64_t misalign, uint64_t n, const uint64_t* reg,
                             uint32_t nreg, const uint32_t* sbreg, uint64_t nsb, uint32_t* J, uint32_t* visit,
                             uint32_t* rstat, uint32_t* Jraw, uint64_t* Jsub, uint64_t* cbit, hipStream_t st);
// (Jsub: nsb * fb_region_nodes() 64-bit words; cbit: nsb * fb_region_entries() words)
uint32_t fb_region_entries();
hipError_t launch_fb_decode(const uint32_t* in_words, uint64_t misalign, uint64_t n,
                            const uint64_t* starts, const uint64_t* stops, const uint8_t* vmode,
                            const uint64_t* vhdr, uint64_t nunits, uint64_t u0, uint64_t count,
                            const uint64_t* tokoff, uint32_t* tok, FbUnit* units, uint32_t flags,
                            bool parallel, uint32_t* stats, const uint64_t* cbit, const uint32_t* ucb,
                            hipStream_t st);
// (cbit / ucb: the region units' exact chunk entries, see FbDecodeArgs; nullptr when none)
// replay + window hand-off + final resolve; *err (zeroed by the caller) becomes nonzero when a
// copy reaches before the stream start.  win (fb_window_entries(nchain) words, 0 = not
// available) and open (fb_window_rounds(nchain) words): the parallel hand-off; win == nullptr:
// the serial one (k_fb_tails).  workgroup: the workgroup replay k_fb_units (pieces in LDS),
// else the one-wave replay k_fb_replay
uint64_t fb_window_entries(uint64_t nchain);
uint32_t fb_window_rounds(uint64_t nchain);
hipError_t launch_fb_resolve(const uint8_t* stream, const uint64_t* starts, const uint32_t* chain,
                             const uint64_t* offs, const uint64_t* sizes, uint64_t nchain,
                             const uint64_t* tokoff, const uint32_t* tok, const FbUnit* units,
                             uint16_t* img, uint64_t total, uint8_t* out, uint32_t* err,
                             uint32_t* win, uint32_t* open, bool workgroup, unsigned long long* ph,
                             hipStream_t st);
// checksums (checksum.hip): scratch of checksum_scratch_bytes(n) bytes; results land in device
// memory (*d_out).  CRC-32: the zero-start register; crc32_finish applies start value and xor.
uint64_t checksum_scratch_bytes(uint64_t n);
hipError_t launch_adler32(const uint8_t* d, uint64_t n, uint32_t init, void* scratch, uint32_t* d_out,
                          hipStream_t st);
hipError_t launch_crc32_raw(const uint8_t* d, uint64_t n, void* scratch, uint32_t* d_out, hipStream_t st);
uint32_t crc32_finish(uint32_t raw, uint64_t n, uint32_t init);

hipError_t launch_place_segments(const uint8_t* src, uint32_t slot, const uint64_t* chain, const uint64_t* offs,
                                 const uint32_t* sizes, uint64_t nch, uint8_t* dst, hipStream_t st);
hipError_t launch_segment_check(const InflateArgs& A, const uint64_t* starts, uint64_t k, uint64_t* ends,
                                hipStream_t st);
hipError_t launch_inflate_serial(const InflateArgs& A, int count_only, InflateResult* res,
                                 hipStream_t st);

// batch inflate (inflate_batch.hip): one wavefront per stream on a persistent grid.  order
// lists the norder streams to decode (indices into desc / res), longest first; workgroups draw
// positions of it from *ticket (zeroed by the launch).  flags: DMX_CFG_RFC_STRICT.
// launch_inflate_batch_dict: dict holds the preset dictionary's last dl bytes, 0 < dl <=
// kInflateDictMax (device memory, any alignment), which every stream's window holds before its
// first byte.
// norder_dev (dmx_inflate_batch_async): the list's length lives on the device (<= norder, which
// is then the capacity the grid is sized for); nullptr: norder is the length.
hipError_t launch_inflate_batch(const InflateBatchDesc* desc, const uint32_t* order, uint64_t norder,
                                ::dmx_batch_result* res, unsigned int* ticket, uint32_t flags, hipStream_t st,
                                const uint32_t* norder_dev = nullptr);
hipError_t launch_inflate_batch_dict(const InflateBatchDesc* desc, const uint32_t* order, uint64_t norder,
                                     ::dmx_batch_result* res, unsigned int* ticket, uint32_t flags,
                                     const uint8_t* dict, uint32_t dl, hipStream_t st,
                                     const uint32_t* norder_dev = nullptr);

// seek index (inflate_span.hip; the plans: seek_plan.h).
// launch_inflate_spans: one wavefront per span on a persistent grid; span k starts at its bit of
// the stream behind window slot spans[k].slot of `windows` and writes its bytes from `skip` on to
// out + spans[k].out_off.  *head: {ticket 0, key all ones} from the caller; key ends as the minimum
// of k << 32 | (uint32_t)status over the failing spans.  flags: DMX_CFG_RFC_STRICT.
hipError_t launch_inflate_spans(const uint32_t* in_words, uint64_t misalign, uint64_t n, const SeekSpan* spans,
                                uint32_t nspans, const uint8_t* windows, uint8_t* out, SeekSpanHead* head,
                                uint32_t flags, hipStream_t st);
// window slot list[b].slot of `windows` = out[list[b].uoffset - 32768, list[b].uoffset)
hipError_t launch_seek_gather(const uint8_t* out, const SeekSlot* list, uint64_t nlist, uint8_t* windows,
                              hipStream_t st);

// Batch tables from device-resident descriptor arrays (batch_table.hip; the steps: batch_table.h).
// launch_batch_segtab: the deflate's segment table for `count` buffers and a capacity of `cap`
// entries, cap >= 1: counts (count words) and bfirst (scan_words(count) entries) are scratch and
// the first-segment list; tab holds cap entries, flag count bytes; *nseg = the segments the batch
// kernels work on.  dtail: the dictionary's last du bytes (du == 0: none).
hipError_t launch_batch_segtab(const uint8_t* const* in, const uint64_t* n, uint64_t count, uint64_t max_n,
                               uint64_t cap, uint32_t seg, uint32_t du, const uint8_t* dtail, uint32_t* counts,
                               uint64_t* bfirst, DeflateBatchSeg* tab, uint8_t* flag, uint64_t* nseg,
                               hipStream_t st);
// launch_batch_desc: desc[i] = {in[i], n[i], out[i], cap[i]}; order = the streams the batch kernel
// keeps, longest class first, *norder of them; a stream above max_n gets DMX_ERR_ARG and one above
// route_bytes (0: no routing) with an output buffer DMX_BATCH_DEFERRED in res.  work: 2 *
// kBatchClasses words (the class histogram and the scatter's cursors), zeroed by the launch.
hipError_t launch_batch_desc(const uint8_t* const* in, const uint64_t* n, uint8_t* const* out, const uint64_t* cap,
                             uint64_t count, uint64_t max_n, uint64_t route_bytes, InflateBatchDesc* desc,
                             uint32_t* order, uint32_t* norder, uint32_t* work, ::dmx_batch_result* res,
                             hipStream_t st);


// framed batch calls (checksum.hip, frame_batch.hip; FrameHead and the parse: container_parse.h).
// side holds one FrameHead per buffer.
// launch_checksum_batch: side[k].ck = the Adler-32 (crc false) / CRC-32 of every buffer in one
// launch.  res == nullptr: buffer k is desc[k].in, desc[k].n bytes (the deflate's plain input);
// else desc[k].out with the length in res[k].bytes, for the buffers whose res[k].status and
// side[k].status are DMX_OK (the inflate's output).  *ticket is zeroed by the launch.
hipError_t launch_checksum_batch(const InflateBatchDesc* desc, const ::dmx_batch_result* res, FrameHead* side,
                                 uint64_t count, bool crc, unsigned int* ticket, hipStream_t st);
// inflate, before the decode: parses buffer k's header into side[k] and narrows desc[k] to the raw
// stream (a header error leaves desc[k].n = 0: nothing is decoded)
hipError_t launch_frame_parse(InflateBatchDesc* desc, FrameHead* side, uint64_t count, uint32_t format,
                              hipStream_t st);
// inflate, after the decode and the checksums: header errors and (verify) trailer verdicts into res
hipError_t launch_frame_verdict(const FrameHead* side, ::dmx_batch_result* res, uint64_t count, uint32_t format,
                                bool verify, hipStream_t st);
// deflate, after the batch deflate wrote the raw streams at desc[k].out + head: headers, trailers
// (side[k].ck) and the framed res[k]; desc[k] = {plain input, its size, framed output, its capacity}
hipError_t launch_frame_write(const InflateBatchDesc* desc, const FrameHead* side, ::dmx_batch_result* res,
                              uint64_t count, uint32_t format, int level, hipStream_t st);

// BGZF files in device memory (bgzf_chain.hip; the steps: bgzf_chain.h).
struct BgzfChainHead {
    uint64_t members;  // chain: members before the walk stops; launch_bgzf_pack: the file's bytes
    uint64_t total;    // chain: plain bytes (the sum of ISIZE); launch_bgzf_pack: the members' bytes
    int32_t status;    // chain: DMX_OK or where the serial walk stops; pack: DMX_OK, DMX_ERR_CAPACITY
                       // or the first failing member's status
    uint32_t pad_;
};
// The candidate scans (launch_bgzf_count, launch_gzm_count, launch_zip_count) are cand_scan.h's:
// tile_counts holds scan_tiles(region) words, tile_offs scan_words(tiles) entries.
// *ncand = the offsets of in[0, n) where bgzf_next succeeds (n > 0)
hipError_t launch_bgzf_count(const uint8_t* in, uint64_t n, uint32_t* tile_counts, uint64_t* tile_offs,
                             uint64_t* ncand, hipStream_t st);
// The jump tables of a chain of records [off, off + size) that must end at `end`: J = bgzf_levels(ncand)
// * ncand words, level 0 by bgzf_link, each further one by bgzf_double (BGZF members, ZIP central records)
hipError_t launch_chain_links(const BgzfCand* cands, uint64_t ncand, uint64_t end, uint32_t* J, hipStream_t st);
// The member table for the ncand the host read back: rows[r] (r < head->members) in chain order,
// uoff = the exclusive prefix sum of their ISIZE, *head.  cands / rows / isz: ncand entries, J:
// bgzf_levels(ncand) * ncand words, uoff: scan_words(ncand) entries.  ncand == 0 (and n == 0):
// only *head is written.
hipError_t launch_bgzf_chain(const uint8_t* in, uint64_t n, const uint64_t* tile_offs, uint64_t ncand,
                             BgzfCand* cands, uint32_t* J, BgzfCand* rows, uint32_t* isz, uint64_t* uoff,
                             BgzfChainHead* head, hipStream_t st);
// entries[0 .. members]: member starts in both coordinate systems and the sentinel {n, *total}
hipError_t launch_bgzf_entries(const BgzfCand* rows, const uint64_t* uoff, uint64_t members, uint64_t n,
                               const uint64_t* total, ::dmx_bgzf_entry* entries, hipStream_t st);
// desc[k] = {in + coff, size, out + uoff, isize}, order[k] = k: the arrays of the framed batch inflate
hipError_t launch_bgzf_desc(const uint8_t* in, const BgzfCand* rows, const uint64_t* uoff, uint64_t members,
                            uint8_t* out, InflateBatchDesc* desc, uint32_t* order, hipStream_t st);
// ranged read over the index slice idx[0 .. count] (device copy): members inside the plain range
// [u0, u1) decode into out, the first / last one into edge when they stick out; launch_bgzf_range_copy
// moves their slices to out after the decode
hipError_t launch_bgzf_range_desc(const uint8_t* in, const ::dmx_bgzf_entry* idx, uint64_t count, uint64_t u0,
                                  uint64_t u1, uint8_t* out, uint8_t* edge, InflateBatchDesc* desc, uint32_t* order,
                                  hipStream_t st);
hipError_t launch_bgzf_range_copy(const ::dmx_bgzf_entry* idx, uint64_t count, uint64_t u0, uint64_t u1,
                                  const uint8_t* edge, uint8_t* out, hipStream_t st);
// *key (preset to all ones by the caller) = min over the members whose result is not DMX_OK of
// index << 32 | (uint32_t)status.  DMX_ERR_CAPACITY or a decoded size other than desc[k].cap is
// mismatch_status: DMX_ERR_CHECKSUM for BGZF (dmx_inflate_bgzf's mapping; cap is ISIZE),
// DMX_ERR_INTERNAL for multi-member gzip (cap is the size the measuring pass found)
hipError_t launch_member_status(const ::dmx_batch_result* res, const InflateBatchDesc* desc, uint64_t members,
                                int mismatch_status, unsigned long long* key, hipStream_t st);
// deflate: member i (res[i].bytes at slots + i * stride) to out + the prefix sum, then the EOF
// member; *head as above.  Nothing is written to out unless every member is DMX_OK and the file
// fits cap.  sizes: count words, offs: scan_words(count) entries, *key preset to all ones.
hipError_t launch_bgzf_pack(const uint8_t* slots, uint64_t stride, const ::dmx_batch_result* res, uint64_t count,
                            uint32_t* sizes, uint64_t* offs, unsigned long long* key, uint8_t* out, uint64_t cap,
                            BgzfChainHead* head, hipStream_t st);


// multi-member gzip files in device memory (gzip_members.hip; the walk: gzip_members.h).
// a tile's bytes of the candidate scan
uint32_t gzm_tile_bytes();
// *ncand = the offsets of in[0, n) where 1f 8b 08 starts a header that gzip_head_len accepts (n > 0)
hipError_t launch_gzm_count(const uint8_t* in, uint64_t n, uint32_t* tile_counts, uint64_t* tile_offs,
                            uint64_t* ncand, hipStream_t st);
// the candidates in offset order, for the ncand the host read back
hipError_t launch_gzm_write(const uint8_t* in, uint64_t n, const uint64_t* tile_offs, GzmCand* cands,
                            uint64_t ncand, hipStream_t st);
// recs[k] = candidate k's stream measured over at most `limit` bytes, one wavefront per candidate
// on a persistent grid (*ticket is zeroed by the launch).  flags: DMX_CFG_RFC_STRICT.  *occupancy
// (or nullptr): the workgroups per compute unit the runtime reported for the kernel.
hipError_t launch_gzm_measure(const uint8_t* in, uint64_t n, const GzmCand* cands, uint64_t ncand, GzmRec* recs,
                              unsigned int* ticket, uint32_t flags, uint64_t limit, hipStream_t st,
                              int* occupancy = nullptr);
// res[0] = the least offset of a non-zero byte in the ngaps ranges (device memory, file order;
// longest: the longest range's bytes), all ones when there is none; res[1] = the status of a gzip
// header at that offset.  forced != all ones: the ranges are not looked at, res = {forced, the
// status of a header there}.  *flag: a scratch word.
hipError_t launch_gzm_gaps(const uint8_t* in, uint64_t n, const GzmGap* gaps, uint64_t ngaps, uint64_t longest,
                           uint64_t forced, unsigned long long* flag, uint64_t* res, hipStream_t st);

// ZIP archives in device memory (zip_dir.hip; the steps: zip_dir.h).
// *head = the end record of in[0, n), n >= 22: directory region, count, base; status DMX_ERR_DATA
// where there is none or it spans disks
hipError_t launch_zip_tail(const uint8_t* in, uint64_t n, ZipHead* head, hipStream_t st);
// *ncand = the offsets of h's directory region where a central record starts (h.dir_size > 0)
hipError_t launch_zip_count(const uint8_t* in, const ZipHead& h, uint32_t* tile_counts, uint64_t* tile_offs,
                            uint64_t* ncand, hipStream_t st);
// The entry table for the ncand the host read back, 0 < ncand and h.count <= ncand: *head = h with
// the chain's status and the plain bytes, ents[r] (r < h.count) in directory order when the status
// is DMX_OK.  cands: ncand entries, J: bgzf_levels(ncand) * ncand words, ents / lo / hi: h.count
// entries, off_lo / off_hi: scan_words(h.count) entries each, totals: 2 words.
hipError_t launch_zip_chain(const uint8_t* in, uint64_t n, const ZipHead& h, const uint64_t* tile_offs, uint64_t ncand,
                            BgzfCand* cands, uint32_t* J, ::dmx_zip_entry* ents, uint32_t* lo, uint32_t* hi,
                            uint64_t* off_lo, uint64_t* off_hi, uint64_t* totals, ZipHead* head, hipStream_t st);
// Extraction of ents[0, count) (device memory; uoffset = the entry's slot in out), count > 0:
// kind[k] = zip_job's verdict, desc[k] = {in + data_off, csize, out + slot, usize}, res[k] = the
// result of an entry that is not extracted (a job of the host's: DMX_BATCH_DEFERRED), side[k]
// zeroed, order = the ZIP_JOB_BATCH entries, longest class first.  work: 2 * kBatchClasses words.
hipError_t launch_zip_jobs(const ::dmx_zip_entry* ents, uint64_t count, const uint8_t* in, uint64_t n, uint8_t* out,
                           uint64_t route_bytes, InflateBatchDesc* desc, ::dmx_batch_result* res, FrameHead* side,
                           uint32_t* kind, uint32_t* order, uint32_t* work, hipStream_t st);
// the ZIP_JOB_COPY entries' bytes and results {csize, DMX_OK, 0}, one workgroup per entry
hipError_t launch_zip_copy(const InflateBatchDesc* desc, const uint32_t* kind, uint64_t count,
                           ::dmx_batch_result* res, hipStream_t st);
// res[k].status of the decoded and the copied entries by zip_verdict (side[k].ck: the output's CRC-32)
hipError_t launch_zip_verdict(const ::dmx_zip_entry* ents, const uint32_t* kind, const FrameHead* side, uint64_t count,
                              bool verify, ::dmx_batch_result* res, hipStream_t st);

// ZIP archives written in device memory (zip_write.hip; the records and the steps: zip_write.h).
// The layout of `count` > 0 entries: src[k] and desc[k] = {plain input, n, payload source, -} as
// uploaded, res = the batch deflate's results over the method 8 entries.  csize / loff: count
// entries, lo / hi / cbytes: count words, off_lo / off_hi / coff: scan_words(count) entries each,
// totals: 3 words (the local records' low and high halves, the directory), *key preset to all ones.
hipError_t launch_zipw_layout(const ZipwSrc* src, const InflateBatchDesc* desc, const ::dmx_batch_result* res,
                              uint64_t count, bool force64, uint64_t* csize, uint32_t* lo, uint32_t* hi,
                              uint64_t* off_lo, uint64_t* off_hi, uint64_t* loff, uint32_t* cbytes, uint64_t* coff,
                              uint64_t* totals, unsigned long long* key, hipStream_t st);
// Behind the layout and launch_checksum_batch (side[k].ck = the CRC-32 of plain input k): the
// payloads, the records, the comment, *head and the written table rows[0, count).  first: the
// exclusive prefix sum of zipw_chunk_bound over the entries' payload bounds, nchunks = first[count]
// < 2^31 - 1.  Nothing is written to out unless every entry is DMX_OK and the archive fits cap.
hipError_t launch_zipw_pack(const ZipwSrc* src, const InflateBatchDesc* desc, const FrameHead* side,
                            const uint8_t* names, const uint8_t* comment, uint32_t comment_len, const uint64_t* first,
                            uint64_t count, uint64_t nchunks, const uint64_t* csize, const uint64_t* loff,
                            const uint64_t* coff, const uint64_t* totals, const unsigned long long* key, bool force64,
                            uint8_t* out, uint64_t cap, ZipwHead* head, ::dmx_zip_entry* rows, hipStream_t st);

}  // namespace dmx
