// cand_scan.h -- the candidate scan of the formats whose records are found in device memory (BGZF
// members: bgzf_chain.hip, gzip members: gzip_members.hip, ZIP central records: zip_dir.hip).
//
// A region reg[0, len) is cut into tiles of kScanTile bytes of its 16-byte aligned view.  One
// workgroup stages a tile in LDS and tests every offset of it: the FORMAT F says by four bytes
// whether an offset can start a record (magic) and then by the record itself (candidate).  Per-tile
// counts, launch_scan_u32, then the candidates in offset order; the list is sized by the count,
// which the host reads in between, so a payload of fake headers cannot overflow it.
//
//   struct F {                       // carries what its predicate reads (in, n / in, d0, d1)
//       using Cand = ...;            // a 16-byte record
//       static constexpr uint32_t kMinBytes = ...;   // no record is shorter
//       bool magic(uint32_t word) const;             // the four bytes at an offset, little-endian
//       bool candidate(uint64_t off, Cand* c) const; // off: relative to reg
//   };
//
// The first part is plain C++ (DMX_HD as in container_parse.h; tests/cpp/bgzf_chain_test.cpp checks
// the ragged-end rule); the kernels follow under hipcc.  Each format's .hip instantiates them in
// its own translation unit.
//
// Every store is a plain vector store.  The staging is the only code of these paths that loads
// outside [reg, reg + len) on purpose: its 16-byte loads start at the 16-byte boundary below reg,
// every one shares its line with a byte of the region, and the bytes outside are zeroed.
#pragma once
#include "container_parse.h"

namespace dmx {

constexpr uint32_t kScanThreads = 256;
constexpr uint32_t kScanTile = kScanThreads * 16;  // staged bytes per workgroup (16 per thread)

// tiles of the scan over reg[0, len) (0 for len == 0); the tile counts are as many words, the tile
// offsets scan_words(tiles) entries
DMX_HD inline uint64_t scan_tiles(const uint8_t* reg, uint64_t len) {
    return len ? (((uintptr_t)reg & 15) + len + kScanTile - 1) / kScanTile : 0;
}

// The ragged-end rule.  The region is [lead, vend) of its aligned view (lead = reg & 15); q is a
// line of it, a multiple of 16.  A line inside the region is staged as it is ...
DMX_HD inline bool scan_line_inside(uint64_t q, uint64_t lead, uint64_t vend) { return q >= lead && q + 16 <= vend; }
// ... and of any other one the bytes that lie in the region: byte b of m[k] is 0xFF for the line's
// byte 4 * k + b inside [lead, vend), else 0
DMX_HD inline void scan_line_mask(uint64_t q, uint64_t lead, uint64_t vend, uint32_t m[4]) {
    for (int k = 0; k < 4; k++) {
        m[k] = 0;
        for (int b = 0; b < 4; b++) {
            const uint64_t p = q + 4 * k + b;
            if (p >= lead && p < vend) m[k] |= 0xFFu << (8 * b);
        }
    }
}

}  // namespace dmx

#if defined(__HIPCC__)
#include "dmx_device.h"
#include "dmx_internal.h"

namespace dmx {

// Stages tile `tile` of the aligned view (plus 16 bytes of the next tile) and tests this thread's
// 16 offsets: bit j of the result = a candidate starts at aligned position tile * kScanTile +
// 16 * t + j.  The magic comes from the staged bytes; the predicate reads the region itself, past
// the tile's edge where the record goes there.  Ends past a barrier; lds holds kScanTile / 4 + 4
// words.
template <class F>
__device__ __forceinline__ uint32_t scan_tile_mask(const F& f, const uint8_t* reg, uint64_t len, uint64_t tile,
                                                   uint32_t* lds) {
    const uint32_t t = threadIdx.x;
    const uint64_t lead = (uintptr_t)reg & 15, vend = lead + len;
    const uint8_t* vbase = reg - lead;
    // (an aligned 16-byte load at q < vend shares its 16-byte line with a byte of the region)
    auto load = [&](uint64_t q, uint32_t* dst) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (q < vend) v = *reinterpret_cast<const uint4*>(vbase + q);
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
        if (!scan_line_inside(q, lead, vend)) {
            uint32_t m[4];
            scan_line_mask(q, lead, vend, m);
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] &= m[k];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) dst[k] = w[k];
    };
    const uint64_t p0 = tile * kScanTile + 16ull * t;
    load(p0, lds + 4 * t);
    if (t == 0) load(tile * kScanTile + kScanTile, lds + kScanTile / 4);
    __syncthreads();
    uint32_t w[5];
#pragma unroll
    for (int k = 0; k < 5; k++) w[k] = lds[4 * t + k];
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t word = __builtin_amdgcn_alignbyte(w[(j >> 2) + 1], w[j >> 2], j & 3);
        const uint64_t p = p0 + j;
        if (f.magic(word) && p >= lead && p + F::kMinBytes <= vend) {  // (fewer than kMinBytes: no record)
            typename F::Cand c;
            if (f.candidate(p - lead, &c)) mask |= 1u << j;
        }
    }
    __syncthreads();
    return mask;
}

// the workgroup's exclusive scan of `v` (result) and its sum (*total); sm holds kScanThreads / 64 words
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* sm, uint32_t* total) {
    const uint32_t t = threadIdx.x;
    const uint32_t inc = wave_incl_scan(v);
    if ((t & 63) == 63) sm[t >> 6] = inc;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanThreads / 64; k++) {
        if (k < (t >> 6)) before += sm[k];
        sum += sm[k];
    }
    *total = sum;
    return before + inc - v;
}

template <class F>
__global__ __launch_bounds__(kScanThreads) void k_scan_count(F f, const uint8_t* reg, uint64_t len,
                                                             uint32_t* tile_counts) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kScanTile / 4 + 4];
    __shared__ uint32_t sm[kScanThreads / 64];
    const uint32_t mask = scan_tile_mask(f, reg, len, blockIdx.x, lds);
    uint32_t total;
    (void)block_scan(__popc(mask), sm, &total);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// cands holds ncand entries (the count the host read): nothing is written past them
template <class F>
__global__ __launch_bounds__(kScanThreads) void k_scan_list(F f, const uint8_t* reg, uint64_t len,
                                                            const uint64_t* tile_offs, typename F::Cand* cands,
                                                            uint64_t ncand) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kScanTile / 4 + 4];
    __shared__ uint32_t sm[kScanThreads / 64];
    uint32_t mask = scan_tile_mask(f, reg, len, blockIdx.x, lds);
    uint32_t total;
    uint64_t at = tile_offs[blockIdx.x] + block_scan(__popc(mask), sm, &total);
    const uint64_t lead = (uintptr_t)reg & 15;
    const uint64_t p0 = (uint64_t)blockIdx.x * kScanTile + 16ull * threadIdx.x;
    while (mask) {
        const int j = __ffs(mask) - 1;
        mask &= mask - 1;
        typename F::Cand c;
        if (f.candidate(p0 + j - lead, &c) && at < ncand) cands[at] = c;
        at++;
    }
}

// *ncand = the offsets of reg[0, len) where a candidate starts (len > 0; len == 0: nothing is launched)
template <class F>
hipError_t launch_scan_count(const F& f, const uint8_t* reg, uint64_t len, uint32_t* tile_counts, uint64_t* tile_offs,
                             uint64_t* ncand, hipStream_t st) {
    const uint64_t nt = scan_tiles(reg, len);
    if (!nt) return hipSuccess;
    hipLaunchKernelGGL(k_scan_count<F>, dim3((uint32_t)nt), dim3(kScanThreads), 0, st, f, reg, len, tile_counts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_u32(tile_counts, tile_offs, nt, ncand, st);
}

// the candidates in offset order, for the ncand the host read back
template <class F>
hipError_t launch_scan_list(const F& f, const uint8_t* reg, uint64_t len, const uint64_t* tile_offs,
                            typename F::Cand* cands, uint64_t ncand, hipStream_t st) {
    if (!ncand) return hipSuccess;
    hipLaunchKernelGGL(k_scan_list<F>, dim3((uint32_t)scan_tiles(reg, len)), dim3(kScanThreads), 0, st, f, reg, len,
                       tile_offs, cands, ncand);
    return hipGetLastError();
}

}  // namespace dmx
#endif
