// bgzf_chain.hip -- BGZF files in device memory (gfx950): the member chain found in parallel, the
// descriptors of the framed batch inflate built from it, the file status, and the compaction of
// the framed batch deflate's member slots into one file.
//
// A BGZF file is a linked list through 16-bit BSIZE fields.  The steps are bgzf_chain.h's (plain
// C++, run serially by tests/cpp/bgzf_chain_test.cpp):
//   k_bgzf_count / k_bgzf_list   every offset that starts with 1f 8b 08 + FEXTRA is tested with
//                                bgzf_next; per-tile counts, launch_scan_u32, then the candidates
//                                in offset order.  The list is sized by the count, which the host
//                                reads in between: a payload of fake headers cannot overflow it.
//   k_bgzf_link                  successor = the candidate at off + size (binary search)
//   k_bgzf_double                level k -> level k + 1, once per level
//   k_bgzf_head                  one thread: members reachable from offset 0, chain status
//   k_bgzf_rank                  member r = r hops from candidate 0, along the bits of r
//   launch_scan_u32              uoff = exclusive prefix sum of ISIZE, total plain bytes
// False candidates inside payloads take part in the links and the doubling, but only what is
// reachable from candidate 0 at offset 0 is ever counted or ranked.
//
// Every store is a plain vector store.  No byte at or beyond in + n is read; the 16-byte staging
// loads start at the 16-byte boundary below `in` and bytes outside [in, in + n) are zeroed.
#include "bgzf_chain.h"
#include "dmx_device.h"
#include "dmx_internal.h"

namespace dmx {

constexpr uint32_t BC_NT = 256;
constexpr uint32_t BC_TILE = BC_NT * 16;  // staged bytes per workgroup (16 per thread)

// Stages tile `tile` of the 16-byte aligned view of the file (plus 16 bytes of the next tile) and
// tests this thread's 16 offsets: bit j of the result = a member starts at aligned position
// tile * BC_TILE + 16 * t + j.  Ends past a barrier; lds holds BC_TILE / 4 + 4 words.
__device__ __forceinline__ uint32_t bc_tile_mask(const uint8_t* in, uint64_t n, uint64_t tile, uint32_t* lds) {
    const uint32_t t = threadIdx.x;
    const uint64_t lead = (uintptr_t)in & 15, vend = lead + n;
    const uint8_t* vbase = in - lead;
    // (an aligned 16-byte load at q < vend shares its 16-byte line with a byte of the file)
    auto load = [&](uint64_t q, uint32_t* dst) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (q < vend) v = *reinterpret_cast<const uint4*>(vbase + q);
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
        if (q < lead || q + 16 > vend) {  // the ragged ends
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t m = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const uint64_t p = q + 4 * k + b;
                    if (p >= lead && p < vend) m |= 0xFFu << (8 * b);
                }
                w[k] &= m;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) dst[k] = w[k];
    };
    const uint64_t p0 = tile * BC_TILE + 16ull * t;
    load(p0, lds + 4 * t);
    if (t == 0) load(tile * BC_TILE + BC_TILE, lds + BC_TILE / 4);
    __syncthreads();
    uint32_t w[5];
#pragma unroll
    for (int k = 0; k < 5; k++) w[k] = lds[4 * t + k];
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t word = __builtin_amdgcn_alignbyte(w[(j >> 2) + 1], w[j >> 2], j & 3);
        const uint64_t p = p0 + j;
        if (bgzf_magic(word) && p >= lead && p + 18 <= vend) {  // (fewer than 18 bytes: no member)
            BgzfCand c;
            if (bgzf_candidate(in, n, p - lead, &c)) mask |= 1u << j;
        }
    }
    __syncthreads();
    return mask;
}

// the workgroup's exclusive scan of `v` (result) and its sum (*total); sm holds BC_NT / 64 words
__device__ __forceinline__ uint32_t bc_block_scan(uint32_t v, uint32_t* sm, uint32_t* total) {
    const uint32_t t = threadIdx.x;
    const uint32_t inc = wave_incl_scan(v);
    if ((t & 63) == 63) sm[t >> 6] = inc;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < BC_NT / 64; k++) {
        if (k < (t >> 6)) before += sm[k];
        sum += sm[k];
    }
    *total = sum;
    return before + inc - v;
}

__global__ __launch_bounds__(BC_NT) void k_bgzf_count(const uint8_t* in, uint64_t n, uint32_t* tile_counts) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[BC_TILE / 4 + 4];
    __shared__ uint32_t sm[BC_NT / 64];
    const uint32_t mask = bc_tile_mask(in, n, blockIdx.x, lds);
    uint32_t total;
    (void)bc_block_scan(__popc(mask), sm, &total);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// cands holds ncand entries (the count the host read): nothing is written past them
__global__ __launch_bounds__(BC_NT) void k_bgzf_list(const uint8_t* in, uint64_t n, const uint64_t* tile_offs,
                                                     BgzfCand* cands, uint64_t ncand) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[BC_TILE / 4 + 4];
    __shared__ uint32_t sm[BC_NT / 64];
    uint32_t mask = bc_tile_mask(in, n, blockIdx.x, lds);
    uint32_t total;
    uint64_t at = tile_offs[blockIdx.x] + bc_block_scan(__popc(mask), sm, &total);
    const uint64_t lead = (uintptr_t)in & 15;
    const uint64_t p0 = (uint64_t)blockIdx.x * BC_TILE + 16ull * threadIdx.x;
    while (mask) {
        const int j = __ffs(mask) - 1;
        mask &= mask - 1;
        BgzfCand c;
        if (bgzf_candidate(in, n, p0 + j - lead, &c) && at < ncand) cands[at] = c;
        at++;
    }
}

__global__ __launch_bounds__(BC_NT) void k_bgzf_link(const BgzfCand* cands, uint64_t ncand, uint64_t n, uint32_t* J) {
    const uint64_t i = (uint64_t)blockIdx.x * BC_NT + threadIdx.x;
    if (i < ncand) J[i] = bgzf_link(cands, ncand, i, n);
}

__global__ __launch_bounds__(BC_NT) void k_bgzf_double(const uint32_t* Jk, uint32_t* Jn, uint64_t ncand) {
    const uint64_t i = (uint64_t)blockIdx.x * BC_NT + threadIdx.x;
    if (i < ncand) Jn[i] = bgzf_double(Jk, i);
}

__global__ void k_bgzf_head(const uint8_t* in, uint64_t n, const BgzfCand* cands, uint64_t ncand, const uint32_t* J,
                            uint32_t levels, BgzfChainHead* head) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t members = 0;
    const int status = bgzf_chain_status(in, n, cands, ncand, J, levels, &members);
    head->members = members;
    head->status = status;
    head->pad_ = 0;
}

// rows / isz hold ncand entries; isz[r] = 0 behind the chain, so that one scan of ncand values
// gives the members' output offsets and the total
__global__ __launch_bounds__(BC_NT) void k_bgzf_rank(const BgzfCand* cands, uint64_t ncand, const uint32_t* J,
                                                     uint32_t levels, const BgzfChainHead* head, BgzfCand* rows,
                                                     uint32_t* isz) {
    const uint64_t r = (uint64_t)blockIdx.x * BC_NT + threadIdx.x;
    if (r >= ncand) return;
    if (r >= head->members) {
        isz[r] = 0;
        return;
    }
    const BgzfCand c = cands[bgzf_rank_lookup(J, ncand, levels, r)];
    rows[r] = c;
    isz[r] = c.isize;
}

// entries[k] = member k's start in both coordinate systems; entries[members] = {n, plain bytes}
__global__ __launch_bounds__(BC_NT) void k_bgzf_entries(const BgzfCand* rows, const uint64_t* uoff, uint64_t members,
                                                        uint64_t n, const uint64_t* total, ::dmx_bgzf_entry* entries) {
    const uint64_t k = (uint64_t)blockIdx.x * BC_NT + threadIdx.x;
    if (k > members) return;
    ::dmx_bgzf_entry e;
    e.coffset = k < members ? rows[k].off : n;
    e.uoffset = k < members ? uoff[k] : *total;
    entries[k] = e;
}

__global__ __launch_bounds__(BC_NT) void k_bgzf_desc(const uint8_t* in, const BgzfCand* rows, const uint64_t* uoff,
                                                     uint64_t members, uint8_t* out, InflateBatchDesc* desc,
                                                     uint32_t* order) {
    const uint64_t k = (uint64_t)blockIdx.x * BC_NT + threadIdx.x;
    if (k >= members) return;
    const BgzfCand c = rows[k];
    InflateBatchDesc d;
    d.in = in + c.off;
    d.n = c.size;
    d.out = out + uoff[k];
    d.cap = c.isize;
    desc[k] = d;
    order[k] = (uint32_t)k;
}

// Ranged read: members [0, count) of an index slice idx[0 .. count] (idx[count] closes the last
// one).  A member that lies inside the plain range [u0, u1) decodes straight into out; the first
// and the last member may stick out and decode into edge (the first at 0, the last behind it).
__global__ __launch_bounds__(BC_NT) void k_bgzf_range_desc(const uint8_t* in, const ::dmx_bgzf_entry* idx,
                                                           uint64_t count, uint64_t u0, uint64_t u1, uint8_t* out,
                                                           uint8_t* edge, InflateBatchDesc* desc, uint32_t* order) {
    const uint64_t k = (uint64_t)blockIdx.x * BC_NT + threadIdx.x;
    if (k >= count) return;
    const ::dmx_bgzf_entry a = idx[k], b = idx[k + 1];
    InflateBatchDesc d;
    d.in = in + a.coffset;
    d.n = b.coffset - a.coffset;
    d.cap = b.uoffset - a.uoffset;
    if (a.uoffset >= u0 && b.uoffset <= u1) d.out = out + (a.uoffset - u0);
    else d.out = k == 0 ? edge : edge + (idx[1].uoffset - idx[0].uoffset);
    desc[k] = d;
    order[k] = (uint32_t)k;
}

// the slices of the (at most two) edge members: blockIdx.y = 0 the first member, 1 the last
__global__ __launch_bounds__(BC_NT) void k_bgzf_range_copy(const ::dmx_bgzf_entry* idx, uint64_t count, uint64_t u0,
                                                           uint64_t u1, const uint8_t* edge, uint8_t* out) {
    const uint64_t k = blockIdx.y == 0 ? 0 : count - 1;
    if (blockIdx.y == 1 && count == 1) return;
    const uint64_t a = idx[k].uoffset, b = idx[k + 1].uoffset;
    if (a >= u0 && b <= u1) return;  // decoded in place
    const uint8_t* src = k == 0 ? edge : edge + (idx[1].uoffset - idx[0].uoffset);
    const uint64_t lo = a > u0 ? a : u0, hi = b < u1 ? b : u1;
    for (uint64_t p = lo + (uint64_t)blockIdx.x * BC_NT + threadIdx.x; p < hi; p += (uint64_t)gridDim.x * BC_NT)
        out[p - u0] = src[p - a];
}

// The file status of dmx_inflate_bgzf: the first member whose result is not DMX_OK, with
// DMX_ERR_CAPACITY or a decoded size other than ISIZE (desc[k].cap) read as DMX_ERR_CHECKSUM.
// *key (preset to all ones) = min over the failing members of index << 32 | status.
__global__ __launch_bounds__(BC_NT) void k_bgzf_status(const ::dmx_batch_result* res, const InflateBatchDesc* desc,
                                                       uint64_t members, unsigned long long* key) {
    const uint64_t k = (uint64_t)blockIdx.x * BC_NT + threadIdx.x;
    if (k >= members) return;
    int st = res[k].status;
    if (st == DMX_ERR_CAPACITY || (st == DMX_OK && res[k].bytes != desc[k].cap)) st = DMX_ERR_CHECKSUM;
    if (st != DMX_OK) atomicMin(key, (unsigned long long)((k << 32) | (uint32_t)st));
}

// ---- deflate: the members of the framed batch, slot i at slots + i * stride, to one file --------
constexpr uint8_t kEofMember[kBgzfEofBytes] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                                               0x02, 0,    0x1b, 0,    0x03, 0, 0, 0, 0, 0,    0,    0, 0,    0};

__global__ __launch_bounds__(BC_NT) void k_bgzf_sizes(const ::dmx_batch_result* res, uint64_t count, uint32_t* sizes,
                                                      unsigned long long* key) {
    const uint64_t k = (uint64_t)blockIdx.x * BC_NT + threadIdx.x;
    if (k >= count) return;
    const int st = res[k].status;
    sizes[k] = st == DMX_OK ? (uint32_t)res[k].bytes : 0u;
    if (st != DMX_OK) atomicMin(key, (unsigned long long)((k << 32) | (uint32_t)st));
}

// Workgroup i < count copies member i to out + offs[i]; workgroup `count` appends the EOF member
// and writes head = {file bytes, status}.  A member that failed, or a file that does not fit cap:
// nothing is written to out.  16-byte copies where source and destination agree mod 16 (heads
// and tails by bytes), bytes otherwise.
__global__ __launch_bounds__(BC_NT) void k_bgzf_pack(const uint8_t* slots, uint64_t stride, const uint32_t* sizes,
                                                     const uint64_t* offs, const uint64_t* members_total,
                                                     const unsigned long long* key, uint64_t count, uint8_t* out,
                                                     uint64_t cap, BgzfChainHead* head) {
    const uint32_t t = threadIdx.x;
    const uint64_t i = blockIdx.x;
    const uint64_t total = *members_total + kBgzfEofBytes;
    const unsigned long long fail = *key;
    const int status = fail != ~0ull ? (int)(uint32_t)fail : total > cap ? DMX_ERR_CAPACITY : DMX_OK;
    if (i == count && t == 0) {
        head->members = total;
        head->status = status;
        head->pad_ = 0;
    }
    if (status != DMX_OK) return;
    if (i == count) {
        if (t < kBgzfEofBytes) out[total - kBgzfEofBytes + t] = kEofMember[t];
        return;
    }
    const uint8_t* src = slots + i * stride;
    uint8_t* dst = out + offs[i];
    const uint32_t len = sizes[i];
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0) {
        const uint32_t lead = min(len, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
        const uint32_t body = (len - lead) & ~15u;
        if (t < lead) dst[t] = src[t];
        for (uint32_t p = lead + 16 * t; p < lead + body; p += 16 * BC_NT)
            *reinterpret_cast<uint4*>(dst + p) = *reinterpret_cast<const uint4*>(src + p);
        for (uint32_t p = lead + body + t; p < len; p += BC_NT) dst[p] = src[p];
    } else {
        for (uint32_t p = t; p < len; p += BC_NT) dst[p] = src[p];
    }
}

// ---- launches -----------------------------------------------------------------------------------
static uint32_t bc_grid(uint64_t count) { return (uint32_t)((count + BC_NT - 1) / BC_NT); }

uint64_t bgzf_tiles(const uint8_t* in, uint64_t n) {
    return n ? (((uintptr_t)in & 15) + n + BC_TILE - 1) / BC_TILE : 0;
}

hipError_t launch_bgzf_count(const uint8_t* in, uint64_t n, uint32_t* tile_counts, uint64_t* tile_offs,
                             uint64_t* ncand, hipStream_t st) {
    const uint64_t nt = bgzf_tiles(in, n);
    if (!nt) return hipSuccess;
    hipLaunchKernelGGL(k_bgzf_count, dim3((uint32_t)nt), dim3(BC_NT), 0, st, in, n, tile_counts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_scan_u32(tile_counts, tile_offs, nt, ncand, st);
}

hipError_t launch_bgzf_chain(const uint8_t* in, uint64_t n, const uint64_t* tile_offs, uint64_t ncand,
                             BgzfCand* cands, uint32_t* J, BgzfCand* rows, uint32_t* isz, uint64_t* uoff,
                             BgzfChainHead* head, hipStream_t st) {
    const uint32_t levels = bgzf_levels(ncand);
    if (ncand) {
        hipLaunchKernelGGL(k_bgzf_list, dim3((uint32_t)bgzf_tiles(in, n)), dim3(BC_NT), 0, st, in, n, tile_offs, cands,
                           ncand);
        hipLaunchKernelGGL(k_bgzf_link, dim3(bc_grid(ncand)), dim3(BC_NT), 0, st, cands, ncand, n, J);
        for (uint32_t k = 0; k + 1 < levels; k++)
            hipLaunchKernelGGL(k_bgzf_double, dim3(bc_grid(ncand)), dim3(BC_NT), 0, st, J + (uint64_t)k * ncand,
                               J + (uint64_t)(k + 1) * ncand, ncand);
    }
    hipLaunchKernelGGL(k_bgzf_head, dim3(1), dim3(64), 0, st, in, n, cands, ncand, J, levels, head);
    if (ncand)
        hipLaunchKernelGGL(k_bgzf_rank, dim3(bc_grid(ncand)), dim3(BC_NT), 0, st, cands, ncand, J, levels, head, rows,
                           isz);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (ncand == 0: the scan of nothing writes the total 0)
    return launch_scan_u32(isz, uoff, ncand, &head->total, st);
}

hipError_t launch_bgzf_entries(const BgzfCand* rows, const uint64_t* uoff, uint64_t members, uint64_t n,
                               const uint64_t* total, ::dmx_bgzf_entry* entries, hipStream_t st) {
    hipLaunchKernelGGL(k_bgzf_entries, dim3(bc_grid(members + 1)), dim3(BC_NT), 0, st, rows, uoff, members, n, total,
                       entries);
    return hipGetLastError();
}

hipError_t launch_bgzf_desc(const uint8_t* in, const BgzfCand* rows, const uint64_t* uoff, uint64_t members,
                            uint8_t* out, InflateBatchDesc* desc, uint32_t* order, hipStream_t st) {
    if (!members) return hipSuccess;
    hipLaunchKernelGGL(k_bgzf_desc, dim3(bc_grid(members)), dim3(BC_NT), 0, st, in, rows, uoff, members, out, desc,
                       order);
    return hipGetLastError();
}

hipError_t launch_bgzf_range_desc(const uint8_t* in, const ::dmx_bgzf_entry* idx, uint64_t count, uint64_t u0,
                                  uint64_t u1, uint8_t* out, uint8_t* edge, InflateBatchDesc* desc, uint32_t* order,
                                  hipStream_t st) {
    hipLaunchKernelGGL(k_bgzf_range_desc, dim3(bc_grid(count)), dim3(BC_NT), 0, st, in, idx, count, u0, u1, out, edge,
                       desc, order);
    return hipGetLastError();
}

hipError_t launch_bgzf_range_copy(const ::dmx_bgzf_entry* idx, uint64_t count, uint64_t u0, uint64_t u1,
                                  const uint8_t* edge, uint8_t* out, hipStream_t st) {
    hipLaunchKernelGGL(k_bgzf_range_copy, dim3(64, 2), dim3(BC_NT), 0, st, idx, count, u0, u1, edge, out);
    return hipGetLastError();
}

hipError_t launch_bgzf_status(const ::dmx_batch_result* res, const InflateBatchDesc* desc, uint64_t members,
                              unsigned long long* key, hipStream_t st) {
    if (!members) return hipSuccess;
    hipLaunchKernelGGL(k_bgzf_status, dim3(bc_grid(members)), dim3(BC_NT), 0, st, res, desc, members, key);
    return hipGetLastError();
}

hipError_t launch_bgzf_pack(const uint8_t* slots, uint64_t stride, const ::dmx_batch_result* res, uint64_t count,
                            uint32_t* sizes, uint64_t* offs, unsigned long long* key, uint8_t* out, uint64_t cap,
                            BgzfChainHead* head, hipStream_t st) {
    hipLaunchKernelGGL(k_bgzf_sizes, dim3(bc_grid(count)), dim3(BC_NT), 0, st, res, count, sizes, key);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_scan_u32(sizes, offs, count, &head->total, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bgzf_pack, dim3((uint32_t)count + 1), dim3(BC_NT), 0, st, slots, stride, sizes, offs,
                       &head->total, key, count, out, cap, head);
    return hipGetLastError();
}

}  // namespace dmx
