// bgzf_chain.hip -- BGZF files in device memory (gfx950): the member chain found in parallel, the
// descriptors of the framed batch inflate built from it, the file status, and the compaction of
// the framed batch deflate's member slots into one file.
//
// A BGZF file is a linked list through 16-bit BSIZE fields.  The steps are bgzf_chain.h's (plain
// C++, run serially by tests/cpp/bgzf_chain_test.cpp):
//   k_scan_count / k_scan_list   cand_scan.h's scan over BgzfScan: every offset that starts with
//                                1f 8b 08 + FEXTRA is tested with bgzf_next
//   k_bgzf_link                  successor = the candidate at off + size (binary search)
//   k_bgzf_double                level k -> level k + 1, once per level (launch_chain_links runs
//                                both, for the ZIP directory's records too)
//   k_bgzf_head                  one thread: members reachable from offset 0, chain status
//   k_bgzf_rank                  member r = r hops from candidate 0, along the bits of r
//   launch_scan_u32              uoff = exclusive prefix sum of ISIZE, total plain bytes
// False candidates inside payloads take part in the links and the doubling, but only what is
// reachable from candidate 0 at offset 0 is ever counted or ranked.
// k_member_status is the file status of every decode of a member list (BGZF, multi-member gzip).
//
// Every store is a plain vector store.  No byte at or beyond in + n is read, but by the scan's
// staging (cand_scan.h).
#include "bgzf_chain.h"
#include "cand_scan.h"

namespace dmx {

constexpr uint32_t BC_NT = 256;

// the candidate scan's format (cand_scan.h): a member is what bgzf_next accepts
struct BgzfScan {
    const uint8_t* in;
    uint64_t n;
    using Cand = BgzfCand;
    static constexpr uint32_t kMinBytes = 18;
    __device__ bool magic(uint32_t word) const { return bgzf_magic(word); }
    __device__ bool candidate(uint64_t off, BgzfCand* c) const { return bgzf_candidate(in, n, off, c); }
};

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

// The status of a file of members: the first member whose result is not DMX_OK, with
// DMX_ERR_CAPACITY or a decoded size other than the one expected (desc[k].cap) read as `mismatch`.
// *key (preset to all ones) = min over the failing members of index << 32 | status.
__global__ __launch_bounds__(BC_NT) void k_member_status(const ::dmx_batch_result* res, const InflateBatchDesc* desc,
                                                         uint64_t members, int mismatch, unsigned long long* key) {
    const uint64_t k = (uint64_t)blockIdx.x * BC_NT + threadIdx.x;
    if (k >= members) return;
    int st = res[k].status;
    if (st == DMX_ERR_CAPACITY || (st == DMX_OK && res[k].bytes != desc[k].cap)) st = mismatch;
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

hipError_t launch_bgzf_count(const uint8_t* in, uint64_t n, uint32_t* tile_counts, uint64_t* tile_offs,
                             uint64_t* ncand, hipStream_t st) {
    return launch_scan_count(BgzfScan{in, n}, in, n, tile_counts, tile_offs, ncand, st);
}

hipError_t launch_chain_links(const BgzfCand* cands, uint64_t ncand, uint64_t end, uint32_t* J, hipStream_t st) {
    if (!ncand) return hipSuccess;
    hipLaunchKernelGGL(k_bgzf_link, dim3(bc_grid(ncand)), dim3(BC_NT), 0, st, cands, ncand, end, J);
    for (uint32_t k = 0; k + 1 < bgzf_levels(ncand); k++)
        hipLaunchKernelGGL(k_bgzf_double, dim3(bc_grid(ncand)), dim3(BC_NT), 0, st, J + (uint64_t)k * ncand,
                           J + (uint64_t)(k + 1) * ncand, ncand);
    return hipGetLastError();
}

hipError_t launch_bgzf_chain(const uint8_t* in, uint64_t n, const uint64_t* tile_offs, uint64_t ncand,
                             BgzfCand* cands, uint32_t* J, BgzfCand* rows, uint32_t* isz, uint64_t* uoff,
                             BgzfChainHead* head, hipStream_t st) {
    const uint32_t levels = bgzf_levels(ncand);
    hipError_t e = launch_scan_list(BgzfScan{in, n}, in, n, tile_offs, cands, ncand, st);
    if (e != hipSuccess) return e;
    e = launch_chain_links(cands, ncand, n, J, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bgzf_head, dim3(1), dim3(64), 0, st, in, n, cands, ncand, J, levels, head);
    if (ncand)
        hipLaunchKernelGGL(k_bgzf_rank, dim3(bc_grid(ncand)), dim3(BC_NT), 0, st, cands, ncand, J, levels, head, rows,
                           isz);
    e = hipGetLastError();
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

hipError_t launch_member_status(const ::dmx_batch_result* res, const InflateBatchDesc* desc, uint64_t members,
                                int mismatch_status, unsigned long long* key, hipStream_t st) {
    if (!members) return hipSuccess;
    hipLaunchKernelGGL(k_member_status, dim3(bc_grid(members)), dim3(BC_NT), 0, st, res, desc, members,
                       mismatch_status, key);
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
