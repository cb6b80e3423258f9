// huff_fit.h -- the arithmetic of the deflate's length-limited code build and of the run-length
// header: the code-length limits, the initial length of a symbol (init_len), the Kraft repair and
// slack fill on the class sizes (fit_classes) and the RLE plan of one run of code lengths
// (plan_run).  Plain C++, no HIP: DMX_HF is `inline` under g++ and __host__ __device__, force-inlined,
// under hipcc, so the code the emission kernels run (deflate_kernels.hip: em_build_codes,
// wave_build_lengths64, em_segment) is the code tests/test_huff_fit.py checks on the CPU,
// sanitizers included.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DMX_HF __host__ __device__ __forceinline__
#define DMX_HF_UNROLL _Pragma("unroll")
#else
#define DMX_HF inline
#define DMX_HF_UNROLL
#endif

namespace dmx {

// Code-length limits of the emitted lit/len and distance codes.  RFC 1951 allows 15; 9 and 6
// keep every code inside the one-level lookup tables of the lane decoder
// (inflate_lanes.hip: 512 + 64 entries per segment in LDS).  The cost against an optimal code at
// the same limits is tabulated in DESIGN.md (section 5, "ratio accounting").
constexpr int DF_LIT_MAXBITS = 9;
constexpr int DF_DIST_MAXBITS = 6;
constexpr int DF_PRE_MAXBITS = 7;  // the precode: its lengths are 3-bit fields (RFC 1951 3.2.7)

// leading zeros of x != 0 (the device's own instruction under hipcc)
DMX_HF int hf_clz(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz(x);
#else
    return __builtin_clz(x);
#endif
}
DMX_HF uint32_t hf_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
DMX_HF uint32_t hf_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// Kraft repair and slack fill on the class sizes cnt[1..15] of a code whose lengths are
// non-decreasing in frequency rank: lengthen the last (least frequent) members of a class while
// the code is over-full, then shorten the first (most frequent) members while slack remains.
// Ends with a complete code (Kraft sum exactly 2^maxbits), as zlib and the reference require,
// provided at least two symbols are used (cnt sums to >= 2) and every class lies in [1, maxbits].
// Not an optimal length-limited code.  Measured against package-merge at the same limit
// (tests/cpp/huff_fit_test.cpp --excess; table in DESIGN.md section 5): at most 1.67 % more token
// bits on level-1 histograms of a 32 KiB segment (geometric, ratio 0.97; mean 0.18 %), and on
// fuzzed, adversarial histograms up to 8.1 % (lit/len, 9 bits), 12.5 % (distance, 6 bits) and
// 12.2 % (precode, 7 bits) with means below 0.5 %.
// passes (tests): the number of slack-fill passes that changed something.
DMX_HF void fit_classes(uint32_t (&cnt)[17], int maxbits, int* passes = nullptr) {
    // Kraft sums in units of 2^-maxbits (<= 288 * 2^8: 32-bit); every class weight is a power
    // of two, so the divisions are shifts
    const int32_t U = 1 << maxbits;
    int32_t K = 0;
    DMX_HF_UNROLL
    for (int L = 1; L <= 15; L++) K += L <= maxbits ? (int32_t)cnt[L] << (maxbits - L) : 0;
    while (K > U) {
        DMX_HF_UNROLL
        for (int L = 14; L >= 1; L--) {
            if (L < maxbits && K > U && cnt[L]) {
                const int sh = maxbits - L - 1;  // gain of one lengthening: 2^sh
                const uint32_t need = (uint32_t)((K - U + (1 << sh) - 1) >> sh);
                const uint32_t k = hf_min(need, cnt[L]);
                cnt[L] -= k;
                cnt[L + 1] += k;
                K -= (int32_t)k << sh;
            }
        }
    }
    uint32_t R = (uint32_t)(U - K);
    for (int pass = 0; pass < 64 && R; pass++) {
        bool changed = false;
        DMX_HF_UNROLL
        for (int L = 2; L <= 15; L++) {
            if (L <= maxbits && cnt[L] && (1u << (maxbits - L)) <= R) {
                const uint32_t k = hf_min(cnt[L], R >> (maxbits - L));
                cnt[L] -= k;
                cnt[L - 1] += k;
                R -= k << (maxbits - L);
                changed = true;
            }
        }
        if (!changed) break;
        if (passes) ++*passes;
    }
}

// initial length round(log2(F/f)) clamped to [1, maxbits] (0 for f == 0); f <= F
DMX_HF uint32_t init_len(uint32_t f, uint32_t F, int maxbits) {
    if (!f) return 0;
    // floor(log2(F / f)) without a division: F / f lies in [2^(e-1), 2^(e+1)) for e = the
    // difference of the leading-bit positions, and is >= 2^e exactly when f << e <= F
    const uint32_t e = (uint32_t)(hf_clz(f) - hf_clz(F));
    const uint32_t L0 = e - (((uint64_t)f << e) > F ? 1u : 0u);
    const uint64_t a = (uint64_t)f << (L0 + 1);
    const uint32_t L = L0 + ((a * a <= 2ull * F * F) ? 1u : 0u);
    return hf_max(1u, hf_min((uint32_t)maxbits, L));
}

// the frequency half of a symbol's initial class: 1 when f <= F / 2^L0 (the less frequent half,
// ranked behind the other), else 0.  em_build_codes orders symbols by (2 L0 + half, symbol).
DMX_HF uint32_t init_half(uint32_t f, uint32_t F, uint32_t L0) { return ((uint64_t)f << L0) <= F ? 1u : 0u; }

// RLE plan of one run of code lengths (v, r): zero runs use 18/17, others v then 16s.
// Never a 16 after a 17/18, and sequences never span HLIT/HDIST (the reference
// inflate decodes the two sequences separately, inflate.hpp:216-220, and repeats the last
// *literal* length on 16, inflate.hpp:181).
struct RunPlan {
    uint32_t n18, last18, n17, r17, nlit, n16, last16;  // last18/last16: length of final repeat
};
DMX_HF RunPlan plan_run(uint32_t v, uint32_t r) {
    RunPlan p = {0, 0, 0, 0, 0, 0, 0};
    if (v == 0) {
        p.n18 = r / 138;
        p.last18 = 138;
        uint32_t rem = r % 138;
        if (rem >= 11) { p.n18++; p.last18 = rem; }
        else if (rem >= 3) { p.n17 = 1; p.r17 = rem; }
        else p.nlit = rem;
    } else {
        uint32_t q = r - 1;
        p.nlit = 1;
        p.n16 = q / 6;
        p.last16 = 6;
        uint32_t rem = q % 6;
        if (rem >= 3) { p.n16++; p.last16 = rem; }
        else p.nlit += rem;
    }
    return p;
}

}  // namespace dmx
