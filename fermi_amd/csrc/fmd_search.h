// fmd_search.h -- what the backward-search kernels share (k_bsearch, k_bsearch_pair, k_multi_bsearch; k_reach for the table start): the window a lane
// reads its query through, the prefix-table start, and the result triple.  Each rule is stated here once; included from fmd_kernel_common.h.
#pragma once

// ---- read window: 16 bases of the read around pos -- the four dwords of the 16-byte block of the read buffer that holds base pos, fetched together.
// A lane reads its read backwards, one base per step; fetched one dword every fourth step (round 1-3), each of a line's 16 dwords was a request of
// its own, four steps after the last -- long enough for the random block traffic of the other waves to have pushed the line out of L2: the kernel
// fetched 1.18 x the bytes it asked for, 1 KB per read of refetched read lines (PMC).
struct FmdReadWindow {
    uint4 w = make_uint4(0, 0, 0, 0);
    // The block that holds byte `at`.  THE READ BOUND: only dwords at or below the one that holds byte `top_at` are loaded (the bases above it are
    // behind us, or another read's), the others read as 0 -- so nothing beyond what the contract makes readable (the buffer up to the last base,
    // rounded up to a dword; seqs 4-byte aligned) is touched.  top_at lies in the block of `at`, or above it.
    __device__ __forceinline__ void load(const uint8_t *__restrict__ seqs, uint64_t at, uint64_t top_at)
    {
        const uint64_t b = at & ~15ull, top = top_at & ~3ull;
        const uint32_t *p = (const uint32_t *)(seqs + b);
        w.x = p[0];
        w.y = b + 4 <= top ? p[1] : 0u; w.z = b + 8 <= top ? p[2] : 0u; w.w = b + 12 <= top ? p[3] : 0u;
    }
    // the base at flat offset a, which lies in the block loaded
    __device__ __forceinline__ int base(uint64_t a) const
    {
        const uint32_t q = (uint32_t)(a >> 2) & 3u, d = q == 0 ? w.x : q == 1 ? w.y : q == 2 ? w.z : w.w;
        return (int)((d >> (8 * (a & 3))) & 0xff);
    }
};

// ---- prefix-table start (FmdIndexView::ptab): a search begins ptab_d bases in when all of them are A/C/G/T.  The two index conventions, side by side:
// backward (fm_backward_search): the table string is seqs[beg, end) as it stands, its first base highest: idx = sum (s_j - 1) << 2 (d - 1 - j).
// Returns whether every base was A/C/G/T (idx is meaningless otherwise).  Reads whole dwords from beg & ~3 up to the one that holds end - 1.
__device__ __forceinline__ bool fmd_ptab_fold_back(const uint8_t *__restrict__ seqs, uint64_t beg, uint64_t end, uint64_t &idx)
{
    bool acgt = true;
    idx = 0;
    for (uint64_t a = beg & ~3ull; a < end; a += 4) {
        const uint32_t w = *(const uint32_t *)(seqs + a);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t c = (w >> (8 * b)) & 0xff;
            if (a + b >= beg && a + b < end) { acgt = acgt && c >= 1 && c <= 4; idx = idx << 2 | ((c - 1) & 3); }
        }
    }
    return acgt;
}
// forward (k_reach): the sweep consumes comp(q[p]), comp(q[p + 1]), .. -- the table string read backwards -- so the bases are complemented and the
// FIRST base sits lowest: idx = sum (4 - q[p + j]) << 2 j.  Stops at the first dword with a base that is not A/C/G/T: nothing behind a terminator is read.
__device__ __forceinline__ bool fmd_ptab_fold_fwd(const uint8_t *__restrict__ seqs, size_t p, int d, uint64_t &idx)
{
    bool acgt = true;
    idx = 0;
    for (size_t a = p & ~(size_t)3; a < p + (size_t)d && acgt; a += 4) {
        const uint32_t w = *(const uint32_t *)(seqs + a);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t x = (w >> (8 * b)) & 0xff;
            if (a + b >= p && a + b < p + (size_t)d) { acgt = acgt && x >= 1 && x <= 4; idx |= (uint64_t)((4 - x) & 3) << (2 * (a + b - p)); }
        }
    }
    return acgt;
}
// A table entry: the interval [k, l] (l inclusive) of its string.  AN ABSENT ENTRY IS {1, 0} (k_ptab_level): k > l says the string does not occur and
// nothing else -- not where it would sort.
struct FmdPtabEntry { uint64_t k, l; bool present; };
__device__ __forceinline__ FmdPtabEntry fmd_ptab_unpack(const uint4 e)
{
    FmdPtabEntry t;
    t.k = (uint64_t)e.y << 32 | e.x; t.l = (uint64_t)e.w << 32 | e.z;
    t.present = t.k <= t.l;
    return t;
}

// ---- the result triple of a search: count, first and last row of the interval; a miss is three zeros (exact.c:17-18 leaves the outputs of a miss
// undefined)
struct FmdHitOut {
    uint64_t *__restrict__ cnt, *__restrict__ beg, *__restrict__ end;
    __device__ __forceinline__ void miss(size_t i) const { cnt[i] = 0; beg[i] = 0; end[i] = 0; }
    // the interval [k, l], l inclusive; k > l is a miss
    __device__ __forceinline__ void store(size_t i, uint64_t k, uint64_t l) const
    {
        const bool hit = k <= l;
        cnt[i] = hit ? l - k + 1 : 0; beg[i] = hit ? k : 0; end[i] = hit ? l : 0;
    }
};
