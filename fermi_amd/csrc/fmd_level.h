// fmd_level.h -- what the level-by-level trie walks share (the k-mer harvest, fmd_kmer.hip; locate, fmd_locate.hip): one backward
// extension per lane on the wave engine, output slots reserved per wave in chunks, the frontier cut into one range per XCD.
// A frontier entry is a multiple of 16 bytes whose all-zero image is a hole (size 0) that the next level skips.
#pragma once
#include "fmd_kernel_common.h"

// One backward extension per lane.  Narrow intervals (size <= 63: every level below ~log4(n)) take the
// child sizes from one 64-position window of the lane's block image(s); the absolute rank tk[c] is then
// computed only for the children that are kept (usually one) -- or not at all (k_kmer_emit needs sizes
// only).  Wide intervals: two six-symbol block ranks.
// ALL6 = false: the kept children are the bases A/C/G/T with at least thr occurrences (the harvest).  ALL6 = true: every child that
// occurs, '$' and N included (locate: the rank of the '$' child is where its run of sentinels starts), and x0 = 0 is a legal start.
template <bool NEED_TK, bool ALL6 = false>
__device__ __forceinline__ void km_extend_back(const FmdIndexView &ix, uint4 *lds, bool active, uint64_t x0, uint64_t sz,
                                               uint64_t thr, uint64_t tk[6], uint64_t s[6])
{
    FmdRank2c r = fmd_wave_rank2_fetch_compact(ix, lds, active ? x0 - 1 : NONE64, active ? x0 - 1 + sz : NONE64);
    const bool narrow = active && sz <= 63 && !(r.two_phase && r.l_sep) && (!ALL6 || x0 != 0);   // (x0 = 0 has no k side to hang the window on)
    uint64_t tl[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 6; ++c) { tk[c] = 0; s[c] = 0; }
    if (active && !narrow && r.hk) fmd_block_rank6<false>(r.bk, r.t, r.nk, tk, r.blk_k);
    fmd_wave_l_ready(ix, lds, r);
    if (narrow) {
        uint4 a, b, c;
        grp_window(r.bk, r.t, r.bl, r.tl, r.blk_k, r.blk_l, r.hk, r.l_sep, r.blk_k, r.nk - 1, a, b, c); // window at x0 = (x0 - 1) + 1
        const uint32_t sh = (uint32_t)x0 & 31;
        const uint64_t m = (1ull << (int)sz) - 1;
        const uint64_t X = win64(a.x, b.x, c.x, sh), Y = win64(a.y, b.y, c.y, sh), Z = win64(a.z, b.z, c.z, sh);
        const uint64_t lo = ~Z & m, hi = Z & ~Y & m;
        s[0] = __popcll(lo & ~Y & ~X); s[1] = __popcll(lo & ~Y & X); s[2] = __popcll(lo & Y & ~X); s[3] = __popcll(lo & Y & X);
        s[4] = __popcll(hi & ~X); s[5] = __popcll(hi & X);
        if (NEED_TK) {
            uint32_t todo = (s[1] >= thr ? 2u : 0u) | (s[2] >= thr ? 4u : 0u) | (s[3] >= thr ? 8u : 0u) | (s[4] >= thr ? 16u : 0u);
            if (ALL6) todo |= (s[0] >= thr ? 1u : 0u) | (s[5] >= thr ? 32u : 0u);
            while (__ballot(todo != 0)) {
                const int cc = todo ? __ffs((int)todo) - 1 : 1;
                const uint64_t v = r.hk ? fmd_block_rank1(r.bk, r.t, r.nk, cc, r.blk_k) : 0;
                if (todo) { tk[1] = cc == 1 ? v : tk[1]; tk[2] = cc == 2 ? v : tk[2]; tk[3] = cc == 3 ? v : tk[3]; tk[4] = cc == 4 ? v : tk[4]; }
                if (ALL6 && todo) { tk[0] = cc == 0 ? v : tk[0]; tk[5] = cc == 5 ? v : tk[5]; }
                todo &= todo - 1;
            }
        }
    } else if (active) {
        if (r.hl) fmd_block_rank6<false>(r.bl, r.tl, r.nl, tl, r.blk_l);
#pragma unroll
        for (int c = 0; c < 6; ++c) s[c] = tl[c] - tk[c];
    }
}

// Output space of a level is handed out in chunks of `ch` entries per wave: ONE device-wide atomic
// per chunk instead of one per 64 nodes (a single counter serialises at ~10^8 atomics/s, which
// capped the first version of the harvest kernel at a twelfth of the gather rate).  A wave zero-fills
// what it leaves unused of its last chunk (size 0 = hole; the next level skips holes), so a
// frontier is "children + at most one partial chunk per wave".
struct KmChunk { unsigned long long base; uint32_t fill, ch; bool have; };

template <class E>
__device__ __forceinline__ void km_zero_fill(E *out, uint64_t cap, const KmChunk &k)
{
    static_assert(sizeof(E) % 16 == 0, "entries are whole 16-byte words");
    if (!k.have) return;
    for (uint64_t e = k.base + k.fill + fmd_lane(); e < k.base + k.ch; e += 64)
        if (e < cap) {
            uint4 *q = (uint4 *)(out + e);
#pragma unroll
            for (int j = 0; j < (int)(sizeof(E) / 16); ++j) q[j] = make_uint4(0, 0, 0, 0);
        }
}

// a fresh chunk for this wave (wave-uniform)
__device__ __forceinline__ void km_new_chunk(KmChunk &k, unsigned long long *ctr_next)
{
    unsigned long long first = 0;
    if (fmd_lane() == 0) first = atomicAdd(ctr_next, (unsigned long long)k.ch);
    k.base = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(first >> 32)) << 32) |
             (unsigned int)__builtin_amdgcn_readfirstlane((int)first);
    k.fill = 0; k.have = true;
}

// first output slot for `tot` new entries of this wave (wave-uniform)
template <class E>
__device__ __forceinline__ unsigned long long km_reserve(E *out, uint64_t cap, KmChunk &k, uint32_t tot, unsigned long long *ctr_next)
{
    if (!k.have || k.fill + tot > k.ch) {
        km_zero_fill(out, cap, k);
        km_new_chunk(k, ctr_next);
    }
    const unsigned long long o = k.base + k.fill;
    k.fill += tot;
    return o;
}

// The same for a frontier whose size is bounded exactly (locate): a chunk is filled to its last slot before the next one is taken, so a level holds
// its live entries + the tail of at most ONE chunk per wave, nothing else.  The j-th of the `tot` new entries (tot <= ch) goes to slot
// j < na ? a + j : b + (j - na).
struct KmSpan { unsigned long long a, b; uint32_t na; };
__device__ __forceinline__ KmSpan km_reserve_split(KmChunk &k, uint32_t tot, unsigned long long *ctr_next)
{
    KmSpan sp;
    if (!k.have) km_new_chunk(k, ctr_next);
    const uint32_t rem = k.ch - k.fill;
    sp.a = k.base + k.fill; sp.b = 0; sp.na = tot < rem ? tot : rem;
    k.fill += sp.na;
    if (tot > rem) { km_new_chunk(k, ctr_next); sp.b = k.base; k.fill = tot - rem; }
    return sp;
}
__device__ __forceinline__ unsigned long long km_span_slot(const KmSpan &sp, uint32_t j) { return j < sp.na ? sp.a + j : sp.b + (j - sp.na); }

// Which frontier slots a workgroup walks.  Consecutive workgroups land on different XCDs (8 of them, each
// with its own L2), while consecutive frontier entries are children of neighbouring nodes and touch
// neighbouring rank blocks: give every XCD one contiguous eighth of the frontier so that this locality
// stays inside one L2.
struct KmRange { uint64_t beg, end, stride; };
__device__ __forceinline__ KmRange km_range(uint64_t n, int xcd_aware)
{
    KmRange r;
    if (xcd_aware && (gridDim.x & 7) == 0) {
        const uint32_t x = blockIdx.x & 7, slot = blockIdx.x >> 3, per = gridDim.x >> 3;
        const uint64_t seg = ((n + 7) / 8 + 63) & ~63ull;
        r.beg = (uint64_t)x * seg + (uint64_t)slot * 64;
        r.end = (uint64_t)(x + 1) * seg < n ? (uint64_t)(x + 1) * seg : n;
        r.stride = (uint64_t)per * 64;
    } else { r.beg = (uint64_t)blockIdx.x * 64; r.end = n; r.stride = (uint64_t)gridDim.x * 64; }
    return r;
}
