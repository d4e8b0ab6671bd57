// fmd_level.h -- what the level-by-level trie walks share (the k-mer harvest, fmd_kmer.hip; kcount, fmd_kcount.hip; locate, fmd_locate.hip; asearch, fmd_asearch.hip): one
// backward extension per lane on the wave engine, output slots reserved per wave in chunks, the frontier cut into one range per XCD, the level step of the
// two k-mer walks.
// A frontier entry is a multiple of 16 bytes whose all-zero image is a hole (size 0) that the next level skips.
#pragma once
#include "fmd_kernel_common.h"

// One backward extension per lane.  Narrow intervals (size <= 63: every level below ~log4(n)) take the
// child sizes from one 64-position window of the lane's block image(s); the absolute rank tk[c] is then
// computed only for the children that are kept (usually one) -- or not at all (k_kmer_emit needs sizes
// only).  Wide intervals: two six-symbol block ranks.
// ALL6 = false: the kept children are the bases A/C/G/T with at least thr occurrences (the harvest).  ALL6 = true: every child that
// occurs, '$' and N included (locate: the rank of the '$' child is where its run of sentinels starts), and x0 = 0 is a legal start.
// MASKED = true: of those children, a narrow interval gets tk[c] only where bit c of `keep` is set (asearch: the children its budget still allows).
template <bool NEED_TK, bool ALL6 = false, bool MASKED = false>
__device__ __forceinline__ void km_extend_back(const FmdIndexView &ix, uint4 *lds, bool active, uint64_t x0, uint64_t sz,
                                               uint64_t thr, uint64_t tk[6], uint64_t s[6], uint32_t keep = 0x3fu)
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
            if (MASKED) todo &= keep;
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

// the sum of v over the wave, in every lane
__device__ __forceinline__ uint64_t km_wave_sum(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
    return v;
}

// reverse complement of the k-mer in the low 2k bits of w (kcount, kcmp): complement, reverse the 2-bit groups, shift the k groups down
__device__ __forceinline__ uint64_t kc_revcomp(uint64_t w, int k)
{
    uint64_t x = __brevll(~w);                        // the groups reversed, and the two bits of every group swapped
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    return x >> (64 - 2 * k);
}

// One level of a k-mer trie walk (the harvest, fmd_kmer.hip; kcount, fmd_kcount.hip): the nodes of `in` at depth d -- bi-intervals whose info
// word K holds the d bases, the rightmost in the lowest two bits -- get one backward extension each, and the children A/C/G/T with at least thr
// occurrences go to `out` with the new base at bits 2d of K.  Counters, words of ctr: [d] = the entries of `in` (more than cap when that level
// overflowed: the first cap are there), [d + 1] = the chunk counter of `out`, [i_ovf] is set when a child did not fit cap, [i_ext] counts the extensions.
__device__ __forceinline__ void km_level_step(const FmdIndexView &ix, uint4 *fmd_lds, int d, uint64_t thr, const fmd_intv_t *__restrict__ in,
                                              fmd_intv_t *__restrict__ out, uint64_t cap, uint32_t ch, unsigned long long *__restrict__ ctr, int i_ovf,
                                              int i_ext, int xcd_aware)
{
    const int lane = fmd_lane();
    const uint64_t n = ctr[d] < cap ? ctr[d] : cap;   // an overflowing level counted more than it stored
    const KmRange rg = km_range(n, xcd_aware);
    const uint64_t stride = rg.stride;
    KmChunk ck; ck.base = 0; ck.fill = 0; ck.ch = ch; ck.have = false;
    uint32_t n_ext = 0;
    uint4 na = make_uint4(0, 0, 0, 0), nb = na;       // the entry of the next iteration, loaded one gather ahead
    {
        const uint64_t i0 = rg.beg + lane;
        if (i0 < rg.end) { const uint4 *q = (const uint4 *)(in + i0); na = q[0]; nb = q[1]; }
    }
    for (uint64_t base = rg.beg; base < rg.end; base += stride) {
        const uint4 a = na, b = nb;
        const uint64_t x0 = (uint64_t)a.y << 32 | a.x, x1 = (uint64_t)a.w << 32 | a.z;
        const uint64_t sz = (uint64_t)b.y << 32 | b.x, K = (uint64_t)b.w << 32 | b.z;
        const bool act = base + lane < rg.end && sz != 0;
        {
            const uint64_t i1 = base + stride + lane;
            na = make_uint4(0, 0, 0, 0); nb = na;
            if (i1 < rg.end) { const uint4 *q = (const uint4 *)(in + i1); na = q[0]; nb = q[1]; }
        }
        const uint64_t m_act = __ballot(act);
        if (m_act == 0) continue;                     // a run of holes
        n_ext += (uint32_t)__popcll(m_act);
        uint64_t tk[6], s[6];
        km_extend_back<true>(ix, fmd_lds, act, x0, sz, thr, tk, s);
        // children c = 1..4 (ambiguous bases are skipped, correct.c:77); x[1] = running sum in
        // the order $,T,G,C,A (exact.c:81-86)
        const bool has1 = act && s[1] >= thr, has2 = act && s[2] >= thr, has3 = act && s[3] >= thr, has4 = act && s[4] >= thr;
        const uint64_t m1 = __ballot(has1), m2 = __ballot(has2), m3 = __ballot(has3), m4 = __ballot(has4);
        const uint32_t tot = (uint32_t)(__popcll(m1) + __popcll(m2) + __popcll(m3) + __popcll(m4));
        if (tot == 0) continue;
        const unsigned long long first = km_reserve(out, cap, ck, tot, &ctr[d + 1]);
        uint64_t o1 = first + fmd_below(m1);
        uint64_t o2 = first + __popcll(m1) + fmd_below(m2);
        uint64_t o3 = first + __popcll(m1) + __popcll(m2) + fmd_below(m3);
        uint64_t o4 = first + __popcll(m1) + __popcll(m2) + __popcll(m3) + fmd_below(m4);
        const uint64_t x1_4 = x1 + s[0], x1_3 = x1_4 + s[4], x1_2 = x1_3 + s[3], x1_1 = x1_2 + s[2];
#define KM_PUSH(c, has, o, x1c)                                                                   \
        if (has) {                                                                                \
            if (o < cap) {                                                                        \
                const uint64_t nx0 = ix.cnt[c] + tk[c], nk = K | (uint64_t)(c - 1) << (2 * d);    \
                uint4 *q = (uint4 *)(out + o);                                                    \
                q[0] = make_uint4((uint32_t)nx0, (uint32_t)(nx0 >> 32), (uint32_t)(x1c), (uint32_t)((x1c) >> 32)); \
                q[1] = make_uint4((uint32_t)s[c], (uint32_t)(s[c] >> 32), (uint32_t)nk, (uint32_t)(nk >> 32));     \
            } else ctr[i_ovf] = 1;                                                                \
        }
        KM_PUSH(1, has1, o1, x1_1) KM_PUSH(2, has2, o2, x1_2) KM_PUSH(3, has3, o3, x1_3) KM_PUSH(4, has4, o4, x1_4)
#undef KM_PUSH
    }
    km_zero_fill(out, cap, ck);
    if (lane == 0 && n_ext) atomicAdd(&ctr[i_ext], (unsigned long long)n_ext);
}
