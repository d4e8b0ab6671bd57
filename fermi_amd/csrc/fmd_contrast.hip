// fmd_contrast.hip -- contrast assembly on the GPU: fm6_contrast (cmp.c:45-126) and fm_sub (sub.c:14-97).
//
// CONTRAST.  The reference walks the trie of the strings of two indexes depth-first, one explicit stack per 4-base suffix: a node
// is a pair of intervals of the SAME string, one per index; a node whose string is absent from one index is a TIP, and every read of
// the other index that runs through the tip's string is selected (collect_tips: the trie below the tip, down to the sentinels).  The
// result is two bit arrays that are only OR-ed into, so it does not depend on the visiting order, and the trie is expanded LEVEL BY
// LEVEL as the k-mer harvest does (fmd_kmer.hip): frontier(d) -> one backward extension in EACH index per lane, the two rank blocks
// in flight together -> children appended by wave-aggregated chunked atomics.  Where a child goes is decided when it is pushed, in the
// order of the reference's tests (cmp.c:61-63): side 0 empty -> tip list of index 1; side 1 empty -> tip list of index 0; depth >= k
// -> dropped; else frontier(d + 1).  The tips are expanded afterwards, one index at a time, by a kernel of their own (a wave pays for
// the code of every phase any lane is in), again level by level for CT_TIP_LEVELS levels -- the rows of a tip share their path --
// and what is still open then is LF-walked row by row to its sentinel.  Only x[0] and the size of an interval are ever used (the
// sentinel rows are ok[0].x[0] .. + ok[0].x[2]), so a node is {x0, size} per index: 32 bytes a pair, 16 a tip.
//
// SUB.  mark: one lane per selected sequence, LF-walked from its sentinel row until it is back at a sentinel, a bit per visited row
// (k_merge_walk with one index and one block per step).  select: the kept rows, in order, as nt6 bytes for any slice of the OUTPUT:
// per-4096-row popcounts, a scan, and a kernel that finds the superblock its slice begins in from the scan.
#include <stdlib.h>
#include <string.h>
#include "fmd_kernel_common.h"
#include "fmd_twoside.h"
#include "fmd_bits.h"

#define CT_SUF_LEN 4            // cmp.c:8: the walk starts from all strings of this length, pushed without the min_occ test
#define CT_TIP_LEVELS 64        // levels of a tip's trie expanded as a frontier; the rest is walked row by row
#define CT_MIN_CAP 1024u
// counters in the work area (u64 words)
#define CT_NA 0                 // entries handed out in frontier buffer A / B (holes included)
#define CT_NB 1
#define CT_NT0 2                // the same for the tip lists of index 0 / 1
#define CT_NT1 3
#define CT_EXT 4                // pair nodes expanded                      -> d_status[0]
#define CT_OVF 5                // a list was full: the result is a subset -> d_status[1]
#define CT_TIP0 6               // tip nodes expanded in index 0 / 1        -> d_status[2], [3]
#define CT_TIP1 7
#define CT_DEMAND 8             // the largest list any level asked for
#define CT_WORDS 16

// ------------------------------------------------------------------------------------------------ chunked appends
// Output slots of a list are handed out `ch` entries at a time per wave, one device-wide atomic per chunk; a wave zero-fills what it
// leaves of its last chunk (size 0 = hole, skipped by the reader).  U = uint4 per entry.
struct CtChunk { unsigned long long base; uint32_t fill; bool have; };

template <int U>
__device__ __forceinline__ void ct_zero_fill(uint4 *out, uint64_t cap, uint32_t ch, const CtChunk &k)
{
    if (!k.have) return;
    for (uint64_t e = k.base + k.fill + fmd_lane(); e < k.base + ch; e += 64)
        if (e < cap) {
#pragma unroll
            for (int u = 0; u < U; ++u) out[e * U + u] = make_uint4(0, 0, 0, 0);
        }
}
template <int U>
__device__ __forceinline__ unsigned long long ct_reserve(uint4 *out, uint64_t cap, uint32_t ch, CtChunk &k, uint32_t tot, unsigned long long *ctr)
{
    if (!k.have || k.fill + tot > ch) {
        ct_zero_fill<U>(out, cap, ch, k);
        unsigned long long first = 0;
        if (fmd_lane() == 0) first = atomicAdd(ctr, (unsigned long long)ch);
        k.base = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(first >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)first);
        k.fill = 0; k.have = true;
    }
    const unsigned long long o = k.base + k.fill;
    k.fill += tot;
    return o;
}
// (ct_pack and one side of a backward extension -- CtSide, ct_side, ct_ranks_k / _l -- are in fmd_twoside.h: kcmp walks two indexes the same way)

// rows [r0, r0 + cnt) of a bit array of n_bits: one atomic per touched word
__device__ __forceinline__ void ct_set_range(unsigned long long *sub, uint64_t n_bits, uint64_t r0, uint64_t cnt)
{
    if (cnt == 0 || r0 >= n_bits) return;
    const uint64_t r1 = r0 + cnt < n_bits ? r0 + cnt : n_bits;
    for (uint64_t w = r0 >> 6; w <= (r1 - 1) >> 6; ++w) {
        const uint64_t b = w << 6;
        const uint32_t lo = r0 > b ? (uint32_t)(r0 - b) : 0u, hi = r1 - b < 64 ? (uint32_t)(r1 - b) : 64u;
        atomicOr(sub + w, (unsigned long long)range64(lo, hi));
    }
}

// ------------------------------------------------------------------------------------------------ contrast walk
// depth 1: the single bases of seed_mask (bit c-1 = base c), fm6_set_intv in both indexes (cmp.c:14)
__global__ void k_ct_seed(FmdIndexView a, FmdIndexView b, int seed_mask, uint4 *out, unsigned long long *ctr)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    unsigned long long n = 0;
    for (int c = 1; c <= 4; ++c) {
        const uint64_t sa = a.cnt[c + 1] - a.cnt[c], sb = b.cnt[c + 1] - b.cnt[c];
        if (!((seed_mask >> (c - 1)) & 1) || (sa | sb) == 0) continue;
        out[2 * n] = ct_pack(a.cnt[c], sa); out[2 * n + 1] = ct_pack(b.cnt[c], sb);
        ++n;
    }
    ctr[CT_NA] = n;
}

// one level: pair nodes at depth d -> children at depth d + 1 (frontier, tip lists, or nowhere)
__global__ __launch_bounds__(64) void k_ct_level(FmdIndexView a, FmdIndexView b, int d, int kmer, int min_occ, const uint4 *__restrict__ in,
                                                 uint4 *__restrict__ out, uint4 *__restrict__ tip0, uint4 *__restrict__ tip1, uint64_t cap, uint32_t ch,
                                                 unsigned long long *__restrict__ ctr, int ci, int co)
{
    FMD_DECLARE_WAVE_LDS();
    const int lane = fmd_lane();
    const uint64_t n_raw = ctr[ci], n = n_raw < cap ? n_raw : cap;   // an overflowing level counted more than it stored
    if (blockIdx.x == 0 && lane == 0) { atomicMax(&ctr[CT_DEMAND], (unsigned long long)n_raw); if (n_raw > cap) ctr[CT_OVF] = 1; }
    const int dd = d + 1;
    CtChunk cf, c0, c1;
    cf.base = c0.base = c1.base = 0; cf.fill = c0.fill = c1.fill = 0; cf.have = c0.have = c1.have = false;
    uint32_t n_ext = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n; base += (uint64_t)gridDim.x * 64) {
        const uint64_t i = base + lane;
        uint4 e0 = make_uint4(0, 0, 0, 0), e1 = e0;
        if (i < n) { e0 = in[2 * i]; e1 = in[2 * i + 1]; }
        const uint64_t x0a = (uint64_t)e0.y << 32 | e0.x, sza = (uint64_t)e0.w << 32 | e0.z;
        const uint64_t x0b = (uint64_t)e1.y << 32 | e1.x, szb = (uint64_t)e1.w << 32 | e1.z;
        const bool act = (sza | szb) != 0;
        const uint64_t m_act = __ballot(act);
        if (m_act == 0) continue;                     // a run of holes
        n_ext += (uint32_t)__popcll(m_act);
        // both indexes' blocks in flight together: k sides, then (where the interval does not end inside that block) the l sides
        const CtSide A = ct_side(act && sza != 0, x0a, sza), B = ct_side(act && szb != 0, x0b, szb);
        uint64_t tka[6], tla[6], tkb[6], tlb[6];
        fmd_fetch_slot<0>(a, fmd_lds, A.bk, A.hk);
        fmd_fetch_slot<1>(b, fmd_lds, B.bk, B.hk);
        fmd_fetch_wait();
        ct_ranks_k<0>(fmd_lds, A, tka, tla);
        ct_ranks_k<1>(fmd_lds, B, tkb, tlb);
        if (__ballot(A.lsep || B.lsep)) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the k-side LDS reads have returned
            fmd_fetch_slot<0>(a, fmd_lds, A.bl, A.lsep);
            fmd_fetch_slot<1>(b, fmd_lds, B.bl, B.lsep);
            fmd_fetch_wait();
            ct_ranks_l<0>(fmd_lds, A, tla);
            ct_ranks_l<1>(fmd_lds, B, tlb);
        }
        // children c = 1..4 ('N' is never followed, cmp.c:67); where each goes
        bool tf[5], t0[5], t1[5];
        uint64_t na[5], nb[5];
        uint32_t totf = 0, tot0 = 0, tot1 = 0;
#pragma unroll
        for (int c = 1; c <= 4; ++c) {
            na[c] = tla[c] - tka[c]; nb[c] = tlb[c] - tkb[c];
            // the strings of CT_SUF_LEN bases and shorter are pushed without the min_occ test (descend, cmp.c:10-20); each side is compared on its own
            const bool keep = act && (dd <= CT_SUF_LEN ? (na[c] | nb[c]) != 0 : (na[c] >= (uint64_t)min_occ || nb[c] >= (uint64_t)min_occ));
            const bool cls = dd >= CT_SUF_LEN;        // no tips above the roots
            t1[c] = keep && cls && na[c] == 0;                              // cmp.c:61
            t0[c] = keep && cls && na[c] != 0 && nb[c] == 0;                // cmp.c:62
            tf[c] = keep && !t0[c] && !t1[c] && !(cls && dd >= kmer);       // cmp.c:63
            totf += (uint32_t)__popcll(__ballot(tf[c])); tot0 += (uint32_t)__popcll(__ballot(t0[c])); tot1 += (uint32_t)__popcll(__ballot(t1[c]));
        }
        if (totf) {
            unsigned long long o = ct_reserve<2>(out, cap, ch, cf, totf, &ctr[co]);
#pragma unroll
            for (int c = 1; c <= 4; ++c) {
                const uint64_t m = __ballot(tf[c]);
                const unsigned long long at = o + fmd_below(m);
                if (tf[c]) {
                    if (at < cap) { out[2 * at] = ct_pack(a.cnt[c] + tka[c], na[c]); out[2 * at + 1] = ct_pack(b.cnt[c] + tkb[c], nb[c]); }
                    else ctr[CT_OVF] = 1;
                }
                o += __popcll(m);
            }
        }
        if (tot0) {
            unsigned long long o = ct_reserve<1>(tip0, cap, ch, c0, tot0, &ctr[CT_NT0]);
#pragma unroll
            for (int c = 1; c <= 4; ++c) {
                const uint64_t m = __ballot(t0[c]);
                const unsigned long long at = o + fmd_below(m);
                if (t0[c]) { if (at < cap) tip0[at] = ct_pack(a.cnt[c] + tka[c], na[c]); else ctr[CT_OVF] = 1; }
                o += __popcll(m);
            }
        }
        if (tot1) {
            unsigned long long o = ct_reserve<1>(tip1, cap, ch, c1, tot1, &ctr[CT_NT1]);
#pragma unroll
            for (int c = 1; c <= 4; ++c) {
                const uint64_t m = __ballot(t1[c]);
                const unsigned long long at = o + fmd_below(m);
                if (t1[c]) { if (at < cap) tip1[at] = ct_pack(b.cnt[c] + tkb[c], nb[c]); else ctr[CT_OVF] = 1; }
                o += __popcll(m);
            }
        }
    }
    ct_zero_fill<2>(out, cap, ch, cf); ct_zero_fill<1>(tip0, cap, ch, c0); ct_zero_fill<1>(tip1, cap, ch, c1);
    if (lane == 0 && n_ext) atomicAdd(&ctr[CT_EXT], (unsigned long long)n_ext);
}

// one level of the tips of ONE index (collect_tips, cmp.c:22-43): the sentinel child's rows are selected, children 1..4 go on
__global__ __launch_bounds__(64) void k_ct_tip_level(FmdIndexView ix, const uint4 *__restrict__ in, uint4 *__restrict__ out, uint64_t cap, uint32_t ch,
                                                     unsigned long long *__restrict__ ctr, int ci, int co, int stat, unsigned long long *__restrict__ sub)
{
    FMD_DECLARE_WAVE_LDS();
    const int lane = fmd_lane();
    const uint64_t n_raw = ctr[ci], n = n_raw < cap ? n_raw : cap;
    if (blockIdx.x == 0 && lane == 0) { atomicMax(&ctr[CT_DEMAND], (unsigned long long)n_raw); if (n_raw > cap) ctr[CT_OVF] = 1; }
    CtChunk ck; ck.base = 0; ck.fill = 0; ck.have = false;
    uint32_t n_ext = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n; base += (uint64_t)gridDim.x * 64) {
        const uint64_t i = base + lane;
        uint4 e = make_uint4(0, 0, 0, 0);
        if (i < n) e = in[i];
        const uint64_t x0 = (uint64_t)e.y << 32 | e.x, sz = (uint64_t)e.w << 32 | e.z;
        const bool act = sz != 0;
        const uint64_t m_act = __ballot(act);
        if (m_act == 0) continue;
        n_ext += (uint32_t)__popcll(m_act);
        const CtSide A = ct_side(act, x0, sz);
        uint64_t tk[6], tl[6];
        fmd_fetch_slot<0>(ix, fmd_lds, A.bk, A.hk);
        fmd_fetch_slot<1>(ix, fmd_lds, A.bl, A.lsep);    // one index: both ends can be asked for at once
        fmd_fetch_wait();
        ct_ranks_k<0>(fmd_lds, A, tk, tl);
        ct_ranks_l<1>(fmd_lds, A, tl);
        if (act) ct_set_range(sub, ix.n_seq, tk[0], tl[0] - tk[0]);    // cmp.c:32-39: rows ok[0].x[0] .. + ok[0].x[2]
        bool has[5];
        uint32_t tot = 0;
#pragma unroll
        for (int c = 1; c <= 4; ++c) { has[c] = act && tl[c] != tk[c]; tot += (uint32_t)__popcll(__ballot(has[c])); }
        if (tot == 0) continue;
        unsigned long long o = ct_reserve<1>(out, cap, ch, ck, tot, &ctr[co]);
#pragma unroll
        for (int c = 1; c <= 4; ++c) {
            const uint64_t m = __ballot(has[c]);
            const unsigned long long at = o + fmd_below(m);
            if (has[c]) { if (at < cap) out[at] = ct_pack(ix.cnt[c] + tk[c], tl[c] - tk[c]); else ctr[CT_OVF] = 1; }
            o += __popcll(m);
        }
    }
    ct_zero_fill<1>(out, cap, ch, ck);
    if (lane == 0 && n_ext) atomicAdd(&ctr[stat], (unsigned long long)n_ext);
}

// what CT_TIP_LEVELS levels left open: every row of every node LF-walked to its sentinel (a path through an 'N' ends there: the trie
// never follows one).  Persistent waves, tickets over the nodes; a lane takes the rows of its node one after the other.
__global__ __launch_bounds__(64) void k_ct_tip_walk(FmdIndexView ix, const uint4 *__restrict__ in, uint64_t cap, const unsigned long long *__restrict__ ctr, int ci,
                                                    unsigned long long *__restrict__ sub, uint32_t *queue)
{
    FMD_DECLARE_WAVE_LDS();
    const int q = fmd_lane();
    const uint64_t n = ctr[ci] < cap ? ctr[ci] : cap;
    uint64_t k = 0, nxt = 0, end = 0;
    bool live = false, exhausted = false;
    FmdTickets tk;
    fmd_tickets_init(tk, queue);
    for (;;) {
        {
            const bool want = !live && nxt >= end && !exhausted;
            const size_t my = fmd_tickets_take(tk, queue, want);
            if (want) {
                if (my < n) {
                    const uint4 e = in[my];
                    const uint64_t x0 = (uint64_t)e.y << 32 | e.x, sz = (uint64_t)e.w << 32 | e.z;
                    if (sz != 0 && x0 < ix.n_sym && sz <= ix.n_sym - x0) { nxt = x0; end = x0 + sz; }
                } else exhausted = true;
            }
        }
        if (!live && nxt < end) { k = nxt++; live = true; }
        if (__ballot(live) == 0) { if (__ballot(!exhausted) == 0) break; continue; }
        uint32_t bk, ok_;
        fmd_split(live ? k : 0, bk, ok_);
        fmd_fetch_slot<0>(ix, fmd_lds, bk, live);
        fmd_fetch_wait();
        if (live) {
            uint64_t r[6];
            const int c = fmd_block_rank6<true>(fmd_lds + fmd_lds_base(q, 0), fmd_chunk_xor(q), ok_ + 1, r, bk);
            if (c == 0) { ct_set_range(sub, ix.n_seq, r[0] - 1, 1); live = false; }
            else if (c > 4) live = false;
            else {
                k = ix.cnt[c] + sel6<uint64_t>(c, r[0], r[1], r[2], r[3], r[4], r[5]) - 1;
                if (k >= ix.n_sym) live = false;          // (a corrupt index: never walk outside it)
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ sub-index
// set_bits (sub.c:14-28): one lane per sequence whose bit is set in `sub`; ~the walk of k_merge_walk with one index
__global__ __launch_bounds__(64) void k_sub_mark(FmdIndexView ix, const unsigned long long *__restrict__ sub, unsigned long long *__restrict__ bits, uint32_t *queue)
{
    FMD_DECLARE_WAVE_LDS();
    const int q = fmd_lane();
    const size_t n = ix.n_seq;
    uint64_t k = 0;
    bool live = false, exhausted = false;
    FmdTickets tk;
    fmd_tickets_init(tk, queue, 256, n);
    for (;;) {
        for (int tries = 0; tries < 8; ++tries) {     // a sparse selection: several tickets per step until the lanes are busy
            const bool want = !live && !exhausted;
            if (__ballot(want) == 0) break;
            const size_t my = fmd_tickets_take(tk, queue, want, n);
            if (want) {
                if (my < n) {
                    if ((sub[my >> 6] >> (my & 63)) & 1) { k = my; live = true; atomicOr(bits + (k >> 6), 1ull << (k & 63)); }
                } else exhausted = true;
            }
        }
        if (__ballot(live) == 0) { if (__ballot(!exhausted) == 0) break; continue; }
        uint32_t bk, ok_;
        fmd_split(live ? k : 0, bk, ok_);
        fmd_fetch_slot<0>(ix, fmd_lds, bk, live);
        fmd_fetch_wait();
        if (live) {
            uint64_t r[6];
            const int c = fmd_block_rank6<true>(fmd_lds + fmd_lds_base(q, 0), fmd_chunk_xor(q), ok_ + 1, r, bk);
            if (c == 0 || c > 5) live = false;        // back at a sentinel: the sequence is done (c > 5: not an nt6 index)
            else {
                k = ix.cnt[c] + sel6<uint64_t>(c, r[0], r[1], r[2], r[3], r[4], r[5]) - 1;
                if (k < ix.n_sym) atomicOr(bits + (k >> 6), 1ull << (k & 63));
                else live = false;                     // (a corrupt index: never write outside the array)
            }
        }
    }
}

// gen_idx (sub.c:30-55) without the encoder: kept rows (bit == !is_comp) number [first, first + n) as nt6 bytes.  pre[sb] = set bits
// before superblock sb (pre[n_sb] = all).  One wave per superblock from the one the slice begins in, a lane per word = 64 rows.
__global__ __launch_bounds__(64) void k_sub_select(FmdIndexView ix, const unsigned long long *__restrict__ bits, const uint64_t *__restrict__ pre, uint64_t n_sb,
                                                   int is_comp, uint64_t first, uint64_t n, uint8_t *__restrict__ out)
{
    const int q = fmd_lane();
    const uint64_t n_sym = ix.n_sym, rows_sb = 64ull * FMD_BITS_SB_WORDS;
#define SUB_KEPT_BEFORE(sb) (is_comp ? ((sb) * rows_sb < n_sym ? (sb) * rows_sb : n_sym) - pre[sb] : pre[sb])
    uint64_t lo = 0, hi = n_sb;                        // the first superblock with kept rows beyond `first`
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (SUB_KEPT_BEFORE(mid + 1) > first) hi = mid; else lo = mid + 1;
    }
    for (uint64_t sb = lo + blockIdx.x; sb < n_sb; sb += gridDim.x) {
        const uint64_t kb = SUB_KEPT_BEFORE(sb);
        if (kb >= first + n) break;
        const uint64_t wd = sb * FMD_BITS_SB_WORDS + q, p0 = wd * 64;
        uint64_t m = 0;
        if (p0 < n_sym) {
            m = bits[wd];
            if (is_comp) m = ~m;
            if (n_sym - p0 < 64) m &= bits_below((int)(n_sym - p0));
        }
        const unsigned long long mine = (unsigned long long)__popcll(m);
        unsigned long long x = mine;
        for (int s = 1; s < 64; s <<= 1) { const unsigned long long y = __shfl_up(x, s); if (q >= s) x += y; }
        uint64_t o = kb + x - mine;                    // kept rows before p0
        if (m == 0 || o >= first + n || o + mine <= first) continue;
        const uint4 v0 = ix.blocks[fmd_word_u4(p0 >> 5)], v1 = ix.blocks[fmd_word_u4((p0 >> 5) + 1)];   // the block's own two chunks
        const uint64_t X = (uint64_t)v1.x << 32 | v0.x, Y = (uint64_t)v1.y << 32 | v0.y, Z = (uint64_t)v1.z << 32 | v0.z;
        while (m) {
            const int j = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            if (o >= first && o < first + n) out[o - first] = (uint8_t)(((X >> j) & 1) | ((Y >> j) & 1) << 1 | ((Z >> j) & 1) << 2);
            ++o;
        }
    }
#undef SUB_KEPT_BEFORE
}

// -------------------------------------------------------------------------------------------------- host side
extern "C" size_t fmd_contrast_work_bytes(uint64_t cap)
{
    return (size_t)(CT_WORDS * 8 + 256 + cap * (2 * 32 + 2 * 16));   // counters, two pair frontiers, two tip lists
}

static int contrast_args(const fmd_dev *h0, const fmd_dev *h1, int k, int min_occ)
{
    if (!h0 || !h1 || h0->device != h1->device) return FMD_E_ARG;
    if (k <= CT_SUF_LEN || min_occ < 1) return FMD_E_ARG;           // cmp.c:101; min_occ < 1 would expand all 4^k strings
    return FMD_OK;
}

extern "C" int fmd_contrast_dev(fmd_dev_t *h0, fmd_dev_t *h1, void *stream, int k, int min_occ, int seed_mask, uint64_t *d_sub0, uint64_t *d_sub1,
                                void *d_work, size_t work_bytes, uint64_t cap, uint64_t *d_status)
{
    int rc = contrast_args(h0, h1, k, min_occ);
    if (rc) return rc;
    if (!d_sub0 || !d_sub1 || !d_work || !d_status || !(seed_mask & 0xf) || (seed_mask & ~0xf)) return FMD_E_ARG;
    if (cap < CT_MIN_CAP || cap >= 0xffffff00ull || work_bytes < fmd_contrast_work_bytes(cap)) return FMD_E_ARG;   // 32-bit ticket queue over the lists
    FMD_HIP_TRY(hipSetDevice(h0->device));
    hipStream_t st = S(stream);
    unsigned long long *ctr = (unsigned long long *)d_work;
    uint4 *fa = (uint4 *)(((uintptr_t)((uint8_t *)d_work + CT_WORDS * 8) + 255) & ~(uintptr_t)255);
    uint4 *fb = fa + 2 * cap, *tip[2] = {fb + 2 * cap, fb + 3 * cap};
    FMD_HIP_TRY(hipMemsetAsync(ctr, 0, CT_WORDS * 8, st));
    const FmdIndexView va = fmd_view(h0), vb = fmd_view(h1);
    static int per_cu = 0;
    if (!per_cu) {
        const int a = fmd_resident_per_cu(k_ct_level, FMD_WAVE_LDS_U4 * 16, 16, "k_ct_level");
        const int b = fmd_resident_per_cu(k_ct_tip_level, FMD_WAVE_LDS_U4 * 16, 16, "k_ct_tip_level");
        per_cu = a < b ? a : b;
    }
    // the level kernels walk their list by static strides: no more waves than are resident, and no more than can hold a chunk each
    // of every list without the chunks' unused ends eating the capacity
    uint32_t ch = 1024;
    int grid = fmd_grid_for_lds(h0, cap, FMD_WAVE_LDS_U4 * 16);
    if (grid > h0->n_cu * per_cu) grid = h0->n_cu * per_cu;
    while (ch > 256 && (uint64_t)grid * ch * 8 > cap) ch >>= 1;
    if ((uint64_t)grid * ch * 4 > cap) grid = (int)(cap / (ch * 4ull));
    if (grid < 1) grid = 1;
    k_ct_seed<<<1, 64, 0, st>>>(va, vb, seed_mask, fa, ctr);
    int ci = CT_NA, co = CT_NB;
    uint4 *in = fa, *out = fb;
    for (int d = 1; d < k; ++d) {
        FMD_HIP_TRY(hipMemsetAsync(ctr + co, 0, 8, st));
        k_ct_level<<<grid, 64, 0, st>>>(va, vb, d, k, min_occ, in, out, tip[0], tip[1], cap, ch, ctr, ci, co);
        uint4 *t = in; in = out; out = t;
        const int ti = ci; ci = co; co = ti;
    }
    FMD_HIP_TRY(hipGetLastError());
    // the tips, one index after the other; their frontiers take the pair frontiers' room
    for (int side = 0; side < 2; ++side) {
        fmd_dev *h = side ? h1 : h0;
        const FmdIndexView v = side ? vb : va;
        unsigned long long *sub = (unsigned long long *)(side ? d_sub1 : d_sub0);
        const uint4 *tin = tip[side];
        int ti = side ? CT_NT1 : CT_NT0, to = CT_NA;
        uint4 *tout = fa;
        for (int lv = 0; lv < CT_TIP_LEVELS; ++lv) {
            FMD_HIP_TRY(hipMemsetAsync(ctr + to, 0, 8, st));
            k_ct_tip_level<<<grid, 64, 0, st>>>(v, tin, tout, cap, ch, ctr, ti, to, side ? CT_TIP1 : CT_TIP0, sub);
            tin = tout; ti = to;
            tout = tout == fa ? fb : fa; to = to == CT_NA ? CT_NB : CT_NA;
        }
        uint32_t *queue = fmd_next_queue(h, st);
        k_ct_tip_walk<<<fmd_grid_for(h, cap), 64, 0, st>>>(v, tin, cap, ctr, ti, sub, queue);
        FMD_HIP_TRY(hipGetLastError());
    }
    FMD_HIP_TRY(hipMemcpyAsync(d_status, ctr + CT_EXT, 4 * 8, hipMemcpyDeviceToDevice, st));
    return FMD_OK;
}

// One part of the walk (seed_mask) with the capacity grown until nothing overflows.  The arrays are only OR-ed into and every bit an
// overflowed pass set is a right one, so a pass is simply run again.
static int contrast_part_host(fmd_dev_t *h0, fmd_dev_t *h1, int k, int min_occ, int seed_mask, uint64_t cap0, uint64_t *d_sub0, uint64_t *d_sub1)
{
    uint64_t cap = cap0, demand = 0;
    for (int attempt = 0; attempt < 32; ++attempt) {
        if (attempt) {
            const uint64_t by_demand = demand + demand / 5 + 1024;
            cap = by_demand > 2 * cap ? by_demand : 2 * cap;
        }
        if (cap >= 0xffffff00ull) return FMD_E_OVERFLOW;
        FmdDevBuf work, ds;
        const size_t wb = fmd_contrast_work_bytes(cap);
        int rc;
        if ((rc = work.alloc(wb)) || (rc = ds.alloc(32))) return rc;
        uint64_t status[4] = {0, 0, 0, 0};
        unsigned long long ctr[CT_WORDS];
        rc = fmd_contrast_dev(h0, h1, nullptr, k, min_occ, seed_mask, d_sub0, d_sub1, work.p, wb, cap, ds.as<uint64_t>());
        if (rc == FMD_OK && hipMemcpy(status, ds.p, 32, hipMemcpyDeviceToHost) != hipSuccess) rc = FMD_E_HIP;
        if (rc == FMD_OK && status[1] != 0 && hipMemcpy(ctr, work.p, sizeof(ctr), hipMemcpyDeviceToHost) == hipSuccess) demand = ctr[CT_DEMAND];
        if (rc != FMD_OK) return rc;
        if (status[1] == 0) return FMD_OK;
    }
    return FMD_E_OVERFLOW;
}

// fm6_contrast (cmp.c:94-126): bits by sorted order of the sequences (the i-th '$' of the BWT), before fm6_sub_conv; the arrays are malloc'ed (fmd_host_free).  One pass when
// the frontiers fit beside the two indexes, else the four parts by last base.  FMD_CONTRAST_CAP / FMD_CONTRAST_PARTS (1 or 4): the
// first capacity and the number of parts, for tests of the re-run paths -- the result does not depend on either.
extern "C" int fmd_contrast(fmd_dev_t *h0, fmd_dev_t *h1, int k, int min_occ, uint64_t **sub0, uint64_t **sub1)
{
    int rc = contrast_args(h0, h1, k, min_occ);
    if (rc) return rc;
    if (!sub0 || !sub1) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h0->device));
    const uint64_t nw[2] = {(h0->mcnt[1] + 63) / 64, (h1->mcnt[1] + 63) / 64};
    FmdDevBuf d[2];
    uint64_t *out[2] = {nullptr, nullptr};
    // the widest level holds about one node per distinct k-mer of the two samples: symbols / 24 at 30-fold coverage with a few errors per
    // thousand bases; never more than half of the free memory (96 bytes per entry), and the walk runs again when it was too little
    uint64_t cap0 = (h0->mcnt[0] + h1->mcnt[0]) / 24;
    int parts = 1;
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)16 << 30; }
        if (cap0 > free_b / 2 / 96) cap0 = free_b / 2 / 96;
        if (cap0 < (1u << 20)) cap0 = 1u << 20;
    }
    { const char *e = getenv("FMD_CONTRAST_CAP"); if (e && atoll(e) >= (long long)CT_MIN_CAP) cap0 = (uint64_t)atoll(e); }
    { const char *e = getenv("FMD_CONTRAST_PARTS"); if (e && (atoi(e) == 1 || atoi(e) == 4)) parts = atoi(e); }
    for (int i = 0; i < 2 && rc == FMD_OK; ++i) {
        if ((rc = d[i].alloc((nw[i] + 1) * 8))) break;
        if (hipMemset(d[i].p, 0, (nw[i] + 1) * 8) != hipSuccess) rc = FMD_E_HIP;
    }
    while (rc == FMD_OK) {
        for (int p = 0; p < parts && rc == FMD_OK; ++p) rc = contrast_part_host(h0, h1, k, min_occ, parts == 1 ? 0xf : 1 << p, cap0, d[0].as<uint64_t>(), d[1].as<uint64_t>());
        if (rc != FMD_E_NOMEM || parts != 1) break;
        parts = 4; rc = FMD_OK;      // the frontiers of the whole trie did not fit: a quarter at a time
    }
    for (int i = 0; i < 2 && rc == FMD_OK; ++i) {
        out[i] = (uint64_t *)calloc(nw[i] + 1, 8);
        if (!out[i]) rc = FMD_E_NOMEM;
        else if (nw[i] && hipMemcpy(out[i], d[i].p, nw[i] * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = FMD_E_HIP;
    }
    if (rc) { free(out[0]); free(out[1]); return rc; }
    *sub0 = out[0]; *sub1 = out[1];
    return FMD_OK;
}

// ---- sub-index
extern "C" size_t fmd_sub_work_bytes(uint64_t n_sym) { return fmd_bits_work_bytes(n_sym); }

extern "C" int fmd_sub_mark_dev(fmd_dev_t *h, void *stream, const uint64_t *d_sub, uint64_t *d_bits, void *d_work, size_t work_bytes, uint64_t *d_n_kept)
{
    if (!h || !d_sub || !d_bits || !d_work) return FMD_E_ARG;
    if (h->mcnt[1] >= 0xffffff00ull) return FMD_E_ARG;               // 32-bit ticket queue
    const uint64_t n_sym = h->mcnt[0], n_sb = fmd_bits_n_sb(n_sym);
    if (work_bytes < fmd_sub_work_bytes(n_sym)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h->device));
    uint32_t *queue = fmd_next_queue(h, S(stream));
    k_sub_mark<<<fmd_grid_for(h, h->mcnt[1]), 64, 0, S(stream)>>>(fmd_view(h), (const unsigned long long *)d_sub, (unsigned long long *)d_bits, queue);
    FMD_HIP_TRY(hipGetLastError());
    const int rc = fmd_bits_rank_dev(S(stream), d_bits, n_sym, d_work, work_bytes);
    if (rc) return rc;
    if (d_n_kept) FMD_HIP_TRY(hipMemcpyAsync(d_n_kept, (const uint64_t *)d_work + n_sb, 8, hipMemcpyDeviceToDevice, S(stream)));
    return FMD_OK;
}

extern "C" int fmd_sub_select_dev(fmd_dev_t *h, void *stream, const uint64_t *d_bits, const void *d_work, int is_comp, uint64_t first, uint64_t n, uint8_t *d_out)
{
    if (!h || !d_bits || !d_work || (n && !d_out)) return FMD_E_ARG;
    if (first > h->mcnt[0] || n > h->mcnt[0] - first) return FMD_E_ARG;   // (a slice beyond the kept rows writes nothing)
    if (n == 0) return FMD_OK;
    FMD_HIP_TRY(hipSetDevice(h->device));
    // a slice of n kept rows spans at least n / 4096 superblocks and any number more: the waves stride from the first one until they
    // are past the slice
    k_sub_select<<<fmd_wave_grid(n / (64 * FMD_BITS_SB_WORDS) + 64), 64, 0, S(stream)>>>(fmd_view(h), (const unsigned long long *)d_bits, (const uint64_t *)d_work,
                                                                             fmd_bits_n_sb(h->mcnt[0]), is_comp != 0, first, n, d_out);
    FMD_HIP_TRY(hipGetLastError());
    return FMD_OK;
}

// fm_sub (sub.c:71-97) into a new resident index
#define SUB_SLICE (1ull << 28)
extern "C" int fmd_dev_sub(fmd_dev_t *h0, const uint64_t *sub, int is_comp, unsigned flags, fmd_dev_t **out)
{
    if (!h0 || !sub || !out || (flags & ~FMD_OPEN_NO_TABLES)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h0->device));
    const uint64_t n_sym = h0->mcnt[0], n_words = (n_sym + 63) / 64, sub_words = (h0->mcnt[1] + 63) / 64;
    const size_t wb = fmd_sub_work_bytes(n_sym);
    FmdDevBuf bits, work, d_sub, buf;
    fmd_dev *h = nullptr;
    hipStream_t st = nullptr;
    uint64_t n_set = 0;
    int rc;
    if ((rc = bits.alloc(n_words * 8 + 8)) || (rc = work.alloc(wb)) || (rc = d_sub.alloc(sub_words * 8 + 8))) return rc;
    uint64_t *d_n_set = bits.as<uint64_t>() + n_words;                // the count lands behind the bit array
    if (hipMemsetAsync(bits.p, 0, n_words * 8 + 8, st) != hipSuccess || hipMemcpy(d_sub.p, sub, sub_words * 8, hipMemcpyHostToDevice) != hipSuccess) return FMD_E_HIP;
    rc = fmd_sub_mark_dev(h0, st, d_sub.as<uint64_t>(), bits.as<uint64_t>(), work.p, wb, d_n_set);
    if (rc) return rc;
    if (hipMemcpy(&n_set, d_n_set, 8, hipMemcpyDeviceToHost) != hipSuccess) return FMD_E_HIP;
    const uint64_t n_out = is_comp ? n_sym - n_set : n_set;
    if (n_out == 0) return FMD_E_ARG;                                // nothing selected: there is no resident form of an empty index
    const uint64_t slice = n_out < SUB_SLICE ? n_out : SUB_SLICE;
    if ((rc = buf.alloc(slice))) return rc;
    rc = fmd_index_alloc(h0->device, n_out, &h);
    if (rc) return rc;
    for (uint64_t at = 0; at < n_out && rc == FMD_OK; at += slice) {
        const uint64_t m = n_out - at < slice ? n_out - at : slice;
        rc = fmd_sub_select_dev(h0, st, bits.as<uint64_t>(), work.p, is_comp, at, m, buf.as<uint8_t>());
        if (rc == FMD_OK) rc = fmd_index_put_slice(h, st, buf.as<uint8_t>(), at, m);
    }
    if (rc == FMD_OK) {
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) { fmd_set_hip_error(e, "sub"); rc = FMD_E_HIP; }
    }
    buf.reset(); work.reset(); bits.reset(); d_sub.reset();   // the selection's own arrays go before the counts' scratch comes
    if (rc == FMD_OK) rc = fmd_index_finish(h, !(flags & FMD_OPEN_NO_TABLES));
    if (rc) { fmd_dev_close(h); return rc; }
    *out = h;
    return FMD_OK;
}
