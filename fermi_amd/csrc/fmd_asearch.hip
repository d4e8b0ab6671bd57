// fmd_asearch.hip -- asearch: search with up to max_sub substitutions (the semantics are stated in include/fmd_hip.h).
//
// The patterns within max_sub substitutions of a query form a trie rooted at the query's LAST base; the ones that occur are the trie of the index
// cut to that ball.  The walk is the third user of fmd_level.h: level by level, one backward extension per item (km_extend_back), frontier slots
// reserved in chunks, the frontier cut into one range per XCD, no per-lane stack.  An item is an SA interval, its query and the substitutions
// spent so far -- their list packed in one 64-bit register.  Level 0 (k_asearch_seed) takes the last base from the marginal counts; an item of
// level t >= 1 stands before position L - 1 - t of its query.  The child of base c goes on at the same budget when c is the query's base there and
// at one more otherwise; a child that would face position p - 1 with s substitutions is pushed only if s + lb[p - 1] <= max_sub, lb being the
// lower bound k_asearch_bound computes (BWA's D); the children of position 0 are the hits.  Hits leave through a buffer in LDS, one atomic per
// flush; the strata are counted with atomics on the query's own words.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>
#include "fmd_internal.h"
#include "fmd_kernel_common.h"
#include "fmd_level.h"

// An item: the rows [x0, x0 + size) -- positions and sizes are 64 bits throughout --, the query, the substitutions spent and their list (four
// 16-bit fields, the first substitution found -- the highest position -- lowest, unused fields 0xffff: the image of fmd_asearch_hit_t::sub).
// All zero = a hole (size 0).  A hit has the same shape: {beg, cnt, query, n_sub, sub}.
struct AsrItem { uint64_t x0, size; uint32_t query, n_sub; uint64_t subs; };
static_assert(sizeof(AsrItem) == 32 && sizeof(AsrItem) % 16 == 0 && offsetof(AsrItem, size) == 8 && offsetof(AsrItem, query) == 16 && offsetof(AsrItem, subs) == 24,
              "a frontier entry is two 16-byte words");
static_assert(sizeof(fmd_asearch_hit_t) == 32 && offsetof(fmd_asearch_hit_t, cnt) == 8 && offsetof(fmd_asearch_hit_t, query) == 16 &&
              offsetof(fmd_asearch_hit_t, n_sub) == 20 && offsetof(fmd_asearch_hit_t, sub) == 24 && sizeof(fmd_asearch_stat_t) == 64, "layouts of include/fmd_hip.h");
static_assert(FMD_ASEARCH_MAX_SUB == 4 && (((FMD_ASEARCH_MAX_LEN - 1) << 2) | 3u) < 0xffffu, "four 16-bit fields of pos << 2 | base - 1 (pos < MAX_LEN), 0xffff = unused");

// counters at the head of the work area (u64 words): the frontier sizes rotate through words 0..2 as locate's do -- level t reads word t % 3, counts
// its children in word (t + 1) % 3 and clears word (t + 2) % 3; level 0 counts in word 1
#define ASR_HITS 3       // hits staged for d_hits (counts on when d_hits is full)
#define ASR_SKIP 4       // queries level 0 left out
#define ASR_UNFIN 5      // items still walking after the last level
#define ASR_OVF 6        // a frontier entry did not fit
#define ASR_EXT 7        // backward extensions done
#define ASR_WIDEST 8     // the most slots a level reserved
#define ASR_TRUNC 9      // queries with more than max_hits hits
#define ASR_NHITS 10     // hits of the others
#define ASR_NOCC 11      // ... and the sum of their cnt
#define ASR_WORDS 16
#define ASR_HDR_BYTES 256
// behind the header: one u64 per query, its hits so far (what decides max_hits), then the two frontiers
static inline size_t asr_tot_bytes(size_t n) { return align_up(n * 8, 256); }
// A wave reserves frontier slots a chunk at a time and fills a chunk to its last slot before it takes the next (km_reserve_split): a level holds its
// live items + the tail of at most one chunk per wave.  Chunk and grid follow the capacity so that the tails take at most half of it (asr_plan).
#define ASR_CHUNK 512u
#define ASR_MIN_CHUNK 256u
static_assert(ASR_MIN_CHUNK >= 4 * 64 && FMD_ASEARCH_MIN_CAP >= 2 * 8 * ASR_MIN_CHUNK, "one step's children fit one chunk; the smallest capacity holds eight waves' tails and as much again");
// Hits leave through ASR_HIT_BUF entries in the wave's LDS, behind the rank engine's landing area, flushed with ONE atomic when the next child's hits
// (at most 64) might not fit -- as locate's runs do (loc_flush_runs): one atomic on the hit counter per step costs more than the step.
#define ASR_HIT_BUF 128
#define ASR_LDS_U4 (FMD_COMPACT_LDS_U4 + 2 * ASR_HIT_BUF)
static_assert(ASR_HIT_BUF >= 64, "the hits of one child of one step fit the buffer");

extern "C" size_t fmd_asearch_work_bytes(size_t n, uint64_t cap)
{
    if (cap < FMD_ASEARCH_MIN_CAP || cap > FMD_ASEARCH_MAX_CAP || n >= (1ull << 32)) return 0;
    return ASR_HDR_BYTES + asr_tot_bytes(n) + 2 * (size_t)cap * sizeof(AsrItem);
}

// what the kernels of one walk share
struct AsrArgs {
    const uint8_t *seqs; const uint64_t *off; const uint8_t *lb;   // lb = nullptr: no pruning
    uint32_t max_sub, max_hits;
    unsigned long long *ctr, *tot, *strata;
    fmd_asearch_hit_t *hits; uint64_t hit_cap;                    // hits = nullptr: count only
    uint64_t cap;                                                  // entries of a frontier
};

// ---- the bound: one query per lane, one backward search with restarts over comp(q[0]), comp(q[1]), .. -- after p + 1 bases the interval is that of
// rc(q[s .. p]), s = the position after the last restart, which occurs iff q[s .. p] does on an index of both strands.  When it empties at p the count z
// goes up and the next base starts afresh from the marginal counts; lb[p] = min(z, 255).  A base that is not A/C/G/T empties it by construction.
// both = 0 (not an index of both strands): zeros.
__global__ __launch_bounds__(64) void k_asearch_bound(FmdIndexView ix, size_t n, const uint8_t *__restrict__ seqs, const uint64_t *__restrict__ off,
                                                      uint8_t *__restrict__ lb, int both)
{
    FMD_DECLARE_COMPACT_LDS();
    const int lane = fmd_lane();
    for (size_t base = (size_t)blockIdx.x * 64; base < n; base += (size_t)gridDim.x * 64) {
        const size_t i = base + lane;
        uint64_t o0 = 0, L = 0;
        if (i < n) { o0 = off[i]; L = off[i + 1] - o0; if (L > FMD_ASEARCH_MAX_LEN) L = 0; }
        uint64_t k = 0, l = 0, p = 0;
        uint32_t z = 0;
        bool fresh = true;
        if (!both) {
            for (; p < L; ++p) lb[o0 + p] = 0;
            continue;
        }
        while (__ballot(p < L)) {
            const bool live = p < L;
            int c = 0;
            if (live) { const int qb = seqs[o0 + p]; c = (qb >= 1 && qb <= 4) ? 5 - qb : 0; }
            const bool ext = live && c != 0 && !fresh;
            FmdRank2c r = fmd_wave_rank2_fetch_compact(ix, fmd_lds, ext ? k - 1 : NONE64, ext ? l : NONE64);
            const uint64_t ok = (ext && r.hk) ? fmd_block_rank1(r.bk, r.t, r.nk, c, r.blk_k) : 0;
            fmd_wave_l_ready(ix, fmd_lds, r);
            if (live) {
                bool empty = true;
                if (c != 0 && fresh) { k = ix.cnt[c]; l = ix.cnt[c + 1] - 1; empty = ix.cnt[c + 1] == ix.cnt[c]; }
                else if (c != 0) {
                    const uint64_t ol = fmd_block_rank1(r.bl, r.tl, r.nl, c, r.blk_l);
                    k = ix.cnt[c] + ok; l = ix.cnt[c] + ol - 1;
                    empty = ol <= ok;
                }
                if (empty) ++z;
                fresh = empty;
                lb[o0 + p] = (uint8_t)(z < 255u ? z : 255u);
                ++p;
            }
        }
    }
}

// ---- hits: counted on the query's words, staged in LDS, flushed with one atomic
// the staged hits -> d_hits (all 64 lanes together)
__device__ __forceinline__ void asr_flush_hits(const uint4 *buf, uint32_t &fill, const AsrArgs &a)
{
    if (fill == 0) return;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the lanes that wrote the entries are not the lanes that read them
    unsigned long long first = 0;
    if (fmd_lane() == 0) first = atomicAdd(&a.ctr[ASR_HITS], (unsigned long long)fill);
    first = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(first >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)first);
    for (uint32_t j = (uint32_t)fmd_lane(); j < fill; j += 64) {
        const uint4 e0 = buf[2 * j], e1 = buf[2 * j + 1];
        if (first + j < a.hit_cap) {                      // (past hit_cap: k_asearch_stat sets the flag, the counter went past it)
            uint4 *q = (uint4 *)(a.hits + first + j);
            q[0] = e0; q[1] = e1;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // read before the next step overwrites them
    fill = 0;
}
// One child of one step: the lanes with `hit` have found the pattern with interval [x0, x0 + sz), s substitutions, list `subs`, of query qi.
__device__ __forceinline__ void asr_emit(bool hit, uint64_t x0, uint64_t sz, uint32_t qi, uint32_t s, uint64_t subs, uint4 *buf, uint32_t &fill, const AsrArgs &a)
{
    if (__ballot(hit) == 0) return;
    bool list = false;
    if (hit) {
        unsigned long long *w = a.strata + ((uint64_t)qi * (a.max_sub + 1) + s) * 2;
        atomicAdd(w, 1ull); atomicAdd(w + 1, (unsigned long long)sz);
        list = atomicAdd(&a.tot[qi], 1ull) < a.max_hits && a.hits != nullptr;
    }
    const uint64_t m = __ballot(list);
    if (m == 0) return;
    const uint32_t nl = (uint32_t)__popcll(m);
    if (fill + nl > ASR_HIT_BUF) asr_flush_hits(buf, fill, a);
    if (list) {
        const uint32_t j = fill + (uint32_t)fmd_below(m);
        buf[2 * j] = make_uint4((uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)sz, (uint32_t)(sz >> 32));
        buf[2 * j + 1] = make_uint4(qi, s, (uint32_t)subs, (uint32_t)(subs >> 32));
    }
    fill += nl;
}
// the list with one more entry: the s-th substitution (s < FMD_ASEARCH_MAX_SUB), base c at position p
__device__ __forceinline__ uint64_t asr_subs_add(uint64_t subs, uint32_t s, uint64_t p, int c)
{
    const uint32_t sh = 16 * (s & 3);
    return (subs & ~(0xffffull << sh)) | ((p << 2 | (uint64_t)(c - 1)) << sh);
}
__device__ __forceinline__ void asr_store_item(AsrItem *out, uint64_t o, uint64_t x0, uint64_t sz, uint32_t qi, uint32_t s, uint64_t subs, const AsrArgs &a)
{
    if (o < a.cap) {
        uint4 *q = (uint4 *)(out + o);
        q[0] = make_uint4((uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)sz, (uint32_t)(sz >> 32));
        q[1] = make_uint4(qi, s, (uint32_t)subs, (uint32_t)(subs >> 32));
    } else a.ctr[ASR_OVF] = 1;
}

// The children of one step, c = 1 .. 4: kept[c] says the child occurs and its budget allows it; at position p == 0 they are hits, else items.
#define ASR_CHILDREN(x0_of, sz_of)                                                                \
    const uint64_t m1 = __ballot(kept1 && !last), m2 = __ballot(kept2 && !last), m3 = __ballot(kept3 && !last), m4 = __ballot(kept4 && !last); \
    const uint32_t p1 = (uint32_t)__popcll(m1), p2 = p1 + (uint32_t)__popcll(m2), p3 = p2 + (uint32_t)__popcll(m3), tot = p3 + (uint32_t)__popcll(m4); \
    KmSpan sp; sp.a = 0; sp.b = 0; sp.na = 0;                                                     \
    if (tot) sp = km_reserve_split(ck, tot, &a.ctr[w_out]);                                       \
    ASR_CHILD(1, kept1, m1, 0u, x0_of, sz_of) ASR_CHILD(2, kept2, m2, p1, x0_of, sz_of) ASR_CHILD(3, kept3, m3, p2, x0_of, sz_of) ASR_CHILD(4, kept4, m4, p3, x0_of, sz_of)
#define ASR_CHILD(c, kept, m, before, x0_of, sz_of)                                               \
    {                                                                                             \
        const bool sub_c = qb != (c);                                                             \
        const uint32_t s_c = s + (sub_c ? 1u : 0u);                                               \
        const uint64_t subs_c = sub_c ? asr_subs_add(subs, s, p, (c)) : subs;                     \
        asr_emit((kept) && last, x0_of(c), sz_of(c), qi, s_c, subs_c, hit_buf, hit_fill, a);      \
        if ((kept) && !last) asr_store_item(out, km_span_slot(sp, (before) + (uint32_t)fmd_below(m)), x0_of(c), sz_of(c), qi, s_c, subs_c, a); \
    }
// which children the budget allows: bit c of the result (s = spent so far, qb = the query's base at p, lbv = lb[p - 1], 0 at p = 0 or without the bound)
__device__ __forceinline__ uint32_t asr_allowed(uint32_t s, int qb, uint32_t lbv, uint32_t max_sub)
{
    uint32_t keep = 0;
#pragma unroll
    for (int c = 1; c <= 4; ++c) keep |= (s + (qb != c ? 1u : 0u) + lbv <= max_sub) ? 1u << c : 0u;
    return keep;
}

// level 0: one query per lane, the last base from the marginal counts
__global__ __launch_bounds__(64) void k_asearch_seed(FmdIndexView ix, size_t n, AsrArgs a, AsrItem *__restrict__ out, uint32_t ch)
{
    __shared__ uint4 hit_buf[2 * ASR_HIT_BUF];
    uint32_t hit_fill = 0;                            // wave-uniform
    const int lane = fmd_lane();
    const uint32_t w_out = 1;
    KmChunk ck; ck.base = 0; ck.fill = 0; ck.ch = ch; ck.have = false;
    uint32_t n_skip = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n; base += (uint64_t)gridDim.x * 64) {
        const uint64_t i = base + lane;
        uint64_t o0 = 0, L = 0;
        if (i < n) { o0 = a.off[i]; L = a.off[i + 1] - o0; }
        const bool skip = i < n && (L == 0 || L > FMD_ASEARCH_MAX_LEN);
        const bool act = i < n && !skip;
        n_skip += (uint32_t)__popcll(__ballot(skip));
        const uint32_t qi = (uint32_t)i, s = 0;
        const uint64_t subs = ~0ull, p = act ? L - 1 : 0;
        const bool last = p == 0;
        int qb = 0;
        uint32_t lbv = 0;
        if (act) { qb = a.seqs[o0 + p]; if (!last && a.lb) lbv = a.lb[o0 + p - 1]; }
        const uint32_t keep = act ? asr_allowed(s, qb, lbv, a.max_sub) : 0u;
#define ASR_X0(c) ix.cnt[c]
#define ASR_SZ(c) (ix.cnt[(c) + 1] - ix.cnt[c])
        const bool kept1 = (keep & 2u) && ASR_SZ(1) != 0, kept2 = (keep & 4u) && ASR_SZ(2) != 0, kept3 = (keep & 8u) && ASR_SZ(3) != 0, kept4 = (keep & 16u) && ASR_SZ(4) != 0;
        ASR_CHILDREN(ASR_X0, ASR_SZ)
#undef ASR_X0
#undef ASR_SZ
    }
    km_zero_fill(out, a.cap, ck);
    asr_flush_hits(hit_buf, hit_fill, a);
    if (lane == 0 && n_skip) atomicAdd(&a.ctr[ASR_SKIP], (unsigned long long)n_skip);
}

// one level: the items that stand before position L - 1 - t of their queries -> hits (position 0) + the items of level t + 1
__global__ __launch_bounds__(64) void k_asearch_level(FmdIndexView ix, uint32_t t, AsrArgs a, const AsrItem *__restrict__ in, AsrItem *__restrict__ out, uint32_t ch,
                                                      int xcd_aware)
{
    __shared__ uint4 fmd_lds[ASR_LDS_U4];             // one array: the landing area of the rank engine, then the hit buffer
    uint4 *hit_buf = fmd_lds + FMD_COMPACT_LDS_U4;
    uint32_t hit_fill = 0;                            // wave-uniform
    const int lane = fmd_lane();
    const uint32_t w_in = t % 3, w_out = (t + 1) % 3, w_clr = (t + 2) % 3;
    const uint64_t n_raw = a.ctr[w_in], n = n_raw < a.cap ? n_raw : a.cap;   // an overflowing level counted more than it stored
    if (blockIdx.x == 0 && lane == 0) { a.ctr[w_clr] = 0; if (n_raw > a.ctr[ASR_WIDEST]) a.ctr[ASR_WIDEST] = n_raw; }
    const KmRange rg = km_range(n, xcd_aware);
    const uint64_t stride = rg.stride;
    KmChunk ck; ck.base = 0; ck.fill = 0; ck.ch = ch; ck.have = false;
    uint32_t n_ext = 0;
    uint4 na = make_uint4(0, 0, 0, 0), nb = na;       // the item of the next iteration, loaded one gather ahead
    if (rg.beg + lane < rg.end) { const uint4 *q = (const uint4 *)(in + rg.beg + lane); na = q[0]; nb = q[1]; }
    for (uint64_t base = rg.beg; base < rg.end; base += stride) {
        const uint4 ia = na, ib = nb;
        const uint64_t x0 = (uint64_t)ia.y << 32 | ia.x, sz = (uint64_t)ia.w << 32 | ia.z, subs = (uint64_t)ib.w << 32 | ib.z;
        const uint32_t qi = ib.x, s = ib.y;
        const bool live = base + lane < rg.end && sz != 0;
        na = make_uint4(0, 0, 0, 0); nb = na;
        if (base + stride + lane < rg.end) { const uint4 *q = (const uint4 *)(in + base + stride + lane); na = q[0]; nb = q[1]; }
        if (__ballot(live) == 0) continue;            // a run of holes
        // the query's base at the item's position, and the bound for what is left of the query beyond it
        uint64_t p = 0;
        int qb = 0;
        uint32_t lbv = 0;
        if (live) {
            const uint64_t o0 = a.off[qi];
            p = a.off[qi + 1] - o0 - 1 - t;
            qb = a.seqs[o0 + p];
            if (p != 0 && a.lb) lbv = a.lb[o0 + p - 1];
        }
        const bool last = p == 0;
        const uint32_t keep = live ? asr_allowed(s, qb, lbv, a.max_sub) : 0u;
        const bool act = keep != 0;                   // (budget spent and an N ahead: no child is allowed, nothing to extend)
        const uint64_t m_act = __ballot(act);
        if (m_act == 0) continue;
        n_ext += (uint32_t)__popcll(m_act);
        uint64_t tk[6], sc[6];
        km_extend_back<true, false, true>(ix, fmd_lds, act, x0, sz, 1, tk, sc, keep);
        const bool kept1 = (keep & 2u) && sc[1] != 0, kept2 = (keep & 4u) && sc[2] != 0, kept3 = (keep & 8u) && sc[3] != 0, kept4 = (keep & 16u) && sc[4] != 0;
#define ASR_X0(c) (ix.cnt[c] + tk[c])
#define ASR_SZ(c) sc[c]
        ASR_CHILDREN(ASR_X0, ASR_SZ)
#undef ASR_X0
#undef ASR_SZ
    }
    km_zero_fill(out, a.cap, ck);
    asr_flush_hits(hit_buf, hit_fill, a);
    if (lane == 0 && n_ext) atomicAdd(&a.ctr[ASR_EXT], (unsigned long long)n_ext);
}
#undef ASR_CHILDREN
#undef ASR_CHILD

// after the last level: the items still walking (the frontier level t would read), and per query whether it is truncated
__global__ __launch_bounds__(64) void k_asearch_rest(uint32_t t, size_t n, AsrArgs a, const AsrItem *__restrict__ in)
{
    const uint64_t n_raw = a.ctr[t % 3], m = n_raw < a.cap ? n_raw : a.cap;
    uint64_t unfin = 0, trunc = 0, nh = 0, no = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 64 + fmd_lane(); i < m; i += (uint64_t)gridDim.x * 64) unfin += in[i].size != 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 64 + fmd_lane(); i < n; i += (uint64_t)gridDim.x * 64) {
        const uint64_t v = a.tot[i];
        if (v > a.max_hits) ++trunc;
        else if (v) {
            nh += v;
            for (uint32_t j = 0; j <= a.max_sub; ++j) no += a.strata[(i * (a.max_sub + 1) + j) * 2 + 1];
        }
    }
    unfin = km_wave_sum(unfin); trunc = km_wave_sum(trunc); nh = km_wave_sum(nh); no = km_wave_sum(no);
    if (fmd_lane() == 0) {
        if (unfin) atomicAdd(&a.ctr[ASR_UNFIN], (unsigned long long)unfin);
        if (trunc) atomicAdd(&a.ctr[ASR_TRUNC], (unsigned long long)trunc);
        if (nh) { atomicAdd(&a.ctr[ASR_NHITS], (unsigned long long)nh); atomicAdd(&a.ctr[ASR_NOCC], (unsigned long long)no); }
    }
}
__global__ void k_asearch_stat(uint32_t t, AsrArgs a, fmd_asearch_stat_t *__restrict__ stat)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    fmd_asearch_stat_t s;
    s.n_hits = a.ctr[ASR_NHITS]; s.n_occ = a.ctr[ASR_NOCC]; s.n_skipped = a.ctr[ASR_SKIP]; s.n_truncated = a.ctr[ASR_TRUNC]; s.n_unfinished = a.ctr[ASR_UNFIN];
    s.overflow = (a.ctr[ASR_OVF] != 0 ? 1u : 0u) | (a.hits != nullptr && a.ctr[ASR_HITS] > a.hit_cap ? 2u : 0u);
    s.n_ext = a.ctr[ASR_EXT];
    s.widest_level = a.ctr[ASR_WIDEST] > a.ctr[t % 3] ? a.ctr[ASR_WIDEST] : a.ctr[t % 3];
    *stat = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct AsrPlan {
    FmdIndexView ix;
    AsrArgs a;
    AsrItem *f[2];            // level t reads f[t & 1] and writes f[~t & 1]; level 0 writes f[1]
    int grid;
    uint32_t ch;
};

// Grid and chunk for a capacity: at most the kernel's resident set (the levels walk the frontier by static ranges), chunk tails at most half the capacity.
static void asr_grid(fmd_dev_t *h, uint64_t cap, int &grid, uint32_t &ch)
{
    static int per_cu = 0;
    if (!per_cu) per_cu = fmd_resident_per_cu(k_asearch_level, ASR_LDS_U4 * 16, 16, "k_asearch_level");
    grid = h->n_cu * per_cu;
    ch = ASR_CHUNK;
    while (ch > ASR_MIN_CHUNK && (uint64_t)grid * ch * 2 > cap) ch >>= 1;
    const uint64_t g = cap / (2 * (uint64_t)ch);
    if ((uint64_t)grid > g) grid = (int)g;
    if (grid >= 8) grid &= ~7;                        // (a multiple of 8: km_range gives every XCD its eighth)
    if (grid < 1) grid = 1;
}
static int asr_plan(fmd_dev_t *h, size_t n, const uint8_t *d_seqs, const uint64_t *d_off, const uint8_t *d_lb, int max_sub, uint32_t max_hits, fmd_asearch_hit_t *d_hits,
                    uint64_t hit_cap, uint64_t *d_strata, void *d_work, size_t work_bytes, AsrPlan &p)
{
    const size_t fixed = ASR_HDR_BYTES + asr_tot_bytes(n);
    if (((uintptr_t)d_work & 15) || work_bytes < fixed) return FMD_E_ARG;
    uint64_t cap = (work_bytes - fixed) / (2 * sizeof(AsrItem));
    if (cap < FMD_ASEARCH_MIN_CAP) return FMD_E_ARG;
    if (cap > FMD_ASEARCH_MAX_CAP) cap = FMD_ASEARCH_MAX_CAP;
    p.ix = fmd_view(h);
    p.a.seqs = d_seqs; p.a.off = d_off; p.a.lb = d_lb; p.a.max_sub = (uint32_t)max_sub; p.a.max_hits = max_hits;
    p.a.ctr = (unsigned long long *)d_work; p.a.tot = (unsigned long long *)((uint8_t *)d_work + ASR_HDR_BYTES); p.a.strata = (unsigned long long *)d_strata;
    p.a.hits = hit_cap ? d_hits : nullptr; p.a.hit_cap = p.a.hits ? hit_cap : 0; p.a.cap = cap;
    p.f[0] = (AsrItem *)((uint8_t *)d_work + fixed); p.f[1] = p.f[0] + cap;
    asr_grid(h, cap, p.grid, p.ch);
    return FMD_OK;
}
static void asr_seed(const AsrPlan &p, hipStream_t st, size_t n)
{
    (void)hipMemsetAsync(p.a.ctr, 0, ASR_HDR_BYTES + asr_tot_bytes(n), st);
    (void)hipMemsetAsync(p.a.strata, 0, n * (size_t)(p.a.max_sub + 1) * 16, st);
    int grid = p.grid;
    if ((size_t)grid > (n + 63) / 64) grid = (int)((n + 63) / 64);
    k_asearch_seed<<<grid, 64, 0, st>>>(p.ix, n, p.a, p.f[1], p.ch);
}
static void asr_levels(const AsrPlan &p, hipStream_t st, uint32_t t0, uint32_t n_lev)
{
    for (uint32_t t = t0; t - t0 < n_lev; ++t) k_asearch_level<<<p.grid, 64, 0, st>>>(p.ix, t, p.a, p.f[t & 1], p.f[~t & 1], p.ch, 1);
}
static void asr_finish(const AsrPlan &p, hipStream_t st, uint32_t t, size_t n, fmd_asearch_stat_t *d_stat)
{
    k_asearch_rest<<<p.grid, 64, 0, st>>>(t, n, p.a, p.f[t & 1]);
    k_asearch_stat<<<1, 64, 0, st>>>(t, p.a, d_stat);
}
static bool asr_both_strands(const fmd_dev_t *h) { return h->mcnt[2] == h->mcnt[5] && h->mcnt[3] == h->mcnt[4] && !(h->mcnt[1] & 1); }   // the necessary test of kcount

extern "C" int fmd_asearch_bound_dev(fmd_dev_t *h, void *stream, size_t n, const uint8_t *d_seqs, const uint64_t *d_off, uint8_t *d_lb)
{
    if (!h || (n && (!d_seqs || !d_off || !d_lb))) return FMD_E_ARG;
    if (n == 0) return FMD_OK;
    if (n >= (1ull << 32)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h->device));
    k_asearch_bound<<<fmd_grid_for_lds(h, n, FMD_COMPACT_LDS_U4 * 16), 64, 0, S(stream)>>>(fmd_view(h), n, d_seqs, d_off, d_lb, asr_both_strands(h) ? 1 : 0);
    FMD_CHECK_LAUNCH("asearch bound kernel");
    return FMD_OK;
}

extern "C" int fmd_asearch_dev(fmd_dev_t *h, void *stream, size_t n, const uint8_t *d_seqs, const uint64_t *d_off, const uint8_t *d_lb, int max_sub,
                               uint32_t max_hits, uint32_t levels, fmd_asearch_hit_t *d_hits, uint64_t hit_cap, uint64_t *d_strata,
                               fmd_asearch_stat_t *d_stat, void *d_work, size_t work_bytes)
{
    if (!h || max_sub < 0 || max_sub > FMD_ASEARCH_MAX_SUB) return FMD_E_ARG;
    if (n && (!d_seqs || !d_off || !d_strata || !d_stat || !d_work || (hit_cap && !d_hits))) return FMD_E_ARG;
    if (n == 0) return FMD_OK;
    if (n >= (1ull << 32)) return FMD_E_ARG;           // the query index of an item is 32 bits
    FMD_HIP_TRY(hipSetDevice(h->device));
    AsrPlan p;
    FMD_TRY(asr_plan(h, n, d_seqs, d_off, d_lb, max_sub, max_hits, d_hits, hit_cap, d_strata, d_work, work_bytes, p));
    hipStream_t st = (hipStream_t)stream;
    asr_seed(p, st, n);
    asr_levels(p, st, 1, levels);
    asr_finish(p, st, levels + 1, n, d_stat);
    FMD_CHECK_LAUNCH("asearch kernels");
    return FMD_OK;
}

// ---- the host-array form
// One run at one budget over the queries `ids` (all of them valid: 1 .. FMD_ASEARCH_MAX_LEN bases): strata of the run (ids.size() x (budget + 1) x 2) and the hits of
// the queries that are not truncated, `query` = the position in ids.
struct AsrRun {
    std::vector<uint64_t> strata;
    std::vector<fmd_asearch_hit_t> hits;
};
static int asr_run(fmd_dev_t *h, const uint8_t *seqs, const uint64_t *off, const std::vector<uint32_t> &ids, int budget, uint32_t max_hits, bool prune, bool listed,
                   uint64_t cap_arg, AsrRun &out, fmd_asearch_stat_t *stat)
{
    const size_t n = ids.size(), cols = (size_t)budget + 1;
    out.strata.assign(n * cols * 2, 0); out.hits.clear();
    if (n == 0) return FMD_OK;
    // the queries side by side, every one on a 4-byte boundary
    std::vector<uint64_t> qoff(n + 1);
    uint64_t total = 0, max_len = 0;
    for (size_t i = 0; i < n; ++i) { qoff[i] = total; const uint64_t L = off[ids[i] + 1] - off[ids[i]]; total += L; if (L > max_len) max_len = L; }
    qoff[n] = total;
    std::vector<uint8_t> flat(total + 8, 0);
    for (size_t i = 0; i < n; ++i) memcpy(flat.data() + qoff[i], seqs + off[ids[i]], (size_t)(qoff[i + 1] - qoff[i]));
    FmdDevBuf ds, doff, dlb, dstrata, dstat, dhits;
    FMD_TRY(ds.alloc(total + 8)); FMD_TRY(doff.alloc((n + 1) * 8)); FMD_TRY(dstrata.alloc(n * cols * 16)); FMD_TRY(dstat.alloc(sizeof(fmd_asearch_stat_t)));
    FMD_HIP_TRY(hipMemcpy(ds.p, flat.data(), total + 8, hipMemcpyHostToDevice));
    FMD_HIP_TRY(hipMemcpy(doff.p, qoff.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    if (prune && budget > 0 && asr_both_strands(h)) {                          // (budget 0: the walk is a plain search and stops at the first base that misses)
        FMD_TRY(dlb.alloc(total + 8));
        FMD_TRY(fmd_asearch_bound_dev(h, nullptr, n, ds.as<uint8_t>(), doff.as<uint64_t>(), dlb.as<uint8_t>()));
    }
    // the capacity: the caller's, or sized from the batch, grown for a single query that does not fit while the free memory allows
    uint64_t cap = cap_arg, cap_max = cap_arg;
    if (cap_arg == 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)8 << 30;
        cap_max = (uint64_t)(0.5 * (double)free_b) / (2 * sizeof(AsrItem));
        if (cap_max > FMD_ASEARCH_MAX_CAP) cap_max = FMD_ASEARCH_MAX_CAP;
        if (cap_max < FMD_ASEARCH_MIN_CAP) cap_max = FMD_ASEARCH_MIN_CAP;
        cap = (uint64_t)n * 64 + (1u << 16);
        if (cap > cap_max) cap = cap_max;
    }
    uint64_t hcap = 0;
    if (listed) {
        hcap = (uint64_t)n * max_hits;
        if (hcap > (1u << 22)) hcap = 1u << 22;
        if (hcap < 1024) hcap = 1024;
        FMD_TRY(dhits.alloc(hcap * sizeof(fmd_asearch_hit_t)));
    }
    FmdScratch work;
    FMD_TRY(work.alloc(h, fmd_asearch_work_bytes(n, cap)));
    std::vector<std::pair<size_t, size_t>> todo;       // ranges of queries; the back is next
    todo.push_back(std::make_pair((size_t)0, n));
    std::vector<fmd_asearch_hit_t> part_hits;
    while (!todo.empty()) {
        const size_t b0 = todo.back().first, b1 = todo.back().second, m = b1 - b0;
        todo.pop_back();
        uint64_t part_len = 0;
        for (size_t i = b0; i < b1; ++i) if (qoff[i + 1] - qoff[i] > part_len) part_len = qoff[i + 1] - qoff[i];
        AsrPlan p;
        uint64_t *part_strata = dstrata.as<uint64_t>() + b0 * cols * 2;
        FMD_TRY(asr_plan(h, m, ds.as<uint8_t>(), doff.as<uint64_t>() + b0, dlb.as<uint8_t>(), budget, max_hits, dhits.as<fmd_asearch_hit_t>(), hcap, part_strata,
                         work.p, fmd_asearch_work_bytes(m, cap), p));
        hipStream_t st = nullptr;
        asr_seed(p, st, m);
        uint32_t t = 1;
        while ((uint64_t)t < part_len) {               // groups of levels; the host looks at the frontier between groups only
            unsigned long long left = 0;
            FMD_HIP_TRY(hipMemcpy(&left, p.a.ctr + t % 3, 8, hipMemcpyDeviceToHost));
            if (left == 0) break;
            uint32_t g = 32;
            if (part_len - t < g) g = (uint32_t)(part_len - t);
            asr_levels(p, st, t, g);
            t += g;
        }
        asr_finish(p, st, t, m, dstat.as<fmd_asearch_stat_t>());
        FMD_CHECK_LAUNCH("asearch kernels");
        fmd_asearch_stat_t ps;
        FMD_HIP_TRY(hipMemcpy(&ps, dstat.p, sizeof(ps), hipMemcpyDeviceToHost));
        stat->n_ext += ps.n_ext;                       // (the work of a discarded part was done all the same)
        if (ps.widest_level > stat->widest_level) stat->widest_level = ps.widest_level;
        if (ps.overflow) {                             // discarded whole
            if (m > 1) {
                todo.push_back(std::make_pair(b0 + m / 2, b1));
                todo.push_back(std::make_pair(b0, b0 + m / 2));
                continue;
            }
            bool grown = false;
            if ((ps.overflow & 1) && cap < cap_max) {
                const uint64_t c2 = 2 * cap < cap_max ? 2 * cap : cap_max;
                work.reset();
                if (work.alloc(h, fmd_asearch_work_bytes(n, c2)) == FMD_OK) { cap = c2; grown = true; }
                else { cap_max = cap; FMD_TRY(work.alloc(h, fmd_asearch_work_bytes(n, cap))); }
            }
            if ((ps.overflow & 2) && hcap < max_hits) {
                hcap = 2 * hcap < max_hits ? 2 * hcap : max_hits;
                FMD_TRY(dhits.alloc(hcap * sizeof(fmd_asearch_hit_t)));
                grown = true;
            }
            if (!grown) return FMD_E_OVERFLOW;
            todo.push_back(std::make_pair(b0, b1));
            continue;
        }
        if (ps.n_unfinished) return FMD_E_OVERFLOW;    // (every query of the part has had its L - 1 levels: cannot happen)
        FMD_HIP_TRY(hipMemcpy(out.strata.data() + b0 * cols * 2, part_strata, m * cols * 16, hipMemcpyDeviceToHost));
        stat->n_hits += ps.n_hits; stat->n_occ += ps.n_occ; stat->n_truncated += ps.n_truncated;
        if (!listed) continue;
        const uint64_t stored = ps.n_hits + ps.n_truncated * (uint64_t)max_hits;
        part_hits.resize(stored);
        if (stored) FMD_HIP_TRY(hipMemcpy(part_hits.data(), dhits.p, stored * sizeof(fmd_asearch_hit_t), hipMemcpyDeviceToHost));
        for (uint64_t j = 0; j < stored; ++j) {
            fmd_asearch_hit_t e = part_hits[j];
            const uint64_t *w = out.strata.data() + ((size_t)b0 + e.query) * cols * 2;
            uint64_t nh = 0;
            for (size_t c = 0; c < cols; ++c) nh += w[2 * c];
            if (nh > max_hits) continue;               // a truncated query: none listed
            e.query += (uint32_t)b0;
            out.hits.push_back(e);
        }
    }
    return FMD_OK;
}

static int asr_batch(fmd_dev_t *h, size_t n, const uint8_t *seqs, const uint64_t *off, int max_sub, uint32_t max_hits, unsigned flags, uint64_t cap,
                     fmd_asearch_hit_t **hits, uint64_t *n_hits, uint64_t *strata, fmd_asearch_stat_t *stat)
{
    if (!h || !stat || max_sub < 0 || max_sub > FMD_ASEARCH_MAX_SUB || (flags & ~(FMD_ASEARCH_NO_PRUNE | FMD_ASEARCH_BEST))) return FMD_E_ARG;
    if ((hits && !n_hits) || (n && (!seqs || !off || !strata))) return FMD_E_ARG;
    if (cap && (cap < FMD_ASEARCH_MIN_CAP || cap > FMD_ASEARCH_MAX_CAP)) return FMD_E_ARG;
    memset(stat, 0, sizeof(*stat));
    if (hits) { *hits = nullptr; *n_hits = 0; }
    if (n >= (1ull << 32)) return FMD_E_ARG;
    if (n == 0) {
        if (hits && !(*hits = (fmd_asearch_hit_t *)malloc(sizeof(fmd_asearch_hit_t)))) return FMD_E_NOMEM;
        return FMD_OK;
    }
    FMD_HIP_TRY(hipSetDevice(h->device));
    const size_t cols = (size_t)max_sub + 1;
    memset(strata, 0, n * cols * 16);
    std::vector<uint32_t> ids;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t L = off[i + 1] - off[i];
        if (off[i + 1] < off[i] || L == 0 || L > FMD_ASEARCH_MAX_LEN) ++stat->n_skipped; else ids.push_back((uint32_t)i);
    }
    const bool prune = !(flags & FMD_ASEARCH_NO_PRUNE), listed = hits != nullptr;
    std::vector<fmd_asearch_hit_t> all;
    AsrRun run;
    for (int budget = (flags & FMD_ASEARCH_BEST) ? 0 : max_sub; budget <= max_sub && !ids.empty(); ++budget) {
        FMD_TRY(asr_run(h, seqs, off, ids, budget, max_hits, prune, listed, cap, run, stat));
        const size_t rc = (size_t)budget + 1;
        std::vector<uint32_t> rest;
        for (size_t i = 0; i < ids.size(); ++i) {
            uint64_t nh = 0;
            for (size_t c = 0; c < rc; ++c) nh += run.strata[(i * rc + c) * 2];
            if (nh == 0 && budget < max_sub) { rest.push_back(ids[i]); continue; }
            memcpy(strata + (size_t)ids[i] * cols * 2, run.strata.data() + i * rc * 2, rc * 16);
        }
        for (size_t j = 0; j < run.hits.size(); ++j) { fmd_asearch_hit_t e = run.hits[j]; e.query = ids[e.query]; all.push_back(e); }
        ids.swap(rest);
    }
    if (!listed) return FMD_OK;
    std::sort(all.begin(), all.end(), [](const fmd_asearch_hit_t &x, const fmd_asearch_hit_t &y) {
        return x.query != y.query ? x.query < y.query : x.n_sub != y.n_sub ? x.n_sub < y.n_sub : x.beg < y.beg;
    });
    fmd_asearch_hit_t *r = (fmd_asearch_hit_t *)malloc((all.empty() ? 1 : all.size()) * sizeof(fmd_asearch_hit_t));
    if (!r) return FMD_E_NOMEM;
    if (!all.empty()) memcpy(r, all.data(), all.size() * sizeof(fmd_asearch_hit_t));
    *hits = r; *n_hits = all.size();
    return FMD_OK;
}
extern "C" int fmd_asearch_batch(fmd_dev_t *h, size_t n, const uint8_t *seqs, const uint64_t *off, int max_sub, uint32_t max_hits, unsigned flags, uint64_t cap,
                                 fmd_asearch_hit_t **hits, uint64_t *n_hits, uint64_t *strata, fmd_asearch_stat_t *stat)
{
    try { return asr_batch(h, n, seqs, off, max_sub, max_hits, flags, cap, hits, n_hits, strata, stat); }
    catch (const std::bad_alloc &) { return FMD_E_NOMEM; }   // (the host vectors)
}
