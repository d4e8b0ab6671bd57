// fmd_esearch.hip -- esearch: search within max_edit edits, insertions and deletions included (the semantics are stated in
// include/fmd_hip.h).
//
// The patterns within max_edit edits of a query are strings of L - max_edit .. L + max_edit bases; the ones that occur are nodes of the trie of the index,
// rooted at the END of the pattern.  The walk is the fourth user of fmd_level.h: level by level, one backward extension per item (km_extend_back),
// frontier slots reserved in chunks, the frontier cut into one range per XCD, no per-lane stack.  Level t holds the nodes of pattern length t, so every
// node -- every distinct pattern -- is met exactly once.  An item is the node's SA interval, its query and the column of the edit-distance table of the
// node against the query's suffixes, cut to the band: cell i = -4 .. 4 is ed(the t bases so far, the query's last t + i bases), capped at max_edit + 1 =
// dead, nine cells of three bits in one 32-bit word.  The child of base c takes the next column (esr_kids); a child with no live cell is not pushed; a
// child whose cell for the whole query is <= max_edit is a hit of that distance, and goes on as an item while other cells live.  The lower bound of
// asearch (fmd_asearch_bound_dev) kills the cells whose value + the bound of what is left of the query exceeds max_edit.  Hits leave through a buffer
// in LDS, one atomic per flush; the strata are counted with atomics on the query's own words.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>
#include "fmd_internal.h"
#include "fmd_kernel_common.h"
#include "fmd_level.h"

// An item: the rows [x0, x0 + size) -- positions and sizes are 64 bits throughout --, the query and the column.  All zero = a hole (size 0).
struct EsrItem { uint64_t x0, size; uint32_t query, col; uint64_t unused; };
static_assert(sizeof(EsrItem) == 32 && sizeof(EsrItem) % 16 == 0 && offsetof(EsrItem, size) == 8 && offsetof(EsrItem, query) == 16 && offsetof(EsrItem, col) == 20,
              "a frontier entry is two 16-byte words");
static_assert(sizeof(fmd_esearch_hit_t) == 32 && offsetof(fmd_esearch_hit_t, cnt) == 8 && offsetof(fmd_esearch_hit_t, query) == 16 &&
              offsetof(fmd_esearch_hit_t, n_edit) == 20 && offsetof(fmd_esearch_hit_t, len) == 24 && sizeof(fmd_esearch_stat_t) == 64, "layouts of include/fmd_hip.h");
// the column: cell i = -4 .. 4 in bits 3 (i + 4) .. 3 (i + 4) + 2, values 0 .. max_edit live, max_edit + 1 dead
static_assert(FMD_ESEARCH_MAX_EDIT == 4 && 3 * (2 * FMD_ESEARCH_MAX_EDIT + 1) <= 32 && FMD_ESEARCH_MAX_EDIT + 2 <= 7, "nine cells of 0 .. 5 (+ 1 while a minimum is taken) in three bits each");
#define ESR_CELLS 9
#define ESR_ONES 0x1249249u                        // 1 in every cell
#define ESR_NO_HIT 7u

// counters at the head of the work area (u64 words): the frontier sizes rotate through words 0..2 as asearch's do -- level t reads word t % 3, counts
// its children in word (t + 1) % 3 and clears word (t + 2) % 3; level 0 counts in word 1
#define ESR_HITS 3       // hits staged for d_hits (counts on when d_hits is full)
#define ESR_SKIP 4       // queries level 0 left out
#define ESR_UNFIN 5      // items still walking after the last level
#define ESR_OVF 6        // a frontier entry did not fit
#define ESR_EXT 7        // backward extensions done
#define ESR_WIDEST 8     // the most slots a level reserved
#define ESR_TRUNC 9      // queries with more than max_hits hits
#define ESR_NHITS 10     // hits of the others
#define ESR_NOCC 11      // ... and the sum of their cnt
#define ESR_HDR_BYTES 256
// behind the header: one u64 per query, its hits so far (what decides max_hits), then the two frontiers
static inline size_t esr_tot_bytes(size_t n) { return align_up(n * 8, 256); }
// chunks, grid and the hit buffer: as asearch (fmd_asearch.hip)
#define ESR_CHUNK 512u
#define ESR_MIN_CHUNK 256u
static_assert(ESR_MIN_CHUNK >= 4 * 64 && FMD_ESEARCH_MIN_CAP >= 2 * 8 * ESR_MIN_CHUNK, "one step's children fit one chunk; the smallest capacity holds eight waves' tails and as much again");
#define ESR_HIT_BUF 128
#define ESR_LDS_U4 (FMD_COMPACT_LDS_U4 + 2 * ESR_HIT_BUF)
static_assert(ESR_HIT_BUF >= 64, "the hits of one child of one step fit the buffer");

extern "C" size_t fmd_esearch_work_bytes(size_t n, uint64_t cap)
{
    if (cap < FMD_ESEARCH_MIN_CAP || cap > FMD_ESEARCH_MAX_CAP || n >= (1ull << 32)) return 0;
    return ESR_HDR_BYTES + esr_tot_bytes(n) + 2 * (size_t)cap * sizeof(EsrItem);
}

// what the kernels of one walk share
struct EsrArgs {
    const uint8_t *seqs; const uint64_t *off; const uint8_t *lb;   // lb = nullptr: no pruning
    uint32_t max_edit, max_hits;
    unsigned long long *ctr, *tot, *strata;
    fmd_esearch_hit_t *hits; uint64_t hit_cap;                    // hits = nullptr: count only
    uint64_t cap;                                                  // entries of a frontier
};

// ---- the columns of the four children of a node of t bases with column D, query [o0, o0 + L).
// Cell j (i = j - 4) of a child stands for the query's suffix of sl = t + 1 + i bases, which starts at position p = L - sl = (L - 1 - t) + 4 - j:
//     D'[i] = min(D[i] + (c != q[p]), D[i + 1] + 1, D'[i - 1] + 1)          -- substitution or match; c absent from the query; q[p] absent from the pattern
// dead where |i| > max_edit, sl < 0 or sl > L, and where the value + lb[p - 1] -- the least any pattern spends on q[0 .. p - 1] -- exceeds max_edit.  The
// nine query bases and bounds are one window each, read once for the four children.  hv[c] = the distance of the child as a whole pattern (the cell of
// sl = L), ESR_NO_HIT when there is none; that cell is dead in col[c] when it holds max_edit itself (a longer pattern only pays more).  Bit c of push:
// col[c] has a live cell; bit c of keep: the child is a hit or is pushed.
__device__ __forceinline__ void esr_kids(const EsrArgs &a, uint32_t t, uint64_t o0, uint32_t L, uint32_t D, bool live, uint32_t col[5], uint32_t hv[5], uint32_t &keep,
                                         uint32_t &push)
{
    const uint32_t d = a.max_edit, dead = d + 1;
    const int pos0 = (int)L - 1 - (int)t;
    uint32_t qw = 0, lw = 0, valid = 0;
    if (live) {
#pragma unroll
        for (int j = 0; j < ESR_CELLS; ++j) {
            const int p = pos0 + 4 - j;
            if (j - 4 >= -(int)d && j - 4 <= (int)d && p >= 0 && p <= (int)L) {
                valid |= 1u << j;
                if (p < (int)L) qw |= ((uint32_t)a.seqs[o0 + p] & 7u) << (3 * j);      // (p = L, the empty suffix: no base, 0 equals none)
                if (p >= 1 && a.lb) { const uint32_t v = a.lb[o0 + p - 1]; lw |= (v < 7u ? v : 7u) << (3 * j); }
            }
        }
    }
    const int jh = pos0 + 4;                           // the cell of sl = L
    keep = 0; push = 0;
#pragma unroll
    for (int c = 1; c <= 4; ++c) {
        uint32_t out = 0, prev = dead;
#pragma unroll
        for (int j = 0; j < ESR_CELLS; ++j) {
            const uint32_t up = (D >> (3 * j)) & 7u, right = j + 1 < ESR_CELLS ? (D >> (3 * j + 3)) & 7u : dead;
            uint32_t v = up + (((qw >> (3 * j)) & 7u) != (uint32_t)c ? 1u : 0u);
            v = v < right + 1 ? v : right + 1;
            v = v < prev + 1 ? v : prev + 1;
            if (!((valid >> j) & 1u) || v + ((lw >> (3 * j)) & 7u) > d) v = dead;
            out |= v << (3 * j);
            prev = v;
        }
        uint32_t h = ESR_NO_HIT;
        if (jh >= 0 && jh < ESR_CELLS) {
            const uint32_t v = (out >> (3 * jh)) & 7u;
            if (v <= d) h = v;
            if (v == d) out += 1u << (3 * jh);
        }
        const bool any = out != dead * ESR_ONES;
        col[c] = out; hv[c] = h;
        push |= any ? 1u << c : 0u;
        keep |= (any || h != ESR_NO_HIT) ? 1u << c : 0u;
    }
}
// the column of the empty pattern against a query of L bases: cell i = i for 0 <= i <= min(max_edit, L), dead elsewhere
__device__ __forceinline__ uint32_t esr_col0(uint32_t d, uint32_t L)
{
    uint32_t D = 0;
#pragma unroll
    for (int j = 0; j < ESR_CELLS; ++j) D |= ((j >= 4 && (uint32_t)(j - 4) <= d && (uint32_t)(j - 4) <= L) ? (uint32_t)(j - 4) : d + 1) << (3 * j);
    return D;
}

// ---- hits: counted on the query's words, staged in LDS, flushed with one atomic (the scheme of asr_flush_hits / asr_emit, fmd_asearch.hip)
__device__ __forceinline__ void esr_flush_hits(const uint4 *buf, uint32_t &fill, const EsrArgs &a)
{
    if (fill == 0) return;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the lanes that wrote the entries are not the lanes that read them
    unsigned long long first = 0;
    if (fmd_lane() == 0) first = atomicAdd(&a.ctr[ESR_HITS], (unsigned long long)fill);
    first = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(first >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)first);
    for (uint32_t j = (uint32_t)fmd_lane(); j < fill; j += 64) {
        const uint4 e0 = buf[2 * j], e1 = buf[2 * j + 1];
        if (first + j < a.hit_cap) {                      // (past hit_cap: k_esearch_stat sets the flag, the counter went past it)
            uint4 *q = (uint4 *)(a.hits + first + j);
            q[0] = e0; q[1] = e1;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // read before the next step overwrites them
    fill = 0;
}
// One child of one step: the lanes with `hit` have found the pattern of `len` bases with interval [x0, x0 + sz) at distance e from query qi.
__device__ __forceinline__ void esr_emit(bool hit, uint64_t x0, uint64_t sz, uint32_t qi, uint32_t e, uint32_t len, uint4 *buf, uint32_t &fill, const EsrArgs &a)
{
    if (__ballot(hit) == 0) return;
    bool list = false;
    if (hit) {
        unsigned long long *w = a.strata + ((uint64_t)qi * (a.max_edit + 1) + e) * 2;
        atomicAdd(w, 1ull); atomicAdd(w + 1, (unsigned long long)sz);
        list = atomicAdd(&a.tot[qi], 1ull) < a.max_hits && a.hits != nullptr;
    }
    const uint64_t m = __ballot(list);
    if (m == 0) return;
    const uint32_t nl = (uint32_t)__popcll(m);
    if (fill + nl > ESR_HIT_BUF) esr_flush_hits(buf, fill, a);
    if (list) {
        const uint32_t j = fill + (uint32_t)fmd_below(m);
        buf[2 * j] = make_uint4((uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)sz, (uint32_t)(sz >> 32));
        buf[2 * j + 1] = make_uint4(qi, e, len, 0u);
    }
    fill += nl;
}
__device__ __forceinline__ void esr_store_item(EsrItem *out, uint64_t o, uint64_t x0, uint64_t sz, uint32_t qi, uint32_t col, const EsrArgs &a)
{
    if (o < a.cap) {
        uint4 *q = (uint4 *)(out + o);
        q[0] = make_uint4((uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)sz, (uint32_t)(sz >> 32));
        q[1] = make_uint4(qi, col, 0u, 0u);
    } else a.ctr[ESR_OVF] = 1;
}

// The children of one step, c = 1 .. 4, patterns of t + 1 bases: occ[c] says the child occurs and esr_kids keeps it; it is a hit where hv[c] says so and
// an item of the next level where bit c of push is set -- both, often.
#define ESR_CHILDREN(x0_of, sz_of)                                                                \
    const bool push1 = occ1 && (push & 2u), push2 = occ2 && (push & 4u), push3 = occ3 && (push & 8u), push4 = occ4 && (push & 16u); \
    const uint64_t m1 = __ballot(push1), m2 = __ballot(push2), m3 = __ballot(push3), m4 = __ballot(push4); \
    const uint32_t p1 = (uint32_t)__popcll(m1), p2 = p1 + (uint32_t)__popcll(m2), p3 = p2 + (uint32_t)__popcll(m3), tot = p3 + (uint32_t)__popcll(m4); \
    KmSpan sp; sp.a = 0; sp.b = 0; sp.na = 0;                                                     \
    if (tot) sp = km_reserve_split(ck, tot, &a.ctr[w_out]);                                       \
    ESR_CHILD(1, occ1, push1, m1, 0u, x0_of, sz_of) ESR_CHILD(2, occ2, push2, m2, p1, x0_of, sz_of) ESR_CHILD(3, occ3, push3, m3, p2, x0_of, sz_of) ESR_CHILD(4, occ4, push4, m4, p3, x0_of, sz_of)
#define ESR_CHILD(c, occ, psh, m, before, x0_of, sz_of)                                           \
    {                                                                                             \
        esr_emit((occ) && hv[c] != ESR_NO_HIT, x0_of(c), sz_of(c), qi, hv[c], t + 1, hit_buf, hit_fill, a); \
        if (psh) esr_store_item(out, km_span_slot(sp, (before) + (uint32_t)fmd_below(m)), x0_of(c), sz_of(c), qi, col[c], a); \
    }

// level 0: one query per lane, the four roots -- the patterns of one base -- from the marginal counts
__global__ __launch_bounds__(64) void k_esearch_seed(FmdIndexView ix, size_t n, EsrArgs a, EsrItem *__restrict__ out, uint32_t ch)
{
    __shared__ uint4 hit_buf[2 * ESR_HIT_BUF];
    uint32_t hit_fill = 0;                            // wave-uniform
    const int lane = fmd_lane();
    const uint32_t w_out = 1, t = 0;
    KmChunk ck; ck.base = 0; ck.fill = 0; ck.ch = ch; ck.have = false;
    uint32_t n_skip = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n; base += (uint64_t)gridDim.x * 64) {
        const uint64_t i = base + lane;
        uint64_t o0 = 0, L = 0;
        if (i < n) { o0 = a.off[i]; L = a.off[i + 1] - o0; }
        const bool skip = i < n && (L == 0 || L > FMD_ESEARCH_MAX_LEN);
        const bool act = i < n && !skip;
        n_skip += (uint32_t)__popcll(__ballot(skip));
        const uint32_t qi = (uint32_t)i;
        uint32_t col[5], hv[5], keep, push;
        esr_kids(a, t, o0, act ? (uint32_t)L : 0u, esr_col0(a.max_edit, (uint32_t)L), act, col, hv, keep, push);
#define ESR_X0(c) ix.cnt[c]
#define ESR_SZ(c) (ix.cnt[(c) + 1] - ix.cnt[c])
        const bool occ1 = (keep & 2u) && ESR_SZ(1) != 0, occ2 = (keep & 4u) && ESR_SZ(2) != 0, occ3 = (keep & 8u) && ESR_SZ(3) != 0, occ4 = (keep & 16u) && ESR_SZ(4) != 0;
        ESR_CHILDREN(ESR_X0, ESR_SZ)
#undef ESR_X0
#undef ESR_SZ
    }
    km_zero_fill(out, a.cap, ck);
    esr_flush_hits(hit_buf, hit_fill, a);
    if (lane == 0 && n_skip) atomicAdd(&a.ctr[ESR_SKIP], (unsigned long long)n_skip);
}

// one level: the nodes of t bases -> the hits of t + 1 bases + the items of level t + 1
__global__ __launch_bounds__(64) void k_esearch_level(FmdIndexView ix, uint32_t t, EsrArgs a, const EsrItem *__restrict__ in, EsrItem *__restrict__ out, uint32_t ch,
                                                      int xcd_aware)
{
    __shared__ uint4 fmd_lds[ESR_LDS_U4];             // one array: the landing area of the rank engine, then the hit buffer
    uint4 *hit_buf = fmd_lds + FMD_COMPACT_LDS_U4;
    uint32_t hit_fill = 0;                            // wave-uniform
    const int lane = fmd_lane();
    const uint32_t w_in = t % 3, w_out = (t + 1) % 3, w_clr = (t + 2) % 3;
    const uint64_t n_raw = a.ctr[w_in], n = n_raw < a.cap ? n_raw : a.cap;   // an overflowing level counted more than it stored
    if (blockIdx.x == 0 && lane == 0) { a.ctr[w_clr] = 0; if (n_raw > a.ctr[ESR_WIDEST]) a.ctr[ESR_WIDEST] = n_raw; }
    const KmRange rg = km_range(n, xcd_aware);
    const uint64_t stride = rg.stride;
    KmChunk ck; ck.base = 0; ck.fill = 0; ck.ch = ch; ck.have = false;
    uint32_t n_ext = 0;
    uint4 na = make_uint4(0, 0, 0, 0), nb = na;       // the item of the next iteration, loaded one gather ahead
    if (rg.beg + lane < rg.end) { const uint4 *q = (const uint4 *)(in + rg.beg + lane); na = q[0]; nb = q[1]; }
    for (uint64_t base = rg.beg; base < rg.end; base += stride) {
        const uint4 ia = na, ib = nb;
        const uint64_t x0 = (uint64_t)ia.y << 32 | ia.x, sz = (uint64_t)ia.w << 32 | ia.z;
        const uint32_t qi = ib.x, D = ib.y;
        const bool live = base + lane < rg.end && sz != 0;
        na = make_uint4(0, 0, 0, 0); nb = na;
        if (base + stride + lane < rg.end) { const uint4 *q = (const uint4 *)(in + base + stride + lane); na = q[0]; nb = q[1]; }
        if (__ballot(live) == 0) continue;            // a run of holes
        uint64_t o0 = 0;
        uint32_t L = 0;
        if (live) { o0 = a.off[qi]; L = (uint32_t)(a.off[qi + 1] - o0); }
        uint32_t col[5], hv[5], keep, push;
        esr_kids(a, t, o0, L, D, live, col, hv, keep, push);
        const bool act = keep != 0;                   // (every cell one step from dead and no base of the window fits: no child is kept, nothing to extend)
        const uint64_t m_act = __ballot(act);
        if (m_act == 0) continue;
        n_ext += (uint32_t)__popcll(m_act);
        uint64_t tk[6], sc[6];
        km_extend_back<true, false, true>(ix, fmd_lds, act, x0, sz, 1, tk, sc, keep);
        const bool occ1 = (keep & 2u) && sc[1] != 0, occ2 = (keep & 4u) && sc[2] != 0, occ3 = (keep & 8u) && sc[3] != 0, occ4 = (keep & 16u) && sc[4] != 0;
#define ESR_X0(c) (ix.cnt[c] + tk[c])
#define ESR_SZ(c) sc[c]
        ESR_CHILDREN(ESR_X0, ESR_SZ)
#undef ESR_X0
#undef ESR_SZ
    }
    km_zero_fill(out, a.cap, ck);
    esr_flush_hits(hit_buf, hit_fill, a);
    if (lane == 0 && n_ext) atomicAdd(&a.ctr[ESR_EXT], (unsigned long long)n_ext);
}
#undef ESR_CHILDREN
#undef ESR_CHILD

// after the last level: the items still walking (the frontier level t would read), and per query whether it is truncated
__global__ __launch_bounds__(64) void k_esearch_rest(uint32_t t, size_t n, EsrArgs a, const EsrItem *__restrict__ in)
{
    const uint64_t n_raw = a.ctr[t % 3], m = n_raw < a.cap ? n_raw : a.cap;
    uint64_t unfin = 0, trunc = 0, nh = 0, no = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 64 + fmd_lane(); i < m; i += (uint64_t)gridDim.x * 64) unfin += in[i].size != 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 64 + fmd_lane(); i < n; i += (uint64_t)gridDim.x * 64) {
        const uint64_t v = a.tot[i];
        if (v > a.max_hits) ++trunc;
        else if (v) {
            nh += v;
            for (uint32_t j = 0; j <= a.max_edit; ++j) no += a.strata[(i * (a.max_edit + 1) + j) * 2 + 1];
        }
    }
    unfin = km_wave_sum(unfin); trunc = km_wave_sum(trunc); nh = km_wave_sum(nh); no = km_wave_sum(no);
    if (fmd_lane() == 0) {
        if (unfin) atomicAdd(&a.ctr[ESR_UNFIN], (unsigned long long)unfin);
        if (trunc) atomicAdd(&a.ctr[ESR_TRUNC], (unsigned long long)trunc);
        if (nh) { atomicAdd(&a.ctr[ESR_NHITS], (unsigned long long)nh); atomicAdd(&a.ctr[ESR_NOCC], (unsigned long long)no); }
    }
}
__global__ void k_esearch_stat(uint32_t t, EsrArgs a, fmd_esearch_stat_t *__restrict__ stat)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    fmd_esearch_stat_t s;
    s.n_hits = a.ctr[ESR_NHITS]; s.n_occ = a.ctr[ESR_NOCC]; s.n_skipped = a.ctr[ESR_SKIP]; s.n_truncated = a.ctr[ESR_TRUNC]; s.n_unfinished = a.ctr[ESR_UNFIN];
    s.overflow = (a.ctr[ESR_OVF] != 0 ? 1u : 0u) | (a.hits != nullptr && a.ctr[ESR_HITS] > a.hit_cap ? 2u : 0u);
    s.n_ext = a.ctr[ESR_EXT];
    s.widest_level = a.ctr[ESR_WIDEST] > a.ctr[t % 3] ? a.ctr[ESR_WIDEST] : a.ctr[t % 3];
    *stat = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct EsrPlan {
    FmdIndexView ix;
    EsrArgs a;
    EsrItem *f[2];            // level t reads f[t & 1] and writes f[~t & 1]; level 0 writes f[1]
    int grid;
    uint32_t ch;
};

// Grid and chunk for a capacity: at most the kernel's resident set (the levels walk the frontier by static ranges), chunk tails at most half the capacity.
static void esr_grid(fmd_dev_t *h, uint64_t cap, int &grid, uint32_t &ch)
{
    static int per_cu = 0;
    if (!per_cu) per_cu = fmd_resident_per_cu(k_esearch_level, ESR_LDS_U4 * 16, 16, "k_esearch_level");
    grid = h->n_cu * per_cu;
    ch = ESR_CHUNK;
    while (ch > ESR_MIN_CHUNK && (uint64_t)grid * ch * 2 > cap) ch >>= 1;
    const uint64_t g = cap / (2 * (uint64_t)ch);
    if ((uint64_t)grid > g) grid = (int)g;
    if (grid >= 8) grid &= ~7;                        // (a multiple of 8: km_range gives every XCD its eighth)
    if (grid < 1) grid = 1;
}
static int esr_plan(fmd_dev_t *h, size_t n, const uint8_t *d_seqs, const uint64_t *d_off, const uint8_t *d_lb, int max_edit, uint32_t max_hits, fmd_esearch_hit_t *d_hits,
                    uint64_t hit_cap, uint64_t *d_strata, void *d_work, size_t work_bytes, EsrPlan &p)
{
    const size_t fixed = ESR_HDR_BYTES + esr_tot_bytes(n);
    if (((uintptr_t)d_work & 15) || work_bytes < fixed) return FMD_E_ARG;
    uint64_t cap = (work_bytes - fixed) / (2 * sizeof(EsrItem));
    if (cap < FMD_ESEARCH_MIN_CAP) return FMD_E_ARG;
    if (cap > FMD_ESEARCH_MAX_CAP) cap = FMD_ESEARCH_MAX_CAP;
    p.ix = fmd_view(h);
    p.a.seqs = d_seqs; p.a.off = d_off; p.a.lb = d_lb; p.a.max_edit = (uint32_t)max_edit; p.a.max_hits = max_hits;
    p.a.ctr = (unsigned long long *)d_work; p.a.tot = (unsigned long long *)((uint8_t *)d_work + ESR_HDR_BYTES); p.a.strata = (unsigned long long *)d_strata;
    p.a.hits = hit_cap ? d_hits : nullptr; p.a.hit_cap = p.a.hits ? hit_cap : 0; p.a.cap = cap;
    p.f[0] = (EsrItem *)((uint8_t *)d_work + fixed); p.f[1] = p.f[0] + cap;
    esr_grid(h, cap, p.grid, p.ch);
    return FMD_OK;
}
static void esr_seed(const EsrPlan &p, hipStream_t st, size_t n)
{
    (void)hipMemsetAsync(p.a.ctr, 0, ESR_HDR_BYTES + esr_tot_bytes(n), st);
    (void)hipMemsetAsync(p.a.strata, 0, n * (size_t)(p.a.max_edit + 1) * 16, st);
    int grid = p.grid;
    if ((size_t)grid > (n + 63) / 64) grid = (int)((n + 63) / 64);
    k_esearch_seed<<<grid, 64, 0, st>>>(p.ix, n, p.a, p.f[1], p.ch);
}
static void esr_levels(const EsrPlan &p, hipStream_t st, uint32_t t0, uint32_t n_lev)
{
    for (uint32_t t = t0; t - t0 < n_lev; ++t) k_esearch_level<<<p.grid, 64, 0, st>>>(p.ix, t, p.a, p.f[t & 1], p.f[~t & 1], p.ch, 1);
}
static void esr_finish(const EsrPlan &p, hipStream_t st, uint32_t t, size_t n, fmd_esearch_stat_t *d_stat)
{
    k_esearch_rest<<<p.grid, 64, 0, st>>>(t, n, p.a, p.f[t & 1]);
    k_esearch_stat<<<1, 64, 0, st>>>(t, p.a, d_stat);
}
static bool esr_both_strands(const fmd_dev_t *h) { return h->mcnt[2] == h->mcnt[5] && h->mcnt[3] == h->mcnt[4] && !(h->mcnt[1] & 1); }   // the necessary test of kcount

extern "C" int fmd_esearch_dev(fmd_dev_t *h, void *stream, size_t n, const uint8_t *d_seqs, const uint64_t *d_off, const uint8_t *d_lb, int max_edit,
                               uint32_t max_hits, uint32_t levels, fmd_esearch_hit_t *d_hits, uint64_t hit_cap, uint64_t *d_strata,
                               fmd_esearch_stat_t *d_stat, void *d_work, size_t work_bytes)
{
    if (!h || max_edit < 0 || max_edit > FMD_ESEARCH_MAX_EDIT) return FMD_E_ARG;
    if (n && (!d_seqs || !d_off || !d_strata || !d_stat || !d_work || (hit_cap && !d_hits))) return FMD_E_ARG;
    if (n == 0) return FMD_OK;
    if (n >= (1ull << 32)) return FMD_E_ARG;           // the query index of an item is 32 bits
    FMD_HIP_TRY(hipSetDevice(h->device));
    EsrPlan p;
    FMD_TRY(esr_plan(h, n, d_seqs, d_off, d_lb, max_edit, max_hits, d_hits, hit_cap, d_strata, d_work, work_bytes, p));
    hipStream_t st = (hipStream_t)stream;
    esr_seed(p, st, n);
    esr_levels(p, st, 1, levels);
    esr_finish(p, st, levels + 1, n, d_stat);
    FMD_CHECK_LAUNCH("esearch kernels");
    return FMD_OK;
}

// ---- the host-array form (the scheme of asr_run / asr_batch, fmd_asearch.hip)
// One run at one budget over the queries `ids` (all of them valid: 1 .. FMD_ESEARCH_MAX_LEN bases): strata of the run (ids.size() x (budget + 1) x 2) and the hits of
// the queries that are not truncated, `query` = the position in ids.
struct EsrRun {
    std::vector<uint64_t> strata;
    std::vector<fmd_esearch_hit_t> hits;
};
static int esr_run(fmd_dev_t *h, const uint8_t *seqs, const uint64_t *off, const std::vector<uint32_t> &ids, int budget, uint32_t max_hits, bool prune, bool listed,
                   uint64_t cap_arg, EsrRun &out, fmd_esearch_stat_t *stat)
{
    const size_t n = ids.size(), cols = (size_t)budget + 1;
    out.strata.assign(n * cols * 2, 0); out.hits.clear();
    if (n == 0) return FMD_OK;
    // the queries side by side
    std::vector<uint64_t> qoff(n + 1);
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) { qoff[i] = total; total += off[ids[i] + 1] - off[ids[i]]; }
    qoff[n] = total;
    std::vector<uint8_t> flat(total + 8, 0);
    for (size_t i = 0; i < n; ++i) memcpy(flat.data() + qoff[i], seqs + off[ids[i]], (size_t)(qoff[i + 1] - qoff[i]));
    FmdDevBuf ds, doff, dlb, dstrata, dstat, dhits;
    FMD_TRY(ds.alloc(total + 8)); FMD_TRY(doff.alloc((n + 1) * 8)); FMD_TRY(dstrata.alloc(n * cols * 16)); FMD_TRY(dstat.alloc(sizeof(fmd_esearch_stat_t)));
    FMD_HIP_TRY(hipMemcpy(ds.p, flat.data(), total + 8, hipMemcpyHostToDevice));
    FMD_HIP_TRY(hipMemcpy(doff.p, qoff.data(), (n + 1) * 8, hipMemcpyHostToDevice));
    if (prune && budget > 0 && esr_both_strands(h)) {                          // (budget 0: the walk is a plain search and stops at the first base that misses)
        FMD_TRY(dlb.alloc(total + 8));
        FMD_TRY(fmd_asearch_bound_dev(h, nullptr, n, ds.as<uint8_t>(), doff.as<uint64_t>(), dlb.as<uint8_t>()));
    }
    // the capacity: the caller's, or sized from the batch, grown for a single query that does not fit while the free memory allows
    uint64_t cap = cap_arg, cap_max = cap_arg;
    if (cap_arg == 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)8 << 30;
        cap_max = (uint64_t)(0.5 * (double)free_b) / (2 * sizeof(EsrItem));
        if (cap_max > FMD_ESEARCH_MAX_CAP) cap_max = FMD_ESEARCH_MAX_CAP;
        if (cap_max < FMD_ESEARCH_MIN_CAP) cap_max = FMD_ESEARCH_MIN_CAP;
        cap = ((uint64_t)n * 64 << budget) + (1u << 16);                       // (every edit of the budget widens the walk)
        if (cap > cap_max) cap = cap_max;
    }
    uint64_t hcap = 0;
    if (listed) {
        hcap = (uint64_t)n * max_hits;
        if (hcap > (1u << 22)) hcap = 1u << 22;
        if (hcap < 1024) hcap = 1024;
        FMD_TRY(dhits.alloc(hcap * sizeof(fmd_esearch_hit_t)));
    }
    FmdScratch work;
    FMD_TRY(work.alloc(h, fmd_esearch_work_bytes(n, cap)));
    std::vector<std::pair<size_t, size_t>> todo;       // ranges of queries; the back is next
    todo.push_back(std::make_pair((size_t)0, n));
    std::vector<fmd_esearch_hit_t> part_hits;
    while (!todo.empty()) {
        const size_t b0 = todo.back().first, b1 = todo.back().second, m = b1 - b0;
        todo.pop_back();
        uint64_t part_len = 0;
        for (size_t i = b0; i < b1; ++i) if (qoff[i + 1] - qoff[i] > part_len) part_len = qoff[i + 1] - qoff[i];
        EsrPlan p;
        uint64_t *part_strata = dstrata.as<uint64_t>() + b0 * cols * 2;
        FMD_TRY(esr_plan(h, m, ds.as<uint8_t>(), doff.as<uint64_t>() + b0, dlb.as<uint8_t>(), budget, max_hits, dhits.as<fmd_esearch_hit_t>(), hcap, part_strata,
                         work.p, fmd_esearch_work_bytes(m, cap), p));
        hipStream_t st = nullptr;
        esr_seed(p, st, m);
        uint32_t t = 1;
        while ((uint64_t)t < part_len + (uint64_t)budget) {   // patterns of up to L + budget bases; groups of levels, the host looks at the frontier between groups only
            unsigned long long left = 0;
            FMD_HIP_TRY(hipMemcpy(&left, p.a.ctr + t % 3, 8, hipMemcpyDeviceToHost));
            if (left == 0) break;
            uint32_t g = 32;
            if (part_len + budget - t < g) g = (uint32_t)(part_len + budget - t);
            esr_levels(p, st, t, g);
            t += g;
        }
        esr_finish(p, st, t, m, dstat.as<fmd_esearch_stat_t>());
        FMD_CHECK_LAUNCH("esearch kernels");
        fmd_esearch_stat_t ps;
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
                if (work.alloc(h, fmd_esearch_work_bytes(n, c2)) == FMD_OK) { cap = c2; grown = true; }
                else { cap_max = cap; FMD_TRY(work.alloc(h, fmd_esearch_work_bytes(n, cap))); }
            }
            if ((ps.overflow & 2) && hcap < max_hits) {
                hcap = 2 * hcap < max_hits ? 2 * hcap : max_hits;
                FMD_TRY(dhits.alloc(hcap * sizeof(fmd_esearch_hit_t)));
                grown = true;
            }
            if (!grown) return FMD_E_OVERFLOW;
            todo.push_back(std::make_pair(b0, b1));
            continue;
        }
        if (ps.n_unfinished) return FMD_E_OVERFLOW;    // (every query of the part has had its L + budget - 1 levels: cannot happen)
        FMD_HIP_TRY(hipMemcpy(out.strata.data() + b0 * cols * 2, part_strata, m * cols * 16, hipMemcpyDeviceToHost));
        stat->n_hits += ps.n_hits; stat->n_occ += ps.n_occ; stat->n_truncated += ps.n_truncated;
        if (!listed) continue;
        const uint64_t stored = ps.n_hits + ps.n_truncated * (uint64_t)max_hits;
        part_hits.resize(stored);
        if (stored) FMD_HIP_TRY(hipMemcpy(part_hits.data(), dhits.p, stored * sizeof(fmd_esearch_hit_t), hipMemcpyDeviceToHost));
        for (uint64_t j = 0; j < stored; ++j) {
            fmd_esearch_hit_t e = part_hits[j];
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

static int esr_batch(fmd_dev_t *h, size_t n, const uint8_t *seqs, const uint64_t *off, int max_edit, uint32_t max_hits, unsigned flags, uint64_t cap,
                     fmd_esearch_hit_t **hits, uint64_t *n_hits, uint64_t *strata, fmd_esearch_stat_t *stat)
{
    if (!h || !stat || max_edit < 0 || max_edit > FMD_ESEARCH_MAX_EDIT || (flags & ~(FMD_ESEARCH_NO_PRUNE | FMD_ESEARCH_BEST))) return FMD_E_ARG;
    if ((hits && !n_hits) || (n && (!seqs || !off || !strata))) return FMD_E_ARG;
    if (cap && (cap < FMD_ESEARCH_MIN_CAP || cap > FMD_ESEARCH_MAX_CAP)) return FMD_E_ARG;
    memset(stat, 0, sizeof(*stat));
    if (hits) { *hits = nullptr; *n_hits = 0; }
    if (n >= (1ull << 32)) return FMD_E_ARG;
    if (n == 0) {
        if (hits && !(*hits = (fmd_esearch_hit_t *)malloc(sizeof(fmd_esearch_hit_t)))) return FMD_E_NOMEM;
        return FMD_OK;
    }
    FMD_HIP_TRY(hipSetDevice(h->device));
    const size_t cols = (size_t)max_edit + 1;
    memset(strata, 0, n * cols * 16);
    std::vector<uint32_t> ids;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t L = off[i + 1] - off[i];
        if (off[i + 1] < off[i] || L == 0 || L > FMD_ESEARCH_MAX_LEN) ++stat->n_skipped; else ids.push_back((uint32_t)i);
    }
    const bool prune = !(flags & FMD_ESEARCH_NO_PRUNE), listed = hits != nullptr;
    std::vector<fmd_esearch_hit_t> all;
    EsrRun run;
    for (int budget = (flags & FMD_ESEARCH_BEST) ? 0 : max_edit; budget <= max_edit && !ids.empty(); ++budget) {
        FMD_TRY(esr_run(h, seqs, off, ids, budget, max_hits, prune, listed, cap, run, stat));
        const size_t rc = (size_t)budget + 1;
        std::vector<uint32_t> rest;
        for (size_t i = 0; i < ids.size(); ++i) {
            uint64_t nh = 0;
            for (size_t c = 0; c < rc; ++c) nh += run.strata[(i * rc + c) * 2];
            if (nh == 0 && budget < max_edit) { rest.push_back(ids[i]); continue; }
            memcpy(strata + (size_t)ids[i] * cols * 2, run.strata.data() + i * rc * 2, rc * 16);
        }
        for (size_t j = 0; j < run.hits.size(); ++j) { fmd_esearch_hit_t e = run.hits[j]; e.query = ids[e.query]; all.push_back(e); }
        ids.swap(rest);
    }
    if (!listed) return FMD_OK;
    std::sort(all.begin(), all.end(), [](const fmd_esearch_hit_t &x, const fmd_esearch_hit_t &y) {
        return x.query != y.query ? x.query < y.query : x.n_edit != y.n_edit ? x.n_edit < y.n_edit : x.beg != y.beg ? x.beg < y.beg : x.len < y.len;
    });
    fmd_esearch_hit_t *r = (fmd_esearch_hit_t *)malloc((all.empty() ? 1 : all.size()) * sizeof(fmd_esearch_hit_t));
    if (!r) return FMD_E_NOMEM;
    if (!all.empty()) memcpy(r, all.data(), all.size() * sizeof(fmd_esearch_hit_t));
    *hits = r; *n_hits = all.size();
    return FMD_OK;
}
extern "C" int fmd_esearch_batch(fmd_dev_t *h, size_t n, const uint8_t *seqs, const uint64_t *off, int max_edit, uint32_t max_hits, unsigned flags, uint64_t cap,
                                 fmd_esearch_hit_t **hits, uint64_t *n_hits, uint64_t *strata, fmd_esearch_stat_t *stat)
{
    try { return esr_batch(h, n, seqs, off, max_edit, max_hits, flags, cap, hits, n_hits, strata, stat); }
    catch (const std::bad_alloc &) { return FMD_E_NOMEM; }   // (the host vectors)
}
