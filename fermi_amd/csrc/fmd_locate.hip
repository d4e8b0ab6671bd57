// fmd_locate.hip -- locate: which sequences hold the rows of an SA interval, and at which offset.
//
// The FMD-index keeps no suffix-array samples (the reference never locates).  It needs none: every sequence ends at a '$' at most one
// read length to the left, so the LF-walk from a row reaches '$' within that many steps; the row it lands on is the sequence's sentinel
// rank -- what fm_retrieve returns (exact.c:59-70), the index into seqsort's map -- and the number of steps is the offset of the row's
// suffix in that sequence.  k_retrieve does this for one row per lane.  The rows of one interval share their left context, though (at
// 30x the ~25 rows of a 25-mer all read the same genome to their left), so locate walks INTERVALS, level by level, the way the k-mer
// harvest walks its trie (fmd_kmer.hip): one backward extension per item splits it by the preceding symbol; the '$' child is a
// contiguous range of sentinel ranks, all at the current depth, and leaves as ONE run; the other children -- N included: a walk does
// not stop at an N -- are the items of the next level.  One launch per level, frontier sizes in device counters, no per-lane stacks.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "fmd_internal.h"
#include "fmd_kernel_common.h"
#include "fmd_level.h"

// An item: the rows [x0, x0 + size) of query `query`; its depth is the level it stands in.  All zero = a hole.
struct LocItem { uint32_t x0_lo, x0_hi, size, query; };
static_assert(sizeof(LocItem) == 16 && sizeof(fmd_locate_run_t) == 24 && sizeof(fmd_locate_stat_t) == 48, "layouts of include/fmd_hip.h");

// counters at the head of the work area (u64 words): the frontier sizes rotate through three words -- level d reads word d % 3, counts
// its children in word (d + 1) % 3 and clears word (d + 2) % 3, which the level before it read and the level after it will count in
#define LOC_RUNS 3       // runs emitted (counts on when d_runs is full)
#define LOC_ROWS 4       // rows in the runs that were stored
#define LOC_SKIP 5       // intervals level 0 left out
#define LOC_UNFIN 6      // rows still walking after the last level
#define LOC_OVF 7        // a run or an item did not fit
#define LOC_EXT 8        // backward extensions done
#define LOC_WORDS 16
#define LOC_HDR_BYTES 256
// A wave reserves frontier slots LOC_CHUNK at a time (one device-wide atomic per chunk; at least the 5 x 64 children of one step) and fills a chunk
// to its last slot before it takes the next (km_reserve_split), so a level holds its live items + the tail of at most one chunk per wave.  Level
// d + 1 holds disjoint non-empty sub-ranges of the rows still walking: never more live items than rows.  Hence the capacity of a frontier:
#define LOC_CHUNK 512u
#define LOC_MAX_WAVES 4096u
static_assert(LOC_CHUNK >= 5 * 64, "one step's children fit one chunk");
// Runs leave through a buffer of LOC_RUN_BUF entries {rank, n, query} in the wave's LDS, behind the rank engine's landing area: nearly every step of a wave ends
// some sequence, and one atomic on the run counter per step -- 10^6 of them on one address at ~14 ns each -- cost more than the walk (the first version of this
// kernel: 20 ms where the row-by-row walk took 17).  The buffer is flushed with ONE atomic when the next step's runs might not fit, into slots that are exactly
// as many as the runs: d_runs stays dense and total_rows entries always suffice.
#define LOC_RUN_BUF 128
static_assert(LOC_RUN_BUF >= 64, "one step's runs fit the buffer");

static inline uint64_t loc_waves(uint64_t n, uint64_t rows)
{
    const uint64_t m = n > rows ? n : rows;
    uint64_t w = ((m + 63) / 64 + 7) & ~7ull;                 // (a multiple of 8: km_range gives every XCD its eighth)
    return w < 8 ? 8 : w > LOC_MAX_WAVES ? LOC_MAX_WAVES : w;
}
static inline uint64_t loc_cap(uint64_t n, uint64_t rows) { return rows + loc_waves(n, rows) * LOC_CHUNK; }

extern "C" size_t fmd_locate_work_bytes(size_t n, uint64_t total_rows)
{
    if (total_rows >> 58) return 0;
    return LOC_HDR_BYTES + 2 * (size_t)loc_cap(n, total_rows) * sizeof(LocItem);
}

// level 0: interval i -> item {beg[i], cnt[i], i}; empty intervals give nothing, those above max_occ -- and those that do not lie in the index -- are
// skipped whole and counted
__global__ __launch_bounds__(64) void k_locate_seed(uint64_t n_sym, size_t n, const uint64_t *__restrict__ beg, const uint64_t *__restrict__ cnt, uint32_t max_occ,
                                                    LocItem *__restrict__ out, uint64_t cap, unsigned long long *__restrict__ ctr)
{
    const int lane = fmd_lane();
    KmChunk ck; ck.base = 0; ck.fill = 0; ck.ch = LOC_CHUNK; ck.have = false;
    uint32_t n_skip = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < n; base += (uint64_t)gridDim.x * 64) {
        const uint64_t i = base + lane;
        const uint64_t c = i < n ? cnt[i] : 0, b = i < n ? beg[i] : 0;
        const bool skip = c != 0 && (c > max_occ || b >= n_sym || c > n_sym - b);
        const bool keep = c != 0 && !skip;
        n_skip += (uint32_t)__popcll(__ballot(skip));
        const uint64_t m = __ballot(keep);
        if (m == 0) continue;
        const KmSpan sp = km_reserve_split(ck, (uint32_t)__popcll(m), &ctr[0]);
        if (keep) {
            const uint64_t o = km_span_slot(sp, (uint32_t)fmd_below(m));
            if (o < cap) *(uint4 *)(out + o) = make_uint4((uint32_t)b, (uint32_t)(b >> 32), (uint32_t)c, (uint32_t)i);
            else ctr[LOC_OVF] = 1;
        }
    }
    km_zero_fill(out, cap, ck);
    if (lane == 0 && n_skip) atomicAdd(&ctr[LOC_SKIP], (unsigned long long)n_skip);
}

// the buffered runs -> d_runs (all 64 lanes together); rows = the rows of the runs this lane stored
__device__ __forceinline__ void loc_flush_runs(const uint4 *buf, uint32_t &fill, uint32_t d, unsigned long long *ctr, fmd_locate_run_t *runs, uint64_t run_cap, uint64_t &rows)
{
    if (fill == 0) return;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the lanes that wrote the entries are not the lanes that read them
    unsigned long long first = 0;
    if (fmd_lane() == 0) first = atomicAdd(&ctr[LOC_RUNS], (unsigned long long)fill);
    first = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(first >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)first);
    for (uint32_t j = (uint32_t)fmd_lane(); j < fill; j += 64) {
        const uint4 e = buf[j];
        if (first + j < run_cap) {
            fmd_locate_run_t r;
            r.rank = (uint64_t)e.y << 32 | e.x; r.n = e.z; r.off = d; r.query = e.w; r.reserved = 0;
            runs[first + j] = r;
            rows += e.z;
        } else ctr[LOC_OVF] = 1;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // read before the next step overwrites them
    fill = 0;
}

// one level: items at depth d -> runs at offset d + items at depth d + 1
__global__ __launch_bounds__(64) void k_locate_level(FmdIndexView ix, uint32_t d, const LocItem *__restrict__ in, LocItem *__restrict__ out, uint64_t cap,
                                                     unsigned long long *__restrict__ ctr, fmd_locate_run_t *__restrict__ runs, uint64_t run_cap, int xcd_aware)
{
    __shared__ uint4 fmd_lds[FMD_COMPACT_LDS_U4 + LOC_RUN_BUF];   // one array: the landing area of the rank engine, then the run buffer
    uint4 *run_buf = fmd_lds + FMD_COMPACT_LDS_U4;
    uint32_t run_fill = 0;                            // wave-uniform
    const int lane = fmd_lane();
    const uint32_t w_in = d % 3, w_out = (d + 1) % 3, w_clr = (d + 2) % 3;
    const uint64_t n = ctr[w_in] < cap ? ctr[w_in] : cap;   // an overflowing level counted more than it stored
    if (blockIdx.x == 0 && lane == 0) ctr[w_clr] = 0;
    const KmRange rg = km_range(n, xcd_aware);
    const uint64_t stride = rg.stride;
    KmChunk ck; ck.base = 0; ck.fill = 0; ck.ch = LOC_CHUNK; ck.have = false;
    uint32_t n_ext = 0;
    uint64_t rows = 0;
    uint4 nx = make_uint4(0, 0, 0, 0);                // the item of the next iteration, loaded one gather ahead
    if (rg.beg + lane < rg.end) nx = *(const uint4 *)(in + rg.beg + lane);
    for (uint64_t base = rg.beg; base < rg.end; base += stride) {
        const uint4 it = nx;
        const uint64_t x0 = (uint64_t)it.y << 32 | it.x, sz = it.z;
        const uint32_t q = it.w;
        const bool act = base + lane < rg.end && sz != 0;
        nx = make_uint4(0, 0, 0, 0);
        if (base + stride + lane < rg.end) nx = *(const uint4 *)(in + base + stride + lane);
        const uint64_t m_act = __ballot(act);
        if (m_act == 0) continue;                     // a run of holes
        n_ext += (uint32_t)__popcll(m_act);
        uint64_t tk[6], s[6];
        km_extend_back<true, true>(ix, fmd_lds, act, x0, sz, 1, tk, s);
        // the '$' child: the sequences that begin here.  tk[0] = the number of '$' before row x0 = the sentinel rank of the first of them
        const bool has0 = act && s[0] != 0;
        const uint64_t m0 = __ballot(has0);
        if (m0) {
            const uint32_t n0 = (uint32_t)__popcll(m0);
            if (run_fill + n0 > LOC_RUN_BUF) loc_flush_runs(run_buf, run_fill, d, ctr, runs, run_cap, rows);
            if (has0) run_buf[run_fill + (uint32_t)fmd_below(m0)] = make_uint4((uint32_t)tk[0], (uint32_t)(tk[0] >> 32), (uint32_t)s[0], q);
            run_fill += n0;
        }
        // children 1..5 (A, C, G, T, N) walk on
        const bool has1 = act && s[1] != 0, has2 = act && s[2] != 0, has3 = act && s[3] != 0, has4 = act && s[4] != 0, has5 = act && s[5] != 0;
        const uint64_t m1 = __ballot(has1), m2 = __ballot(has2), m3 = __ballot(has3), m4 = __ballot(has4), m5 = __ballot(has5);
        const uint32_t p1 = (uint32_t)__popcll(m1), p2 = p1 + (uint32_t)__popcll(m2), p3 = p2 + (uint32_t)__popcll(m3), p4 = p3 + (uint32_t)__popcll(m4);
        const uint32_t tot = p4 + (uint32_t)__popcll(m5);
        if (tot == 0) continue;
        const KmSpan sp = km_reserve_split(ck, tot, &ctr[w_out]);
#define LOC_PUSH(c, has, j)                                                                       \
        if (has) {                                                                                \
            const uint64_t o = km_span_slot(sp, (j)), nx0 = ix.cnt[c] + tk[c];                    \
            if (o < cap) *(uint4 *)(out + o) = make_uint4((uint32_t)nx0, (uint32_t)(nx0 >> 32), (uint32_t)s[c], q); \
            else ctr[LOC_OVF] = 1;                                                                \
        }
        LOC_PUSH(1, has1, (uint32_t)fmd_below(m1)) LOC_PUSH(2, has2, p1 + (uint32_t)fmd_below(m2)) LOC_PUSH(3, has3, p2 + (uint32_t)fmd_below(m3))
        LOC_PUSH(4, has4, p3 + (uint32_t)fmd_below(m4)) LOC_PUSH(5, has5, p4 + (uint32_t)fmd_below(m5))
#undef LOC_PUSH
    }
    km_zero_fill(out, cap, ck);
    loc_flush_runs(run_buf, run_fill, d, ctr, runs, run_cap, rows);
    rows = km_wave_sum(rows);
    if (lane == 0 && n_ext) atomicAdd(&ctr[LOC_EXT], (unsigned long long)n_ext);
    if (lane == 0 && rows) atomicAdd(&ctr[LOC_ROWS], (unsigned long long)rows);
}

// the rows of the frontier the last level left
__global__ __launch_bounds__(64) void k_locate_rest(uint32_t d, const LocItem *__restrict__ in, uint64_t cap, unsigned long long *__restrict__ ctr)
{
    const uint64_t n = ctr[d % 3] < cap ? ctr[d % 3] : cap;
    uint64_t rows = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 64 + fmd_lane(); i < n; i += (uint64_t)gridDim.x * 64) rows += in[i].size;
    rows = km_wave_sum(rows);
    if (fmd_lane() == 0 && rows) atomicAdd(&ctr[LOC_UNFIN], (unsigned long long)rows);
}
__global__ void k_locate_stat(const unsigned long long *__restrict__ ctr, uint64_t run_cap, fmd_locate_stat_t *__restrict__ stat)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    fmd_locate_stat_t s;
    s.n_runs = ctr[LOC_RUNS] < run_cap ? ctr[LOC_RUNS] : run_cap;
    s.n_rows = ctr[LOC_ROWS]; s.n_skipped = ctr[LOC_SKIP]; s.n_unfinished = ctr[LOC_UNFIN];
    s.overflow = (ctr[LOC_OVF] != 0 || ctr[LOC_RUNS] > run_cap) ? 1 : 0;
    s.n_ext = ctr[LOC_EXT];
    *stat = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct LocPlan {
    FmdIndexView ix;
    unsigned long long *ctr;
    LocItem *f[2];            // level d reads f[d & 1] and writes f[~d & 1]
    uint64_t cap;             // entries of each
    int grid;
};

// The frontier capacity follows from the work area; the grid from the rows that capacity was sized for (never more waves than the chunk tails it allows for).
static int loc_plan(fmd_dev_t *h, size_t n, void *d_work, size_t work_bytes, LocPlan &p)
{
    if (work_bytes < fmd_locate_work_bytes(n, 0) || ((uintptr_t)d_work & 15)) return FMD_E_ARG;
    p.cap = (work_bytes - LOC_HDR_BYTES) / (2 * sizeof(LocItem));
    uint64_t lo = 0, hi = p.cap;                       // the largest `rows` with loc_cap(n, rows) <= cap (loc_cap grows with rows)
    while (lo < hi) { const uint64_t mid = lo + (hi - lo + 1) / 2; if (loc_cap(n, mid) <= p.cap) lo = mid; else hi = mid - 1; }
    static int per_cu = 0;
    if (!per_cu) per_cu = fmd_resident_per_cu(k_locate_level, (FMD_COMPACT_LDS_U4 + LOC_RUN_BUF) * 16, 16, "k_locate_level");
    int grid = (int)loc_waves(n, lo);
    const int resident = (h->n_cu * per_cu) & ~7;
    if (grid > resident && resident >= 8) grid = resident;
    p.grid = grid;
    p.ix = fmd_view(h);
    p.ctr = (unsigned long long *)d_work;
    p.f[0] = (LocItem *)((uint8_t *)d_work + LOC_HDR_BYTES); p.f[1] = p.f[0] + p.cap;
    return FMD_OK;
}
static void loc_seed(const LocPlan &p, hipStream_t st, size_t n, const uint64_t *d_beg, const uint64_t *d_cnt, uint32_t max_occ)
{
    (void)hipMemsetAsync(p.ctr, 0, LOC_WORDS * 8, st);
    k_locate_seed<<<p.grid, 64, 0, st>>>(p.ix.n_sym, n, d_beg, d_cnt, max_occ, p.f[0], p.cap, p.ctr);
}
static void loc_levels(const LocPlan &p, hipStream_t st, uint32_t d0, uint32_t n_lev, fmd_locate_run_t *d_runs, uint64_t run_cap)
{
    static const int xcd_aware = getenv("FMD_LOCATE_XCD") ? atoi(getenv("FMD_LOCATE_XCD")) : 1;
    for (uint32_t d = d0; d - d0 < n_lev; ++d)
        k_locate_level<<<p.grid, 64, 0, st>>>(p.ix, d, p.f[d & 1], p.f[~d & 1], p.cap, p.ctr, d_runs, run_cap, xcd_aware);
}
static void loc_finish(const LocPlan &p, hipStream_t st, uint32_t d, uint64_t run_cap, fmd_locate_stat_t *d_stat)
{
    k_locate_rest<<<p.grid, 64, 0, st>>>(d, p.f[d & 1], p.cap, p.ctr);
    k_locate_stat<<<1, 64, 0, st>>>(p.ctr, run_cap, d_stat);
}

extern "C" int fmd_locate_dev(fmd_dev_t *h, void *stream, size_t n, const uint64_t *d_beg, const uint64_t *d_cnt, uint32_t max_occ, uint32_t levels,
                              fmd_locate_run_t *d_runs, uint64_t run_cap, fmd_locate_stat_t *d_stat, void *d_work, size_t work_bytes)
{
    if (!h || (n && (!d_beg || !d_cnt || !d_stat || !d_work || (run_cap && !d_runs)))) return FMD_E_ARG;
    if (n == 0) return FMD_OK;
    if (n >= (1ull << 32)) return FMD_E_ARG;           // the query index of an item is 32 bits
    if (work_bytes < fmd_locate_work_bytes(n, 0)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h->device));
    LocPlan p;
    FMD_TRY(loc_plan(h, n, d_work, work_bytes, p));
    hipStream_t st = (hipStream_t)stream;
    loc_seed(p, st, n, d_beg, d_cnt, max_occ);
    loc_levels(p, st, 0, levels, d_runs, run_cap);
    loc_finish(p, st, levels, run_cap, d_stat);
    FMD_CHECK_LAUNCH("locate kernels");
    return FMD_OK;
}

extern "C" int fmd_locate_batch(fmd_dev_t *h, size_t n, const uint64_t *beg, const uint64_t *cnt, uint32_t max_occ, uint32_t max_len,
                                fmd_locate_run_t **runs, uint64_t *n_runs, fmd_locate_stat_t *stat)
{
    if (!h || !runs || !n_runs || !stat || (n && (!beg || !cnt))) return FMD_E_ARG;
    *runs = nullptr; *n_runs = 0; memset(stat, 0, sizeof(*stat));
    if (n >= (1ull << 32)) return FMD_E_ARG;
    if (n == 0) { *runs = (fmd_locate_run_t *)malloc(sizeof(fmd_locate_run_t)); return *runs ? FMD_OK : FMD_E_NOMEM; }
    FMD_HIP_TRY(hipSetDevice(h->device));
    uint64_t total = 0;                                // the rows level 0 will keep
    for (size_t i = 0; i < n; ++i) if (cnt[i] && cnt[i] <= max_occ && beg[i] < h->mcnt[0] && cnt[i] <= h->mcnt[0] - beg[i]) total += cnt[i];
    const size_t wb = fmd_locate_work_bytes(n, total);
    if (wb == 0) return FMD_E_ARG;
    FmdDevBuf db, dc, dr, ds, work;
    FMD_TRY(db.alloc(n * 8)); FMD_TRY(dc.alloc(n * 8)); FMD_TRY(dr.alloc((total ? total : 1) * sizeof(fmd_locate_run_t))); FMD_TRY(ds.alloc(sizeof(fmd_locate_stat_t)));
    FMD_TRY(work.alloc(wb));
    FMD_HIP_TRY(hipMemcpy(db.p, beg, n * 8, hipMemcpyHostToDevice));
    FMD_HIP_TRY(hipMemcpy(dc.p, cnt, n * 8, hipMemcpyHostToDevice));
    LocPlan p;
    FMD_TRY(loc_plan(h, n, work.p, wb, p));
    hipStream_t st = nullptr;
    loc_seed(p, st, n, db.as<uint64_t>(), dc.as<uint64_t>(), max_occ);
    uint32_t d = 0;
    for (;;) {                                         // groups of levels; the host looks at the frontier between groups only
        unsigned long long left = 0;
        FMD_HIP_TRY(hipMemcpy(&left, p.ctr + d % 3, 8, hipMemcpyDeviceToHost));
        if (left == 0 || (max_len && d >= max_len) || (uint64_t)d > h->mcnt[0]) break;
        uint32_t g = 64;
        if (max_len && max_len - d < g) g = max_len - d;
        loc_levels(p, st, d, g, dr.as<fmd_locate_run_t>(), total);
        d += g;
    }
    loc_finish(p, st, d, total, ds.as<fmd_locate_stat_t>());
    FMD_CHECK_LAUNCH("locate kernels");
    FMD_HIP_TRY(hipMemcpy(stat, ds.p, sizeof(*stat), hipMemcpyDeviceToHost));
    if (stat->overflow) return FMD_E_OVERFLOW;
    fmd_locate_run_t *r = (fmd_locate_run_t *)malloc((stat->n_runs ? stat->n_runs : 1) * sizeof(fmd_locate_run_t));
    if (!r) return FMD_E_NOMEM;
    if (stat->n_runs && hipMemcpy(r, dr.p, stat->n_runs * sizeof(fmd_locate_run_t), hipMemcpyDeviceToHost) != hipSuccess) { free(r); return FMD_E_HIP; }
    std::sort(r, r + stat->n_runs, [](const fmd_locate_run_t &a, const fmd_locate_run_t &b) {
        return a.query != b.query ? a.query < b.query : a.off != b.off ? a.off < b.off : a.rank < b.rank;
    });
    *runs = r; *n_runs = stat->n_runs;
    return FMD_OK;
}
