// fmd_kcount.hip -- kcount: the k-mer spectrum and the counted k-mers of the indexed reads.
//
// The index holds both strands of every read, so one backward extension counts a k-mer exactly: occ(W) = the size of W's interval, and
// occ(W) = occ(rc(W)).  The walk is the harvest's (fmd_kmer.hip): the trie of the k-mers, rooted at the LAST base, level by level, one
// backward extension per node (km_level_step, fmd_level.h), with one threshold at every depth -- occ only shrinks as a k-mer grows, so
// pruning below min_occ is exact.  What differs is the end and the memory:
//   - the leaf kernel runs on the frontier at depth k - 1 and takes the child SIZES only; the depth-k frontier -- the widest level, with
//     min_occ = 1 mostly singletons -- is never stored.  A child W is kept iff rc(W) <= W and counts occ(W), or occ(W) / 2 when
//     W = rc(W); what is kept goes to the histogram, to two sums, and -- when a list is wanted -- out as (rc(W), count): the canonical
//     k-mer, whose FIRST bases are the reverse complement of the root's;
//   - a part is a run of roots (suffixes of one length) walked inside a fixed capacity.  A part that overflows is discarded whole and its
//     run is cut: in two, or -- a single root -- into its children one base deeper.  Parts taken in the order of rc(suffix) emit ascending
//     slices, so the list is globally sorted without a final sort and never held whole.
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include "fmd_prim.h"
#include "fmd_internal.h"
#include "fmd_kernel_common.h"
#include "fmd_level.h"

static_assert(sizeof(fmd_kcount_stat_t) == 56, "layout of include/fmd_hip.h");

// counters at the head of the work area (u64 words): [d] = the entries of the frontier at depth d (d = root_len .. k - 1 <= 31), then
#define KC_OUT 40        // pairs emitted (counts on when the list is full)
#define KC_OVF 41        // a frontier entry did not fit
#define KC_NKMER 42      // k-mers kept
#define KC_NTOTAL 43     // the sum of their counts
#define KC_EXT 44        // backward extensions done
#define KC_WORDS 48
#define KC_HDR_BYTES 512
// the low bins of the histogram live in the wave's LDS behind the rank engine's landing area (KC_LBINS x u32) and reach the global
// histogram in one pass at the end; a count of KC_LBINS and more -- rare at any coverage a spectrum is read at -- goes straight to global
#define KC_LBINS 256
#define KC_LDS_U4 (FMD_COMPACT_LDS_U4 + KC_LBINS / 4)
#define KC_EMIT_BUF 256     // pairs staged per wave, (u64 k-mer, u32 count) in two arrays: one step's at most (4 x 64)
#define KC_EMIT_U4 (KC_EMIT_BUF * 12 / 16)
#define KC_MIN_CHUNK 256u   // one step's children (4 x 64) fit one chunk
static_assert(FMD_KCOUNT_MIN_CAP >= 2 * KC_MIN_CHUNK, "the smallest capacity holds one wave's chunk tail and as much again");

extern "C" size_t fmd_kcount_work_bytes(uint64_t cap)
{
    if (cap < FMD_KCOUNT_MIN_CAP || cap > FMD_KCOUNT_MAX_CAP) return 0;
    return KC_HDR_BYTES + 256 + 2 * (size_t)cap * sizeof(fmd_intv_t);
}

__global__ void k_kcount_init(unsigned long long *__restrict__ ctr, int root_len, unsigned long long n_roots)
{
    const int i = (int)threadIdx.x;
    if (blockIdx.x == 0 && i < KC_WORDS) ctr[i] = i == root_len ? n_roots : 0;
}

// one inner level: nodes at depth d -> children with at least min_occ occurrences at depth d + 1
__global__ __launch_bounds__(64) void k_kcount_level(FmdIndexView ix, int d, uint64_t min_occ, const fmd_intv_t *__restrict__ in, fmd_intv_t *__restrict__ out,
                                                     uint64_t cap, uint32_t ch, unsigned long long *__restrict__ ctr, int xcd_aware)
{
    FMD_DECLARE_COMPACT_LDS();
    km_level_step(ix, fmd_lds, d, min_occ, in, out, cap, ch, ctr, KC_OVF, KC_EXT, xcd_aware);
}

// the staged pairs -> the list (all 64 lanes together): ONE atomic for `fill` dense slots, stores of consecutive lanes side by side
__device__ __forceinline__ void kc_flush_pairs(const uint64_t *ek, const uint32_t *ec, uint32_t &fill, unsigned long long *ctr, uint64_t *o_kmer, uint32_t *o_count,
                                               uint64_t out_cap)
{
    if (fill == 0) return;
    __syncthreads();                                  // the lanes that staged the pairs are not the lanes that store them
    unsigned long long first = 0;
    if (fmd_lane() == 0) first = atomicAdd(&ctr[KC_OUT], (unsigned long long)fill);
    first = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(first >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)first);
    for (uint32_t j = (uint32_t)fmd_lane(); j < fill; j += 64)
        if (first + j < out_cap) { o_kmer[first + j] = ek[j]; o_count[first + j] = ec[j]; }   // (k_kcount_stat sets the flag: the counter went past out_cap)
    __syncthreads();                                  // read before the next step stages over them
    fill = 0;
}

// the leaves: nodes at depth k - 1 -> the k-mers W = c . node, by size alone.  LIST: the kept ones leave as (rc(W), count) through KC_EMIT_BUF pairs staged in
// LDS -- one atomic on the list's counter per wave and step, 10^6 of them on one address, cost as much as the walk of the leaves itself (14.1 ms against
// 7.7 ms without a list at 10^6 reads, k = 21; the same was seen in locate) -- flushed when the next step's pairs might not fit.
template <bool LIST>
__global__ __launch_bounds__(64) void k_kcount_leaf(FmdIndexView ix, int k, uint64_t min_occ, const fmd_intv_t *__restrict__ in, uint64_t cap, uint32_t n_bins,
                                                    unsigned long long *__restrict__ hist, uint64_t *__restrict__ o_kmer, uint32_t *__restrict__ o_count,
                                                    uint64_t out_cap, unsigned long long *__restrict__ ctr, int xcd_aware)
{
    __shared__ uint4 fmd_lds[KC_LDS_U4 + (LIST ? KC_EMIT_U4 : 0)];   // one array: the landing area of the rank engine, the low bins, the staged pairs
    uint32_t *bins = (uint32_t *)(fmd_lds + FMD_COMPACT_LDS_U4);
    uint64_t *ek = (uint64_t *)(fmd_lds + KC_LDS_U4);
    uint32_t *ec = (uint32_t *)(ek + KC_EMIT_BUF);
    uint32_t fill = 0;                                // wave-uniform
    const int lane = fmd_lane();
    const uint32_t last = n_bins - 1;                 // the bin of `last` and more
    const uint32_t n_low = n_bins < KC_LBINS ? n_bins : KC_LBINS;   // bins below n_low are kept in LDS (a short histogram whole, its last bin too: with
                                                      // n_bins = 2 every k-mer lands there, and 2 x 10^7 atomics on one global word took 0.22 s)
    for (int j = lane; j < KC_LBINS; j += 64) bins[j] = 0;
    __syncthreads();
    const uint64_t n = ctr[k - 1] < cap ? ctr[k - 1] : cap;
    const KmRange rg = km_range(n, xcd_aware);
    const uint64_t stride = rg.stride;
    uint32_t n_keep = 0, n_ext = 0;
    uint64_t total = 0;
    uint4 na = make_uint4(0, 0, 0, 0), nb = na;       // the entry of the next iteration, loaded one gather ahead
    {
        const uint64_t i0 = rg.beg + lane;
        if (i0 < rg.end) { const uint4 *q = (const uint4 *)(in + i0); na = q[0]; nb = q[1]; }
    }
    for (uint64_t base = rg.beg; base < rg.end; base += stride) {
        const uint4 a = na, b = nb;
        const uint64_t x0 = (uint64_t)a.y << 32 | a.x;
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
        km_extend_back<false>(ix, fmd_lds, act, x0, sz, 0, tk, s);
        uint64_t rc[5], cnt[5], m[5];
        bool keep[5];
        uint32_t tot = 0;
#pragma unroll
        for (int c = 1; c <= 4; ++c) {
            const uint64_t W = K | (uint64_t)(c - 1) << (2 * (k - 1));
            rc[c] = kc_revcomp(W, k);
            cnt[c] = rc[c] == W ? s[c] >> 1 : s[c];   // a k-mer that is its own reverse complement is seen twice per occurrence
            keep[c] = act && rc[c] <= W && cnt[c] >= min_occ;   // (min_occ >= 1: a child that does not occur is not kept)
            m[c] = __ballot(keep[c]);
            tot += (uint32_t)__popcll(m[c]);
        }
        if (tot == 0) continue;
        n_keep += tot;
#pragma unroll
        for (int c = 1; c <= 4; ++c)
            if (keep[c]) {
                total += cnt[c];
                const uint32_t bin = cnt[c] < last ? (uint32_t)cnt[c] : last;
                if (bin < n_low) atomicAdd(&bins[bin], 1u);
                else atomicAdd(&hist[bin], 1ull);
            }
        if (LIST) {
            if (fill + tot > KC_EMIT_BUF) kc_flush_pairs(ek, ec, fill, ctr, o_kmer, o_count, out_cap);
#pragma unroll
            for (int c = 1; c <= 4; ++c) {
                if (keep[c]) {
                    const uint32_t j = fill + (uint32_t)fmd_below(m[c]);
                    ek[j] = rc[c]; ec[j] = cnt[c] > 0xffffffffull ? 0xffffffffu : (uint32_t)cnt[c];
                }
                fill += (uint32_t)__popcll(m[c]);
            }
        }
    }
    if (LIST) kc_flush_pairs(ek, ec, fill, ctr, o_kmer, o_count, out_cap);
    __syncthreads();
    for (uint32_t j = (uint32_t)lane; j < n_low; j += 64) {
        const uint32_t v = bins[j];
        if (v) atomicAdd(&hist[j], (unsigned long long)v);
    }
    total = km_wave_sum(total);
    if (lane == 0 && n_ext) atomicAdd(&ctr[KC_EXT], (unsigned long long)n_ext);
    if (lane == 0 && n_keep) { atomicAdd(&ctr[KC_NKMER], (unsigned long long)n_keep); atomicAdd(&ctr[KC_NTOTAL], (unsigned long long)total); }
}

__global__ void k_kcount_stat(const unsigned long long *__restrict__ ctr, int root_len, int k, uint64_t out_cap, int listed, fmd_kcount_stat_t *__restrict__ stat)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    fmd_kcount_stat_t s;
    s.n_kmers = ctr[KC_NKMER]; s.n_total = ctr[KC_NTOTAL]; s.n_ext = ctr[KC_EXT];
    s.overflow = (ctr[KC_OVF] != 0 || (listed && ctr[KC_OUT] > out_cap)) ? 1 : 0;
    s.widest_level = 0;
    for (int d = root_len; d < k; ++d) if (ctr[d] > s.widest_level) s.widest_level = ctr[d];
    s.n_parts = 1; s.n_retries = 0;
    *stat = s;
}

// Grids and chunk for a capacity.  The kernels walk the frontier by static ranges: a grid is at most the kernel's resident set.  A wave of a level leaves at
// most one partial chunk, and those tails take at most half of the capacity: chunk and grid shrink with it.  The leaves run on no more waves than the levels.
static void kc_plan(fmd_dev_t *h, uint64_t cap, bool listed, int &grid, int &leaf_grid, uint32_t &ch)
{
    static int per_cu[3] = {0, 0, 0};
    if (!per_cu[0]) {
        per_cu[1] = fmd_resident_per_cu(k_kcount_leaf<false>, KC_LDS_U4 * 16, 16, "k_kcount_leaf<false>");
        per_cu[2] = fmd_resident_per_cu(k_kcount_leaf<true>, (KC_LDS_U4 + KC_EMIT_U4) * 16, 16, "k_kcount_leaf<true>");
        per_cu[0] = fmd_resident_per_cu(k_kcount_level, FMD_COMPACT_LDS_U4 * 16, 16, "k_kcount_level");
    }
    grid = fmd_grid_for_lds(h, cap, FMD_COMPACT_LDS_U4 * 16);
    if (grid > h->n_cu * per_cu[0]) grid = h->n_cu * per_cu[0];
    ch = 1024;
    while (ch > KC_MIN_CHUNK && (uint64_t)grid * ch * 8 > cap) ch >>= 1;
    const uint64_t g = cap / (2 * (uint64_t)ch);
    if ((uint64_t)grid > g) grid = (int)g;
    if (grid >= 8) grid &= ~7;                        // (a multiple of 8: km_range gives every XCD its eighth)
    if (grid < 1) grid = 1;
    leaf_grid = h->n_cu * per_cu[listed ? 2 : 1];
    if (leaf_grid > grid) leaf_grid = grid;
    if (leaf_grid >= 8) leaf_grid &= ~7;
    if (leaf_grid < 1) leaf_grid = 1;
}

static_assert(FMD_KCOUNT_CTR_OVF == KC_OVF && FMD_KCOUNT_CTR_EXT == KC_EXT, "the counters fmd_internal.h names for fmd_kcount_levels");

// The walk without its end (fmd_internal.h): the counters start from the roots, and the levels root_len .. depth - 1 run; *d_frontier = the nodes at `depth`
// (d_roots itself when depth = root_len), ctr[depth] of them with the holes, ctr = the head of d_work.  The arguments are the caller's to check.
int fmd_kcount_levels(fmd_dev_t *h, hipStream_t st, int depth, int min_occ, int root_len, size_t n_roots, const fmd_intv_t *d_roots, uint64_t cap, void *d_work,
                      const fmd_intv_t **d_frontier, int *level_grid)
{
    unsigned long long *ctr = (unsigned long long *)d_work;
    fmd_intv_t *f[2];
    f[0] = (fmd_intv_t *)(((uintptr_t)((uint8_t *)d_work + KC_HDR_BYTES) + 255) & ~(uintptr_t)255); f[1] = f[0] + cap;
    const FmdIndexView ix = fmd_view(h);
    int grid, leaf_grid; uint32_t ch;
    kc_plan(h, cap, false, grid, leaf_grid, ch);
    k_kcount_init<<<1, 64, 0, st>>>(ctr, root_len, (unsigned long long)n_roots);
    const fmd_intv_t *in = d_roots;
    for (int d = root_len; d < depth; ++d) {
        fmd_intv_t *out = f[(d - root_len) & 1];
        k_kcount_level<<<grid, 64, 0, st>>>(ix, d, (uint64_t)min_occ, in, out, cap, ch, ctr, 1);
        in = out;
    }
    *d_frontier = in;
    if (level_grid) *level_grid = grid;
    return FMD_OK;
}

extern "C" int fmd_kcount_part_dev(fmd_dev_t *h, void *stream, int k, int min_occ, int root_len, size_t n_roots, const fmd_intv_t *d_roots, uint64_t cap,
                                   uint32_t n_bins, uint64_t *d_hist, uint64_t *d_kmer, uint32_t *d_count, uint64_t out_cap, fmd_kcount_stat_t *d_stat,
                                   void *d_work, size_t work_bytes)
{
    if (!h || !d_hist || !d_stat || !d_work || (n_roots && !d_roots) || (d_kmer && !d_count)) return FMD_E_ARG;
    if (k < 2 || k > 32 || min_occ < 1 || n_bins < 2 || root_len < 1 || root_len >= k) return FMD_E_ARG;
    const size_t wb = fmd_kcount_work_bytes(cap);
    if (wb == 0 || work_bytes < wb || n_roots > cap || ((uintptr_t)d_work & 15) || ((uintptr_t)d_roots & 15)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *ctr = (unsigned long long *)d_work;
    const FmdIndexView ix = fmd_view(h);
    int grid, leaf_grid; uint32_t ch;
    kc_plan(h, cap, d_kmer != nullptr, grid, leaf_grid, ch);
    const fmd_intv_t *in = nullptr;
    FMD_TRY(fmd_kcount_levels(h, st, k - 1, min_occ, root_len, n_roots, d_roots, cap, d_work, &in, nullptr));
    if (d_kmer) k_kcount_leaf<true><<<leaf_grid, 64, 0, st>>>(ix, k, (uint64_t)min_occ, in, cap, n_bins, (unsigned long long *)d_hist, d_kmer, d_count, out_cap, ctr, 1);
    else k_kcount_leaf<false><<<leaf_grid, 64, 0, st>>>(ix, k, (uint64_t)min_occ, in, cap, n_bins, (unsigned long long *)d_hist, nullptr, nullptr, 0, ctr, 1);
    k_kcount_stat<<<1, 64, 0, st>>>(ctr, root_len, k, out_cap, d_kmer != nullptr, d_stat);
    FMD_CHECK_LAUNCH("kcount kernels");
    return FMD_OK;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct KcRoot { fmd_intv_t iv; int len; };
typedef std::vector<KcRoot> KcRun;                    // roots of one length, rc(suffix) ascending

// What a run of parts keeps, sized by the capacity.  The large buffers come from the handle's scratch cache (fmd_scratch_acquire): a second call on the
// handle finds them there -- at 10^6 reads hipMalloc of the frontiers alone took 0.4 s, fifty times the walk -- and fmd_dev_trim / fmd_dev_close return them.
// The list leaves through two pinned slices of KC_SLICE pairs: a part is never held whole on the host.
#define KC_SLICE (1u << 20)
struct KcBufs {
    uint64_t cap = 0, out_cap = 0;
    size_t wb = 0, tmp_bytes = 0;
    FmdScratch work, kmer[2], count[2], tmp;
    FmdDevBuf roots, hist, stat;
    FmdHostBuf h_kmer, h_count;
    int alloc(fmd_dev_t *h, uint64_t cap_, uint32_t n_bins, bool listed, int k)
    {
        cap = cap_; out_cap = listed ? cap_ : 0; wb = fmd_kcount_work_bytes(cap_);
        work.reset(); tmp.reset();
        for (int i = 0; i < 2; ++i) { kmer[i].reset(); count[i].reset(); }
        FMD_TRY(work.alloc(h, wb)); FMD_TRY(roots.need(4 * sizeof(fmd_intv_t))); FMD_TRY(hist.need((size_t)n_bins * 8)); FMD_TRY(stat.need(sizeof(fmd_kcount_stat_t)));
        if (!listed) return FMD_OK;
        for (int i = 0; i < 2; ++i) { FMD_TRY(kmer[i].alloc(h, out_cap * 8)); FMD_TRY(count[i].alloc(h, out_cap * 4)); }
        tmp_bytes = 0;
        FMD_HIP_TRY(fmd_sort_pairs(nullptr, tmp_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)out_cap, 0, 2 * k));
        FMD_TRY(tmp.alloc(h, tmp_bytes ? tmp_bytes : 16));
        FMD_TRY(h_kmer.need((size_t)KC_SLICE * 8));
        return h_count.need((size_t)KC_SLICE * 4);
    }
};

// every k-mer of one base: the marginal counts, no kernel
static int kc_single_bases(fmd_dev_t *h, int min_occ, uint32_t n_bins, uint64_t *hist, fmd_kcount_sink_fn sink, void *ctx, fmd_kcount_stat_t *stat)
{
    uint64_t kmer[2]; uint32_t count[2]; uint64_t n = 0;
    for (int c = 0; c < 2; ++c) {                     // A (= T on the other strand) and C (= G)
        const uint64_t v = h->mcnt[2 + c];
        if (v == 0 || v < (uint64_t)min_occ) continue;
        kmer[n] = (uint64_t)c; count[n] = v > 0xffffffffull ? 0xffffffffu : (uint32_t)v; ++n;
        ++hist[v < n_bins - 1 ? v : n_bins - 1]; ++stat->n_kmers; stat->n_total += v;
    }
    if (sink && n && sink(ctx, n, kmer, count)) return FMD_E_IO;
    return FMD_OK;
}

static int kc_run(fmd_dev_t *h, int k, int min_occ, uint32_t n_bins, uint64_t *hist, uint64_t cap, fmd_kcount_sink_fn sink, void *ctx, fmd_kcount_stat_t *stat);
extern "C" int fmd_kcount(fmd_dev_t *h, int k, int min_occ, uint32_t n_bins, uint64_t *hist, uint64_t cap, fmd_kcount_sink_fn sink, void *ctx,
                          fmd_kcount_stat_t *stat)
{
    try { return kc_run(h, k, min_occ, n_bins, hist, cap, sink, ctx, stat); }
    catch (const std::bad_alloc &) { return FMD_E_NOMEM; }   // (the host vectors)
}
static int kc_run(fmd_dev_t *h, int k, int min_occ, uint32_t n_bins, uint64_t *hist, uint64_t cap, fmd_kcount_sink_fn sink, void *ctx, fmd_kcount_stat_t *stat)
{
    if (!h || !hist || !stat || k < 1 || k > 32 || min_occ < 1 || n_bins < 2) return FMD_E_ARG;
    if (cap && (cap < FMD_KCOUNT_MIN_CAP || cap > FMD_KCOUNT_MAX_CAP)) return FMD_E_ARG;
    if (h->mcnt[2] != h->mcnt[5] || h->mcnt[3] != h->mcnt[4] || (h->mcnt[1] & 1)) return FMD_E_ARG;   // not an index of both strands
    memset(stat, 0, sizeof(*stat));
    memset(hist, 0, (size_t)n_bins * 8);
    if (k == 1) return kc_single_bases(h, min_occ, n_bins, hist, sink, ctx, stat);
    FMD_HIP_TRY(hipSetDevice(h->device));
    const bool listed = sink != nullptr;
    // capacity: the caller's, or -- cap = 0 -- half the symbols to start with, doubled after an overflow as long as it fits beside the index
    // (a level never holds more live entries than the index has symbols, and the chunk tails take at most as much again)
    uint64_t cap_max = cap;
    if (cap == 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)8 << 30;
        const uint64_t per = 2 * sizeof(fmd_intv_t) + (listed ? 2 * 12 + 4 : 0);
        cap_max = (uint64_t)(0.7 * (double)free_b) / per;
        if (cap_max > 2 * h->mcnt[0] + FMD_KCOUNT_MIN_CAP) cap_max = 2 * h->mcnt[0] + FMD_KCOUNT_MIN_CAP;
        if (cap_max > FMD_KCOUNT_MAX_CAP) cap_max = FMD_KCOUNT_MAX_CAP;
        if (cap_max < FMD_KCOUNT_MIN_CAP) cap_max = FMD_KCOUNT_MIN_CAP;
        cap = h->mcnt[0] / 2 + (1u << 16);
        if (cap > cap_max) cap = cap_max;
    }
    KcBufs b;
    for (;;) {                                        // (what hipMemGetInfo calls free is not always one piece)
        const int rc = b.alloc(h, cap, n_bins, listed, k);
        if (rc == FMD_OK) break;
        if (rc != FMD_E_NOMEM || cap_max == cap || cap / 2 < FMD_KCOUNT_MIN_CAP) return rc;
        cap /= 2; cap_max = cap;
    }
    std::vector<uint64_t> part_hist(n_bins);
    std::vector<KcRun> todo;                          // the back is next
    {
        KcRun first;
        for (int c = 4; c >= 1; --c) {                // suffix T, G, C, A: rc(suffix) = A, C, G, T
            KcRoot r;
            r.iv.x[0] = h->cnt[c]; r.iv.x[1] = h->cnt[5 - c]; r.iv.x[2] = h->cnt[c + 1] - h->cnt[c]; r.iv.info = (uint64_t)(c - 1); r.len = 1;
            if (r.iv.x[2] >= (uint64_t)min_occ) first.push_back(r);
        }
        todo.push_back(first);
    }
    while (!todo.empty()) {
        KcRun run = todo.back(); todo.pop_back();
        if (run.empty()) continue;
        fmd_intv_t roots[4];
        for (size_t i = 0; i < run.size(); ++i) roots[i] = run[i].iv;
        fmd_kcount_stat_t ps;
        FMD_HIP_TRY(hipMemcpy(b.roots.p, roots, run.size() * sizeof(fmd_intv_t), hipMemcpyHostToDevice));
        FMD_HIP_TRY(hipMemsetAsync(b.hist.p, 0, (size_t)n_bins * 8, nullptr));
        FMD_TRY(fmd_kcount_part_dev(h, nullptr, k, min_occ, run[0].len, run.size(), b.roots.as<fmd_intv_t>(), b.cap, n_bins, b.hist.as<uint64_t>(),
                                    listed ? b.kmer[0].as<uint64_t>() : nullptr, listed ? b.count[0].as<uint32_t>() : nullptr, b.out_cap,
                                    b.stat.as<fmd_kcount_stat_t>(), b.work.p, b.wb));
        FMD_HIP_TRY(hipMemcpy(&ps, b.stat.p, sizeof(ps), hipMemcpyDeviceToHost));
        ++stat->n_parts;
        stat->n_ext += ps.n_ext;                      // (the work of a discarded part was done all the same)
        if (ps.widest_level > stat->widest_level) stat->widest_level = ps.widest_level;
        if (ps.overflow) {                            // discarded whole
            ++stat->n_retries;
            if (b.cap < cap_max) {                    // there is room: the same run again in twice the capacity
                const uint64_t c2 = 2 * b.cap < cap_max ? 2 * b.cap : cap_max;
                if (b.alloc(h, c2, n_bins, listed, k) == FMD_OK) { cap = c2; todo.push_back(run); continue; }
                cap_max = cap;                        // it does not fit after all: back to what did, and cut the run
                FMD_TRY(b.alloc(h, cap, n_bins, listed, k));
            }
            if (run.size() > 1) {
                const size_t half = run.size() / 2;
                todo.push_back(KcRun(run.begin() + half, run.end()));
                todo.push_back(KcRun(run.begin(), run.begin() + half));
            } else {
                if (run[0].len >= k - 1) return FMD_E_OVERFLOW;   // (a single leaf root emits four pairs at most: cannot happen)
                fmd_intv_t ok[6];
                const uint8_t back = 1;
                FMD_TRY(fmd_extend_batch(h, 1, &run[0].iv, &back, ok));
                KcRun kids;
                for (int c = 4; c >= 1; --c) {        // c . suffix: rc = rc(suffix) . comp(c), ascending in comp(c)
                    KcRoot r;
                    r.iv = ok[c]; r.iv.info = run[0].iv.info | (uint64_t)(c - 1) << (2 * run[0].len); r.len = run[0].len + 1;
                    if (r.iv.x[2] >= (uint64_t)min_occ) kids.push_back(r);
                }
                todo.push_back(kids);
            }
            continue;
        }
        FMD_HIP_TRY(hipMemcpy(part_hist.data(), b.hist.p, (size_t)n_bins * 8, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n_bins; ++i) hist[i] += part_hist[i];
        stat->n_kmers += ps.n_kmers; stat->n_total += ps.n_total;
        if (listed && ps.n_kmers) {
            const uint64_t n = ps.n_kmers;
            size_t tb = b.tmp_bytes;
            FMD_HIP_TRY(fmd_sort_pairs(b.tmp.p, tb, b.kmer[0].as<uint64_t>(), b.kmer[1].as<uint64_t>(), b.count[0].as<uint32_t>(), b.count[1].as<uint32_t>(), (size_t)n, 0, 2 * k));
            for (uint64_t at = 0; at < n; at += KC_SLICE) {
                const uint64_t m = n - at < KC_SLICE ? n - at : KC_SLICE;
                FMD_HIP_TRY(hipMemcpy(b.h_kmer.p, b.kmer[1].as<uint64_t>() + at, m * 8, hipMemcpyDeviceToHost));
                FMD_HIP_TRY(hipMemcpy(b.h_count.p, b.count[1].as<uint32_t>() + at, m * 4, hipMemcpyDeviceToHost));
                if (sink(ctx, m, b.h_kmer.as<uint64_t>(), b.h_count.as<uint32_t>())) return FMD_E_IO;
            }
        }
    }
    return FMD_OK;
}
