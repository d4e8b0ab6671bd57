// fmd_kmat.hip -- kmat: the joint k-mer counts of up to FMD_KMAT_MAX_IDX indexes of both strands.
//
// kcmp (fmd_kcmp.hip) walks the k-mer tries of TWO indexes together; this walks N of them, 1 <= N <= 8.  A node is one suffix's interval (start,
// size) in EACH index plus the packed suffix: 16 (N + 1) bytes, so a run over three indexes does not pay for eight.  A level gives every node one
// backward extension per non-empty side, the sides taken two at a time through the two dense LDS slots (kp_extend's order, once per pair of sides;
// the last side of an odd N alone in its round, and a round in which no lane has a live side posts nothing).  The leaf kernel runs on the frontier at
// depth k - 1, takes the child SIZES in every index, keeps W iff rc(W) <= W, halves every size when W = rc(W), applies the selection to the exact
// counts and adds to the pattern histogram (bit i: c_i >= present), the sums and -- when a list is wanted -- the list.  Pruning at the inner levels
// uses the lower bounds only (occ_i >= min_i for every i, and not all 0), side by side the argument of section 24.  Parts, split and order are
// kcount's and kcmp's.
// N is a template parameter of both kernels: the per-side state (4 child starts and 4 child sizes a side) is indexed by constants only and stays in
// registers, and a side that is not there is not compiled in, let alone fetched.
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include "fmd_prim.h"
#include "fmd_internal.h"
#include "fmd_kernel_common.h"
#include "fmd_ktrie.h"   // the frontier entry, its counters and kt_extend: shared with kcgraph

static_assert(sizeof(fmd_kmat_stat_t) == 176 && sizeof(fmd_kmat_sel_t) == 72 && FMD_KMAT_MAX_IDX == 8, "layout of include/fmd_hip.h");

#define KT_EMIT_BUF 128     // list entries staged per wave: one k-mer (u64) and N counts (u32) each; one child's at most 64 fit twice over
static_assert(FMD_KMAT_MIN_CAP >= 2 * KT_MIN_CHUNK, "the smallest capacity holds one wave's chunk tail and as much again");
static_assert(KT_WORDS <= 64 && KT_WORDS * 8 <= KT_HDR_BYTES, "k_kmat_init clears the counters with one wave");

template <int N> struct KtSel { uint64_t min[N], max[N], present; };                      // max: NONE64 = no upper bound

extern "C" size_t fmd_kmat_node_bytes(int n_idx) { return n_idx < 1 || n_idx > FMD_KMAT_MAX_IDX ? 0 : 16 * ((size_t)n_idx + 1); }

extern "C" size_t fmd_kmat_work_bytes(int n_idx, uint64_t cap)
{
    if (n_idx < 1 || n_idx > FMD_KMAT_MAX_IDX || cap < FMD_KMAT_MIN_CAP || cap > FMD_KMAT_MAX_CAP) return 0;
    return KT_HDR_BYTES + 256 + 2 * (size_t)cap * fmd_kmat_node_bytes(n_idx);
}

__global__ void k_kmat_init(unsigned long long *__restrict__ ctr, int root_len, unsigned long long n_roots)
{
    const int i = (int)threadIdx.x;
    if (blockIdx.x == 0 && i < KT_WORDS) ctr[i] = i == root_len ? n_roots : 0;
}

// one inner level: nodes at depth d -> the children at depth d + 1 that the pruning rule keeps
template <int N>
__global__ __launch_bounds__(64) void k_kmat_level(KtViews<N> v, int d, KtSel<N> sel, const KtNode<N> *__restrict__ in, KtNode<N> *__restrict__ out, uint64_t cap,
                                                   uint32_t ch, unsigned long long *__restrict__ ctr, int xcd_aware)
{
    FMD_DECLARE_WAVE_LDS();
    const int lane = fmd_lane();
    const uint64_t n_in = ctr[d] < cap ? ctr[d] : cap;   // an overflowing level counted more than it stored
    const KmRange rg = km_range(n_in, xcd_aware);
    const uint64_t stride = rg.stride;
    KmChunk ck; ck.base = 0; ck.fill = 0; ck.ch = ch; ck.have = false;
    uint32_t n_ext = 0;
    constexpr bool AHEAD = N < 8;                     // (eight sides: the 36 registers of a second entry would take the kernel past 256, to one wave per SIMD)
    uint4 nx[N + 1];                                  // the entry of the next iteration, loaded one gather ahead
    if (AHEAD) kt_load<N>(in, rg.beg + lane, rg.end, nx);
    for (uint64_t base = rg.beg; base < rg.end; base += stride) {
        uint64_t K, x0[N], sz[N];
        if (!AHEAD) kt_load<N>(in, base + lane, rg.end, nx);
        const bool act = kt_unpack<N>(nx, base + lane < rg.end, K, x0, sz);
        if (AHEAD) kt_load<N>(in, base + stride + lane, rg.end, nx);
        if (__ballot(act) == 0) continue;             // a run of holes
#pragma unroll
        for (int i = 0; i < N; ++i) n_ext += (uint32_t)__popcll(__ballot(act && sz[i] != 0));   // an empty side is never fetched again
        uint64_t tk[N][5], n[N][5];
        kt_extend<N>(v, fmd_lds, act, x0, sz, tk, n);
        bool has[5];
        uint32_t tot = 0;
#pragma unroll
        for (int c = 1; c <= 4; ++c) {                // (N is never followed)
            bool ok = act;
            uint64_t any = 0;
#pragma unroll
            for (int i = 0; i < N; ++i) { ok = ok && n[i][c] >= sel.min[i]; any |= n[i][c]; }
            has[c] = ok && any != 0;
            tot += (uint32_t)__popcll(__ballot(has[c]));
        }
        if (tot == 0) continue;
        unsigned long long o = km_reserve(out, cap, ck, tot, &ctr[d + 1]);
#pragma unroll
        for (int c = 1; c <= 4; ++c) {
            const uint64_t m = __ballot(has[c]);
            const unsigned long long at = o + fmd_below(m);
            if (has[c]) {
                if (at < cap) {
                    uint64_t w[2 * N];
#pragma unroll
                    for (int i = 0; i < N; ++i) { w[i] = n[i][c] ? v.ix[i].cnt[c] + tk[i][c] : 0; w[N + i] = n[i][c]; }
                    uint4 *q = (uint4 *)(out + at);
                    q[0] = ct_pack(K | (uint64_t)(c - 1) << (2 * d), 0);
#pragma unroll
                    for (int j = 0; j < N; ++j) q[1 + j] = ct_pack(w[2 * j], w[2 * j + 1]);
                } else ctr[KT_OVF] = 1;
            }
            o += __popcll(m);
        }
    }
    km_zero_fill(out, cap, ck);
    if (lane == 0 && n_ext) atomicAdd(&ctr[KT_EXT], (unsigned long long)n_ext);
}

// the staged entries -> the list (all 64 lanes together): ONE atomic for `fill` dense slots, stores of consecutive lanes side by side in every column
template <int N>
__device__ __forceinline__ void kt_flush_list(const uint64_t *ek, const uint32_t *ec, uint32_t &fill, unsigned long long *ctr, uint64_t *o_kmer, uint32_t *o_cnt,
                                              uint64_t out_cap)
{
    if (fill == 0) return;
    __syncthreads();                                  // the lanes that staged the entries are not the lanes that store them
    unsigned long long first = 0;
    if (fmd_lane() == 0) first = atomicAdd(&ctr[KT_OUT], (unsigned long long)fill);
    first = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(first >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)first);
    for (uint32_t j = (uint32_t)fmd_lane(); j < fill; j += 64)
        if (first + j < out_cap) {                    // (k_kmat_stat sets the flag: the counter went past out_cap)
            o_kmer[first + j] = ek[j];
#pragma unroll
            for (int i = 0; i < N; ++i) o_cnt[(uint64_t)i * out_cap + first + j] = ec[i * KT_EMIT_BUF + j];
        }
    __syncthreads();                                  // read before the next child stages over them
    fill = 0;
}

// the leaves: nodes at depth k - 1 -> the k-mers W = c . node, by their sizes in every index alone; the depth-k frontier is never stored.
// The pattern histogram (2^N cells) is private to the wave in LDS behind the two block slots and reaches the global one in one pass at the end.
// LIST: the reported ones leave as rc(W) and N saturated counts through KT_EMIT_BUF entries staged in LDS, one atomic per flush (kc_flush_pairs,
// fmd_kcount.hip); the spectrum's instance pays no LDS for it.
template <int N, bool LIST>
__global__ __launch_bounds__(64) void k_kmat_leaf(KtViews<N> v, int k, KtSel<N> sel, const KtNode<N> *__restrict__ in, uint64_t cap, unsigned long long *__restrict__ hist,
                                                  uint64_t *__restrict__ o_kmer, uint32_t *__restrict__ o_cnt, uint64_t out_cap, unsigned long long *__restrict__ ctr,
                                                  int xcd_aware)
{
    constexpr int CELLS = 1 << N, HIST_U4 = CELLS >= 4 ? CELLS / 4 : 1, EMIT_U4 = LIST ? KT_EMIT_BUF * (8 + 4 * N) / 16 : 0;
    __shared__ uint4 fmd_lds[FMD_WAVE_LDS_U4 + HIST_U4 + EMIT_U4];   // one array: the two block slots, the pattern cells, the staged entries
    uint32_t *bins = (uint32_t *)(fmd_lds + FMD_WAVE_LDS_U4);
    uint64_t *ek = (uint64_t *)(fmd_lds + FMD_WAVE_LDS_U4 + HIST_U4);
    uint32_t *ec = (uint32_t *)(ek + KT_EMIT_BUF);
    uint32_t fill = 0;                                // wave-uniform
    const int lane = fmd_lane();
    for (int j = lane; j < CELLS; j += 64) bins[j] = 0;
    __syncthreads();
    const uint64_t n_in = ctr[k - 1] < cap ? ctr[k - 1] : cap;
    const KmRange rg = km_range(n_in, xcd_aware);
    const uint64_t stride = rg.stride;
    uint32_t n_keep = 0, n_ext = 0;                   // wave-uniform
    uint64_t total[N];                                // per lane
    uint32_t pres[N];
#pragma unroll
    for (int i = 0; i < N; ++i) { total[i] = 0; pres[i] = 0; }
    uint4 nx[N + 1];                                  // the entry of the next iteration, loaded one gather ahead
    kt_load<N>(in, rg.beg + lane, rg.end, nx);
    for (uint64_t base = rg.beg; base < rg.end; base += stride) {
        uint64_t K, x0[N], sz[N];
        const bool act = kt_unpack<N>(nx, base + lane < rg.end, K, x0, sz);
        kt_load<N>(in, base + stride + lane, rg.end, nx);
        if (__ballot(act) == 0) continue;             // a run of holes
#pragma unroll
        for (int i = 0; i < N; ++i) n_ext += (uint32_t)__popcll(__ballot(act && sz[i] != 0));
        uint64_t tk[N][5], n[N][5];
        kt_extend<N>(v, fmd_lds, act, x0, sz, tk, n);
#pragma unroll
        for (int c = 1; c <= 4; ++c) {
            const uint64_t W = K | (uint64_t)(c - 1) << (2 * (k - 1));
            const uint64_t rc = kc_revcomp(W, k);
            const int half = rc == W ? 1 : 0;         // a k-mer that is its own reverse complement is seen twice per occurrence, in every index
            bool keep = act && rc <= W;
            uint64_t any = 0;
            uint32_t pat = 0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                n[i][c] >>= half;
                keep = keep && n[i][c] >= sel.min[i] && n[i][c] <= sel.max[i];
                any |= n[i][c];
                pat |= n[i][c] >= sel.present ? 1u << i : 0u;
            }
            keep = keep && any != 0;
            const uint64_t m = __ballot(keep);
            if (m == 0) continue;
            const uint32_t cnt = (uint32_t)__popcll(m);
            n_keep += cnt;
            if (keep) {
                atomicAdd(&bins[pat], 1u);
#pragma unroll
                for (int i = 0; i < N; ++i) { total[i] += n[i][c]; pres[i] += pat >> i & 1u; }
            }
            if (LIST) {
                if (fill + cnt > KT_EMIT_BUF) kt_flush_list<N>(ek, ec, fill, ctr, o_kmer, o_cnt, out_cap);
                if (keep) {
                    const uint32_t j = fill + (uint32_t)fmd_below(m);
                    ek[j] = rc;
#pragma unroll
                    for (int i = 0; i < N; ++i) ec[i * KT_EMIT_BUF + j] = n[i][c] > 0xffffffffull ? 0xffffffffu : (uint32_t)n[i][c];
                }
                fill += cnt;
            }
        }
    }
    if (LIST) kt_flush_list<N>(ek, ec, fill, ctr, o_kmer, o_cnt, out_cap);
    __syncthreads();
    for (int j = lane; j < CELLS; j += 64)
        if (bins[j]) atomicAdd(&hist[j], (unsigned long long)bins[j]);
    if (lane == 0 && n_ext) atomicAdd(&ctr[KT_EXT], (unsigned long long)n_ext);
    if (n_keep == 0) return;                          // (wave-uniform)
    if (lane == 0) atomicAdd(&ctr[KT_NKMER], (unsigned long long)n_keep);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint64_t t = km_wave_sum(total[i]), p = km_wave_sum((uint64_t)pres[i]);
        if (lane == 0 && t) atomicAdd(&ctr[KT_TOTAL + i], (unsigned long long)t);
        if (lane == 0 && p) atomicAdd(&ctr[KT_PRESENT + i], (unsigned long long)p);
    }
}

__global__ void k_kmat_stat(const unsigned long long *__restrict__ ctr, int root_len, int k, uint64_t out_cap, int listed, fmd_kmat_stat_t *__restrict__ stat)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    fmd_kmat_stat_t s;
    s.n_kmers = ctr[KT_NKMER];
    for (int i = 0; i < FMD_KMAT_MAX_IDX; ++i) { s.n_total[i] = ctr[KT_TOTAL + i]; s.n_present[i] = ctr[KT_PRESENT + i]; }
    s.n_ext = ctr[KT_EXT];
    s.overflow = (ctr[KT_OVF] != 0 || (listed && ctr[KT_OUT] > out_cap)) ? 1 : 0;
    s.widest_level = 0;
    for (int d = root_len; d < k; ++d) if (ctr[d] > s.widest_level) s.widest_level = ctr[d];
    s.n_parts = 1; s.n_retries = 0;
    *stat = s;
}

// dst[i] += src[i]: a part's histogram into the run's
__global__ void k_kmat_add(unsigned long long *__restrict__ dst, const unsigned long long *__restrict__ src, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (src[i]) dst[i] += src[i];
}

// slot[i] = i: what the sort of a part's k-mers carries along
__global__ void k_kmat_iota(uint32_t *__restrict__ slot, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) slot[i] = (uint32_t)i;
}

// the sorted (k-mer, slot) pairs -> the n_idx count columns in the order of the k-mers (columns out_cap entries apart on both sides)
__global__ void k_kmat_gather(const uint32_t *__restrict__ slot, const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, uint64_t n, uint64_t out_cap, int n_idx)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t s = slot[i];
        for (int c = 0; c < n_idx; ++c) dst[(uint64_t)c * out_cap + i] = src[(uint64_t)c * out_cap + s];
    }
}

// Grids and chunk for a capacity (kp_plan, fmd_kcmp.hip): a grid is at most the kernel's resident set, the chunk tails of a level take at most
// half of the capacity, the leaves run on no more waves than the levels.
template <int N>
static void kt_plan(fmd_dev_t *h, uint64_t cap, bool listed, int &grid, int &leaf_grid, uint32_t &ch)
{
    static int per_cu[3] = {0, 0, 0};
    const size_t leaf_lds = (FMD_WAVE_LDS_U4 + ((1 << N) >= 4 ? (1 << N) / 4 : 1)) * 16;
    if (!per_cu[0]) {
        per_cu[1] = fmd_resident_per_cu(k_kmat_leaf<N, false>, leaf_lds, 16, "k_kmat_leaf<N, false>");
        per_cu[2] = fmd_resident_per_cu(k_kmat_leaf<N, true>, leaf_lds + KT_EMIT_BUF * (8 + 4 * N), 16, "k_kmat_leaf<N, true>");
        per_cu[0] = fmd_resident_per_cu(k_kmat_level<N>, FMD_WAVE_LDS_U4 * 16, 16, "k_kmat_level<N>");
    }
    grid = fmd_grid_for_lds(h, cap, FMD_WAVE_LDS_U4 * 16);
    if (grid > h->n_cu * per_cu[0]) grid = h->n_cu * per_cu[0];
    ch = 1024;
    while (ch > KT_MIN_CHUNK && (uint64_t)grid * ch * 8 > cap) ch >>= 1;
    const uint64_t g = cap / (2 * (uint64_t)ch);
    if ((uint64_t)grid > g) grid = (int)g;
    if (grid >= 8) grid &= ~7;                        // (a multiple of 8: km_range gives every XCD its eighth)
    if (grid < 1) grid = 1;
    leaf_grid = h->n_cu * per_cu[listed ? 2 : 1];
    if (leaf_grid > grid) leaf_grid = grid;
    if (leaf_grid >= 8) leaf_grid &= ~7;
    if (leaf_grid < 1) leaf_grid = 1;
}

// the kernels of one part, for N indexes
template <int N>
static void kt_enqueue(fmd_dev_t *const *h, hipStream_t st, int k, const fmd_kmat_sel_t *sel, int root_len, size_t n_roots, const void *d_roots, uint64_t cap,
                       uint64_t *d_hist, uint64_t *d_kmer, uint32_t *d_count, uint64_t out_cap, fmd_kmat_stat_t *d_stat, unsigned long long *ctr, void *frontiers)
{
    KtViews<N> v;
    KtSel<N> s;
    for (int i = 0; i < N; ++i) {
        v.ix[i] = fmd_view(h[i]);
        s.min[i] = sel->min[i]; s.max[i] = sel->max[i] == FMD_KMAT_NO_MAX ? NONE64 : sel->max[i];
    }
    s.present = sel->present;
    KtNode<N> *f[2];
    f[0] = (KtNode<N> *)frontiers; f[1] = f[0] + cap;
    int grid, leaf_grid; uint32_t ch;
    kt_plan<N>(h[0], cap, d_kmer != nullptr, grid, leaf_grid, ch);
    k_kmat_init<<<1, 64, 0, st>>>(ctr, root_len, (unsigned long long)n_roots);
    const KtNode<N> *in = (const KtNode<N> *)d_roots;
    for (int d = root_len; d < k - 1; ++d) {
        KtNode<N> *out = f[(d - root_len) & 1];
        k_kmat_level<N><<<grid, 64, 0, st>>>(v, d, s, in, out, cap, ch, ctr, 1);
        in = out;
    }
    if (d_kmer) k_kmat_leaf<N, true><<<leaf_grid, 64, 0, st>>>(v, k, s, in, cap, (unsigned long long *)d_hist, d_kmer, d_count, out_cap, ctr, 1);
    else k_kmat_leaf<N, false><<<leaf_grid, 64, 0, st>>>(v, k, s, in, cap, (unsigned long long *)d_hist, nullptr, nullptr, 0, ctr, 1);
    k_kmat_stat<<<1, 64, 0, st>>>(ctr, root_len, k, out_cap, d_kmer != nullptr, d_stat);
}

// a necessary sign of an index of both strands (fmd_kcount); an empty index passes
static bool kt_both_strands(const fmd_dev_t *h) { return h->mcnt[2] == h->mcnt[5] && h->mcnt[3] == h->mcnt[4] && !(h->mcnt[1] & 1); }

static int kt_args(int n_idx, fmd_dev_t *const *h, int k, int k_min, const fmd_kmat_sel_t *sel)
{
    if (n_idx < 1 || n_idx > FMD_KMAT_MAX_IDX || !h || !sel || k < k_min || k > 32 || sel->present < 1) return FMD_E_ARG;
    for (int i = 0; i < n_idx; ++i) {
        if (!h[i] || h[i]->device != h[0]->device || sel->min[i] > sel->max[i]) return FMD_E_ARG;
        if (!kt_both_strands(h[i])) return FMD_E_ARG;
    }
    return FMD_OK;
}

extern "C" int fmd_kmat_part_dev(int n_idx, fmd_dev_t *const *h, void *stream, int k, const fmd_kmat_sel_t *sel, int root_len, size_t n_roots, const void *d_roots,
                                 uint64_t cap, uint64_t *d_hist, uint64_t *d_kmer, uint32_t *d_count, uint64_t out_cap, fmd_kmat_stat_t *d_stat, void *d_work,
                                 size_t work_bytes)
{
    FMD_TRY(kt_args(n_idx, h, k, 2, sel));
    if (!d_hist || !d_stat || !d_work || (n_roots && !d_roots) || (d_kmer && !d_count) || root_len < 1 || root_len >= k) return FMD_E_ARG;
    const size_t wb = fmd_kmat_work_bytes(n_idx, cap);
    if (wb == 0 || work_bytes < wb || n_roots > cap || ((uintptr_t)d_work & 15) || ((uintptr_t)d_roots & 15)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h[0]->device));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *ctr = (unsigned long long *)d_work;
    void *fr = (void *)(((uintptr_t)((uint8_t *)d_work + KT_HDR_BYTES) + 255) & ~(uintptr_t)255);
    switch (n_idx) {
#define KT_CASE(N) case N: kt_enqueue<N>(h, st, k, sel, root_len, n_roots, d_roots, cap, d_hist, d_kmer, d_count, out_cap, d_stat, ctr, fr); break;
        KT_CASE(1) KT_CASE(2) KT_CASE(3) KT_CASE(4) KT_CASE(5) KT_CASE(6) KT_CASE(7) KT_CASE(8)
#undef KT_CASE
    }
    FMD_CHECK_LAUNCH("kmat kernels");
    return FMD_OK;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct KtRoot { uint64_t kmer, x0[FMD_KMAT_MAX_IDX], size[FMD_KMAT_MAX_IDX]; int len; };
typedef std::vector<KtRoot> KtRun;                    // roots of one length, rc(suffix) ascending

static bool kt_pruned(int n_idx, const KtRoot &r, const fmd_kmat_sel_t &sel)
{
    uint64_t any = 0;
    for (int i = 0; i < n_idx; ++i) { if (r.size[i] < sel.min[i]) return true; any |= r.size[i]; }
    return any == 0;
}

// a root as the frontier entry of n_idx indexes: 2 (n_idx + 1) words
static void kt_entry(int n_idx, const KtRoot &r, uint64_t *w)
{
    w[0] = r.kmer; w[1] = 0;
    for (int i = 0; i < n_idx; ++i) { w[2 + i] = r.x0[i]; w[2 + n_idx + i] = r.size[i]; }
}

// What a run of parts keeps, sized by the capacity (KpBufs, fmd_kcmp.hip): the large buffers from h[0]'s scratch cache, the list out through pinned
// slices of KT_SLICE entries.  hist[0] = the run's histogram, hist[1] = the part's; cnt[0] = the columns as the leaves left them, cnt[1] = in the
// order of the sorted k-mers.
#define KT_SLICE (1u << 20)
struct KtBufs {
    uint64_t cap = 0, out_cap = 0;
    size_t wb = 0, tmp_bytes = 0;
    FmdScratch work, kmer[2], slot[2], cnt[2], tmp;
    FmdDevBuf roots, hist[2], stat;
    FmdHostBuf h_kmer, h_cnt;
    int alloc(int n_idx, fmd_dev_t *h, uint64_t cap_, bool listed, int k)
    {
        cap = cap_; out_cap = listed ? cap_ : 0; wb = fmd_kmat_work_bytes(n_idx, cap_);
        work.reset(); tmp.reset();
        for (int i = 0; i < 2; ++i) { kmer[i].reset(); slot[i].reset(); cnt[i].reset(); }
        FMD_TRY(work.alloc(h, wb)); FMD_TRY(roots.need(4 * fmd_kmat_node_bytes(n_idx))); FMD_TRY(stat.need(sizeof(fmd_kmat_stat_t)));
        for (int i = 0; i < 2; ++i) FMD_TRY(hist[i].need(((size_t)1 << n_idx) * 8));
        if (!listed) return FMD_OK;
        for (int i = 0; i < 2; ++i) { FMD_TRY(kmer[i].alloc(h, out_cap * 8)); FMD_TRY(slot[i].alloc(h, out_cap * 4)); FMD_TRY(cnt[i].alloc(h, out_cap * 4 * n_idx)); }
        tmp_bytes = 0;
        FMD_HIP_TRY(fmd_sort_pairs(nullptr, tmp_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)out_cap, 0, 2 * k));
        FMD_TRY(tmp.alloc(h, tmp_bytes ? tmp_bytes : 16));
        FMD_TRY(h_kmer.need((size_t)KT_SLICE * 8));
        return h_cnt.need((size_t)KT_SLICE * 4 * n_idx);
    }
};

// every k-mer of one base: the marginal counts, no kernel
static int kt_single_bases(int n_idx, fmd_dev_t *const *h, const fmd_kmat_sel_t &sel, uint64_t *hist, fmd_kmat_sink_fn sink, void *ctx, fmd_kmat_stat_t *stat)
{
    uint64_t kmer[2]; uint32_t cnt[FMD_KMAT_MAX_IDX][2]; const uint32_t *col[FMD_KMAT_MAX_IDX]; uint64_t n = 0;
    for (int c = 0; c < 2; ++c) {                     // A (= T on the other strand) and C (= G)
        bool keep = true; uint64_t any = 0; uint32_t pat = 0;
        for (int i = 0; i < n_idx; ++i) {
            const uint64_t v = h[i]->mcnt[2 + c];
            if (v < sel.min[i] || (sel.max[i] != FMD_KMAT_NO_MAX && v > sel.max[i])) keep = false;
            any |= v;
            if (v >= sel.present) pat |= 1u << i;
        }
        if (!keep || any == 0) continue;
        kmer[n] = (uint64_t)c;
        for (int i = 0; i < n_idx; ++i) {
            const uint64_t v = h[i]->mcnt[2 + c];
            cnt[i][n] = v > 0xffffffffull ? 0xffffffffu : (uint32_t)v;
            stat->n_total[i] += v;
            if (pat >> i & 1) ++stat->n_present[i];
        }
        ++n; ++hist[pat]; ++stat->n_kmers;
    }
    for (int i = 0; i < n_idx; ++i) col[i] = cnt[i];
    if (sink && n && sink(ctx, n, kmer, col)) return FMD_E_IO;
    return FMD_OK;
}

static int kt_run(int n_idx, fmd_dev_t *const *h, int k, const fmd_kmat_sel_t *sel, uint64_t *hist, uint64_t cap, fmd_kmat_sink_fn sink, void *ctx, fmd_kmat_stat_t *stat);
extern "C" int fmd_kmat(int n_idx, fmd_dev_t *const *h, int k, const fmd_kmat_sel_t *sel, uint64_t *hist, uint64_t cap, fmd_kmat_sink_fn sink, void *ctx,
                        fmd_kmat_stat_t *stat)
{
    try { return kt_run(n_idx, h, k, sel, hist, cap, sink, ctx, stat); }
    catch (const std::bad_alloc &) { return FMD_E_NOMEM; }   // (the host vectors)
}
static int kt_run(int n_idx, fmd_dev_t *const *h, int k, const fmd_kmat_sel_t *sel, uint64_t *hist, uint64_t cap, fmd_kmat_sink_fn sink, void *ctx, fmd_kmat_stat_t *stat)
{
    FMD_TRY(kt_args(n_idx, h, k, 1, sel));
    if (!hist || !stat) return FMD_E_ARG;
    if (cap && (cap < FMD_KMAT_MIN_CAP || cap > FMD_KMAT_MAX_CAP)) return FMD_E_ARG;
    const size_t n_cells = (size_t)1 << n_idx, nb = fmd_kmat_node_bytes(n_idx);
    memset(stat, 0, sizeof(*stat));
    memset(hist, 0, n_cells * 8);
    if (k == 1) return kt_single_bases(n_idx, h, *sel, hist, sink, ctx, stat);
    FMD_HIP_TRY(hipSetDevice(h[0]->device));
    const bool listed = sink != nullptr;
    // capacity: the caller's, or -- cap = 0 -- half the symbols of the distinct indexes to start with, doubled after an overflow as long as it fits beside
    // them (a level never holds more live entries than the indexes have symbols, and the chunk tails take at most as much again)
    uint64_t n_sym = 0;
    for (int i = 0; i < n_idx; ++i) {
        bool seen = false;
        for (int j = 0; j < i; ++j) seen = seen || h[j] == h[i];
        if (!seen) n_sym += h[i]->mcnt[0];
    }
    uint64_t cap_max = cap;
    if (cap == 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)8 << 30;
        const uint64_t per = 2 * nb + (listed ? 2 * (8 + 4 + 4 * (uint64_t)n_idx) + 8 : 0);
        cap_max = (uint64_t)(0.7 * (double)free_b) / per;
        if (cap_max > 2 * n_sym + FMD_KMAT_MIN_CAP) cap_max = 2 * n_sym + FMD_KMAT_MIN_CAP;
        if (cap_max > FMD_KMAT_MAX_CAP) cap_max = FMD_KMAT_MAX_CAP;
        if (cap_max < FMD_KMAT_MIN_CAP) cap_max = FMD_KMAT_MIN_CAP;
        cap = n_sym / 2 + (1u << 16);
        if (cap > cap_max) cap = cap_max;
    }
    KtBufs b;
    for (;;) {                                        // (what hipMemGetInfo calls free is not always one piece)
        const int rc = b.alloc(n_idx, h[0], cap, listed, k);
        if (rc == FMD_OK) break;
        if (rc != FMD_E_NOMEM || cap_max == cap || cap / 2 < FMD_KMAT_MIN_CAP) return rc;
        cap /= 2; cap_max = cap;
    }
    FMD_HIP_TRY(hipMemsetAsync(b.hist[0].p, 0, n_cells * 8, nullptr));
    std::vector<KtRun> todo;                          // the back is next
    {
        KtRun first;
        for (int c = 4; c >= 1; --c) {                // suffix T, G, C, A: rc(suffix) = A, C, G, T
            KtRoot r;
            memset(&r, 0, sizeof(r));
            for (int i = 0; i < n_idx; ++i) {
                r.size[i] = h[i]->cnt[c + 1] - h[i]->cnt[c];
                r.x0[i] = r.size[i] ? h[i]->cnt[c] : 0;
            }
            r.kmer = (uint64_t)(c - 1); r.len = 1;
            if (!kt_pruned(n_idx, r, *sel)) first.push_back(r);
        }
        todo.push_back(first);
    }
    const uint32_t *col[FMD_KMAT_MAX_IDX];
    while (!todo.empty()) {
        KtRun run = todo.back(); todo.pop_back();
        if (run.empty()) continue;
        uint64_t roots[4 * 2 * (FMD_KMAT_MAX_IDX + 1)];
        for (size_t i = 0; i < run.size(); ++i) kt_entry(n_idx, run[i], roots + i * (nb / 8));
        fmd_kmat_stat_t ps;
        FMD_HIP_TRY(hipMemcpy(b.roots.p, roots, run.size() * nb, hipMemcpyHostToDevice));
        FMD_HIP_TRY(hipMemsetAsync(b.hist[1].p, 0, n_cells * 8, nullptr));
        FMD_TRY(fmd_kmat_part_dev(n_idx, h, nullptr, k, sel, run[0].len, run.size(), b.roots.p, b.cap, b.hist[1].as<uint64_t>(),
                                  listed ? b.kmer[0].as<uint64_t>() : nullptr, listed ? b.cnt[0].as<uint32_t>() : nullptr, b.out_cap, b.stat.as<fmd_kmat_stat_t>(),
                                  b.work.p, b.wb));
        FMD_HIP_TRY(hipMemcpy(&ps, b.stat.p, sizeof(ps), hipMemcpyDeviceToHost));
        ++stat->n_parts;
        stat->n_ext += ps.n_ext;                      // (the work of a discarded part was done all the same)
        if (ps.widest_level > stat->widest_level) stat->widest_level = ps.widest_level;
        if (ps.overflow) {                            // discarded whole
            ++stat->n_retries;
            if (b.cap < cap_max) {                    // there is room: the same run again in twice the capacity
                const uint64_t c2 = 2 * b.cap < cap_max ? 2 * b.cap : cap_max;
                if (b.alloc(n_idx, h[0], c2, listed, k) == FMD_OK) { cap = c2; todo.push_back(run); continue; }
                cap_max = cap;                        // it does not fit after all: back to what did, and cut the run
                FMD_TRY(b.alloc(n_idx, h[0], cap, listed, k));
            }
            if (run.size() > 1) {
                const size_t half = run.size() / 2;
                todo.push_back(KtRun(run.begin() + half, run.end()));
                todo.push_back(KtRun(run.begin(), run.begin() + half));
            } else {
                if (run[0].len >= k - 1) return FMD_E_OVERFLOW;   // (a single leaf root emits four entries at most: cannot happen)
                fmd_intv_t ok[FMD_KMAT_MAX_IDX][6];
                memset(ok, 0, sizeof(ok));
                const uint8_t back = 1;
                for (int i = 0; i < n_idx; ++i) {     // (only x[0] and the size of a child are used: x[1] of the root is not kept)
                    if (run[0].size[i] == 0) continue;
                    fmd_intv_t ik;
                    ik.x[0] = run[0].x0[i]; ik.x[1] = 0; ik.x[2] = run[0].size[i]; ik.info = 0;
                    FMD_TRY(fmd_extend_batch(h[i], 1, &ik, &back, ok[i]));
                }
                KtRun kids;
                for (int c = 4; c >= 1; --c) {        // c . suffix: rc = rc(suffix) . comp(c), ascending in comp(c)
                    KtRoot r;
                    memset(&r, 0, sizeof(r));
                    for (int i = 0; i < n_idx; ++i) { r.size[i] = ok[i][c].x[2]; r.x0[i] = r.size[i] ? ok[i][c].x[0] : 0; }
                    r.kmer = run[0].kmer | (uint64_t)(c - 1) << (2 * run[0].len); r.len = run[0].len + 1;
                    if (!kt_pruned(n_idx, r, *sel)) kids.push_back(r);
                }
                todo.push_back(kids);
            }
            continue;
        }
        k_kmat_add<<<1, 256, 0, nullptr>>>(b.hist[0].as<unsigned long long>(), b.hist[1].as<unsigned long long>(), (uint64_t)n_cells);
        FMD_CHECK_LAUNCH("k_kmat_add");
        stat->n_kmers += ps.n_kmers;
        for (int i = 0; i < n_idx; ++i) { stat->n_total[i] += ps.n_total[i]; stat->n_present[i] += ps.n_present[i]; }
        if (listed && ps.n_kmers) {
            const uint64_t n = ps.n_kmers;
            const unsigned g = fmd_nblk(n, 256) < 4096 ? fmd_nblk(n, 256) : 4096;
            size_t tb = b.tmp_bytes;
            k_kmat_iota<<<g, 256, 0, nullptr>>>(b.slot[0].as<uint32_t>(), n);
            FMD_HIP_TRY(fmd_sort_pairs(b.tmp.p, tb, b.kmer[0].as<uint64_t>(), b.kmer[1].as<uint64_t>(), b.slot[0].as<uint32_t>(), b.slot[1].as<uint32_t>(), (size_t)n, 0, 2 * k));
            k_kmat_gather<<<g, 256, 0, nullptr>>>(b.slot[1].as<uint32_t>(), b.cnt[0].as<uint32_t>(), b.cnt[1].as<uint32_t>(), n, b.out_cap, n_idx);
            FMD_CHECK_LAUNCH("k_kmat_gather");
            for (uint64_t at = 0; at < n; at += KT_SLICE) {
                const uint64_t m = n - at < KT_SLICE ? n - at : KT_SLICE;
                FMD_HIP_TRY(hipMemcpy(b.h_kmer.p, b.kmer[1].as<uint64_t>() + at, m * 8, hipMemcpyDeviceToHost));
                for (int i = 0; i < n_idx; ++i) {
                    FMD_HIP_TRY(hipMemcpy(b.h_cnt.as<uint32_t>() + (size_t)i * KT_SLICE, b.cnt[1].as<uint32_t>() + (uint64_t)i * b.out_cap + at, m * 4, hipMemcpyDeviceToHost));
                    col[i] = b.h_cnt.as<uint32_t>() + (size_t)i * KT_SLICE;
                }
                if (sink(ctx, m, b.h_kmer.as<uint64_t>(), col)) return FMD_E_IO;
            }
        }
    }
    FMD_HIP_TRY(hipMemcpy(hist, b.hist[0].p, n_cells * 8, hipMemcpyDeviceToHost));
    return FMD_OK;
}
