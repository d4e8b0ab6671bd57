// fmd_kcmp.hip -- kcmp: the joint k-mer counts of two indexes of both strands.
//
// kcount (fmd_kcount.hip) walks the trie of the k-mers of ONE index and counts at the leaves; contrast (fmd_contrast.hip) walks the tries of TWO
// indexes together and keeps read bitmaps.  This is both at once: a node is one suffix's interval (start, size) in EACH index plus the packed
// suffix; a level gives every node one backward extension per non-empty side, the two rank blocks in flight together (k_ct_level's order); the
// leaf kernel runs on the frontier at depth k - 1, takes the child SIZES in both indexes, keeps W iff rc(W) <= W, halves both sizes when
// W = rc(W), applies the selection to the pair (c0, c1) and adds to the 2-D histogram, the sums and -- when a list is wanted -- the list.
// Pruning at the inner levels uses the lower bounds only (occ0 >= min0 and occ1 >= min1 and not both 0): occ shrinks as a k-mer grows and a
// palindrome's occ is at least its count, so nothing that the leaf would report is lost.  Parts, split and order are kcount's: a run of roots
// walked inside a fixed capacity, discarded whole and cut when it overflows, taken in the order of rc(suffix) so that the sorted lists of the
// parts are ascending over the whole run.
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include "fmd_prim.h"
#include "fmd_internal.h"
#include "fmd_kernel_common.h"
#include "fmd_level.h"
#include "fmd_twoside.h"

static_assert(sizeof(fmd_kcmp_stat_t) == 88 && sizeof(fmd_kcmp_node_t) == 48 && sizeof(fmd_kcmp_sel_t) == 16, "layout of include/fmd_hip.h");

// counters at the head of the work area (u64 words): [d] = the entries of the frontier at depth d (d = root_len .. k - 1 <= 31), then
#define KP_OUT 40        // list entries emitted (counts on when the list is full)
#define KP_OVF 41        // a frontier entry did not fit
#define KP_NKMER 42      // k-mers reported
#define KP_TOTAL0 43     // the sums of their counts
#define KP_TOTAL1 44
#define KP_ONLY0 45      // those with c1 = 0 / with c0 = 0
#define KP_ONLY1 46
#define KP_EXT 47        // backward extensions done: one per (node, non-empty side)
#define KP_WORDS 48
#define KP_HDR_BYTES 512
// the cells of the histogram with both coordinates below KP_LB live in the wave's LDS behind the two block slots (KP_LB x KP_LB x u32) and reach the
// global histogram in one pass at the end: with n_bins = 2 every k-mer lands in three cells, and 2 x 10^7 atomics on one global word took 0.22 s (section 21)
#define KP_LB 16
#define KP_LDS_U4 (FMD_WAVE_LDS_U4 + KP_LB * KP_LB / 4)
#define KP_EMIT_BUF 256     // list entries staged per wave, (u64 k-mer, u64 c0 | c1 << 32) in two arrays: one step's at most (4 x 64)
#define KP_EMIT_U4 (KP_EMIT_BUF * 16 / 16)
#define KP_MIN_CHUNK 256u   // one step's children (4 x 64) fit one chunk
static_assert(FMD_KCMP_MIN_CAP >= 2 * KP_MIN_CHUNK, "the smallest capacity holds one wave's chunk tail and as much again");

extern "C" size_t fmd_kcmp_work_bytes(uint64_t cap)
{
    if (cap < FMD_KCMP_MIN_CAP || cap > FMD_KCMP_MAX_CAP) return 0;
    return KP_HDR_BYTES + 256 + 2 * (size_t)cap * sizeof(fmd_kcmp_node_t);
}

__global__ void k_kcmp_init(unsigned long long *__restrict__ ctr, int root_len, unsigned long long n_roots)
{
    const int i = (int)threadIdx.x;
    if (blockIdx.x == 0 && i < KP_WORDS) ctr[i] = i == root_len ? n_roots : 0;
}

// One backward extension per lane in each index whose side is live -> the ranks before the interval (tka, tkb) and the child sizes (na, nb; 0 on a
// side that is not live).  Both indexes' blocks in flight together: the k sides, then (where an interval does not end inside that block) the l sides.
__device__ __forceinline__ void kp_extend(const FmdIndexView &a, const FmdIndexView &b, uint4 *lds, bool acta, uint64_t x0a, uint64_t sza, bool actb,
                                          uint64_t x0b, uint64_t szb, uint64_t tka[6], uint64_t tkb[6], uint64_t na[5], uint64_t nb[5])
{
    const CtSide A = ct_side(acta, x0a, sza), B = ct_side(actb, x0b, szb);
    uint64_t tla[6], tlb[6];
    fmd_fetch_slot<0>(a, lds, A.bk, A.hk);
    fmd_fetch_slot<1>(b, lds, B.bk, B.hk);
    fmd_fetch_wait();
    ct_ranks_k<0>(lds, A, tka, tla);
    ct_ranks_k<1>(lds, B, tkb, tlb);
    if (__ballot(A.lsep || B.lsep)) {
        __syncthreads();                              // (one wave: a wait) the k-side LDS reads have returned before the slots are written again
        fmd_fetch_slot<0>(a, lds, A.bl, A.lsep);
        fmd_fetch_slot<1>(b, lds, B.bl, B.lsep);
        fmd_fetch_wait();
        ct_ranks_l<0>(lds, A, tla);
        ct_ranks_l<1>(lds, B, tlb);
    }
#pragma unroll
    for (int c = 1; c <= 4; ++c) { na[c] = tla[c] - tka[c]; nb[c] = tlb[c] - tkb[c]; }
}

// a frontier entry as three 16-byte words, and back
struct KpNode { uint64_t x0a, x0b, sza, szb, K; };
__device__ __forceinline__ KpNode kp_unpack(const uint4 &e0, const uint4 &e1, const uint4 &e2)
{
    KpNode n;
    n.x0a = (uint64_t)e0.y << 32 | e0.x; n.x0b = (uint64_t)e0.w << 32 | e0.z;
    n.sza = (uint64_t)e1.y << 32 | e1.x; n.szb = (uint64_t)e1.w << 32 | e1.z;
    n.K = (uint64_t)e2.y << 32 | e2.x;
    return n;
}
__device__ __forceinline__ void kp_load(const fmd_kcmp_node_t *in, uint64_t i, uint64_t end, uint4 &e0, uint4 &e1, uint4 &e2)
{
    e0 = make_uint4(0, 0, 0, 0); e1 = e0; e2 = e0;
    if (i < end) { const uint4 *q = (const uint4 *)(in + i); e0 = q[0]; e1 = q[1]; e2 = q[2]; }
}

// one inner level: pair nodes at depth d -> the children at depth d + 1 that the pruning rule keeps
__global__ __launch_bounds__(64) void k_kcmp_level(FmdIndexView a, FmdIndexView b, int d, uint64_t min0, uint64_t min1, const fmd_kcmp_node_t *__restrict__ in,
                                                   fmd_kcmp_node_t *__restrict__ out, uint64_t cap, uint32_t ch, unsigned long long *__restrict__ ctr, int xcd_aware)
{
    FMD_DECLARE_WAVE_LDS();
    const int lane = fmd_lane();
    const uint64_t n = ctr[d] < cap ? ctr[d] : cap;   // an overflowing level counted more than it stored
    const KmRange rg = km_range(n, xcd_aware);
    const uint64_t stride = rg.stride;
    KmChunk ck; ck.base = 0; ck.fill = 0; ck.ch = ch; ck.have = false;
    uint32_t n_ext = 0;
    uint4 n0, n1, n2;                                 // the entry of the next iteration, loaded one gather ahead
    kp_load(in, rg.beg + lane, rg.end, n0, n1, n2);
    for (uint64_t base = rg.beg; base < rg.end; base += stride) {
        const KpNode nd = kp_unpack(n0, n1, n2);
        const bool act = base + lane < rg.end && (nd.sza | nd.szb) != 0;
        kp_load(in, base + stride + lane, rg.end, n0, n1, n2);
        if (__ballot(act) == 0) continue;             // a run of holes
        const bool acta = act && nd.sza != 0, actb = act && nd.szb != 0;   // an empty side is never fetched again
        n_ext += (uint32_t)(__popcll(__ballot(acta)) + __popcll(__ballot(actb)));
        uint64_t tka[6], tkb[6], na[5], nb[5];
        kp_extend(a, b, fmd_lds, acta, nd.x0a, nd.sza, actb, nd.x0b, nd.szb, tka, tkb, na, nb);
        bool has[5];
        uint32_t tot = 0;
#pragma unroll
        for (int c = 1; c <= 4; ++c) {                // (N is never followed)
            has[c] = act && na[c] >= min0 && nb[c] >= min1 && (na[c] | nb[c]) != 0;
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
                    uint4 *q = (uint4 *)(out + at);
                    q[0] = ct_pack(na[c] ? a.cnt[c] + tka[c] : 0, nb[c] ? b.cnt[c] + tkb[c] : 0);
                    q[1] = ct_pack(na[c], nb[c]);
                    q[2] = ct_pack(nd.K | (uint64_t)(c - 1) << (2 * d), 0);
                } else ctr[KP_OVF] = 1;
            }
            o += __popcll(m);
        }
    }
    km_zero_fill(out, cap, ck);
    if (lane == 0 && n_ext) atomicAdd(&ctr[KP_EXT], (unsigned long long)n_ext);
}

// the staged entries -> the list (all 64 lanes together): ONE atomic for `fill` dense slots, stores of consecutive lanes side by side
__device__ __forceinline__ void kp_flush_list(const uint64_t *ek, const uint64_t *ec, uint32_t &fill, unsigned long long *ctr, uint64_t *o_kmer, uint64_t *o_c01,
                                              uint64_t out_cap)
{
    if (fill == 0) return;
    __syncthreads();                                  // the lanes that staged the entries are not the lanes that store them
    unsigned long long first = 0;
    if (fmd_lane() == 0) first = atomicAdd(&ctr[KP_OUT], (unsigned long long)fill);
    first = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(first >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)first);
    for (uint32_t j = (uint32_t)fmd_lane(); j < fill; j += 64)
        if (first + j < out_cap) { o_kmer[first + j] = ek[j]; o_c01[first + j] = ec[j]; }   // (k_kcmp_stat sets the flag: the counter went past out_cap)
    __syncthreads();                                  // read before the next step stages over them
    fill = 0;
}

// the leaves: pair nodes at depth k - 1 -> the k-mers W = c . node, by their sizes in both indexes alone; the depth-k frontier is never stored.
// LIST: the reported ones leave as (rc(W), c0 | c1 << 32) through KP_EMIT_BUF entries staged in LDS, one atomic per flush (kc_flush_pairs, fmd_kcount.hip);
// the spectrum's instance pays no LDS for it.
template <bool LIST>
__global__ __launch_bounds__(64) void k_kcmp_leaf(FmdIndexView a, FmdIndexView b, int k, fmd_kcmp_sel_t sel, const fmd_kcmp_node_t *__restrict__ in, uint64_t cap,
                                                  uint32_t n_bins, unsigned long long *__restrict__ hist, uint64_t *__restrict__ o_kmer, uint64_t *__restrict__ o_c01,
                                                  uint64_t out_cap, unsigned long long *__restrict__ ctr, int xcd_aware)
{
    __shared__ uint4 fmd_lds[KP_LDS_U4 + (LIST ? KP_EMIT_U4 : 0)];   // one array: the two block slots, the low cells, the staged entries
    uint32_t *bins = (uint32_t *)(fmd_lds + FMD_WAVE_LDS_U4);
    uint64_t *ek = (uint64_t *)(fmd_lds + KP_LDS_U4);
    uint64_t *ec = ek + KP_EMIT_BUF;
    uint32_t fill = 0;                                // wave-uniform
    const int lane = fmd_lane();
    const uint64_t last = n_bins - 1;                 // the coordinate of `last` and more
    const uint64_t max0 = sel.max0 == FMD_KCMP_NO_MAX ? NONE64 : sel.max0, max1 = sel.max1 == FMD_KCMP_NO_MAX ? NONE64 : sel.max1;
    for (int j = lane; j < KP_LB * KP_LB; j += 64) bins[j] = 0;
    __syncthreads();
    const uint64_t n = ctr[k - 1] < cap ? ctr[k - 1] : cap;
    const KmRange rg = km_range(n, xcd_aware);
    const uint64_t stride = rg.stride;
    uint32_t n_keep = 0, n_only0 = 0, n_only1 = 0, n_ext = 0;   // wave-uniform
    uint64_t total0 = 0, total1 = 0;                  // per lane
    uint4 n0, n1, n2;                                 // the entry of the next iteration, loaded one gather ahead
    kp_load(in, rg.beg + lane, rg.end, n0, n1, n2);
    for (uint64_t base = rg.beg; base < rg.end; base += stride) {
        const KpNode nd = kp_unpack(n0, n1, n2);
        const bool act = base + lane < rg.end && (nd.sza | nd.szb) != 0;
        kp_load(in, base + stride + lane, rg.end, n0, n1, n2);
        if (__ballot(act) == 0) continue;             // a run of holes
        const bool acta = act && nd.sza != 0, actb = act && nd.szb != 0;
        n_ext += (uint32_t)(__popcll(__ballot(acta)) + __popcll(__ballot(actb)));
        uint64_t tka[6], tkb[6], na[5], nb[5];
        kp_extend(a, b, fmd_lds, acta, nd.x0a, nd.sza, actb, nd.x0b, nd.szb, tka, tkb, na, nb);
        uint64_t rc[5], m[5];
        bool keep[5];
        uint32_t tot = 0;
#pragma unroll
        for (int c = 1; c <= 4; ++c) {
            const uint64_t W = nd.K | (uint64_t)(c - 1) << (2 * (k - 1));
            rc[c] = kc_revcomp(W, k);
            if (rc[c] == W) { na[c] >>= 1; nb[c] >>= 1; }   // a k-mer that is its own reverse complement is seen twice per occurrence, in each index
            keep[c] = act && rc[c] <= W && (na[c] | nb[c]) != 0 && na[c] >= sel.min0 && na[c] <= max0 && nb[c] >= sel.min1 && nb[c] <= max1;
            m[c] = __ballot(keep[c]);
            tot += (uint32_t)__popcll(m[c]);
            n_only0 += (uint32_t)__popcll(__ballot(keep[c] && nb[c] == 0));
            n_only1 += (uint32_t)__popcll(__ballot(keep[c] && na[c] == 0));
        }
        if (tot == 0) continue;
        n_keep += tot;
#pragma unroll
        for (int c = 1; c <= 4; ++c)
            if (keep[c]) {
                total0 += na[c]; total1 += nb[c];
                const uint32_t b0 = (uint32_t)(na[c] < last ? na[c] : last), b1 = (uint32_t)(nb[c] < last ? nb[c] : last);
                if (b0 < KP_LB && b1 < KP_LB) atomicAdd(&bins[b0 * KP_LB + b1], 1u);
                else atomicAdd(&hist[(uint64_t)b0 * n_bins + b1], 1ull);
            }
        if (LIST) {
            if (fill + tot > KP_EMIT_BUF) kp_flush_list(ek, ec, fill, ctr, o_kmer, o_c01, out_cap);
#pragma unroll
            for (int c = 1; c <= 4; ++c) {
                if (keep[c]) {
                    const uint32_t j = fill + (uint32_t)fmd_below(m[c]);
                    const uint64_t s0 = na[c] > 0xffffffffull ? 0xffffffffull : na[c], s1 = nb[c] > 0xffffffffull ? 0xffffffffull : nb[c];
                    ek[j] = rc[c]; ec[j] = s0 | s1 << 32;
                }
                fill += (uint32_t)__popcll(m[c]);
            }
        }
    }
    if (LIST) kp_flush_list(ek, ec, fill, ctr, o_kmer, o_c01, out_cap);
    __syncthreads();
    for (uint32_t j = (uint32_t)lane; j < KP_LB * KP_LB; j += 64) {
        const uint32_t v = bins[j], b0 = j / KP_LB, b1 = j % KP_LB;   // (a count is clamped below n_bins before it gets here: v = 0 outside the histogram)
        if (v && b0 < n_bins && b1 < n_bins) atomicAdd(&hist[(uint64_t)b0 * n_bins + b1], (unsigned long long)v);
    }
    total0 = km_wave_sum(total0); total1 = km_wave_sum(total1);
    if (lane == 0 && n_ext) atomicAdd(&ctr[KP_EXT], (unsigned long long)n_ext);
    if (lane == 0 && n_keep) {
        atomicAdd(&ctr[KP_NKMER], (unsigned long long)n_keep); atomicAdd(&ctr[KP_TOTAL0], (unsigned long long)total0); atomicAdd(&ctr[KP_TOTAL1], (unsigned long long)total1);
        if (n_only0) atomicAdd(&ctr[KP_ONLY0], (unsigned long long)n_only0);
        if (n_only1) atomicAdd(&ctr[KP_ONLY1], (unsigned long long)n_only1);
    }
}

__global__ void k_kcmp_stat(const unsigned long long *__restrict__ ctr, int root_len, int k, uint64_t out_cap, int listed, fmd_kcmp_stat_t *__restrict__ stat)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    fmd_kcmp_stat_t s;
    s.n_kmers = ctr[KP_NKMER]; s.n_total0 = ctr[KP_TOTAL0]; s.n_total1 = ctr[KP_TOTAL1];
    s.n_only0 = ctr[KP_ONLY0]; s.n_only1 = ctr[KP_ONLY1]; s.n_shared = s.n_kmers - s.n_only0 - s.n_only1;
    s.n_ext = ctr[KP_EXT];
    s.overflow = (ctr[KP_OVF] != 0 || (listed && ctr[KP_OUT] > out_cap)) ? 1 : 0;
    s.widest_level = 0;
    for (int d = root_len; d < k; ++d) if (ctr[d] > s.widest_level) s.widest_level = ctr[d];
    s.n_parts = 1; s.n_retries = 0;
    *stat = s;
}

// dst[i] += src[i]: a part's histogram into the run's
__global__ void k_kcmp_add(unsigned long long *__restrict__ dst, const unsigned long long *__restrict__ src, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (src[i]) dst[i] += src[i];
}

// the sorted c0 | c1 << 32 -> the two columns the sink takes
__global__ void k_kcmp_split(const uint64_t *__restrict__ c01, uint32_t *__restrict__ c0, uint32_t *__restrict__ c1, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t v = c01[i];
        c0[i] = (uint32_t)v; c1[i] = (uint32_t)(v >> 32);
    }
}

// Grids and chunk for a capacity (kc_plan, fmd_kcount.hip): a grid is at most the kernel's resident set, the chunk tails of a level take at most
// half of the capacity, the leaves run on no more waves than the levels.
static void kp_plan(fmd_dev_t *h, uint64_t cap, bool listed, int &grid, int &leaf_grid, uint32_t &ch)
{
    static int per_cu[3] = {0, 0, 0};
    if (!per_cu[0]) {
        per_cu[1] = fmd_resident_per_cu(k_kcmp_leaf<false>, KP_LDS_U4 * 16, 16, "k_kcmp_leaf<false>");
        per_cu[2] = fmd_resident_per_cu(k_kcmp_leaf<true>, (KP_LDS_U4 + KP_EMIT_U4) * 16, 16, "k_kcmp_leaf<true>");
        per_cu[0] = fmd_resident_per_cu(k_kcmp_level, FMD_WAVE_LDS_U4 * 16, 16, "k_kcmp_level");
    }
    grid = fmd_grid_for_lds(h, cap, FMD_WAVE_LDS_U4 * 16);
    if (grid > h->n_cu * per_cu[0]) grid = h->n_cu * per_cu[0];
    ch = 1024;
    while (ch > KP_MIN_CHUNK && (uint64_t)grid * ch * 8 > cap) ch >>= 1;
    const uint64_t g = cap / (2 * (uint64_t)ch);
    if ((uint64_t)grid > g) grid = (int)g;
    if (grid >= 8) grid &= ~7;                        // (a multiple of 8: km_range gives every XCD its eighth)
    if (grid < 1) grid = 1;
    leaf_grid = h->n_cu * per_cu[listed ? 2 : 1];
    if (leaf_grid > grid) leaf_grid = grid;
    if (leaf_grid >= 8) leaf_grid &= ~7;
    if (leaf_grid < 1) leaf_grid = 1;
}

// a necessary sign of an index of both strands (fmd_kcount); an empty index passes
static bool kp_both_strands(const fmd_dev_t *h) { return h->mcnt[2] == h->mcnt[5] && h->mcnt[3] == h->mcnt[4] && !(h->mcnt[1] & 1); }

static int kp_args(fmd_dev_t *h0, fmd_dev_t *h1, int k, int k_min, const fmd_kcmp_sel_t *sel, uint32_t n_bins)
{
    if (!h0 || !h1 || !sel || h0->device != h1->device) return FMD_E_ARG;
    if (k < k_min || k > 32 || n_bins < 2 || n_bins > 1024 || sel->min0 > sel->max0 || sel->min1 > sel->max1) return FMD_E_ARG;
    if (!kp_both_strands(h0) || !kp_both_strands(h1)) return FMD_E_ARG;
    return FMD_OK;
}

extern "C" int fmd_kcmp_part_dev(fmd_dev_t *h0, fmd_dev_t *h1, void *stream, int k, const fmd_kcmp_sel_t *sel, int root_len, size_t n_roots,
                                 const fmd_kcmp_node_t *d_roots, uint64_t cap, uint32_t n_bins, uint64_t *d_hist, uint64_t *d_kmer, uint64_t *d_c01,
                                 uint64_t out_cap, fmd_kcmp_stat_t *d_stat, void *d_work, size_t work_bytes)
{
    FMD_TRY(kp_args(h0, h1, k, 2, sel, n_bins));
    if (!d_hist || !d_stat || !d_work || (n_roots && !d_roots) || (d_kmer && !d_c01) || root_len < 1 || root_len >= k) return FMD_E_ARG;
    const size_t wb = fmd_kcmp_work_bytes(cap);
    if (wb == 0 || work_bytes < wb || n_roots > cap || ((uintptr_t)d_work & 15) || ((uintptr_t)d_roots & 15)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h0->device));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *ctr = (unsigned long long *)d_work;
    fmd_kcmp_node_t *f[2];
    f[0] = (fmd_kcmp_node_t *)(((uintptr_t)((uint8_t *)d_work + KP_HDR_BYTES) + 255) & ~(uintptr_t)255); f[1] = f[0] + cap;
    const FmdIndexView va = fmd_view(h0), vb = fmd_view(h1);
    int grid, leaf_grid; uint32_t ch;
    kp_plan(h0, cap, d_kmer != nullptr, grid, leaf_grid, ch);
    k_kcmp_init<<<1, 64, 0, st>>>(ctr, root_len, (unsigned long long)n_roots);
    const fmd_kcmp_node_t *in = d_roots;
    for (int d = root_len; d < k - 1; ++d) {
        fmd_kcmp_node_t *out = f[(d - root_len) & 1];
        k_kcmp_level<<<grid, 64, 0, st>>>(va, vb, d, (uint64_t)sel->min0, (uint64_t)sel->min1, in, out, cap, ch, ctr, 1);
        in = out;
    }
    if (d_kmer) k_kcmp_leaf<true><<<leaf_grid, 64, 0, st>>>(va, vb, k, *sel, in, cap, n_bins, (unsigned long long *)d_hist, d_kmer, d_c01, out_cap, ctr, 1);
    else k_kcmp_leaf<false><<<leaf_grid, 64, 0, st>>>(va, vb, k, *sel, in, cap, n_bins, (unsigned long long *)d_hist, nullptr, nullptr, 0, ctr, 1);
    k_kcmp_stat<<<1, 64, 0, st>>>(ctr, root_len, k, out_cap, d_kmer != nullptr, d_stat);
    FMD_CHECK_LAUNCH("kcmp kernels");
    return FMD_OK;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct KpRoot { fmd_kcmp_node_t nd; int len; };
typedef std::vector<KpRoot> KpRun;                    // roots of one length, rc(suffix) ascending

static bool kp_pruned(const fmd_kcmp_node_t &nd, const fmd_kcmp_sel_t &sel)
{
    return nd.size[0] < sel.min0 || nd.size[1] < sel.min1 || (nd.size[0] | nd.size[1]) == 0;
}

// What a run of parts keeps, sized by the capacity (KcBufs, fmd_kcount.hip): the large buffers from h0's scratch cache, the list out through pinned
// slices of KP_SLICE entries.  hist[0] = the run's histogram, hist[1] = the part's.
#define KP_SLICE (1u << 20)
struct KpBufs {
    uint64_t cap = 0, out_cap = 0;
    size_t wb = 0, tmp_bytes = 0;
    FmdScratch work, kmer[2], c01[2], tmp;
    FmdDevBuf roots, hist[2], stat;
    FmdHostBuf h_kmer, h_c0, h_c1;
    int alloc(fmd_dev_t *h, uint64_t cap_, uint32_t n_bins, bool listed, int k)
    {
        cap = cap_; out_cap = listed ? cap_ : 0; wb = fmd_kcmp_work_bytes(cap_);
        work.reset(); tmp.reset();
        for (int i = 0; i < 2; ++i) { kmer[i].reset(); c01[i].reset(); }
        FMD_TRY(work.alloc(h, wb)); FMD_TRY(roots.need(4 * sizeof(fmd_kcmp_node_t))); FMD_TRY(stat.need(sizeof(fmd_kcmp_stat_t)));
        for (int i = 0; i < 2; ++i) FMD_TRY(hist[i].need((size_t)n_bins * n_bins * 8));
        if (!listed) return FMD_OK;
        for (int i = 0; i < 2; ++i) { FMD_TRY(kmer[i].alloc(h, out_cap * 8)); FMD_TRY(c01[i].alloc(h, out_cap * 8)); }
        tmp_bytes = 0;
        FMD_HIP_TRY(fmd_sort_pairs(nullptr, tmp_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)out_cap, 0, 2 * k));
        FMD_TRY(tmp.alloc(h, tmp_bytes ? tmp_bytes : 16));
        FMD_TRY(h_kmer.need((size_t)KP_SLICE * 8)); FMD_TRY(h_c0.need((size_t)KP_SLICE * 4));
        return h_c1.need((size_t)KP_SLICE * 4);
    }
};

// every k-mer of one base: the marginal counts, no kernel
static int kp_single_bases(fmd_dev_t *h0, fmd_dev_t *h1, const fmd_kcmp_sel_t &sel, uint32_t n_bins, uint64_t *hist, fmd_kcmp_sink_fn sink, void *ctx, fmd_kcmp_stat_t *stat)
{
    uint64_t kmer[2]; uint32_t c0[2], c1[2]; uint64_t n = 0;
    for (int c = 0; c < 2; ++c) {                     // A (= T on the other strand) and C (= G)
        const uint64_t v0 = h0->mcnt[2 + c], v1 = h1->mcnt[2 + c];
        if ((v0 | v1) == 0 || v0 < sel.min0 || v1 < sel.min1) continue;
        if ((sel.max0 != FMD_KCMP_NO_MAX && v0 > sel.max0) || (sel.max1 != FMD_KCMP_NO_MAX && v1 > sel.max1)) continue;
        kmer[n] = (uint64_t)c; c0[n] = v0 > 0xffffffffull ? 0xffffffffu : (uint32_t)v0; c1[n] = v1 > 0xffffffffull ? 0xffffffffu : (uint32_t)v1; ++n;
        ++hist[(v0 < n_bins - 1 ? v0 : n_bins - 1) * n_bins + (v1 < n_bins - 1 ? v1 : n_bins - 1)];
        ++stat->n_kmers; stat->n_total0 += v0; stat->n_total1 += v1;
        if (v1 == 0) ++stat->n_only0; else if (v0 == 0) ++stat->n_only1; else ++stat->n_shared;
    }
    if (sink && n && sink(ctx, n, kmer, c0, c1)) return FMD_E_IO;
    return FMD_OK;
}

static int kp_run(fmd_dev_t *h0, fmd_dev_t *h1, int k, const fmd_kcmp_sel_t *sel, uint32_t n_bins, uint64_t *hist, uint64_t cap, fmd_kcmp_sink_fn sink, void *ctx,
                  fmd_kcmp_stat_t *stat);
extern "C" int fmd_kcmp(fmd_dev_t *h0, fmd_dev_t *h1, int k, const fmd_kcmp_sel_t *sel, uint32_t n_bins, uint64_t *hist, uint64_t cap, fmd_kcmp_sink_fn sink, void *ctx,
                        fmd_kcmp_stat_t *stat)
{
    try { return kp_run(h0, h1, k, sel, n_bins, hist, cap, sink, ctx, stat); }
    catch (const std::bad_alloc &) { return FMD_E_NOMEM; }   // (the host vectors)
}
static int kp_run(fmd_dev_t *h0, fmd_dev_t *h1, int k, const fmd_kcmp_sel_t *sel, uint32_t n_bins, uint64_t *hist, uint64_t cap, fmd_kcmp_sink_fn sink, void *ctx,
                  fmd_kcmp_stat_t *stat)
{
    FMD_TRY(kp_args(h0, h1, k, 1, sel, n_bins));
    if (!hist || !stat) return FMD_E_ARG;
    if (cap && (cap < FMD_KCMP_MIN_CAP || cap > FMD_KCMP_MAX_CAP)) return FMD_E_ARG;
    const size_t n_cells = (size_t)n_bins * n_bins;
    memset(stat, 0, sizeof(*stat));
    memset(hist, 0, n_cells * 8);
    if (k == 1) return kp_single_bases(h0, h1, *sel, n_bins, hist, sink, ctx, stat);
    FMD_HIP_TRY(hipSetDevice(h0->device));
    fmd_dev_t *hh[2] = {h0, h1};
    const bool listed = sink != nullptr;
    // capacity: the caller's, or -- cap = 0 -- half the symbols of both indexes to start with, doubled after an overflow as long as it fits beside them
    // (a level never holds more live entries than the two indexes have symbols, and the chunk tails take at most as much again)
    const uint64_t n_sym = h0 == h1 ? h0->mcnt[0] : h0->mcnt[0] + h1->mcnt[0];
    uint64_t cap_max = cap;
    if (cap == 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)8 << 30;
        const uint64_t per = 2 * sizeof(fmd_kcmp_node_t) + (listed ? 2 * 16 + 8 : 0);
        cap_max = (uint64_t)(0.7 * (double)free_b) / per;
        if (cap_max > 2 * n_sym + FMD_KCMP_MIN_CAP) cap_max = 2 * n_sym + FMD_KCMP_MIN_CAP;
        if (cap_max > FMD_KCMP_MAX_CAP) cap_max = FMD_KCMP_MAX_CAP;
        if (cap_max < FMD_KCMP_MIN_CAP) cap_max = FMD_KCMP_MIN_CAP;
        cap = n_sym / 2 + (1u << 16);
        if (cap > cap_max) cap = cap_max;
    }
    KpBufs b;
    for (;;) {                                        // (what hipMemGetInfo calls free is not always one piece)
        const int rc = b.alloc(h0, cap, n_bins, listed, k);
        if (rc == FMD_OK) break;
        if (rc != FMD_E_NOMEM || cap_max == cap || cap / 2 < FMD_KCMP_MIN_CAP) return rc;
        cap /= 2; cap_max = cap;
    }
    FMD_HIP_TRY(hipMemsetAsync(b.hist[0].p, 0, n_cells * 8, nullptr));
    const unsigned add_grid = fmd_nblk(n_cells, 256) < 1024 ? fmd_nblk(n_cells, 256) : 1024;
    std::vector<KpRun> todo;                          // the back is next
    {
        KpRun first;
        for (int c = 4; c >= 1; --c) {                // suffix T, G, C, A: rc(suffix) = A, C, G, T
            KpRoot r;
            memset(&r.nd, 0, sizeof(r.nd));
            for (int i = 0; i < 2; ++i) {
                r.nd.size[i] = hh[i]->cnt[c + 1] - hh[i]->cnt[c];
                r.nd.x0[i] = r.nd.size[i] ? hh[i]->cnt[c] : 0;
            }
            r.nd.kmer = (uint64_t)(c - 1); r.len = 1;
            if (!kp_pruned(r.nd, *sel)) first.push_back(r);
        }
        todo.push_back(first);
    }
    while (!todo.empty()) {
        KpRun run = todo.back(); todo.pop_back();
        if (run.empty()) continue;
        fmd_kcmp_node_t roots[4];
        for (size_t i = 0; i < run.size(); ++i) roots[i] = run[i].nd;
        fmd_kcmp_stat_t ps;
        FMD_HIP_TRY(hipMemcpy(b.roots.p, roots, run.size() * sizeof(fmd_kcmp_node_t), hipMemcpyHostToDevice));
        FMD_HIP_TRY(hipMemsetAsync(b.hist[1].p, 0, n_cells * 8, nullptr));
        FMD_TRY(fmd_kcmp_part_dev(h0, h1, nullptr, k, sel, run[0].len, run.size(), b.roots.as<fmd_kcmp_node_t>(), b.cap, n_bins, b.hist[1].as<uint64_t>(),
                                  listed ? b.kmer[0].as<uint64_t>() : nullptr, listed ? b.c01[0].as<uint64_t>() : nullptr, b.out_cap,
                                  b.stat.as<fmd_kcmp_stat_t>(), b.work.p, b.wb));
        FMD_HIP_TRY(hipMemcpy(&ps, b.stat.p, sizeof(ps), hipMemcpyDeviceToHost));
        ++stat->n_parts;
        stat->n_ext += ps.n_ext;                      // (the work of a discarded part was done all the same)
        if (ps.widest_level > stat->widest_level) stat->widest_level = ps.widest_level;
        if (ps.overflow) {                            // discarded whole
            ++stat->n_retries;
            if (b.cap < cap_max) {                    // there is room: the same run again in twice the capacity
                const uint64_t c2 = 2 * b.cap < cap_max ? 2 * b.cap : cap_max;
                if (b.alloc(h0, c2, n_bins, listed, k) == FMD_OK) { cap = c2; todo.push_back(run); continue; }
                cap_max = cap;                        // it does not fit after all: back to what did, and cut the run
                FMD_TRY(b.alloc(h0, cap, n_bins, listed, k));
            }
            if (run.size() > 1) {
                const size_t half = run.size() / 2;
                todo.push_back(KpRun(run.begin() + half, run.end()));
                todo.push_back(KpRun(run.begin(), run.begin() + half));
            } else {
                if (run[0].len >= k - 1) return FMD_E_OVERFLOW;   // (a single leaf root emits four entries at most: cannot happen)
                fmd_intv_t ok[2][6];
                memset(ok, 0, sizeof(ok));
                const uint8_t back = 1;
                for (int i = 0; i < 2; ++i) {         // (only x[0] and the size of a child are used: x[1] of the root is not kept)
                    if (run[0].nd.size[i] == 0) continue;
                    fmd_intv_t ik;
                    ik.x[0] = run[0].nd.x0[i]; ik.x[1] = 0; ik.x[2] = run[0].nd.size[i]; ik.info = 0;
                    FMD_TRY(fmd_extend_batch(hh[i], 1, &ik, &back, ok[i]));
                }
                KpRun kids;
                for (int c = 4; c >= 1; --c) {        // c . suffix: rc = rc(suffix) . comp(c), ascending in comp(c)
                    KpRoot r;
                    memset(&r.nd, 0, sizeof(r.nd));
                    for (int i = 0; i < 2; ++i) { r.nd.size[i] = ok[i][c].x[2]; r.nd.x0[i] = r.nd.size[i] ? ok[i][c].x[0] : 0; }
                    r.nd.kmer = run[0].nd.kmer | (uint64_t)(c - 1) << (2 * run[0].len); r.len = run[0].len + 1;
                    if (!kp_pruned(r.nd, *sel)) kids.push_back(r);
                }
                todo.push_back(kids);
            }
            continue;
        }
        k_kcmp_add<<<add_grid, 256, 0, nullptr>>>(b.hist[0].as<unsigned long long>(), b.hist[1].as<unsigned long long>(), (uint64_t)n_cells);
        FMD_CHECK_LAUNCH("k_kcmp_add");
        stat->n_kmers += ps.n_kmers; stat->n_total0 += ps.n_total0; stat->n_total1 += ps.n_total1;
        stat->n_only0 += ps.n_only0; stat->n_only1 += ps.n_only1; stat->n_shared += ps.n_shared;
        if (listed && ps.n_kmers) {
            const uint64_t n = ps.n_kmers;
            size_t tb = b.tmp_bytes;
            FMD_HIP_TRY(fmd_sort_pairs(b.tmp.p, tb, b.kmer[0].as<uint64_t>(), b.kmer[1].as<uint64_t>(), b.c01[0].as<uint64_t>(), b.c01[1].as<uint64_t>(), (size_t)n, 0, 2 * k));
            uint32_t *d_c0 = b.c01[0].as<uint32_t>(), *d_c1 = d_c0 + b.out_cap;   // the unsorted column has been read: its room takes the two halves
            k_kcmp_split<<<fmd_nblk(n, 256) < 4096 ? fmd_nblk(n, 256) : 4096, 256, 0, nullptr>>>(b.c01[1].as<uint64_t>(), d_c0, d_c1, n);
            FMD_CHECK_LAUNCH("k_kcmp_split");
            for (uint64_t at = 0; at < n; at += KP_SLICE) {
                const uint64_t m = n - at < KP_SLICE ? n - at : KP_SLICE;
                FMD_HIP_TRY(hipMemcpy(b.h_kmer.p, b.kmer[1].as<uint64_t>() + at, m * 8, hipMemcpyDeviceToHost));
                FMD_HIP_TRY(hipMemcpy(b.h_c0.p, d_c0 + at, m * 4, hipMemcpyDeviceToHost));
                FMD_HIP_TRY(hipMemcpy(b.h_c1.p, d_c1 + at, m * 4, hipMemcpyDeviceToHost));
                if (sink(ctx, m, b.h_kmer.as<uint64_t>(), b.h_c0.as<uint32_t>(), b.h_c1.as<uint32_t>())) return FMD_E_IO;
            }
        }
    }
    FMD_HIP_TRY(hipMemcpy(hist, b.hist[0].p, n_cells * 8, hipMemcpyDeviceToHost));
    return FMD_OK;
}
