// fmd_kcgraph.hip -- kcgraph: the coloured de Bruijn graph of up to FMD_KMAT_MAX_IDX indexes of both strands and its unitigs.
//
// kmat's one-sided walk (fmd_ktrie.h: a node = one suffix's interval in EACH index) run one level further than kmat runs it, with the ANY rule -- an inner
// node is dropped iff occ_i < min_occ for every i --, so that the frontier at depth k holds both orientations of every node (k is odd: nothing is halved).
//   (a) k_kcg_arcs: an oriented k-mer W gets one more extension per live side: c_i(c.W) for the four c, halved where c.W is its own reverse complement
//       (decided from the bases), thresholded right after the round of its pair of sides into colour i's LEFT nibble of W: the child sizes of eight sides
//       are never alive together.  An entry leaves as (canonical << 1 | orientation, the N nibbles in one 32-bit word, and -- from the canonical
//       orientation -- the N counts), unordered and dense.
//   (b) one sort by key carrying the slot, then k_kcg_fold: the two adjacent entries of a node -> its N arc bytes (the left nibble of rc(x) is the
//       complemented and reversed right nibble of x), the union byte, the pattern, and the per-colour node, bit and palindrome sums.
//   (c) compaction is kgraph's (fmd_kgraph_compact_dev) on the union byte, with the pattern bytes under FMD_KCGRAPH_SPLIT; k_kcg_usum adds the per-unitig,
//       per-colour sums.
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <new>
#include "fmd_prim.h"
#include "fmd_internal.h"
#include "fmd_kernel_common.h"
#include "fmd_ktrie.h"

static_assert(sizeof(fmd_kcgraph_stat_t) == 80 + 16 * 8 && FMD_KMAT_MAX_IDX == 8, "layout of include/fmd_hip.h");

// counters (u64 words) beside kgraph's (0 .. 5 and 16 .. 95 are the compaction's, fmd_kgraph.hip)
#define KC_OUT 0          // entries emitted by the arc kernel
#define KC_EXT 1          // backward extensions of the arc kernel
#define KC_BITS 2         // union arc bits set
#define KC_PAL 3          // of them, those of a (k+1)-mer that is its own reverse complement
#define KC_BAD 6          // the sorted entries are not pairs of orientations: not indexes of both strands
#define KC_NODES_IN 96    // .. 103: nodes with pattern bit i
#define KC_BITS_IN 104    // .. 111: arc bits of colour i
#define KC_PAL_IN 112     // .. 119: of them, palindromic ones
#define KC_WORDS 128
#define KC_SLICE (1u << 20)

__device__ __forceinline__ uint32_t kcg_rev4(uint32_t v) { return (v & 1u) << 3 | (v & 2u) << 1 | (v & 4u) >> 1 | (v & 8u) >> 3; }

__global__ void k_kcg_init(unsigned long long *__restrict__ ctr, int root_len, unsigned long long n_roots)
{
    const int i = (int)threadIdx.x;
    if (blockIdx.x == 0 && i < KT_WORDS) ctr[i] = i == root_len ? n_roots : 0;
}

// one inner level: k_kmat_level (fmd_kmat.hip) with the ANY rule -- a child is kept iff occ_i >= min_occ for some i.  Its sides below min_occ stay: the
// counts of a node are exact in every colour.
template <int N>
__global__ __launch_bounds__(64) void k_kcg_level(KtViews<N> v, int d, uint64_t min_occ, const KtNode<N> *__restrict__ in, KtNode<N> *__restrict__ out, uint64_t cap,
                                                  uint32_t ch, unsigned long long *__restrict__ ctr, int xcd_aware)
{
    FMD_DECLARE_WAVE_LDS();
    const int lane = fmd_lane();
    const uint64_t n_in = ctr[d] < cap ? ctr[d] : cap;   // an overflowing level counted more than it stored
    const KmRange rg = km_range(n_in, xcd_aware);
    const uint64_t stride = rg.stride;
    KmChunk ck; ck.base = 0; ck.fill = 0; ck.ch = ch; ck.have = false;
    uint32_t n_ext = 0;
    constexpr bool AHEAD = N < 8;                     // (eight sides: no room for a second entry below 256 registers, as in k_kmat_level)
    uint4 nx[N + 1];
    if (AHEAD) kt_load<N>(in, rg.beg + lane, rg.end, nx);
    for (uint64_t base = rg.beg; base < rg.end; base += stride) {
        uint64_t K, x0[N], sz[N];
        if (!AHEAD) kt_load<N>(in, base + lane, rg.end, nx);
        const bool act = kt_unpack<N>(nx, base + lane < rg.end, K, x0, sz);
        if (AHEAD) kt_load<N>(in, base + stride + lane, rg.end, nx);
        if (__ballot(act) == 0) continue;             // a run of holes
#pragma unroll
        for (int i = 0; i < N; ++i) n_ext += (uint32_t)__popcll(__ballot(act && sz[i] != 0));
        uint64_t tk[N][5], n[N][5];
        kt_extend<N>(v, fmd_lds, act, x0, sz, tk, n);
        bool has[5];
        uint32_t tot = 0;
#pragma unroll
        for (int c = 1; c <= 4; ++c) {
            bool ok = false;
#pragma unroll
            for (int i = 0; i < N; ++i) ok = ok || n[i][c] >= min_occ;
            has[c] = act && ok;
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

// the round of sides 2 P and 2 P + 1, folded at once: the child sizes -> the two left nibbles (bit c - 1 of nibble i: c_i(c.W) >= min_occ)
template <int N, int P>
__device__ __forceinline__ uint32_t kcg_round(const KtViews<N> &v, uint4 *lds, bool act, const uint64_t (&x0)[N], const uint64_t (&sz)[N], uint32_t half,
                                              uint64_t min_occ)
{
    uint64_t tk[N][5], n[N][5];
    kt_round<N, P>(v, lds, act, x0, sz, tk, n);
    constexpr int A = 2 * P, B = 2 * P + 1;
    uint32_t nib = 0;
#pragma unroll
    for (int c = 1; c <= 4; ++c) {
        const int h = (int)(half >> (c - 1) & 1u);
        nib |= (n[A][c] >> h) >= min_occ ? 1u << (4 * A + c - 1) : 0u;
        if (B < N) nib |= (n[B < N ? B : A][c] >> h) >= min_occ ? 1u << (4 * B + c - 1) : 0u;
    }
    return nib;
}

// (a) the frontier at depth k -> (canonical << 1 | orientation, N left nibbles, N counts), unordered and dense
template <int N>
__global__ __launch_bounds__(64) void k_kcg_arcs(KtViews<N> v, int k, uint64_t min_occ, const KtNode<N> *__restrict__ in, uint64_t cap,
                                                 const unsigned long long *__restrict__ lvl, unsigned long long *__restrict__ ctr, uint64_t *__restrict__ o_key,
                                                 uint32_t *__restrict__ o_nib, uint32_t *__restrict__ o_cnt, uint64_t out_cap, int xcd_aware)
{
    FMD_DECLARE_WAVE_LDS();
    const int lane = fmd_lane();
    const uint64_t n_in = lvl[k] < cap ? lvl[k] : cap;
    const KmRange rg = km_range(n_in, xcd_aware);
    const uint64_t stride = rg.stride;
    uint32_t n_ext = 0;
    constexpr bool AHEAD = N < 8;
    uint4 nx[N + 1];
    if (AHEAD) kt_load<N>(in, rg.beg + lane, rg.end, nx);
    for (uint64_t base = rg.beg; base < rg.end; base += stride) {
        uint64_t K, x0[N], sz[N];
        if (!AHEAD) kt_load<N>(in, base + lane, rg.end, nx);
        const bool act = kt_unpack<N>(nx, base + lane < rg.end, K, x0, sz);
        if (AHEAD) kt_load<N>(in, base + stride + lane, rg.end, nx);
        const uint64_t m = __ballot(act);
        if (m == 0) continue;
#pragma unroll
        for (int i = 0; i < N; ++i) n_ext += (uint32_t)__popcll(__ballot(act && sz[i] != 0));
        uint32_t half = 0;                            // bit c - 1: c.W is its own reverse complement -- the same in every colour
#pragma unroll
        for (int c = 1; c <= 4; ++c) {
            const uint64_t P = (uint64_t)(c - 1) << (2 * k) | K;
            half |= kc_revcomp(P, k + 1) == P ? 1u << (c - 1) : 0u;
        }
        uint32_t nib = kcg_round<N, 0>(v, fmd_lds, act, x0, sz, half, min_occ);
        if constexpr (N > 2) nib |= kcg_round<N, 1>(v, fmd_lds, act, x0, sz, half, min_occ);
        if constexpr (N > 4) nib |= kcg_round<N, 2>(v, fmd_lds, act, x0, sz, half, min_occ);
        if constexpr (N > 6) nib |= kcg_round<N, 3>(v, fmd_lds, act, x0, sz, half, min_occ);
        const uint64_t R = kc_revcomp(K, k);
        const bool rev = R < K;                       // k is odd: R != K
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(&ctr[KC_OUT], (unsigned long long)__popcll(m));
        first = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(first >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)first);
        const uint64_t o = first + (uint64_t)fmd_below(m);
        if (act && o < out_cap) {                     // (the host sees the counter past out_cap)
            o_key[o] = (rev ? R : K) << 1 | (rev ? 1u : 0u);
            o_nib[o] = nib;
            if (!rev) {
#pragma unroll
                for (int i = 0; i < N; ++i) o_cnt[(uint64_t)i * out_cap + o] = sz[i] > 0xffffffffull ? 0xffffffffu : (uint32_t)sz[i];
            }
        }
    }
    if (lane == 0 && n_ext) atomicAdd(&ctr[KC_EXT], (unsigned long long)n_ext);
}

__global__ void k_kcg_iota(uint32_t *__restrict__ slot, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) slot[i] = (uint32_t)i;
}

// (b) the sorted (key, slot) pairs, two per node -> k-mer, counts, arc bytes per colour, union byte, pattern; the sums of the statistics.
// Columns: the unsorted ones in_cap entries apart, the node arrays n_cap apart.
__global__ __launch_bounds__(256) void k_kcg_fold(int n_idx, int k, uint32_t min_occ, uint64_t n, const uint64_t *__restrict__ key, const uint32_t *__restrict__ slot,
                                                  const uint32_t *__restrict__ nib, const uint32_t *__restrict__ cnt, uint64_t in_cap, uint64_t *__restrict__ kmer,
                                                  uint32_t *__restrict__ count, uint8_t *__restrict__ arcs, uint8_t *__restrict__ uarcs, uint8_t *__restrict__ pat,
                                                  uint64_t n_cap, unsigned long long *__restrict__ ctr)
{
    __shared__ uint32_t acc[32];                      // 0: union bits, 1: union palindromes, 2: bad, 8 + i: nodes in i, 16 + i: bits, 24 + i: palindromes
    if (threadIdx.x < 32) acc[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t mask1 = ~0ull >> (64 - 2 * (k + 1));
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k0 = key[2 * j], k1 = key[2 * j + 1], x = k0 >> 1;
        if (k1 != (k0 | 1ull) || (k0 & 1ull)) atomicOr(&acc[2], 1u);
        const uint32_t s0 = slot[2 * j], s1 = slot[2 * j + 1];
        const uint32_t l0 = nib[s0], l1 = nib[s1];    // the left nibbles of x, and of rc(x)
        uint32_t pm = 0;                              // the arc bits of x whose (k+1)-mer is its own reverse complement
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t R = (x << 2 | (uint64_t)c) & mask1, L = (uint64_t)c << (2 * k) | x;
            pm |= (kc_revcomp(R, k + 1) == R ? 1u << c : 0u) | (kc_revcomp(L, k + 1) == L ? 16u << c : 0u);
        }
        uint32_t ua = 0, p = 0;
        for (int i = 0; i < n_idx; ++i) {
            const uint32_t cv = cnt[(uint64_t)i * in_cap + s0];
            const uint32_t a = (l0 >> (4 * i) & 15u) << 4 | kcg_rev4(l1 >> (4 * i) & 15u);
            count[(uint64_t)i * n_cap + j] = cv;
            arcs[(uint64_t)i * n_cap + j] = (uint8_t)a;
            ua |= a;
            if (cv >= min_occ) { p |= 1u << i; atomicAdd(&acc[8 + i], 1u); }
            if (a) { atomicAdd(&acc[16 + i], (uint32_t)__popc(a)); if (a & pm) atomicAdd(&acc[24 + i], (uint32_t)__popc(a & pm)); }
        }
        kmer[j] = x; uarcs[j] = (uint8_t)ua; pat[j] = (uint8_t)p;
        if (ua) { atomicAdd(&acc[0], (uint32_t)__popc(ua)); if (ua & pm) atomicAdd(&acc[1], (uint32_t)__popc(ua & pm)); }
    }
    __syncthreads();
    if (threadIdx.x < 32 && acc[threadIdx.x]) {
        const int t = (int)threadIdx.x;
        const int w = t == 0 ? KC_BITS : t == 1 ? KC_PAL : t == 2 ? KC_BAD : t >= 24 ? KC_PAL_IN + t - 24 : t >= 16 ? KC_BITS_IN + t - 16 : t >= 8 ? KC_NODES_IN + t - 8 : -1;
        if (w >= 0) atomicAdd(&ctr[w], (unsigned long long)acc[t]);
    }
}

// (c) the per-unitig, per-colour sums from (unitig, count, pattern); u_pat one 32-bit word per unitig
__global__ __launch_bounds__(256) void k_kcg_usum(int n_idx, uint64_t n, const uint32_t *__restrict__ unitig, const uint32_t *__restrict__ count, uint64_t n_cap,
                                                  const uint8_t *__restrict__ pat, unsigned long long *__restrict__ u_count, uint32_t *__restrict__ u_present,
                                                  uint32_t *__restrict__ u_pat)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t u = unitig[j];
        const uint32_t p = pat[j];
        for (int i = 0; i < n_idx; ++i) {
            const uint32_t c = count[(uint64_t)i * n_cap + j];
            if (c) atomicAdd(&u_count[u * n_idx + i], (unsigned long long)c);
            if (p >> i & 1u) atomicAdd(&u_present[u * n_idx + i], 1u);
        }
        atomicOr(&u_pat[u], p);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
typedef std::chrono::steady_clock KcClock;
static double kc_ms(KcClock::time_point t0) { return std::chrono::duration<double, std::milli>(KcClock::now() - t0).count(); }

static size_t kc_node_bytes(int n_idx) { return 16 * ((size_t)n_idx + 1); }

// the sorted graph on the device: the work area of the walk serves the compaction afterwards when it is large enough
struct KcDev {
    int n_idx = 0;
    uint64_t n = 0, fcap = 0;
    size_t wb = 0, tmp_bytes = 0;
    FmdScratch work, key[2], slot[2], nib, cnt, tmp, nodes;
    FmdDevBuf roots, ctr;
    // the node arrays, one buffer: kmer | count[n_idx] | arcs[n_idx] | uarcs | pat, columns n apart
    uint64_t *kmer() const { return nodes.as<uint64_t>(); }
    uint32_t *count() const { return (uint32_t *)(nodes.as<uint8_t>() + 8 * n); }
    uint8_t *arcs() const { return nodes.as<uint8_t>() + (8 + 4 * (size_t)n_idx) * n; }
    uint8_t *uarcs() const { return arcs() + (size_t)n_idx * n; }
    uint8_t *pat() const { return uarcs() + n; }
    int alloc(int n_idx_, fmd_dev_t *h, uint64_t fc, int k)
    {
        n_idx = n_idx_; fcap = fc; wb = KT_HDR_BYTES + 256 + 2 * (size_t)fc * kc_node_bytes(n_idx_);
        work.reset(); tmp.reset(); nib.reset(); cnt.reset(); nodes.reset();
        for (int i = 0; i < 2; ++i) { key[i].reset(); slot[i].reset(); }
        FMD_TRY(work.alloc(h, wb)); FMD_TRY(roots.need(4 * kc_node_bytes(n_idx_))); FMD_TRY(ctr.need(KC_WORDS * 8));
        for (int i = 0; i < 2; ++i) { FMD_TRY(key[i].alloc(h, fc * 8)); FMD_TRY(slot[i].alloc(h, fc * 4)); }
        FMD_TRY(nib.alloc(h, fc * 4)); FMD_TRY(cnt.alloc(h, fc * 4 * (size_t)n_idx_));
        tmp_bytes = 0;
        FMD_HIP_TRY(fmd_sort_pairs(nullptr, tmp_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)fc, 0, 2 * k + 1));
        return tmp.alloc(h, tmp_bytes ? tmp_bytes : 16);
    }
};

static bool kc_both_strands(const fmd_dev_t *h) { return h->mcnt[2] == h->mcnt[5] && h->mcnt[3] == h->mcnt[4] && !(h->mcnt[1] & 1); }

static int kc_check(int n_idx, fmd_dev_t *const *h, int k, int min_occ, uint64_t cap)
{
    if (n_idx < 1 || n_idx > FMD_KMAT_MAX_IDX || !h || k < 3 || k > 31 || !(k & 1) || min_occ < 1 || cap > FMD_KGRAPH_MAX_NODES) return FMD_E_ARG;
    for (int i = 0; i < n_idx; ++i)
        if (!h[i] || h[i]->device != h[0]->device || !kc_both_strands(h[i])) return FMD_E_ARG;
    return FMD_OK;
}

// grid and chunk of the levels for a capacity (kt_plan, fmd_kmat.hip), and the grid of the arc kernel
template <int N>
static void kc_plan(fmd_dev_t *h, uint64_t cap, int &grid, int &arc_grid, uint32_t &ch)
{
    static int per_cu[2] = {0, 0};
    if (!per_cu[0]) {
        per_cu[1] = fmd_resident_per_cu(k_kcg_arcs<N>, FMD_WAVE_LDS_U4 * 16, 16, "k_kcg_arcs<N>");
        per_cu[0] = fmd_resident_per_cu(k_kcg_level<N>, FMD_WAVE_LDS_U4 * 16, 16, "k_kcg_level<N>");
    }
    grid = fmd_grid_for_lds(h, cap, FMD_WAVE_LDS_U4 * 16);
    if (grid > h->n_cu * per_cu[0]) grid = h->n_cu * per_cu[0];
    ch = 1024;
    while (ch > KT_MIN_CHUNK && (uint64_t)grid * ch * 8 > cap) ch >>= 1;
    const uint64_t g = cap / (2 * (uint64_t)ch);
    if ((uint64_t)grid > g) grid = (int)g;
    if (grid >= 8) grid &= ~7;                        // (a multiple of 8: km_range gives every XCD its eighth)
    if (grid < 1) grid = 1;
    arc_grid = h->n_cu * per_cu[1];
    if (arc_grid > grid) arc_grid = grid;
    if (arc_grid >= 8) arc_grid &= ~7;
    if (arc_grid < 1) arc_grid = 1;
}

// the levels 1 .. k - 1 and the arc kernel, for N indexes
template <int N>
static void kc_enqueue(fmd_dev_t *const *h, int k, int min_occ, size_t n_roots, KcDev &g)
{
    KtViews<N> v;
    for (int i = 0; i < N; ++i) v.ix[i] = fmd_view(h[i]);
    unsigned long long *lvl = (unsigned long long *)g.work.p, *ctr = g.ctr.as<unsigned long long>();
    KtNode<N> *f[2];
    f[0] = (KtNode<N> *)(((uintptr_t)((uint8_t *)g.work.p + KT_HDR_BYTES) + 255) & ~(uintptr_t)255); f[1] = f[0] + g.fcap;
    int grid, arc_grid; uint32_t ch;
    kc_plan<N>(h[0], g.fcap, grid, arc_grid, ch);
    k_kcg_init<<<1, 64, 0, nullptr>>>(lvl, 1, (unsigned long long)n_roots);
    const KtNode<N> *in = (const KtNode<N> *)g.roots.p;
    for (int d = 1; d < k; ++d) {
        KtNode<N> *out = f[(d - 1) & 1];
        k_kcg_level<N><<<grid, 64, 0, nullptr>>>(v, d, (uint64_t)min_occ, in, out, g.fcap, ch, lvl, 1);
        in = out;
    }
    k_kcg_arcs<N><<<arc_grid, 64, 0, nullptr>>>(v, k, (uint64_t)min_occ, in, g.fcap, lvl, ctr, g.key[0].as<uint64_t>(), g.nib.as<uint32_t>(), g.cnt.as<uint32_t>(),
                                               g.fcap, 1);
}

// nodes, counts, arc bytes, union bytes and patterns, sorted, on the device.  cap = the most nodes (0: FMD_KGRAPH_MAX_NODES); the frontiers are sized as
// kmat's driver sizes them and grown after an overflow while they fit; FMD_E_NOMEM when they do not, or when there are more nodes than cap.
static int kc_arcs(int n_idx, fmd_dev_t *const *h, int k, int min_occ, uint64_t cap, KcDev &g, fmd_kcgraph_stat_t *stat)
{
    memset(stat, 0, sizeof(*stat));
    g.n = 0; g.n_idx = n_idx;
    const KcClock::time_point t0 = KcClock::now();
    FMD_HIP_TRY(hipSetDevice(h[0]->device));
    const size_t nb = kc_node_bytes(n_idx);
    uint64_t roots[4 * 2 * (FMD_KMAT_MAX_IDX + 1)];
    size_t n_roots = 0;
    for (int c = 4; c >= 1; --c) {                    // suffix T, G, C, A (kmat's roots), kept by the ANY rule
        uint64_t *w = roots + n_roots * (nb / 8);
        bool any = false;
        w[0] = (uint64_t)(c - 1); w[1] = 0;
        for (int i = 0; i < n_idx; ++i) {
            const uint64_t sz = h[i]->cnt[c + 1] - h[i]->cnt[c];
            w[2 + i] = sz ? h[i]->cnt[c] : 0; w[2 + n_idx + i] = sz;
            any = any || sz >= (uint64_t)min_occ;
        }
        if (any) ++n_roots;
    }
    if (n_roots == 0) return FMD_OK;                  // empty indexes, or nothing that frequent
    uint64_t n_sym = 0;
    for (int i = 0; i < n_idx; ++i) {
        bool seen = false;
        for (int j = 0; j < i; ++j) seen = seen || h[j] == h[i];
        if (!seen) n_sym += h[i]->mcnt[0];
    }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)8 << 30;
    // per frontier entry: two frontiers, two keys, two slots, nibbles, counts, the sort's temporary, and half a node of the graph
    const uint64_t per = 2 * nb + 2 * 8 + 2 * 4 + 4 + 4 * (uint64_t)n_idx + 16 + (10 + 5 * (uint64_t)n_idx) / 2 + 1;
    uint64_t fc_max = (uint64_t)(0.6 * (double)free_b) / per;
    if (fc_max > 2 * n_sym + FMD_KMAT_MIN_CAP) fc_max = 2 * n_sym + FMD_KMAT_MIN_CAP;
    if (fc_max > FMD_KMAT_MAX_CAP) fc_max = FMD_KMAT_MAX_CAP;
    if (fc_max < FMD_KMAT_MIN_CAP) fc_max = FMD_KMAT_MIN_CAP;
    uint64_t fc = n_sym / 2 + (1u << 16);
    if (fc > fc_max) fc = fc_max;
    unsigned long long hc[KC_WORDS], lvl[KT_WORDS];
    for (;;) {
        FMD_TRY(g.alloc(n_idx, h[0], fc, k));
        FMD_HIP_TRY(hipMemcpy(g.roots.p, roots, n_roots * nb, hipMemcpyHostToDevice));
        FMD_HIP_TRY(hipMemsetAsync(g.ctr.p, 0, KC_WORDS * 8, nullptr));
        switch (n_idx) {
#define KC_CASE(N) case N: kc_enqueue<N>(h, k, min_occ, n_roots, g); break;
            KC_CASE(1) KC_CASE(2) KC_CASE(3) KC_CASE(4) KC_CASE(5) KC_CASE(6) KC_CASE(7) KC_CASE(8)
#undef KC_CASE
        }
        FMD_CHECK_LAUNCH("kcgraph walk");
        FMD_HIP_TRY(hipMemcpy(lvl, g.work.p, sizeof(lvl), hipMemcpyDeviceToHost));
        FMD_HIP_TRY(hipMemcpy(hc, g.ctr.p, sizeof(hc), hipMemcpyDeviceToHost));
        stat->g.n_ext += lvl[KT_EXT] + hc[KC_EXT];
        if (!lvl[KT_OVF] && hc[KC_OUT] <= fc) break;
        if (fc >= fc_max) return FMD_E_NOMEM;
        fc = 2 * fc < fc_max ? 2 * fc : fc_max;
    }
    const uint64_t n_ent = hc[KC_OUT], n = n_ent / 2;
    if (n_ent & 1) return FMD_E_ARG;                  // not both orientations of every node: not indexes of both strands
    if (n > (cap ? cap : (uint64_t)FMD_KGRAPH_MAX_NODES)) return FMD_E_NOMEM;
    if (n) {
        const unsigned gr = fmd_nblk(n_ent, 256) < 4096u ? fmd_nblk(n_ent, 256) : 4096u;
        size_t tb = g.tmp_bytes;
        k_kcg_iota<<<gr, 256, 0, nullptr>>>(g.slot[0].as<uint32_t>(), n_ent);
        FMD_HIP_TRY(fmd_sort_pairs(g.tmp.p, tb, g.key[0].as<uint64_t>(), g.key[1].as<uint64_t>(), g.slot[0].as<uint32_t>(), g.slot[1].as<uint32_t>(), (size_t)n_ent, 0,
                                   2 * k + 1));
        g.n = n;
        FMD_TRY(g.nodes.alloc(h[0], (10 + 5 * (size_t)n_idx) * n + 16));
        k_kcg_fold<<<fmd_nblk(n, 256) < 4096u ? fmd_nblk(n, 256) : 4096u, 256, 0, nullptr>>>(n_idx, k, (uint32_t)min_occ, n, g.key[1].as<uint64_t>(), g.slot[1].as<uint32_t>(),
                                                                                             g.nib.as<uint32_t>(), g.cnt.as<uint32_t>(), g.fcap, g.kmer(), g.count(),
                                                                                             g.arcs(), g.uarcs(), g.pat(), n, g.ctr.as<unsigned long long>());
        FMD_CHECK_LAUNCH("kcgraph fold");
        FMD_HIP_TRY(hipMemcpy(hc, g.ctr.p, sizeof(hc), hipMemcpyDeviceToHost));
        if (hc[KC_BAD]) { g.n = 0; return FMD_E_ARG; }
    }
    stat->g.n_nodes = n;
    stat->g.n_arcs = (hc[KC_BITS] + hc[KC_PAL]) / 2;  // a (k+1)-mer sets a bit at its prefix node and one at its suffix node: the same bit when it is its own reverse complement
    for (int i = 0; i < n_idx; ++i) { stat->n_nodes_in[i] = hc[KC_NODES_IN + i]; stat->n_arcs_in[i] = (hc[KC_BITS_IN + i] + hc[KC_PAL_IN + i]) / 2; }
    stat->g.ms_arcs = kc_ms(t0);
    return FMD_OK;
}

static int kc_kcarcs(int n_idx, fmd_dev_t *const *h, int k, int min_occ, uint64_t cap, fmd_kcarcs_sink_fn sink, void *ctx, fmd_kcgraph_stat_t *stat)
{
    if (!stat) return FMD_E_ARG;
    FMD_TRY(kc_check(n_idx, h, k, min_occ, cap));
    KcDev g;
    FMD_TRY(kc_arcs(n_idx, h, k, min_occ, cap, g, stat));
    if (!sink || g.n == 0) return FMD_OK;
    FmdHostBuf hk, hcn, ha;
    FMD_TRY(hk.alloc((size_t)KC_SLICE * 8)); FMD_TRY(hcn.alloc((size_t)KC_SLICE * 4 * n_idx)); FMD_TRY(ha.alloc((size_t)KC_SLICE * (n_idx + 1)));
    const uint32_t *ccol[FMD_KMAT_MAX_IDX];
    const uint8_t *acol[FMD_KMAT_MAX_IDX];
    for (int i = 0; i < n_idx; ++i) { ccol[i] = hcn.as<uint32_t>() + (size_t)i * KC_SLICE; acol[i] = ha.as<uint8_t>() + (size_t)i * KC_SLICE; }
    uint8_t *ua = ha.as<uint8_t>() + (size_t)n_idx * KC_SLICE;
    for (uint64_t at = 0; at < g.n; at += KC_SLICE) {
        const uint64_t m = g.n - at < KC_SLICE ? g.n - at : KC_SLICE;
        FMD_HIP_TRY(hipMemcpy(hk.p, g.kmer() + at, m * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < n_idx; ++i) {
            FMD_HIP_TRY(hipMemcpy((void *)ccol[i], g.count() + (uint64_t)i * g.n + at, m * 4, hipMemcpyDeviceToHost));
            FMD_HIP_TRY(hipMemcpy((void *)acol[i], g.arcs() + (uint64_t)i * g.n + at, m, hipMemcpyDeviceToHost));
        }
        FMD_HIP_TRY(hipMemcpy(ua, g.uarcs() + at, m, hipMemcpyDeviceToHost));
        if (sink(ctx, m, hk.as<uint64_t>(), ccol, acol, ua)) return FMD_E_IO;
    }
    return FMD_OK;
}
extern "C" int fmd_kcarcs(int n_idx, fmd_dev_t *const *h, int k, int min_occ, uint64_t cap, fmd_kcarcs_sink_fn sink, void *ctx, fmd_kcgraph_stat_t *stat)
{
    try { return kc_kcarcs(n_idx, h, k, min_occ, cap, sink, ctx, stat); }
    catch (const std::bad_alloc &) { return FMD_E_NOMEM; }
}

static void kc_free_out(fmd_kcunitig_t *o)
{
    free(o->kmer); free(o->count); free(o->arcs); free(o->uarcs); free(o->pattern); free(o->unitig); free(o->offset); free(o->orient);
    free(o->u_nodes); free(o->u_first); free(o->u_flags); free(o->u_count); free(o->u_present); free(o->u_pattern);
    memset(o, 0, sizeof(*o));
}

// bub != NULL (fmd_kcbubble; flags = 0): the bubble stage runs on the graph before the device lets go of it
static int kc_kcunitig(int n_idx, fmd_dev_t *const *h, int k, int min_occ, unsigned flags, uint64_t cap, fmd_kcunitig_t *out, fmd_kcbubble_t *bub = nullptr,
                       uint32_t max_len = 0)
{
    if (flags & ~FMD_KCGRAPH_SPLIT) return FMD_E_ARG;
    FMD_TRY(kc_check(n_idx, h, k, min_occ, cap));
    KcDev g;
    fmd_kcgraph_stat_t st;
    FMD_TRY(kc_arcs(n_idx, h, k, min_occ, cap, g, &st));
    const uint64_t n = g.n;
    out->stat = st; out->n_idx = n_idx;
    if (n == 0) return FMD_OK;
    // compaction in the work area of the walk when it is large enough (it is, but for graphs of a few nodes in a large capacity: never smaller)
    const size_t need = fmd_kgraph_compact_bytes(n);
    FmdScratch cw;
    void *wp = g.work.p; size_t wbytes = g.wb;
    if (need > g.wb) { FMD_TRY(cw.alloc(h[0], need)); wp = cw.p; wbytes = need; }
    FmdKgLabels lb;
    FMD_TRY(fmd_kgraph_compact_dev(k, n, g.kmer(), g.uarcs(), (flags & FMD_KCGRAPH_SPLIT) ? g.pat() : nullptr, wp, wbytes, g.ctr.as<unsigned long long>(), &lb));
    out->stat.g.ms_links = lb.ms_links; out->stat.g.ms_label = lb.ms_label;
    out->stat.g.n_links = lb.n_links; out->stat.g.n_cycles = lb.n_cycles; out->stat.g.n_rounds = lb.n_rounds;
    out->n_nodes = n;
    out->kmer = (uint64_t *)malloc(n * 8); out->count = (uint32_t *)malloc(n * 4 * n_idx); out->arcs = (uint8_t *)malloc(n * n_idx);
    out->uarcs = (uint8_t *)malloc(n); out->pattern = (uint8_t *)malloc(n);
    out->unitig = (uint32_t *)malloc(n * 4); out->offset = (uint32_t *)malloc(n * 4); out->orient = (uint8_t *)malloc(n);
    if (!out->kmer || !out->count || !out->arcs || !out->uarcs || !out->pattern || !out->unitig || !out->offset || !out->orient) return FMD_E_NOMEM;
    FMD_HIP_TRY(hipMemcpy(out->kmer, g.kmer(), n * 8, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(out->count, g.count(), n * 4 * n_idx, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(out->arcs, g.arcs(), n * n_idx, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(out->uarcs, g.uarcs(), n, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(out->pattern, g.pat(), n, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(out->unitig, lb.label, n * 4, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(out->offset, lb.off, n * 4, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(out->orient, lb.oc, n, hipMemcpyDeviceToHost));
    FMD_TRY(fmd_kgraph_number_host(n, out->unitig, out->offset, out->orient, &out->n_unitigs, &out->u_nodes, &out->u_first, &out->u_flags));
    const uint64_t nu = out->n_unitigs;
    out->stat.g.n_unitigs = nu;
    // the per-unitig sums: the unitig ids go back up (into the label words, done with), the sums come down
    const KcClock::time_point t0 = KcClock::now();
    FmdScratch us;
    const size_t ub = nu * n_idx * 12 + nu * 4;
    FMD_TRY(us.alloc(h[0], ub + 16));
    unsigned long long *d_uc = us.as<unsigned long long>();
    uint32_t *d_up = (uint32_t *)(d_uc + nu * n_idx), *d_pt = d_up + nu * n_idx;
    FMD_HIP_TRY(hipMemsetAsync(us.p, 0, ub, nullptr));
    FMD_HIP_TRY(hipMemcpy(lb.label, out->unitig, n * 4, hipMemcpyHostToDevice));
    k_kcg_usum<<<fmd_nblk(n, 256) < 4096u ? fmd_nblk(n, 256) : 4096u, 256, 0, nullptr>>>(n_idx, n, lb.label, g.count(), n, g.pat(), d_uc, d_up, d_pt);
    FMD_CHECK_LAUNCH("kcgraph usum");
    out->u_count = (uint64_t *)malloc(nu * n_idx * 8); out->u_present = (uint32_t *)malloc(nu * n_idx * 4); out->u_pattern = (uint8_t *)malloc(nu);
    uint32_t *pt = (uint32_t *)malloc(nu * 4);
    if (!out->u_count || !out->u_present || !out->u_pattern || !pt) { free(pt); return FMD_E_NOMEM; }
    hipError_t e = hipMemcpy(out->u_count, d_uc, nu * n_idx * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out->u_present, d_up, nu * n_idx * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(pt, d_pt, nu * 4, hipMemcpyDeviceToHost);
    for (uint64_t u = 0; u < nu && e == hipSuccess; ++u) out->u_pattern[u] = (uint8_t)pt[u];
    free(pt);
    FMD_HIP_TRY(e);
    out->stat.g.ms_label += kc_ms(t0);
    if (bub) FMD_TRY(fmd_kbubble_stage_dev(h[0], k, n, g.kmer(), g.uarcs(), &lb, max_len, 0, &bub->n_forks, &bub->n_bubbles, &bub->bubble, &bub->ms_bubble));
    return FMD_OK;
}
extern "C" int fmd_kcunitig(int n_idx, fmd_dev_t *const *h, int k, int min_occ, unsigned flags, uint64_t cap, fmd_kcunitig_t *out)
{
    if (!out) return FMD_E_ARG;
    memset(out, 0, sizeof(*out));
    int rc;
    try { rc = kc_kcunitig(n_idx, h, k, min_occ, flags, cap, out); }
    catch (const std::bad_alloc &) { rc = FMD_E_NOMEM; }
    if (rc) kc_free_out(out);
    return rc;
}

extern "C" int fmd_kcbubble(int n_idx, fmd_dev_t *const *h, int k, int min_occ, uint32_t max_len, uint64_t cap, fmd_kcbubble_t *out)
{
    if (!out) return FMD_E_ARG;
    memset(out, 0, sizeof(*out));
    int rc;
    try { rc = kc_kcunitig(n_idx, h, k, min_occ, 0, cap, &out->g, out, max_len); }
    catch (const std::bad_alloc &) { rc = FMD_E_NOMEM; }
    if (rc) { kc_free_out(&out->g); free(out->bubble); memset(out, 0, sizeof(*out)); }
    return rc;
}
