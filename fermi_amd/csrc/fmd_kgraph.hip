// fmd_kgraph.hip -- kgraph: the de Bruijn graph of the counted k-mers of the indexed reads and its unitigs.
//
// The nodes are kcount's list for (k, min_occ), k odd; the walk down to them is kcount's (fmd_kcount_levels: km_level_step, fmd_level.h), run ONE level
// further than kcount runs it, so that the frontier at depth k is there: both orientations of every node, each a bi-interval (x0 of W, x1 of rc(W), size).
//   (a) k_kgraph_arcs: the lane of the canonical orientation extends its bi-interval at BOTH ends -- one six-symbol backward extension at x0 gives the
//       four c.W, one at x1 gives the four c'.rc(W) = rc(W.comp(c')) -- and packs the eight thresholded answers into the node's arc byte.  The count of
//       a (k+1)-mer that is its own reverse complement is halved, decided from its bases.  Nodes leave unordered and are sorted by k-mer once.
//   (b) k_kgraph_links: a PORT is (node, side): 2 i + 0 = the right end of the canonical string, 2 i + 1 = its left end.  The port through which a
//       compactable link leaves gets the port of the other node through which it arrives (its mate); a binary search of the sorted list finds that node.
//   (c) k_kgraph_round: pointer doubling over the 2 n directed states "at node i, leaving through port p" -- successor = mate(p) ^ 1 -- carrying the
//       jump, the steps taken and the smallest node id seen.  Chains with ends settle in ceil(log2(length)) + 1 rounds; a state that is still moving when
//       no label changes any more is on a cycle whose every state holds the cycle's smallest id from both directions: k_kgraph_cut opens the cycle at the
//       left port of that node, and the doubling runs again for the states of cycles only.  k_kgraph_final turns the two settled states of a node into
//       (label, offset, orientation).
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <new>
#include "fmd_prim.h"
#include "fmd_internal.h"
#include "fmd_kernel_common.h"
#include "fmd_level.h"

static_assert(sizeof(fmd_kgraph_stat_t) == 80, "layout of include/fmd_hip.h");

// counters (u64 words)
#define KG_OUT 0         // nodes emitted (counts on when the list is full)
#define KG_EXT 1         // backward extensions of the arc kernel
#define KG_BITS 2        // arc bits set
#define KG_PAL 3         // of them, those of a (k+1)-mer that is its own reverse complement
#define KG_MATES 4       // ports with a mate
#define KG_CYC 5         // cycles opened
#define KG_CHG 16        // [KG_CHG + r] != 0: round r changed a label or settled a state
#define KG_MAX_ROUNDS 80
#define KG_WORDS 128
#define KG_NONE 0xffffffffu
#define KG_SLICE (1u << 20)

__device__ __forceinline__ uint32_t kg_rev4(uint32_t v) { return (v & 1u) << 3 | (v & 2u) << 1 | (v & 4u) >> 1 | (v & 8u) >> 3; }

// (a) the frontier at depth k -> (canonical k-mer, count | arcs << 32), unordered and dense
__global__ __launch_bounds__(64) void k_kgraph_arcs(FmdIndexView ix, int k, uint64_t min_occ, const fmd_intv_t *__restrict__ in, uint64_t cap,
                                                    const unsigned long long *__restrict__ lvl, unsigned long long *__restrict__ ctr,
                                                    uint64_t *__restrict__ o_kmer, uint64_t *__restrict__ o_val, uint64_t out_cap, int xcd_aware)
{
    FMD_DECLARE_COMPACT_LDS();
    const int lane = fmd_lane();
    const uint64_t n = lvl[k] < cap ? lvl[k] : cap;
    const KmRange rg = km_range(n, xcd_aware);
    const uint64_t mask1 = ~0ull >> (64 - 2 * (k + 1));   // k + 1 bases
    uint32_t n_ext = 0;
    for (uint64_t base = rg.beg; base < rg.end; base += rg.stride) {
        uint4 a = make_uint4(0, 0, 0, 0), b = a;
        if (base + lane < rg.end) { const uint4 *q = (const uint4 *)(in + base + lane); a = q[0]; b = q[1]; }
        const uint64_t x0 = (uint64_t)a.y << 32 | a.x, x1 = (uint64_t)a.w << 32 | a.z;
        const uint64_t sz = (uint64_t)b.y << 32 | b.x, K = (uint64_t)b.w << 32 | b.z;
        const bool act = sz != 0 && K < kc_revcomp(K, k);   // k is odd: exactly one orientation of a node is the canonical one
        const uint64_t m = __ballot(act);
        if (m == 0) continue;
        n_ext += 2 * (uint32_t)__popcll(m);
        uint64_t tk[6], s[6];
        uint32_t arcs = 0;
        km_extend_back<false>(ix, fmd_lds, act, x0, sz, 0, tk, s);        // c . W
#pragma unroll
        for (int c = 1; c <= 4; ++c) {
            const uint64_t P = (uint64_t)(c - 1) << (2 * k) | K;
            const uint64_t cnt = kc_revcomp(P, k + 1) == P ? s[c] >> 1 : s[c];
            arcs |= cnt >= min_occ ? 16u << (c - 1) : 0u;
        }
        __syncthreads();                                                  // the landing area is read before it is posted to again
        km_extend_back<false>(ix, fmd_lds, act, x1, sz, 0, tk, s);        // c' . rc(W) = rc(W . comp(c'))
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t P = (K << 2 | (uint64_t)c) & mask1;
            const uint64_t cnt = kc_revcomp(P, k + 1) == P ? s[4 - c] >> 1 : s[4 - c];
            arcs |= cnt >= min_occ ? 1u << c : 0u;
        }
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(&ctr[KG_OUT], (unsigned long long)__popcll(m));
        first = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(first >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)first);
        const uint64_t o = first + (uint64_t)fmd_below(m);
        if (act && o < out_cap) {                                         // (the host sees the counter past out_cap)
            o_kmer[o] = K;
            o_val[o] = (sz > 0xffffffffull ? 0xffffffffull : sz) | (uint64_t)arcs << 32;
        }
    }
    if (lane == 0 && n_ext) atomicAdd(&ctr[KG_EXT], (unsigned long long)n_ext);
}

// the sorted values -> counts and arc bytes; the arc bits and how many of them belong to a (k+1)-mer that is its own reverse complement
__global__ __launch_bounds__(256) void k_kgraph_unpack(int k, uint64_t n, const uint64_t *__restrict__ kmer, const uint64_t *__restrict__ val,
                                                       uint32_t *__restrict__ count, uint8_t *__restrict__ arcs, unsigned long long *__restrict__ ctr)
{
    const uint64_t mask1 = ~0ull >> (64 - 2 * (k + 1));
    uint64_t bits = 0, pal = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t v = val[i], x = kmer[i];
        const uint32_t a = (uint32_t)(v >> 32) & 0xffu;
        count[i] = (uint32_t)v; arcs[i] = (uint8_t)a;
        bits += (uint64_t)__popc(a);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint64_t R = (x << 2 | (uint64_t)c) & mask1, L = (uint64_t)c << (2 * k) | x;
            pal += ((a >> c & 1u) && kc_revcomp(R, k + 1) == R) + ((a >> (4 + c) & 1u) && kc_revcomp(L, k + 1) == L);
        }
    }
    bits = km_wave_sum(bits); pal = km_wave_sum(pal);
    if (fmd_lane() == 0 && bits) { atomicAdd(&ctr[KG_BITS], (unsigned long long)bits); atomicAdd(&ctr[KG_PAL], (unsigned long long)pal); }
}

// (b) the mate of every port.  Port p = 2 i + side leaves node i in the orientation u = side ? rc(x) : x through u's right end.
// pat != NULL (kcgraph's split rule): a link is compactable only between nodes of one pattern.
__global__ __launch_bounds__(256) void k_kgraph_links(int k, uint64_t n, const uint64_t *__restrict__ kmer, const uint8_t *__restrict__ arcs,
                                                      const uint8_t *__restrict__ pat, uint32_t *__restrict__ mate, unsigned long long *__restrict__ ctr)
{
    const uint64_t mask = ~0ull >> (64 - 2 * k);
    uint64_t n_mates = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < 2 * n; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = p >> 1;
        const uint32_t side = (uint32_t)p & 1u, a = arcs[i];
        const uint64_t x = kmer[i], u = side ? kc_revcomp(x, k) : x;
        const uint32_t r = side ? kg_rev4(a >> 4) : a & 15u;              // u's right arcs
        uint32_t mt = KG_NONE;
        if (__popc(r) == 1) {
            const uint64_t v = (u << 2 | (uint64_t)(__ffs((int)r) - 1)) & mask, rv = kc_revcomp(v, k), y = v < rv ? v : rv;
            uint64_t lo = 0, hi = n;                                     // the first j with kmer[j] >= y
            while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (kmer[mid] < y) lo = mid + 1; else hi = mid; }
            if (lo < n && kmer[lo] == y && lo != i && (!pat || pat[lo] == pat[i])) {   // (a self-loop or a hairpin is an end)
                const uint32_t b = arcs[lo], l = v == y ? b >> 4 : b & 15u;   // v's left arcs, up to their order
                if (__popc(l) == 1) mt = (uint32_t)(2 * lo) + (v == y ? 1u : 0u);   // v forward is entered through its left port
            }
        }
        mate[p] = mt;
        n_mates += mt != KG_NONE;
    }
    n_mates = km_wave_sum(n_mates);
    if (fmd_lane() == 0 && n_mates) atomicAdd(&ctr[KG_MATES], (unsigned long long)n_mates);
}

// (c) a state: x = where the jump lands (settled: the free port at the chain's end), y = the steps taken, z = the smallest node id among the nodes the
// jump passed, its own first and its landing node last only when settled, w = 1 when settled
__global__ __launch_bounds__(256) void k_kgraph_init(uint64_t n2, const uint32_t *__restrict__ mate, uint4 *__restrict__ st, int moving_only)
{
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n2; p += (uint64_t)gridDim.x * blockDim.x) {
        if (moving_only && st[p].w) continue;
        const uint32_t m = mate[p];
        st[p] = m == KG_NONE ? make_uint4((uint32_t)p, 0u, (uint32_t)(p >> 1), 1u) : make_uint4(m ^ 1u, 1u, (uint32_t)(p >> 1), 0u);
    }
}

__global__ __launch_bounds__(256) void k_kgraph_round(uint64_t n2, const uint4 *__restrict__ in, uint4 *__restrict__ out, unsigned long long *__restrict__ chg)
{
    bool any = false;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n2; p += (uint64_t)gridDim.x * blockDim.x) {
        uint4 a = in[p];
        if (!a.w) {
            const uint4 b = in[a.x];
            any |= b.z < a.z || b.w;
            a = make_uint4(b.x, a.y + b.y, b.z < a.z ? b.z : a.z, b.w);
        }
        out[p] = a;
    }
    if (any) *chg = 1;
}

// what still moves is on a cycle: mark its nodes, and open the cycle at the left port of its smallest node
__global__ __launch_bounds__(256) void k_kgraph_cut(uint64_t n2, const uint4 *__restrict__ st, uint32_t *__restrict__ mate, uint8_t *__restrict__ oc,
                                                    unsigned long long *__restrict__ ctr)
{
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n2; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 a = st[p];
        if (a.w) continue;
        oc[p >> 1] = 2;
        if (p == 2 * (uint64_t)a.z + 1) {                                 // one thread per cycle, and nobody else reads or writes these two words
            const uint32_t q = mate[p];
            mate[p] = KG_NONE; mate[q] = KG_NONE;
            atomicAdd(&ctr[KG_CYC], 1ull);
        }
    }
}

// the string that starts at the free port e: the node forward when e is its left port
__device__ __forceinline__ uint64_t kg_start_kmer(const uint64_t *kmer, uint32_t e, int k) { const uint64_t x = kmer[e >> 1]; return e & 1u ? x : kc_revcomp(x, k); }

__global__ __launch_bounds__(256) void k_kgraph_final(int k, uint64_t n, const uint64_t *__restrict__ kmer, const uint4 *__restrict__ st,
                                                      uint32_t *__restrict__ label, uint32_t *__restrict__ off, uint8_t *__restrict__ oc)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 r = st[2 * i], l = st[2 * i + 1];                     // to the right of the node as stored, and to its left
        const uint32_t lab = r.z < l.z ? r.z : l.z, cyc = oc[i] & 2u;
        // the printed start: of a cycle the left port of its smallest node; else the end whose k-mer is the smaller (two nodes: they differ; one: forward)
        const bool from_left = cyc ? l.x == 2 * lab + 1 : kg_start_kmer(kmer, l.x, k) < kg_start_kmer(kmer, r.x, k);
        label[i] = lab;
        off[i] = from_left ? l.y : r.y;
        oc[i] = (uint8_t)(cyc | (from_left ? 0u : 1u));
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
typedef std::chrono::steady_clock KgClock;
static double kg_ms(KgClock::time_point t0) { return std::chrono::duration<double, std::milli>(KgClock::now() - t0).count(); }

// the sorted nodes on the device; the work area of the walk serves the compaction afterwards
struct KgDev {
    uint64_t n = 0, fcap = 0;
    size_t wb = 0;
    FmdScratch work, key[2], val[2], tmp;
    FmdDevBuf roots, ctr;
    const uint64_t *kmer() const { return key[1].as<uint64_t>(); }
    uint32_t *count() const { return key[0].as<uint32_t>(); }            // (the unsorted keys are done with once the sort is)
    uint8_t *arcs() const { return key[0].as<uint8_t>() + 4 * (fcap / 2 + 64); }
    uint64_t out_cap() const { return fcap / 2 + 64; }                   // a level holds at most fcap live entries, and half of them are canonical
    int alloc(fmd_dev_t *h, uint64_t fc, int k)
    {
        fcap = fc; wb = fmd_kcount_work_bytes(fc);
        work.reset(); tmp.reset();
        for (int i = 0; i < 2; ++i) { key[i].reset(); val[i].reset(); }
        FMD_TRY(work.alloc(h, wb)); FMD_TRY(roots.need(4 * sizeof(fmd_intv_t))); FMD_TRY(ctr.need(KG_WORDS * 8));
        for (int i = 0; i < 2; ++i) { FMD_TRY(key[i].alloc(h, out_cap() * 8)); FMD_TRY(val[i].alloc(h, out_cap() * 8)); }
        size_t tb = 0;
        FMD_HIP_TRY(fmd_sort_pairs(nullptr, tb, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)out_cap(), 0, 2 * k));
        return tmp.alloc(h, tb ? tb : 16);
    }
};

static int kg_check(fmd_dev_t *h, int k, int min_occ, uint64_t cap)
{
    if (!h || k < 3 || k > 31 || !(k & 1) || min_occ < 1 || cap > FMD_KGRAPH_MAX_NODES) return FMD_E_ARG;
    if (h->mcnt[2] != h->mcnt[5] || h->mcnt[3] != h->mcnt[4] || (h->mcnt[1] & 1)) return FMD_E_ARG;   // kcount's test: not an index of both strands
    return FMD_OK;
}

// nodes, counts and arc bytes, sorted, on the device.  cap = the most nodes (0: FMD_KGRAPH_MAX_NODES); the frontiers are sized as kcount sizes them and
// grown after an overflow while they fit; FMD_E_NOMEM when they do not, or when there are more nodes than cap.
static int kg_arcs(fmd_dev_t *h, int k, int min_occ, uint64_t cap, KgDev &g, fmd_kgraph_stat_t *stat)
{
    memset(stat, 0, sizeof(*stat));
    g.n = 0;
    const KgClock::time_point t0 = KgClock::now();
    FMD_HIP_TRY(hipSetDevice(h->device));
    fmd_intv_t roots[4];
    size_t n_roots = 0;
    for (int c = 4; c >= 1; --c) {                    // kcount's roots: suffix T, G, C, A
        fmd_intv_t r;
        r.x[0] = h->cnt[c]; r.x[1] = h->cnt[5 - c]; r.x[2] = h->cnt[c + 1] - h->cnt[c]; r.info = (uint64_t)(c - 1);
        if (r.x[2] >= (uint64_t)min_occ) roots[n_roots++] = r;
    }
    if (n_roots == 0) return FMD_OK;                  // an empty index, or nothing that frequent
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)8 << 30;
    uint64_t fc_max = (uint64_t)(0.6 * (double)free_b) / (2 * sizeof(fmd_intv_t) + 2 * 16 + 8);
    if (fc_max > 2 * h->mcnt[0] + FMD_KCOUNT_MIN_CAP) fc_max = 2 * h->mcnt[0] + FMD_KCOUNT_MIN_CAP;
    if (fc_max > FMD_KCOUNT_MAX_CAP) fc_max = FMD_KCOUNT_MAX_CAP;
    if (fc_max < FMD_KCOUNT_MIN_CAP) fc_max = FMD_KCOUNT_MIN_CAP;
    uint64_t fc = h->mcnt[0] / 2 + (1u << 16);
    if (fc > fc_max) fc = fc_max;
    static int per_cu = 0;
    if (!per_cu) per_cu = fmd_resident_per_cu(k_kgraph_arcs, FMD_COMPACT_LDS_U4 * 16, 16, "k_kgraph_arcs");
    const FmdIndexView ix = fmd_view(h);
    unsigned long long hc[KG_WORDS], lvl[48];
    for (;;) {
        FMD_TRY(g.alloc(h, fc, k));
        unsigned long long *ctr = g.ctr.as<unsigned long long>();
        FMD_HIP_TRY(hipMemcpy(g.roots.p, roots, n_roots * sizeof(fmd_intv_t), hipMemcpyHostToDevice));
        FMD_HIP_TRY(hipMemsetAsync(ctr, 0, KG_WORDS * 8, nullptr));
        const fmd_intv_t *front = nullptr;
        int grid = 1;
        FMD_TRY(fmd_kcount_levels(h, nullptr, k, min_occ, 1, n_roots, g.roots.as<fmd_intv_t>(), fc, g.work.p, &front, &grid));
        if (grid > h->n_cu * per_cu) grid = h->n_cu * per_cu;
        if (grid >= 8) grid &= ~7;
        k_kgraph_arcs<<<grid, 64, 0, nullptr>>>(ix, k, (uint64_t)min_occ, front, fc, (const unsigned long long *)g.work.p, ctr, g.key[0].as<uint64_t>(),
                                                g.val[0].as<uint64_t>(), g.out_cap(), 1);
        FMD_CHECK_LAUNCH("kgraph arcs");
        FMD_HIP_TRY(hipMemcpy(lvl, g.work.p, sizeof(lvl), hipMemcpyDeviceToHost));
        FMD_HIP_TRY(hipMemcpy(hc, ctr, sizeof(hc), hipMemcpyDeviceToHost));
        stat->n_ext += lvl[FMD_KCOUNT_CTR_EXT] + hc[KG_EXT];
        if (!lvl[FMD_KCOUNT_CTR_OVF] && hc[KG_OUT] <= g.out_cap()) break;
        if (fc >= fc_max) return FMD_E_NOMEM;
        fc = 2 * fc < fc_max ? 2 * fc : fc_max;
    }
    const uint64_t n = hc[KG_OUT];
    if (n > (cap ? cap : (uint64_t)FMD_KGRAPH_MAX_NODES)) return FMD_E_NOMEM;
    if (n) {
        size_t tb = 0;
        FMD_HIP_TRY(fmd_sort_pairs(nullptr, tb, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)g.out_cap(), 0, 2 * k));
        FMD_HIP_TRY(fmd_sort_pairs(g.tmp.p, tb, g.key[0].as<uint64_t>(), g.key[1].as<uint64_t>(), g.val[0].as<uint64_t>(), g.val[1].as<uint64_t>(), (size_t)n, 0, 2 * k));
        k_kgraph_unpack<<<fmd_nblk(n, 256) < 4096u ? fmd_nblk(n, 256) : 4096u, 256, 0, nullptr>>>(k, n, g.kmer(), g.val[1].as<uint64_t>(), g.count(), g.arcs(),
                                                                                                   g.ctr.as<unsigned long long>());
        FMD_CHECK_LAUNCH("kgraph unpack");
        FMD_HIP_TRY(hipMemcpy(hc, g.ctr.p, sizeof(hc), hipMemcpyDeviceToHost));
    }
    g.n = n;
    stat->n_nodes = n;
    stat->n_arcs = (hc[KG_BITS] + hc[KG_PAL]) / 2;    // a (k+1)-mer sets a bit at its prefix node and one at its suffix node: the same bit when it is its own reverse complement
    stat->ms_arcs = kg_ms(t0);
    return FMD_OK;
}

static int kg_karcs(fmd_dev_t *h, int k, int min_occ, uint64_t cap, fmd_karcs_sink_fn sink, void *ctx, fmd_kgraph_stat_t *stat)
{
    if (!stat) return FMD_E_ARG;
    FMD_TRY(kg_check(h, k, min_occ, cap));
    KgDev g;
    FMD_TRY(kg_arcs(h, k, min_occ, cap, g, stat));
    if (!sink || g.n == 0) return FMD_OK;
    FmdHostBuf hk, hc, ha;
    FMD_TRY(hk.alloc((size_t)KG_SLICE * 8)); FMD_TRY(hc.alloc((size_t)KG_SLICE * 4)); FMD_TRY(ha.alloc(KG_SLICE));
    for (uint64_t at = 0; at < g.n; at += KG_SLICE) {
        const uint64_t m = g.n - at < KG_SLICE ? g.n - at : KG_SLICE;
        FMD_HIP_TRY(hipMemcpy(hk.p, g.kmer() + at, m * 8, hipMemcpyDeviceToHost));
        FMD_HIP_TRY(hipMemcpy(hc.p, g.count() + at, m * 4, hipMemcpyDeviceToHost));
        FMD_HIP_TRY(hipMemcpy(ha.p, g.arcs() + at, m, hipMemcpyDeviceToHost));
        if (sink(ctx, m, hk.as<uint64_t>(), hc.as<uint32_t>(), ha.as<uint8_t>())) return FMD_E_IO;
    }
    return FMD_OK;
}
extern "C" int fmd_karcs(fmd_dev_t *h, int k, int min_occ, uint64_t cap, fmd_karcs_sink_fn sink, void *ctx, fmd_kgraph_stat_t *stat)
{
    try { return kg_karcs(h, k, min_occ, cap, sink, ctx, stat); }
    catch (const std::bad_alloc &) { return FMD_E_NOMEM; }
}

// the doubling until a round changes nothing; rounds are enqueued four at a time (one that changes nothing leaves the states as they are)
static int kg_double(uint64_t n2, uint4 *st[2], int &cur, unsigned long long *ctr, int &round, unsigned grid)
{
    for (;;) {
        if (round + 4 > KG_MAX_ROUNDS) return FMD_E_OVERFLOW;   // (chains of fewer than 2^31 nodes settle in 32 rounds, twice for cycles: cannot happen)
        for (int j = 0; j < 4; ++j) {
            k_kgraph_round<<<grid, 256, 0, nullptr>>>(n2, st[cur], st[cur ^ 1], ctr + KG_CHG + round + j);
            cur ^= 1;
        }
        FMD_CHECK_LAUNCH("kgraph round");
        unsigned long long chg[4];
        FMD_HIP_TRY(hipMemcpy(chg, ctr + KG_CHG + round, sizeof(chg), hipMemcpyDeviceToHost));
        for (int j = 0; j < 4; ++j)
            if (!chg[j]) { round += j + 1; return FMD_OK; }
        round += 4;
    }
}

static void kg_free_out(fmd_kunitig_t *o)
{
    free(o->kmer); free(o->count); free(o->arcs); free(o->unitig); free(o->offset); free(o->orient); free(o->u_nodes); free(o->u_first); free(o->u_flags);
    memset(o, 0, sizeof(*o));
}

// (b) + (c) on sorted nodes and their arc bytes, for kgraph and kcgraph alike (fmd_internal.h)
size_t fmd_kgraph_compact_bytes(uint64_t n) { return 1024 + 6 * 256 + 2 * n * (4 + 16 + 16) + n * (4 + 4 + 1); }

int fmd_kgraph_compact_dev(int k, uint64_t n, const uint64_t *d_kmer, const uint8_t *d_arcs, const uint8_t *d_pat, void *d_work, size_t work_bytes,
                           unsigned long long *ctr, FmdKgLabels *out)
{
    const uint64_t n2 = 2 * n;
    uint8_t *w = (uint8_t *)d_work + 1024;
    auto carve = [&w](size_t bytes) { uint8_t *p = (uint8_t *)(((uintptr_t)w + 255) & ~(uintptr_t)255); w = p + bytes; return p; };
    uint32_t *mate = (uint32_t *)carve(n2 * 4);
    uint4 *sts[2] = {(uint4 *)carve(n2 * 16), (uint4 *)carve(n2 * 16)};
    uint32_t *label = (uint32_t *)carve(n * 4), *off = (uint32_t *)carve(n * 4);
    uint8_t *oc = carve(n);
    if ((size_t)(w - (uint8_t *)d_work) > work_bytes) return FMD_E_OVERFLOW;
    unsigned long long hc[KG_WORDS];
    const unsigned grid = fmd_nblk(n2, 256) < 8192u ? fmd_nblk(n2, 256) : 8192u;
    KgClock::time_point t0 = KgClock::now();
    k_kgraph_links<<<grid, 256, 0, nullptr>>>(k, n, d_kmer, d_arcs, d_pat, mate, ctr);
    FMD_CHECK_LAUNCH("kgraph links");
    FMD_HIP_TRY(hipStreamSynchronize(nullptr));
    out->ms_links = kg_ms(t0);
    t0 = KgClock::now();
    int cur = 0, round = 0;
    FMD_HIP_TRY(hipMemsetAsync(oc, 0, n, nullptr));
    k_kgraph_init<<<grid, 256, 0, nullptr>>>(n2, mate, sts[0], 0);
    FMD_TRY(kg_double(n2, sts, cur, ctr, round, grid));
    k_kgraph_cut<<<grid, 256, 0, nullptr>>>(n2, sts[cur], mate, oc, ctr);
    FMD_CHECK_LAUNCH("kgraph cut");
    FMD_HIP_TRY(hipMemcpy(hc, ctr, sizeof(hc), hipMemcpyDeviceToHost));
    if (hc[KG_CYC]) {
        k_kgraph_init<<<grid, 256, 0, nullptr>>>(n2, mate, sts[cur], 1);
        FMD_TRY(kg_double(n2, sts, cur, ctr, round, grid));
    }
    k_kgraph_final<<<grid, 256, 0, nullptr>>>(k, n, d_kmer, sts[cur], label, off, oc);
    FMD_CHECK_LAUNCH("kgraph final");
    FMD_HIP_TRY(hipStreamSynchronize(nullptr));
    out->ms_label = kg_ms(t0);
    out->n_links = hc[KG_MATES] / 2;
    out->n_cycles = hc[KG_CYC];
    out->n_rounds = (uint64_t)round;
    out->label = label; out->off = off; out->oc = oc;
    out->st = sts[cur]; out->st_spare = sts[cur ^ 1];
    return FMD_OK;
}

// labels (the smallest node of the chain; in `unitig`) -> unitig ids in the order of the labels, and the per-unitig arrays (calloc'ed here)
int fmd_kgraph_number_host(uint64_t n, uint32_t *unitig, const uint32_t *offset, uint8_t *orient, uint64_t *n_unitigs, uint32_t **u_nodes, uint32_t **u_first,
                           uint8_t **u_flags)
{
    uint64_t nu = 0;
    for (uint64_t i = 0; i < n; ++i) nu += unitig[i] == i;
    *n_unitigs = nu;
    *u_nodes = (uint32_t *)calloc(nu, 4); *u_first = (uint32_t *)malloc(nu * 4); *u_flags = (uint8_t *)calloc(nu, 1);
    if (!*u_nodes || !*u_first || !*u_flags) return FMD_E_NOMEM;
    nu = 0;
    for (uint64_t i = 0; i < n; ++i) {                // a label is the smallest node of its chain: it is met before the chain's other nodes
        const uint32_t lab = unitig[i];
        const uint32_t u = lab == i ? (uint32_t)nu++ : unitig[lab];
        unitig[i] = u;
        ++(*u_nodes)[u];
        if (offset[i] == 0) (*u_first)[u] = (uint32_t)i;
        if (orient[i] & 2) (*u_flags)[u] = FMD_KGRAPH_CYCLE;
        orient[i] &= 1;
    }
    return FMD_OK;
}

static int kg_kunitig(fmd_dev_t *h, int k, int min_occ, uint64_t cap, fmd_kunitig_t *out)
{
    FMD_TRY(kg_check(h, k, min_occ, cap));
    KgDev g;
    fmd_kgraph_stat_t st;
    FMD_TRY(kg_arcs(h, k, min_occ, cap, g, &st));
    const uint64_t n = g.n;
    out->stat = st;
    if (n == 0) return FMD_OK;
    // (b) + (c) in the work area of the walk, behind its counters: 81 n bytes and the alignment, where the frontiers had 128 n and more
    FmdKgLabels lb;
    FMD_TRY(fmd_kgraph_compact_dev(k, n, g.kmer(), g.arcs(), nullptr, g.work.p, g.wb, g.ctr.as<unsigned long long>(), &lb));   // (n <= fcap / 2 + 64, fcap >= 4096: it fits)
    out->stat.ms_links = lb.ms_links; out->stat.ms_label = lb.ms_label;
    out->stat.n_links = lb.n_links; out->stat.n_cycles = lb.n_cycles; out->stat.n_rounds = lb.n_rounds;
    out->n_nodes = n;
    out->kmer = (uint64_t *)malloc(n * 8); out->count = (uint32_t *)malloc(n * 4); out->arcs = (uint8_t *)malloc(n);
    out->unitig = (uint32_t *)malloc(n * 4); out->offset = (uint32_t *)malloc(n * 4); out->orient = (uint8_t *)malloc(n);
    if (!out->kmer || !out->count || !out->arcs || !out->unitig || !out->offset || !out->orient) return FMD_E_NOMEM;
    FMD_HIP_TRY(hipMemcpy(out->kmer, g.kmer(), n * 8, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(out->count, g.count(), n * 4, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(out->arcs, g.arcs(), n, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(out->unitig, lb.label, n * 4, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(out->offset, lb.off, n * 4, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(out->orient, lb.oc, n, hipMemcpyDeviceToHost));
    FMD_TRY(fmd_kgraph_number_host(n, out->unitig, out->offset, out->orient, &out->n_unitigs, &out->u_nodes, &out->u_first, &out->u_flags));
    out->stat.n_unitigs = out->n_unitigs;
    return FMD_OK;
}
extern "C" int fmd_kunitig(fmd_dev_t *h, int k, int min_occ, uint64_t cap, fmd_kunitig_t *out)
{
    if (!out) return FMD_E_ARG;
    memset(out, 0, sizeof(*out));
    int rc;
    try { rc = kg_kunitig(h, k, min_occ, cap, out); }
    catch (const std::bad_alloc &) { rc = FMD_E_NOMEM; }
    if (rc) kg_free_out(out);
    return rc;
}
