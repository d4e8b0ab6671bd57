// fmd_kbubble.hip -- kbubble: the simple variant bubbles of kcgraph's graph (the definitions are in include/fmd_hip.h).
//
// One more pass over the ports of the graph that fmd_kgraph_compact_dev (fmd_kgraph.hip) has just compacted and that is still on the device.  A port p =
// 2 id + o IS the oriented node that leaves through its right end, and the settled doubling state of p says where the chain of compactable links out of p
// ends (x: the oriented last node) and how many links it has (y).  A branch of a bubble is such a chain -- its first node has left degree 1, so the link
// into it is not compactable and the chain starts there; every link inside it is compactable by the branch rule --, so a fork reads its two branches in O(1):
//   (a) k_kbubble_flag: a port with exactly two right arcs resolves its two successors (the link kernel's binary search), reads the two chains, checks the
//       degrees the definition names from the arc bytes, resolves the two targets, and sets its flag byte when it is the source the bubble is reported from;
//   (b) an exclusive sum over the flag bytes: the place of every record, ascending by src whatever the order the blocks ran in;
//   (c) k_kbubble_emit: the flagged ports evaluate once more and write their record.
// The flags and the places live in the doubling's spare state buffer (32 n bytes, 10 n + 5 used).
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <new>
#include "fmd_prim.h"
#include "fmd_internal.h"
#include "fmd_kernel_common.h"
#include "fmd_level.h"

static_assert(sizeof(fmd_kbubble_t) == 24, "layout of include/fmd_hip.h");

#define KB_NONE 0xffffffffu

struct KbGraph { int k; uint32_t max_len; uint64_t n; const uint64_t *kmer; const uint8_t *arcs; const uint4 *st; };

__device__ __forceinline__ uint32_t kb_rev4(uint32_t v) { return (v & 1u) << 3 | (v & 2u) << 1 | (v & 4u) >> 1 | (v & 8u) >> 3; }

// the right arcs of the oriented node u
__device__ __forceinline__ uint32_t kb_right(const KbGraph &g, uint32_t u)
{
    const uint32_t a = g.arcs[u >> 1];
    return u & 1u ? kb_rev4(a >> 4) : a & 15u;
}

// follow(u, c): the oriented node of text(u)[1:] + c, KB_NONE when it is no node (an arc bit always has its node: never on a graph of kcgraph's)
__device__ __forceinline__ uint32_t kb_follow(const KbGraph &g, uint32_t u, uint32_t c)
{
    const uint64_t mask = ~0ull >> (64 - 2 * g.k), x = g.kmer[u >> 1], w = u & 1u ? kc_revcomp(x, g.k) : x;
    const uint64_t v = (w << 2 | (uint64_t)c) & mask, rv = kc_revcomp(v, g.k), y = v < rv ? v : rv;
    uint64_t lo = 0, hi = g.n;                        // the first j with kmer[j] >= y
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (g.kmer[mid] < y) lo = mid + 1; else hi = mid; }
    if (lo >= g.n || g.kmer[lo] != y) return KB_NONE;
    return (uint32_t)(2 * lo) + (v == y ? 0u : 1u);
}

// the branch that starts at the oriented node a: its target and its nodes, false when a starts none.  The chain of compactable links out of a ends at e =
// st[a].x.  Every node behind a has left degree 1 and every node before e right degree 1 by the link rule; a's left degree and e's right degree are checked
// here.  The link e -> t is then not compactable because t's left degree is not 1 -- t is the target -- or because t is e's own node (a hairpin; its left
// degree is 1, the branch runs back to s ^ 1 by the definition and is no bubble): the caller's test of t's left degree refuses that one too.
__device__ __forceinline__ bool kb_branch(const KbGraph &g, uint32_t a, uint32_t &t, uint32_t &len)
{
    if (a == KB_NONE || __popc(kb_right(g, a ^ 1u)) != 1) return false;
    const uint4 s = g.st[a];
    if (!s.w || (uint64_t)s.x >= 2 * g.n) return false;   // (every state is settled once the cycles are cut: cannot happen)
    const uint32_t r = kb_right(g, s.x);
    if (__popc(r) != 1) return false;
    t = kb_follow(g, s.x, (uint32_t)__ffs((int)r) - 1u);
    len = s.y + 1u;
    return t != KB_NONE;
}

// the bubble whose source is port p with the two right arcs r, when it is reported from p
__device__ __forceinline__ bool kb_eval(const KbGraph &g, uint32_t p, uint32_t r, fmd_kbubble_t &b)
{
    const uint32_t c0 = (uint32_t)__ffs((int)r) - 1u, c1 = 31u - (uint32_t)__clz((int)r);
    uint32_t t0 = 0, t1 = 0;
    b.src = p;
    b.first[0] = kb_follow(g, p, c0); b.first[1] = kb_follow(g, p, c1);
    if (!kb_branch(g, b.first[0], t0, b.len[0]) || !kb_branch(g, b.first[1], t1, b.len[1])) return false;
    if (t0 != t1 || __popc(kb_right(g, t0 ^ 1u)) != 2) return false;
    if (g.max_len && (b.len[0] > g.max_len || b.len[1] > g.max_len)) return false;
    b.dst = t0;
    return (p >> 1) < (t0 >> 1);                      // id(s) != id(t), and the one side of the two it is met from
}

// (a) flag[p] = 1 when port p is the source of a reported bubble; flag[2 n] = 0 (the scan's last place is the number of bubbles)
__global__ __launch_bounds__(256) void k_kbubble_flag(KbGraph g, uint8_t *__restrict__ flag, unsigned long long *__restrict__ n_forks)
{
    const uint64_t n2 = 2 * g.n;
    uint64_t forks = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= n2; p += (uint64_t)gridDim.x * blockDim.x) {
        uint8_t f = 0;
        if (p < n2) {
            const uint32_t r = kb_right(g, (uint32_t)p);
            if (__popc(r) == 2) {
                fmd_kbubble_t b;
                ++forks;
                f = kb_eval(g, (uint32_t)p, r, b) ? 1 : 0;
            }
        }
        flag[p] = f;
    }
    forks = km_wave_sum(forks);
    if (fmd_lane() == 0 && forks) atomicAdd(n_forks, (unsigned long long)forks);
}

// (c) the record of every flagged port at its place
__global__ __launch_bounds__(256) void k_kbubble_emit(KbGraph g, const uint8_t *__restrict__ flag, const uint32_t *__restrict__ pos, fmd_kbubble_t *__restrict__ out,
                                                      uint64_t n_out)
{
    const uint64_t n2 = 2 * g.n;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n2; p += (uint64_t)gridDim.x * blockDim.x) {
        if (!flag[p]) continue;
        fmd_kbubble_t b;
        const uint32_t at = pos[p];
        if (kb_eval(g, (uint32_t)p, kb_right(g, (uint32_t)p), b) && at < n_out) out[at] = b;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
typedef std::chrono::steady_clock KbClock;
static double kb_ms(KbClock::time_point t0) { return std::chrono::duration<double, std::milli>(KbClock::now() - t0).count(); }

struct KbWiden { __host__ __device__ uint32_t operator()(uint8_t v) const { return (uint32_t)v; } };

int fmd_kbubble_stage_dev(fmd_dev *h, int k, uint64_t n, const uint64_t *d_kmer, const uint8_t *d_arcs, const FmdKgLabels *lb, uint32_t max_len, int grid,
                          uint64_t *n_forks, uint64_t *n_bubbles, fmd_kbubble_t **bubble, double *ms)
{
    *n_forks = 0; *n_bubbles = 0; *bubble = nullptr; *ms = 0;
    if (n == 0) return FMD_OK;
    if (n > FMD_KGRAPH_MAX_NODES || grid < 0 || !lb->st || !lb->st_spare) return FMD_E_ARG;
    const KbClock::time_point t0 = KbClock::now();
    const uint64_t n2 = 2 * n;
    // the spare state buffer: 2 n + 1 places of 4 bytes, then 2 n + 1 flag bytes (10 n + 5 <= 32 n)
    uint32_t *pos = (uint32_t *)lb->st_spare;
    uint8_t *flag = (uint8_t *)(pos + n2 + 1);
    const unsigned gr = grid ? (unsigned)grid : (fmd_nblk(n2 + 1, 256) < 8192u ? fmd_nblk(n2 + 1, 256) : 8192u);
    const KbGraph g = {k, max_len, n, d_kmer, d_arcs, lb->st};
    FmdScratch ctr, tmp, rec;
    FMD_TRY(ctr.alloc(h, 16));
    FMD_HIP_TRY(hipMemsetAsync(ctr.p, 0, 16, nullptr));
    k_kbubble_flag<<<gr, 256, 0, nullptr>>>(g, flag, ctr.as<unsigned long long>());
    FMD_CHECK_LAUNCH("kbubble flag");
    const rocprim::transform_iterator<const uint8_t *, KbWiden, uint32_t> in(flag, KbWiden());
    size_t tb = 0;
    FMD_HIP_TRY(fmd_exclusive_sum(nullptr, tb, in, pos, (size_t)(n2 + 1)));
    FMD_TRY(tmp.alloc(h, tb ? tb : 16));
    FMD_HIP_TRY(fmd_exclusive_sum(tmp.p, tb, in, pos, (size_t)(n2 + 1)));
    unsigned long long forks = 0;
    uint32_t nb = 0;
    FMD_HIP_TRY(hipMemcpy(&forks, ctr.p, 8, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(&nb, pos + n2, 4, hipMemcpyDeviceToHost));
    *n_forks = forks;
    if (nb) {
        FMD_TRY(rec.alloc(h, (size_t)nb * sizeof(fmd_kbubble_t)));
        k_kbubble_emit<<<gr, 256, 0, nullptr>>>(g, flag, pos, rec.as<fmd_kbubble_t>(), nb);
        FMD_CHECK_LAUNCH("kbubble emit");
        fmd_kbubble_t *out = (fmd_kbubble_t *)malloc((size_t)nb * sizeof(fmd_kbubble_t));
        if (!out) return FMD_E_NOMEM;
        const hipError_t e = hipMemcpy(out, rec.p, (size_t)nb * sizeof(fmd_kbubble_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) { free(out); FMD_HIP_TRY(e); }
        *bubble = out; *n_bubbles = nb;
    }
    *ms = kb_ms(t0);
    return FMD_OK;
}

static int kb_kcbubble_dev(fmd_dev_t *h, int k, uint64_t n, const uint64_t *d_kmer, const uint8_t *d_uarcs, uint32_t max_len, int grid, uint64_t *n_forks,
                           uint64_t *n_bubbles, fmd_kbubble_t **bubble)
{
    if (!h || !n_forks || !n_bubbles || !bubble || k < 3 || k > 31 || !(k & 1) || n > FMD_KGRAPH_MAX_NODES || grid < 0 || (n && (!d_kmer || !d_uarcs))) return FMD_E_ARG;
    *n_forks = 0; *n_bubbles = 0; *bubble = nullptr;
    if (n == 0) return FMD_OK;
    FMD_HIP_TRY(hipSetDevice(h->device));
    const size_t wb = fmd_kgraph_compact_bytes(n);
    FmdScratch work, ctr;
    FMD_TRY(work.alloc(h, wb)); FMD_TRY(ctr.alloc(h, 128 * 8));
    FMD_HIP_TRY(hipMemsetAsync(ctr.p, 0, 128 * 8, nullptr));
    FmdKgLabels lb;
    FMD_TRY(fmd_kgraph_compact_dev(k, n, d_kmer, d_uarcs, nullptr, work.p, wb, ctr.as<unsigned long long>(), &lb));
    double ms;
    return fmd_kbubble_stage_dev(h, k, n, d_kmer, d_uarcs, &lb, max_len, grid, n_forks, n_bubbles, bubble, &ms);
}
extern "C" int fmd_kcbubble_dev(fmd_dev_t *h, int k, uint64_t n, const uint64_t *d_kmer, const uint8_t *d_uarcs, uint32_t max_len, int grid, uint64_t *n_forks,
                                uint64_t *n_bubbles, fmd_kbubble_t **bubble)
{
    try { return kb_kcbubble_dev(h, k, n, d_kmer, d_uarcs, max_len, grid, n_forks, n_bubbles, bubble); }
    catch (const std::bad_alloc &) { return FMD_E_NOMEM; }
}
