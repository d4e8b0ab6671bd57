// fmd_ktrie.h -- the joint trie walk over N indexes, what kmat (fmd_kmat.hip) and kcgraph (fmd_kcgraph.hip) share: the frontier entry, its loads, and one
// backward extension of a node in every index whose side is live (DESIGN.md sections 26 and 28).  Device code only; N is a template parameter everywhere.
#pragma once
#include "fmd_kernel_common.h"
#include "fmd_level.h"
#include "fmd_twoside.h"

// counters at the head of the work area (u64 words): [d] = the entries of the frontier at depth d (d = root_len .. 31), then
#define KT_OUT 40        // list entries emitted (counts on when the list is full)
#define KT_OVF 41        // a frontier entry did not fit
#define KT_NKMER 42      // k-mers reported
#define KT_EXT 43        // backward extensions done: one per (node, non-empty side)
#define KT_TOTAL 44      // .. 51: the sums of their counts, per index
#define KT_PRESENT 52    // .. 59: those with c_i >= present, per index
#define KT_WORDS 60
#define KT_HDR_BYTES 512
#define KT_MIN_CHUNK 256u   // one step's children (4 x 64) fit one chunk

template <int N> struct alignas(16) KtNode { uint64_t kmer, reserved, x0[N], size[N]; };   // a frontier entry: all sizes 0 = a hole
template <int N> struct KtViews { FmdIndexView ix[N]; };
static_assert(sizeof(KtNode<1>) == 32 && sizeof(KtNode<3>) == 64 && sizeof(KtNode<8>) == 144, "16 (N + 1) bytes");

// a frontier entry as N + 1 16-byte words, and its j-th 64-bit word (j a constant once the loops are unrolled: 0 = the suffix, 2 + i = x0[i],
// 2 + N + i = size[i])
template <int N>
__device__ __forceinline__ void kt_load(const KtNode<N> *in, uint64_t i, uint64_t end, uint4 (&e)[N + 1])
{
#pragma unroll
    for (int j = 0; j <= N; ++j) e[j] = make_uint4(0, 0, 0, 0);
    if (i < end) {
        const uint4 *q = (const uint4 *)(in + i);
#pragma unroll
        for (int j = 0; j <= N; ++j) e[j] = q[j];
    }
}
template <int N>
__device__ __forceinline__ uint64_t kt_word(const uint4 (&e)[N + 1], int j)
{
    const uint4 &w = e[j >> 1];
    return (j & 1) ? (uint64_t)w.w << 32 | w.z : (uint64_t)w.y << 32 | w.x;
}

// Sides 2 P and 2 P + 1 (the second only where N has it): one backward extension per lane in each index whose side is live -> the ranks before the
// interval (tk) and the child sizes (n; 0 on a side that is not live).  kp_extend (fmd_kcmp.hip) with the indexes by number: both k-side blocks are
// posted before one wait, the l sides get a second round only where an interval does not end inside its k block.  A round in which no lane has a
// live side returns before it posts anything.
template <int N, int P>
__device__ __forceinline__ void kt_round(const KtViews<N> &v, uint4 *lds, bool act, const uint64_t (&x0)[N], const uint64_t (&sz)[N], uint64_t (&tk)[N][5],
                                         uint64_t (&n)[N][5])
{
    constexpr int A = 2 * P, B = 2 * P + 1 < N ? 2 * P + 1 : A;
    constexpr bool TWO = 2 * P + 1 < N;
    const bool acta = act && sz[A] != 0, actb = TWO && act && sz[B] != 0;
#pragma unroll
    for (int c = 1; c <= 4; ++c) { tk[A][c] = 0; n[A][c] = 0; tk[B][c] = 0; n[B][c] = 0; }
    if (__ballot(acta || actb) == 0) return;
    uint64_t ka[6], la[6], kb[6], lb[6];
    const CtSide SA = ct_side(acta, x0[A], sz[A]), SB = ct_side(actb, x0[B], sz[B]);
    __syncthreads();                                  // (one wave: a wait) the LDS reads of the round before have returned before the slots are written again
    fmd_fetch_slot<0>(v.ix[A], lds, SA.bk, SA.hk);
    if (TWO) fmd_fetch_slot<1>(v.ix[B], lds, SB.bk, SB.hk);
    fmd_fetch_wait();
    ct_ranks_k<0>(lds, SA, ka, la);
    if (TWO) ct_ranks_k<1>(lds, SB, kb, lb);
    if (__ballot(SA.lsep || (TWO && SB.lsep))) {
        __syncthreads();                              // the k-side LDS reads have returned
        fmd_fetch_slot<0>(v.ix[A], lds, SA.bl, SA.lsep);
        if (TWO) fmd_fetch_slot<1>(v.ix[B], lds, SB.bl, SB.lsep);
        fmd_fetch_wait();
        ct_ranks_l<0>(lds, SA, la);
        if (TWO) ct_ranks_l<1>(lds, SB, lb);
    }
#pragma unroll
    for (int c = 1; c <= 4; ++c) {
        tk[A][c] = ka[c]; n[A][c] = la[c] - ka[c];
        if (TWO) { tk[B][c] = kb[c]; n[B][c] = lb[c] - kb[c]; }
    }
}
template <int N>
__device__ __forceinline__ void kt_extend(const KtViews<N> &v, uint4 *lds, bool act, const uint64_t (&x0)[N], const uint64_t (&sz)[N], uint64_t (&tk)[N][5],
                                          uint64_t (&n)[N][5])
{
    kt_round<N, 0>(v, lds, act, x0, sz, tk, n);
    if constexpr (N > 2) kt_round<N, 1>(v, lds, act, x0, sz, tk, n);
    if constexpr (N > 4) kt_round<N, 2>(v, lds, act, x0, sz, tk, n);
    if constexpr (N > 6) kt_round<N, 3>(v, lds, act, x0, sz, tk, n);
}

// the entry of this iteration out of its words -> is the lane on a node (not past the end, not a hole)
template <int N>
__device__ __forceinline__ bool kt_unpack(const uint4 (&e)[N + 1], bool in_range, uint64_t &K, uint64_t (&x0)[N], uint64_t (&sz)[N])
{
    uint64_t any = 0;
    K = kt_word<N>(e, 0);
#pragma unroll
    for (int i = 0; i < N; ++i) { x0[i] = kt_word<N>(e, 2 + i); sz[i] = kt_word<N>(e, 2 + N + i); any |= sz[i]; }
    return in_range && any != 0;
}
