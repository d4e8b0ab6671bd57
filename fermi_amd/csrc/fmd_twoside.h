// fmd_twoside.h -- one side of a backward extension whose block image lies in a dense LDS slot, for the walks that extend in TWO indexes per lane
// with both blocks in flight together (contrast, fmd_contrast.hip; kcmp, fmd_kcmp.hip).
#pragma once
#include "fmd_kernel_common.h"

__device__ __forceinline__ uint4 ct_pack(uint64_t a, uint64_t b) { return make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)); }

// ------------------------------------------------------------------------------------------------ one side of a backward extension
// The two ends of [x0, x0 + sz) as a rank pair (x0 - 1, x0 - 1 + sz): the block of the k side first; the l side is read from the same
// image whenever that (overlapped) block reaches it, else from a block of its own in a second round (lsep).
struct CtSide { uint32_t bk, ok, bl, ol; bool hk, hl, lsep; };

__device__ __forceinline__ CtSide ct_side(bool act, uint64_t x0, uint64_t sz)
{
    CtSide s;
    const uint64_t k = act ? x0 - 1 : NONE64, l = act ? x0 - 1 + sz : NONE64;   // x0 = 0: no k side, every count before it is 0
    s.hk = k != NONE64; s.hl = l != NONE64;
    fmd_split(s.hk ? k : 0, s.bk, s.ok); fmd_split(s.hl ? l : 0, s.bl, s.ol);
    fmd_l_from_k(s.hk && s.hl, l, s.bk, s.bl, s.ol);
    s.lsep = s.hl && !(s.hk && s.bk == s.bl);
    return s;
}
template <int SLOT>
__device__ __forceinline__ void ct_ranks_k(const uint4 *lds, const CtSide &s, uint64_t tk[6], uint64_t tl[6])
{
    const int q = fmd_lane();
#pragma unroll
    for (int c = 0; c < 6; ++c) { tk[c] = 0; tl[c] = 0; }
    if (s.hk) fmd_block_rank6<false>(lds + fmd_lds_base(q, SLOT), fmd_chunk_xor(q), s.ok + 1, tk, s.bk);
    if (s.hl && !s.lsep) fmd_block_rank6<false>(lds + fmd_lds_base(q, SLOT), fmd_chunk_xor(q), s.ol + 1, tl, s.bk);
}
template <int SLOT>
__device__ __forceinline__ void ct_ranks_l(const uint4 *lds, const CtSide &s, uint64_t tl[6])
{
    const int q = fmd_lane();
    if (s.lsep) fmd_block_rank6<false>(lds + fmd_lds_base(q, SLOT), fmd_chunk_xor(q), s.ol + 1, tl, s.bl);
}
