// fmd_bits.h -- ranking a bit array over the rows of an index: set bits before every superblock of 4096 rows.  The merge's
// interleave and the sub-index's select read the result: per row, rank1 = pre[superblock] + popcounts inside it.
#pragma once
#include "fmd_prim.h"
#include "fmd_internal.h"

#define FMD_BITS_SB_WORDS 64                 // 64-bit words per prefix-count superblock (4096 rows)

// set bits of each superblock: one wave per superblock, a lane per word
static __global__ __launch_bounds__(64) void k_bits_sb_count(const unsigned long long *__restrict__ bits, uint64_t n_words, uint64_t n_sb,
                                                             uint64_t *__restrict__ cnt)
{
    for (uint64_t sb = blockIdx.x; sb < n_sb; sb += gridDim.x) {
        const uint64_t wd = sb * FMD_BITS_SB_WORDS + threadIdx.x;
        int c = wd < n_words ? __popcll(bits[wd]) : 0;
        for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s);
        if (threadIdx.x == 0) cnt[sb] = (uint64_t)c;
    }
}

static inline uint64_t fmd_bits_n_sb(uint64_t rows) { return ((rows + 63) / 64 + FMD_BITS_SB_WORDS - 1) / FMD_BITS_SB_WORDS; }

// work area: prefix counts (n_sb + 1) at offset 0, superblock counts (n_sb + 1), 256 bytes of alignment, the scan's temporary storage
static inline size_t fmd_bits_work_bytes(uint64_t rows)
{
    const uint64_t n_sb = fmd_bits_n_sb(rows);
    size_t b = 0;
    if (fmd_exclusive_sum(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n_sb + 1, 0) != hipSuccess) b = 0;
    return (size_t)(2 * (n_sb + 1) * 8 + 256 + b);
}

// d_work (fmd_bits_work_bytes(rows) at least) <- pre[0 .. n_sb]: set bits of d_bits before each superblock, pre[n_sb] = all of them.
// Asynchronous on `stream`.
static inline int fmd_bits_rank_dev(hipStream_t stream, const uint64_t *d_bits, uint64_t rows, void *d_work, size_t work_bytes)
{
    const uint64_t n_words = (rows + 63) / 64, n_sb = fmd_bits_n_sb(rows);
    uint64_t *pre = (uint64_t *)d_work, *cnt = pre + n_sb + 1;
    void *tmp = (void *)(((uintptr_t)(cnt + n_sb + 1) + 255) & ~(uintptr_t)255);
    size_t tmp_bytes = work_bytes - (size_t)((uint8_t *)tmp - (uint8_t *)d_work);
    FMD_HIP_TRY(hipMemsetAsync(cnt + n_sb, 0, 8, stream));
    k_bits_sb_count<<<fmd_wave_grid(n_sb), 64, 0, stream>>>((const unsigned long long *)d_bits, n_words, n_sb, cnt);
    FMD_HIP_TRY(hipGetLastError());
    FMD_HIP_TRY(fmd_exclusive_sum(tmp, tmp_bytes, (const uint64_t *)cnt, pre, (size_t)n_sb + 1, stream));
    return FMD_OK;
}
