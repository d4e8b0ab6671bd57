// fmd_multi.hip -- fm_multi_backward_search (exact.c:25-57): backward search over SEVERAL FMD indexes at once, the SA interval of the merged index
// from the parts alone, and its C-ABI entry points (include/fmd_hip.h).
//
// The merged index's suffix array interleaves the parts' suffixes in order, so the rows of the merged index below a string W are the sum over the
// parts of the rows below W in each: with [k_j, l_j) the interval of W in part j (l exclusive, exact.c:35-36) -- or, where part j does not hold W,
// k_j = l_j = the INSERTION POINT, the row W would sort to -- the merged interval is [sum k_j, sum l_j).  A backward step by c takes both ends through
// LF in every part; an end that has become an insertion point is one rank (exact.c:48) and stays one: rank_c(k - 1) of a row count is the row count of
// c W below it, whether c W occurs or not.
//
// Kernel: the persistent waves and ticketed refill of k_bsearch (fmd_ops.hip); a lane owns one query and, for it, the (k_j, l_j) of ALL parts.
//   - State: registers.  The kernel is compiled for 1, 2, 4, 8 and FMD_MULTI_MAX = 16 parts with the loop over the parts unrolled, so k[j] and l[j] are
//     named registers (4 per part: 64 VGPRs at 16 parts), never an indexed array.  In LDS the same state is 16 KiB per wave at 16 parts -- twice the
//     landing area of the rank engine, a third of the waves a CU holds -- and two ds_read_b64 + two ds_write_b64 per part and step.
//   - `done` is not stored: part j is done exactly when k_j == l_j.  A step keeps an empty interval empty, whichever of the two forms takes it
//     (rank21 of (k - 1, k - 1) is rank11 twice), so the flag of exact.c:47 is sticky by construction.
//   - The rank engine is wave-cooperative on ONE index (fmd_wave.h): the parts take turns, view j wave-uniform, read from a device array with scalar
//     loads.  Two landing areas (dense slot + pool each, 2 x 8.25 KiB): the gathers of two parts are in flight before one wait.
//   - cnt_j[c] is per lane (c is the lane's base): the C arrays of all parts sit in LDS, 64 bytes per part.
//   - Prefix tables: a search starts ptab_d bases in only when every part has a table of that one depth AND the entry is present in every part -- an
//     absent entry is {1, 0} (k_ptab_level) and says nothing about where the string would sort.  Otherwise it starts from the last base.
//   - Two-base blocks on a handle are not used.
#include <stdlib.h>
#include <string.h>
#include "fmd_kernel_common.h"

static_assert(FMD_POOL_BLOCKS >= 64, "the pool takes the l side of every lane: no two-phase step here");

struct FmdMultiView {            // what the kernel needs of one part; d_work holds n_idx of them
    const uint4 *blocks;
    const uint4 *ptab;
    unsigned long long *stat;
    uint64_t cnt[7];
};

__global__ void k_multi_put_view(FmdMultiView v, FmdMultiView *__restrict__ dst)
{
    if (threadIdx.x == 0) *dst = v;
}

template <int NI>
__global__ __launch_bounds__(64) void k_multi_bsearch(const FmdMultiView *__restrict__ views, int n_idx, int tab_d, size_t n,
                                                      const uint8_t *__restrict__ seqs, const uint64_t *__restrict__ off,
                                                      uint64_t *__restrict__ d_cnt, uint64_t *__restrict__ d_beg, uint64_t *__restrict__ d_end,
                                                      uint32_t *__restrict__ queue)
{
    constexpr int B = NI > 1 ? 2 : 1;                       // parts whose gathers share a wait
    __shared__ uint4 fmd_lds[B * FMD_COMPACT_LDS_U4];
    __shared__ uint64_t cnt_lds[NI * 8];                    // cnt_j[c] at [8 j + c]; zeros for j >= n_idx: such a part is empty at row 0 for ever
    const int lane = fmd_lane();
    for (int i = lane; i < NI * 8; i += 64) {
        const int j = i >> 3, c = i & 7;
        cnt_lds[i] = (j < n_idx && c < 7) ? views[j].cnt[c] : 0;
    }
    __syncthreads();

    size_t rid = (size_t)-1;
    uint64_t sbase = 0;
    int pos = -1;
    uint64_t k[NI], l[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) k[j] = l[j] = 0;
    FmdReadWindow cq;                                       // the 16 bases around pos, nothing above pos (fmd_search.h)
    const FmdHitOut out = {d_cnt, d_beg, d_end};
    bool live = false, exhausted = false;

    FmdTickets tk_;
    fmd_tickets_init(tk_, queue, 64, n);
    for (;;) {
        // ---- refill finished lanes from the queue
        {
            const size_t my = fmd_tickets_take(tk_, queue, !live && !exhausted, n);
            if (!live && !exhausted) {
                if (my < n) {
                    rid = my; sbase = off[my];
                    const int len = (int)(off[my + 1] - sbase);
                    if (len <= 0) out.miss(my);
                    else {
                        bool from_table = false;
                        uint64_t idx;
                        if (tab_d > 0 && len >= tab_d && fmd_ptab_fold_back(seqs, sbase + (uint64_t)(len - tab_d), sbase + (uint64_t)len, idx)) {
                            from_table = true;          // (if every part holds the string: the intervals are the walk's after tab_d bases)
#pragma unroll
                            for (int j = 0; j < NI; ++j)
                                if (j < n_idx) {
                                    const FmdPtabEntry e = fmd_ptab_unpack(views[j].ptab[idx]);
                                    { FmdIndexView t_; t_.stat = views[j].stat; fmd_count_lane(t_, 1, 1); }
                                    k[j] = e.k; l[j] = e.l + 1;
                                    from_table = from_table && e.present;
                                }
                            pos = len - tab_d - 1;
                        }
                        if (!from_table) {
                            int c = seqs[sbase + len - 1];
                            c = c > 5 ? 5 : c;
#pragma unroll
                            for (int j = 0; j < NI; ++j) { k[j] = cnt_lds[8 * j + c]; l[j] = cnt_lds[8 * j + c + 1]; }
                            pos = len - 2;
                        }
                        bool empty = true;
#pragma unroll
                        for (int j = 0; j < NI; ++j) empty = empty && k[j] == l[j];
                        if (empty) out.miss(my);                    // no part holds the last base
                        else {
                            live = true;
                            if (pos >= 0) cq.load(seqs, sbase + pos, sbase + pos);
                        }
                    }
                } else exhausted = true;
            }
        }
        if (__ballot(live) == 0) { if (__ballot(!exhausted) == 0) break; else continue; }

        // ---- retire lanes that have consumed their whole query, then one backward step for the others
        bool fin = live && pos < 0;
        int c = 0;
        if (live && !fin) {
            c = cq.base(sbase + pos);
            c = c > 5 ? 5 : c;
        }
        const bool step = live && !fin;
#pragma unroll
        for (int j0 = 0; j0 < NI; j0 += B) {
            if (j0 < n_idx) {                                       // wave-uniform
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the images of the parts before have been read
                FmdIndexView ix0, ix1;
                FmdRank2c r0, r1;
                ix0.blocks = views[j0].blocks; ix0.stat = views[j0].stat;
                // part j: rank21(k - 1, l - 1, c) while its interval is not empty, rank11(k - 1, c) once it is; k = 0: k - 1 is "none" and ranks to 0
                r0 = fmd_wave_rank2_post_compact(ix0, fmd_lds, step ? k[j0] - 1 : NONE64, step && k[j0] != l[j0] ? l[j0] - 1 : NONE64);
                const bool two = B == 2 && j0 + 1 < n_idx;
                if (two) {
                    const int j1 = j0 + 1 < NI ? j0 + 1 : j0;
                    ix1.blocks = views[j1].blocks; ix1.stat = views[j1].stat;
                    r1 = fmd_wave_rank2_post_compact(ix1, fmd_lds + (B - 1) * FMD_COMPACT_LDS_U4, step ? k[j1] - 1 : NONE64, step && k[j1] != l[j1] ? l[j1] - 1 : NONE64);
                }
                fmd_fetch_wait();
                if (step) {
                    const uint64_t ok = r0.hk ? fmd_block_rank1(r0.bk, r0.t, r0.nk, c, r0.blk_k) : 0;
                    const uint64_t ol = r0.hl ? fmd_block_rank1(r0.bl, r0.tl, r0.nl, c, r0.blk_l) : ok;
                    const uint64_t cb = cnt_lds[8 * j0 + c];
                    k[j0] = cb + ok; l[j0] = cb + ol;
                }
                if (two && step) {
                    const int j1 = j0 + 1 < NI ? j0 + 1 : j0;
                    const uint64_t ok = r1.hk ? fmd_block_rank1(r1.bk, r1.t, r1.nk, c, r1.blk_k) : 0;
                    const uint64_t ol = r1.hl ? fmd_block_rank1(r1.bl, r1.tl, r1.nl, c, r1.blk_l) : ok;
                    const uint64_t cb = cnt_lds[8 * j1 + c];
                    k[j1] = cb + ok; l[j1] = cb + ol;
                }
            }
        }
        if (live) {
            if (step) --pos;
            uint64_t sk = 0, sl = 0;
            bool empty = true;
#pragma unroll
            for (int j = 0; j < NI; ++j) { sk += k[j]; sl += l[j]; empty = empty && k[j] == l[j]; }
            if (empty) { out.miss(rid); live = false; }              // empty in every part: the search ends at once (exact.c:50)
            else if (pos < 0) { out.store(rid, sk, sl - 1); live = false; }   // exact.c:53-56 (not empty: sl > sk)
            else if (step && ((sbase + pos) & 15) == 15) cq.load(seqs, sbase + pos, sbase + pos);
        }
    }
}

// ------------------------------------------------------------------------------- host entry
static int multi_check(int n_idx, fmd_dev_t *const *h)
{
    if (n_idx < 1 || n_idx > FMD_MULTI_MAX || !h) return FMD_E_ARG;
    for (int j = 0; j < n_idx; ++j)
        if (!h[j] || h[j]->device != h[0]->device) return FMD_E_ARG;
    return FMD_OK;
}

extern "C" size_t fmd_multi_bsearch_work_bytes(int n_idx, size_t n)
{
    (void)n;                                                          // (the area holds the views; nothing in it grows with the queries)
    if (n_idx < 1 || n_idx > FMD_MULTI_MAX) return 0;
    return ((size_t)n_idx * sizeof(FmdMultiView) + 255) & ~(size_t)255;
}

template <int NI>
static void multi_launch(fmd_dev_t *h0, hipStream_t st, const FmdMultiView *views, int n_idx, int tab_d, size_t n, const uint8_t *d_seqs, const uint64_t *d_off,
                         uint64_t *d_cnt, uint64_t *d_beg, uint64_t *d_end, uint32_t *q)
{
    const size_t lds = (size_t)(NI > 1 ? 2 : 1) * FMD_COMPACT_LDS_U4 * 16 + (size_t)NI * 64;
    k_multi_bsearch<NI><<<fmd_grid_for_lds(h0, n, lds), 64, 0, st>>>(views, n_idx, tab_d, n, d_seqs, d_off, d_cnt, d_beg, d_end, q);
}

extern "C" int fmd_multi_bsearch_dev(int n_idx, fmd_dev_t *const *h, void *stream, size_t n, const uint8_t *d_seqs, const uint64_t *d_off,
                                     uint64_t *d_cnt, uint64_t *d_beg, uint64_t *d_end, void *d_work, size_t work_bytes)
{
    FMD_TRY(multi_check(n_idx, h));
    if (n == 0) return FMD_OK;
    if (!d_seqs || !d_off || !d_cnt || !d_beg || !d_end || !d_work || work_bytes < fmd_multi_bsearch_work_bytes(n_idx, n)) return FMD_E_ARG;
    if (((uintptr_t)d_seqs & 3) || ((uintptr_t)d_work & 15)) return FMD_E_ARG;
    if (n >= 0xffffff00ull) return FMD_E_ARG; // 32-bit queue head
    FMD_HIP_TRY(hipSetDevice(h[0]->device));
    FmdMultiView *views = (FmdMultiView *)d_work;
    int tab_d = h[0]->ptab ? h[0]->ptab_d : 0;                        // the one depth of all tables, 0 = no table start
    for (int j = 0; j < n_idx; ++j) {
        FmdMultiView v;
        v.blocks = h[j]->blocks; v.ptab = h[j]->ptab; v.stat = h[j]->stat;
        for (int c = 0; c < 7; ++c) v.cnt[c] = h[j]->cnt[c];
        if (!h[j]->ptab || h[j]->ptab_d != tab_d) tab_d = 0;
        k_multi_put_view<<<1, 64, 0, S(stream)>>>(v, views + j);      // (by value through the launch: nothing of the host's is read after the return)
    }
    uint32_t *q = fmd_next_queue(h[0], S(stream));
    if (n_idx == 1) multi_launch<1>(h[0], S(stream), views, n_idx, tab_d, n, d_seqs, d_off, d_cnt, d_beg, d_end, q);
    else if (n_idx == 2) multi_launch<2>(h[0], S(stream), views, n_idx, tab_d, n, d_seqs, d_off, d_cnt, d_beg, d_end, q);
    else if (n_idx <= 4) multi_launch<4>(h[0], S(stream), views, n_idx, tab_d, n, d_seqs, d_off, d_cnt, d_beg, d_end, q);
    else if (n_idx <= 8) multi_launch<8>(h[0], S(stream), views, n_idx, tab_d, n, d_seqs, d_off, d_cnt, d_beg, d_end, q);
    else multi_launch<FMD_MULTI_MAX>(h[0], S(stream), views, n_idx, tab_d, n, d_seqs, d_off, d_cnt, d_beg, d_end, q);
    FMD_CHECK_LAUNCH("kernel launch");
    return FMD_OK;
}

extern "C" int fmd_multi_bsearch_batch(int n_idx, fmd_dev_t *const *h, size_t n, const uint8_t *seqs, const uint64_t *off,
                                       uint64_t *cnt, uint64_t *beg, uint64_t *end)
{
    FMD_TRY(multi_check(n_idx, h));
    if (n == 0) return FMD_OK;
    if (!seqs || !off || !cnt || !beg || !end) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h[0]->device));
    const size_t total = off[n], wb = fmd_multi_bsearch_work_bytes(n_idx, n);
    FmdDevBuf ds, doff, dc, dbg, den, dw;
    FMD_TRY(ds.alloc(total + 8)); FMD_TRY(doff.alloc((n + 1) * 8)); FMD_TRY(dc.alloc(n * 8)); FMD_TRY(dbg.alloc(n * 8)); FMD_TRY(den.alloc(n * 8)); FMD_TRY(dw.alloc(wb));
    FMD_HIP_TRY(hipMemcpy(ds.p, seqs, total, hipMemcpyHostToDevice));
    FMD_HIP_TRY(hipMemcpy(doff.p, off, (n + 1) * 8, hipMemcpyHostToDevice));
    FMD_TRY(fmd_multi_bsearch_dev(n_idx, h, nullptr, n, (uint8_t *)ds.p, (uint64_t *)doff.p, (uint64_t *)dc.p, (uint64_t *)dbg.p, (uint64_t *)den.p, dw.p, wb));
    FMD_HIP_TRY(hipMemcpy(cnt, dc.p, n * 8, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(beg, dbg.p, n * 8, hipMemcpyDeviceToHost));
    FMD_HIP_TRY(hipMemcpy(end, den.p, n * 8, hipMemcpyDeviceToHost));
    return FMD_OK;
}
