// fmd_merge.hip -- merging two FMD indexes on the GPU: fm_merge (merge.c:100-134) and the gap array behind it,
// fm_compute_gap_bits (merge.c:33-96).
//
// The merged BWT interleaves the two inputs: row p of the merged index comes from e0 or from e1, and a bit per row says
// which.  Every sequence x of one index (the WALKED one) is LF-walked from its sentinel row until it meets '$'; beside it
// runs the insertion row i in the OTHER index -- the last row of the other index whose suffix is smaller than the walked
// suffix -- and the walked row k lands on merged row k + i + 1, whose bit is set.  Per step: one rank in the walked index
// (symbol + LF) and one single-symbol rank in the other, two independent 64-byte blocks that the wave engine of fmd_wave.h
// gathers together.  The reference always walks e1; here the smaller index is walked (fewer steps, same merged BWT):
//   walked = e1 (e1's strings come after e0's): i starts at n$0 - 1 and never falls below 0;
//   walked = e0 (e0's strings come first):      i starts at -1 (occ(., <= -1) = 0, as rld_rank1a(e, -1) gives).
// The interleave then takes merged row p from the walked index at rank1(p) (set bits before p) when bit p is set, from
// the other index at p - rank1(p) when it is not; rank1 comes from per-4096-bit prefix counts the walk leaves in d_work.
#include <stdlib.h>
#include <string.h>
#include "fmd_kernel_common.h"
#include "fmd_bits.h"

// ------------------------------------------------------------------------------------------------ gap walk
// One lane per walked sequence (persistent waves, tickets); ~0 in `i` is row -1 of the other index.
// mark = 0 walks without setting a bit: a measurement aid (what the atomics cost) behind FMD_MERGE_TEST_HOOKS=1 FMD_MERGE_MARK=0, which
// makes every merge of the process wrong -- the product never reads FMD_MERGE_MARK without the gate (as FMD_RLD_TEST_HOOKS, rld_writer.c)
__global__ __launch_bounds__(64) void k_merge_walk(FmdIndexView w, FmdIndexView o, int walked_second, uint64_t n_tot,
                                                   unsigned long long *__restrict__ bits, uint32_t *__restrict__ queue, int mark)
{
    FMD_DECLARE_WAVE_LDS();
    const int q = fmd_lane();
    const size_t n = w.n_seq;
    uint64_t k = 0, i = NONE64;
    bool live = false, exhausted = false;
    FmdTickets tk;
    fmd_tickets_init(tk, queue);
    for (;;) {
        {
            const size_t my = fmd_tickets_take(tk, queue, !live && !exhausted);
            if (!live && !exhausted) {
                if (my < n) {
                    k = my; i = walked_second ? o.n_seq - 1 : NONE64; live = true;
                    const uint64_t p = k + i + 1;      // the sequence's sentinel row (i = ~0 wraps to k)
                    if (p < n_tot && mark) atomicOr(bits + (p >> 6), 1ull << (p & 63));
                } else exhausted = true;
            }
        }
        if (__ballot(live) == 0) break;
        // both blocks of the step in flight at once: the walked row's and the insertion row's
        uint32_t bk, ok_, bo, oo;
        fmd_split(live ? k : 0, bk, ok_);
        const bool has_o = live && i != NONE64;
        fmd_split(has_o ? i : 0, bo, oo);
        fmd_fetch_slot<0>(w, fmd_lds, bk, live);
        fmd_fetch_slot<1>(o, fmd_lds, bo, has_o);
        fmd_fetch_wait();
        if (live) {
            uint64_t r[6];
            const int c = fmd_block_rank6<true>(fmd_lds + fmd_lds_base(q, 0), fmd_chunk_xor(q), ok_ + 1, r, bk);
            if (c == 0 || c > 5) live = false;        // back at a sentinel: the sequence is done (c > 5: not an nt6 index)
            else {
                const uint64_t occ = has_o ? fmd_block_rank1(fmd_lds + fmd_lds_base(q, 1), fmd_chunk_xor(q), oo + 1, c, bo) : 0;
                k = w.cnt[c] + r[c] - 1;
                i = o.cnt[c] + occ - 1;
                const uint64_t p = k + i + 1;
                if (p < n_tot && k < w.n_sym) { if (mark) atomicOr(bits + (p >> 6), 1ull << (p & 63)); }
                else live = false;                     // (a corrupt index: never write outside the array, never walk forever)
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ interleave
// Symbol q of an index, read one 32-position plane word at a time (the caller walks q upwards).
struct MergeCursor {
    const uint4 *blocks;
    uint64_t n_sym;
    uint64_t word;   // plane word held in v (~0 = none)
    uint4 v;
    __device__ __forceinline__ int get(uint64_t q)
    {
        if (q >= n_sym) return 0;                  // (only a bit array that does not belong to these indexes gets here)
        if ((q >> 5) != word) { word = q >> 5; v = blocks[fmd_word_u4(word)]; }
        const uint32_t b = (uint32_t)q & 31;
        return (int)(((v.x >> b) & 1) | ((v.y >> b) & 1) << 1 | ((v.z >> b) & 1) << 2);
    }
};

// One wave per superblock of 64 bit words, a lane per word = 64 merged rows; rows [first, first + n) land in out.
__global__ __launch_bounds__(64) void k_merge_interleave(FmdIndexView w, FmdIndexView o, const unsigned long long *__restrict__ bits,
                                                         const uint64_t *__restrict__ pre, uint64_t n_tot, uint64_t first, uint64_t n,
                                                         uint8_t *__restrict__ out)
{
    const int q = fmd_lane();
    const uint64_t sb0 = first / (64 * FMD_BITS_SB_WORDS), sb1 = (first + n - 1) / (64 * FMD_BITS_SB_WORDS);
    for (uint64_t sb = sb0 + blockIdx.x; sb <= sb1; sb += gridDim.x) {
        const uint64_t wd = sb * FMD_BITS_SB_WORDS + q, p0 = wd * 64;
        const bool any = p0 < first + n && p0 + 64 > first;
        const uint64_t m = p0 < n_tot ? bits[wd] : 0;   // (the words before the slice count too: they are in the prefix of those in it)
        // exclusive prefix of the popcounts over the wave
        unsigned long long x = (unsigned long long)__popcll(m);
        for (int s = 1; s < 64; s <<= 1) { const unsigned long long y = __shfl_up(x, s); if (q >= s) x += y; }
        const uint64_t r = pre[sb] + x - (uint64_t)__popcll(m);   // set bits before p0
        if (!any) continue;
        MergeCursor cw{w.blocks, w.n_sym, NONE64, make_uint4(0, 0, 0, 0)}, co{o.blocks, o.n_sym, NONE64, make_uint4(0, 0, 0, 0)};
        uint64_t rw = r, ro = p0 - r;
        const uint64_t lo = first > p0 ? first - p0 : 0, hi = first + n - p0 < 64 ? first + n - p0 : 64;
        for (uint64_t j = 0; j < 64; ++j) {
            const bool from_w = (m >> j) & 1;
            if (j < lo || j >= hi) { if (from_w) ++rw; else ++ro; continue; }
            out[p0 + j - first] = (uint8_t)(from_w ? cw.get(rw++) : co.get(ro++));
        }
    }
}

// -------------------------------------------------------------------------------------------------- host side
// the walked index: the smaller one (e1 on a tie, as the reference)
static inline int merge_walked(const fmd_dev *h0, const fmd_dev *h1) { return h1->mcnt[0] <= h0->mcnt[0] ? 1 : 0; }

extern "C" size_t fmd_merge_work_bytes(uint64_t n_tot) { return fmd_bits_work_bytes(n_tot); }

static int merge_args(const fmd_dev *h0, const fmd_dev *h1)
{
    if (!h0 || !h1) return FMD_E_ARG;
    if (h0->device != h1->device) return FMD_E_ARG;
    if (h0->mcnt[0] + h1->mcnt[0] >= (1ull << 40)) return FMD_E_ARG;   // 40-bit counts of the merged index
    if (h0->mcnt[1] >= 0xffffff00ull || h1->mcnt[1] >= 0xffffff00ull) return FMD_E_ARG;   // 32-bit ticket queue
    return FMD_OK;
}

extern "C" int fmd_merge_walk_dev(fmd_dev_t *h0, fmd_dev_t *h1, void *stream, uint64_t *d_bits, void *d_work, size_t work_bytes, int *walked)
{
    int rc = merge_args(h0, h1);
    if (rc) return rc;
    const uint64_t n_tot = h0->mcnt[0] + h1->mcnt[0];
    if (!d_bits || !d_work || work_bytes < fmd_merge_work_bytes(n_tot)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h0->device));
    const int wk = merge_walked(h0, h1);
    fmd_dev *hw = wk ? h1 : h0, *ho = wk ? h0 : h1;
    uint32_t *queue = fmd_next_queue(hw, S(stream));
    const char *e = getenv("FMD_MERGE_MARK"), *on = getenv("FMD_MERGE_TEST_HOOKS");
    const int mark = !(on && atoi(on) == 1 && e && atoi(e) == 0);
    k_merge_walk<<<fmd_grid_for(hw, hw->mcnt[1]), 64, 0, S(stream)>>>(fmd_view(hw), fmd_view(ho), wk, n_tot, (unsigned long long *)d_bits, queue, mark);
    FMD_HIP_TRY(hipGetLastError());
    rc = fmd_bits_rank_dev(S(stream), d_bits, n_tot, d_work, work_bytes);
    if (rc) return rc;
    if (walked) *walked = wk;
    return FMD_OK;
}

extern "C" int fmd_merge_interleave_dev(fmd_dev_t *h0, fmd_dev_t *h1, void *stream, const uint64_t *d_bits, const void *d_work,
                                        uint64_t first, uint64_t n, uint8_t *d_out)
{
    int rc = merge_args(h0, h1);
    if (rc) return rc;
    const uint64_t n_tot = h0->mcnt[0] + h1->mcnt[0];
    if (!d_bits || !d_work || (n && !d_out) || first > n_tot || n > n_tot - first) return FMD_E_ARG;
    if (n == 0) return FMD_OK;
    FMD_HIP_TRY(hipSetDevice(h0->device));
    const int wk = merge_walked(h0, h1);
    const fmd_dev *hw = wk ? h1 : h0, *ho = wk ? h0 : h1;
    const uint64_t sb0 = first / (64 * FMD_BITS_SB_WORDS), sb1 = (first + n - 1) / (64 * FMD_BITS_SB_WORDS);
    k_merge_interleave<<<fmd_wave_grid(sb1 - sb0 + 1), 64, 0, S(stream)>>>(fmd_view(hw), fmd_view(ho), (const unsigned long long *)d_bits,
                                                                      (const uint64_t *)d_work, n_tot, first, n, d_out);
    FMD_HIP_TRY(hipGetLastError());
    return FMD_OK;
}

// ------------------------------------------------------------------------------------------- whole merge, resident
#define MERGE_SLICE (1ull << 28)
extern "C" int fmd_dev_merge_ex(fmd_dev_t *h0, fmd_dev_t *h1, unsigned flags, fmd_dev_t **out)
{
    int rc = merge_args(h0, h1);
    if (rc) return rc;
    if (!out || (flags & ~FMD_OPEN_NO_TABLES)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h0->device));
    const uint64_t n_tot = h0->mcnt[0] + h1->mcnt[0], n_words = (n_tot + 63) / 64;
    const size_t wb = fmd_merge_work_bytes(n_tot);
    const uint64_t slice = n_tot < MERGE_SLICE ? n_tot : MERGE_SLICE;
    FmdDevBuf bits, work, buf;
    fmd_dev *h = nullptr;
    hipStream_t st = nullptr;
    if ((rc = bits.alloc(n_words * 8)) || (rc = work.alloc(wb)) || (rc = buf.alloc(slice))) return rc;
    if (hipMemsetAsync(bits.p, 0, n_words * 8, st) != hipSuccess) return FMD_E_HIP;
    rc = fmd_merge_walk_dev(h0, h1, st, bits.as<uint64_t>(), work.p, wb, nullptr);
    if (rc) return rc;
    rc = fmd_index_alloc(h0->device, n_tot, &h);
    if (rc) return rc;
    for (uint64_t at = 0; at < n_tot && rc == FMD_OK; at += slice) {
        const uint64_t m = n_tot - at < slice ? n_tot - at : slice;
        rc = fmd_merge_interleave_dev(h0, h1, st, bits.as<uint64_t>(), work.p, at, m, buf.as<uint8_t>());
        if (rc == FMD_OK) rc = fmd_index_put_slice(h, st, buf.as<uint8_t>(), at, m);
    }
    if (rc == FMD_OK) {
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) { fmd_set_hip_error(e, "merge"); rc = FMD_E_HIP; }
    }
    buf.reset(); work.reset(); bits.reset();   // the merge's own arrays go before the counts' scratch comes
    if (rc == FMD_OK) rc = fmd_index_finish(h, !(flags & FMD_OPEN_NO_TABLES));
    if (rc) { fmd_dev_close(h); return rc; }
    *out = h;
    return FMD_OK;
}
extern "C" int fmd_dev_merge(fmd_dev_t *h0, fmd_dev_t *h1, fmd_dev_t **out) { return fmd_dev_merge_ex(h0, h1, 0, out); }
