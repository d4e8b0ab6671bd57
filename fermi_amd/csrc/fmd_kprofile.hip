// fmd_kprofile.hip -- kprofile: kcount's COUNT of every k-window of the query sequences.
//
// Window j of sequence i is its bases [j, j + k); windows are numbered through all sequences (woff[i] + j) and a lane owns one.  A wave takes 64
// consecutive windows, so a wave of short sequences holds windows of several of them: it finds them by bisecting woff.  A lane's search is the plain
// backward search of k_bsearch (fmd_ops.hip) on its window -- the prefix table for the last ptab_d bases, then one rank pair per base, the whole wave in
// lockstep -- and because every window of a wave has the same k there is no queue and no refill: the wave makes exactly max(0, k - ptab_d) steps, fewer
// when every interval has emptied.  The bases come in once per wave: the windows of one sequence inside a wave are one run of at most 64 + k - 1 bytes
// (a SEGMENT), copied dword by dword, coalesced, into the wave's LDS, where a lane reads its window.  Nothing is packed: k is bounded only by the bytes a
// segment may take (FMD_KPROFILE_MAX_K).  A window with a base outside A/C/G/T counts 0 and is never searched; a window that is its own reverse
// complement -- seen from its bases -- counts half its interval.
#include <stdlib.h>
#include <string.h>
#include "fmd_internal.h"
#include "fmd_kernel_common.h"

static_assert(sizeof(fmd_kprofile_stat_t) == 40, "layout of include/fmd_hip.h");

// The bases of a wave: KP_BASE_DW dwords.  A segment lands on a dword boundary with the misalignment its bytes have in the query buffer, so it is copied in
// whole dwords and the table fold reads it as it reads the buffer: at most 3 bytes in front, 64 + k - 1 bytes, 3 behind.  A wave whose segments do
// not fit together -- many sequences of one or two windows each, a large k -- takes them in several passes; the first segment left always fits.
#define KP_BASE_DW 512
#define KP_SEG_MAX_DW ((3 + 64 + FMD_KPROFILE_MAX_K - 1 + 3) / 4)
static_assert(KP_SEG_MAX_DW <= KP_BASE_DW, "one segment fits the wave's bases");

// the sequence of window g: the i in [lo, hi) with woff[i] <= g < woff[i + 1], given woff[lo] <= g < woff[hi] (sequences without windows are passed over)
__device__ __forceinline__ uint32_t kp_seq_of(const uint64_t *__restrict__ woff, uint32_t lo, uint32_t hi, uint64_t g)
{
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (woff[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void k_kprofile(FmdIndexView ix, uint32_t n, const uint8_t *__restrict__ seqs, const uint64_t *__restrict__ off,
                                                 const uint64_t *__restrict__ woff, int k, uint32_t *__restrict__ count,
                                                 unsigned long long *__restrict__ stat)
{
    FMD_DECLARE_COMPACT_LDS();
    __shared__ uint32_t kp_dw[KP_BASE_DW];
    const uint8_t *kb = (const uint8_t *)kp_dw;
    const int lane = fmd_lane();
    const uint64_t W = woff[n];
    const int D = ix.ptab_d;
    const bool empty = ix.n_sym == 0;
    unsigned long long s_win = 0, s_valid = 0, s_hit = 0, s_ext = 0, s_tab = 0;   // wave-uniform
    for (uint64_t w0 = (uint64_t)blockIdx.x * 64; w0 < W; w0 += (uint64_t)gridDim.x * 64) {
        // ---- who holds which window: the sequences of the wave's first and last window, then each lane between them
        const uint32_t nv = W - w0 < 64 ? (uint32_t)(W - w0) : 64u;
        const uint32_t ia = kp_seq_of(woff, 0, n, w0), ib = kp_seq_of(woff, ia, n, w0 + nv - 1);
        const uint64_t g = w0 + (uint64_t)lane;
        const bool have = (uint32_t)lane < nv;
        const uint32_t i = have ? kp_seq_of(woff, ia, ib + 1, g) : ib;
        const uint64_t ga = have ? off[i] + (g - woff[i]) : 0;          // where the window begins in the query buffer
        // ---- segments: a head is the first lane of a sequence in this wave; its dwords, and where they land (a running sum over the heads)
        const uint32_t i_up = (uint32_t)__shfl_up((int)i, 1);
        const bool head = have && (lane == 0 || i != i_up);
        const uint64_t hm = __ballot(head);
        const int hl = have ? 63 - __clzll((long long)(hm & bits_below(lane + 1))) : 0;   // my head
        const uint64_t rest = lane == 63 ? 0ull : hm >> (lane + 1);
        const uint32_t nxt = rest ? (uint32_t)(lane + __ffsll((long long)rest)) : nv;        // the next head, or the end: where my segment ends
        const uint32_t nd = head ? ((uint32_t)(ga & 3) + (nxt - (uint32_t)lane) + (uint32_t)k - 1 + 3) >> 2 : 0u;
        uint32_t E = nd;                                                  // inclusive: the end of my segment, in dwords from the wave's first
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)E, d); if (lane >= d) E += t; }
        const uint32_t seg_dw = (uint32_t)__shfl((int)nd, hl), seg_at = E - seg_dw;
        const uint32_t in_seg = (uint32_t)(lane - hl) + (uint32_t)((ga - (uint64_t)(lane - hl)) & 3);   // my first base, in bytes from the segment's first dword
        uint32_t pbase = 0;                                               // dwords of the passes before this one
        bool done = !have;
        while (__ballot(!done) != 0) {
            const bool in = !done && E - pbase <= KP_BASE_DW;           // whole segments, a prefix of what is left
            // ---- the bases of this pass, once, coalesced: segment after segment, lane d takes dword d
            __syncthreads();                                              // the pass before has read its bases
            for (uint64_t mh = __ballot(in && head); mh != 0; mh &= mh - 1) {
                const int h = __ffsll((long long)mh) - 1;
                const uint64_t a = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(ga >> 32), h) << 32 | (uint32_t)__shfl((int)(uint32_t)ga, h)) & ~3ull;
                const uint32_t at = (uint32_t)__shfl((int)(seg_at - pbase), h), c = (uint32_t)__shfl((int)nd, h);
                for (uint32_t d = (uint32_t)lane; d < c; d += 64) kp_dw[at + d] = *(const uint32_t *)(seqs + a + 4ull * d);
            }
            __syncthreads();
            const uint32_t wb = in ? 4 * (seg_at - pbase) + in_seg : 0u; // my window: kb[wb .. wb + k)
            // ---- no N, and W = rc(W)?  from the bases
            bool valid = in, pal = (k & 1) == 0;
            for (int p = 0; p < k; ++p) {
                const int c = kb[wb + p];
                valid = valid && c >= 1 && c <= 4;
                if (2 * p < k) pal = pal && c + (int)kb[wb + k - 1 - p] == 5;
            }
            uint64_t size = 0;
            // ---- the start: the table for the last D bases, or the interval of the last base
            const bool tab = ix.ptab != nullptr && k >= D;
            uint64_t lo = 0, hi = 0;
            int pos = -1;
            bool live = false;
            const bool go = valid && !empty;
            if (go) {
                if (tab) {
                    uint64_t idx;
                    fmd_ptab_fold_back(kb, wb + (uint32_t)(k - D), wb + (uint32_t)k, idx);
                    const FmdPtabEntry e = fmd_ptab_unpack(ix.ptab[idx]);
                    fmd_count_lane(ix, 1, 1);
                    lo = e.k; hi = e.l; pos = k - D - 1; live = e.present;
                } else {
                    const int c = kb[wb + k - 1];
                    lo = ix.cnt[c]; hi = ix.cnt[c + 1];
                    live = hi > lo; hi -= 1; pos = k - 2;
                }
                if (live && pos < 0) { size = hi - lo + 1; live = false; }
            }
            if (tab) s_tab += (unsigned long long)__popcll(__ballot(go));
            // ---- the walk: one rank pair per base, every live lane (k_bsearch's step)
            for (;;) {
                const uint64_t ml = __ballot(live);
                if (ml == 0) break;
                s_ext += (unsigned long long)__popcll(ml);
                const int c = live ? kb[wb + pos] : 0;
                FmdRank2c r = fmd_wave_rank2_fetch_compact(ix, fmd_lds, live ? lo - 1 : NONE64, live ? hi : NONE64);
                const uint64_t ok = (live && r.hk) ? fmd_block_rank1(r.bk, r.t, r.nk, c, r.blk_k) : 0;
                fmd_wave_l_ready(ix, fmd_lds, r);
                if (live) {
                    const uint64_t ol = fmd_block_rank1(r.bl, r.tl, r.nl, c, r.blk_l);
                    lo = ix.cnt[c] + ok; hi = ix.cnt[c] + ol - 1;
                    --pos;
                    if (lo > hi) live = false;
                    else if (pos < 0) { size = hi - lo + 1; live = false; }
                }
            }
            if (pal) size >>= 1;                                          // seen once on each strand per occurrence
            if (in) count[g] = size > 0xffffffffull ? 0xffffffffu : (uint32_t)size;
            const uint64_t m_in = __ballot(in);
            s_win += (unsigned long long)__popcll(m_in);
            s_valid += (unsigned long long)__popcll(__ballot(valid));
            s_hit += (unsigned long long)__popcll(__ballot(in && size != 0));
            pbase = (uint32_t)__shfl((int)E, 63 - __clzll((long long)m_in));   // (m_in != 0: the first segment left always fits)
            done = done || in;
        }
    }
    if (stat && lane < 5) {
        const unsigned long long v = lane == 0 ? s_win : lane == 1 ? s_valid : lane == 2 ? s_hit : lane == 3 ? s_ext : s_tab;
        if (v) atomicAdd(&stat[lane], v);                                 // one atomic instruction per wave
    }
}

extern "C" int fmd_kprofile_dev(fmd_dev_t *h, void *stream, size_t n, const uint8_t *d_seqs, const uint64_t *d_off, const uint64_t *d_woff, int k,
                                unsigned flags, uint32_t *d_count, fmd_kprofile_stat_t *d_stat)
{
    if (!h || k < 1 || k > FMD_KPROFILE_MAX_K || (flags & ~FMD_KPROFILE_PLAIN)) return FMD_E_ARG;   // (one path: flags = 0 chooses it too)
    if (n && (!d_seqs || !d_off || !d_woff || !d_count)) return FMD_E_ARG;
    if (n >= 0xffffffffull || ((uintptr_t)d_seqs & 3)) return FMD_E_ARG;
    if (h->mcnt[2] != h->mcnt[5] || h->mcnt[3] != h->mcnt[4] || (h->mcnt[1] & 1)) return FMD_E_ARG;   // not an index of both strands (kcount's test)
    if (n == 0) return FMD_OK;
    FMD_HIP_TRY(hipSetDevice(h->device));
    static int per_cu = 0;
    if (!per_cu) per_cu = fmd_resident_per_cu(k_kprofile, FMD_COMPACT_LDS_U4 * 16 + KP_BASE_DW * 4, 16, "k_kprofile");
    // the number of windows is on the device (d_woff[n]): the grid is the resident set, and a wave without a chunk returns at once
    k_kprofile<<<h->n_cu * per_cu, 64, 0, S(stream)>>>(fmd_view(h), (uint32_t)n, d_seqs, d_off, d_woff, k, d_count, (unsigned long long *)d_stat);
    FMD_CHECK_LAUNCH("k_kprofile");
    return FMD_OK;
}

extern "C" int fmd_kprofile_batch(fmd_dev_t *h, size_t n, const uint8_t *seqs, const uint64_t *off, int k, unsigned flags, uint64_t *woff,
                                  uint32_t **count, fmd_kprofile_stat_t *stat)
{
    if (!h || !woff || !count || !stat || (n && (!seqs || !off))) return FMD_E_ARG;
    *count = nullptr;
    memset(stat, 0, sizeof(*stat));
    // (the argument tests of the _dev form, made before anything is written or allocated)
    if (k < 1 || k > FMD_KPROFILE_MAX_K || (flags & ~FMD_KPROFILE_PLAIN) || n >= 0xffffffffull) return FMD_E_ARG;
    if (h->mcnt[2] != h->mcnt[5] || h->mcnt[3] != h->mcnt[4] || (h->mcnt[1] & 1)) return FMD_E_ARG;
    woff[0] = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t len = off[i + 1] - off[i];
        woff[i + 1] = woff[i] + (len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0);
    }
    const uint64_t W = woff[n];
    if (n == 0 || W == 0) return FMD_OK;
    FMD_HIP_TRY(hipSetDevice(h->device));
    const size_t total = off[n];
    FmdDevBuf ds, doff, dwoff, dc, dst;
    FMD_TRY(ds.alloc(total + 8)); FMD_TRY(doff.alloc((n + 1) * 8)); FMD_TRY(dwoff.alloc((n + 1) * 8)); FMD_TRY(dc.alloc(W * 4));
    FMD_TRY(dst.alloc(sizeof(fmd_kprofile_stat_t)));
    FMD_HIP_TRY(hipMemcpy(ds.p, seqs, total, hipMemcpyHostToDevice));
    FMD_HIP_TRY(hipMemcpy(doff.p, off, (n + 1) * 8, hipMemcpyHostToDevice));
    FMD_HIP_TRY(hipMemcpy(dwoff.p, woff, (n + 1) * 8, hipMemcpyHostToDevice));
    FMD_HIP_TRY(hipMemset(dst.p, 0, sizeof(fmd_kprofile_stat_t)));
    FMD_TRY(fmd_kprofile_dev(h, nullptr, n, ds.as<uint8_t>(), doff.as<uint64_t>(), dwoff.as<uint64_t>(), k, flags, dc.as<uint32_t>(),
                             dst.as<fmd_kprofile_stat_t>()));
    uint32_t *out = (uint32_t *)malloc(W * 4);
    if (!out) return FMD_E_NOMEM;
    if (hipMemcpy(out, dc.p, W * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(stat, dst.p, sizeof(*stat), hipMemcpyDeviceToHost) != hipSuccess) {
        free(out);
        fmd_set_hip_error(hipGetLastError(), "kprofile: copy back");
        return FMD_E_HIP;
    }
    *count = out;
    return FMD_OK;
}
