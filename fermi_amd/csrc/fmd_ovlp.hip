// fmd_ovlp.hip -- all-vs-all overlap discovery for unitig construction: the read-only front half
// of unitig1 (unitig.c:274-300) for a batch of sequence ids, one lane per read-strand:
//     fm_retrieve (exact.c:59)  ->  fm6_is_contained / overlap_intv (unitig.c:38-91)
//                               ->  fm6_get_nei (unitig.c:93-179, used = sorted = NULL)
// Phase-uniform persistent kernels on the wave engine (fmd_wave.h): the fused LF-walk + overlap_intv (k_ovl_walk, fmd_ovlp_walk.hip), then fm6_get_nei by
// group kernels (fmd_ovlp_grp.hip, fmd_ovlp_lane.hip) and, for what they set aside, one lane per strand (k_ovl_nei, fmd_ovlp_nei.hip); candidate interval lists
// travel between the phases through an HBM work area.  Every lane free-runs its own search and posts one rank2a request per wave step; finished lanes refill
// from a queue.  This file: the buffers of a batch, the two phases, the pipe, the work-area layouts and every entry point.
#include <stdlib.h>
#include <string.h>
#include "fmd_ovlp_internal.h"

// Work area of one batch of n strands (fmd_ovlp_dev and everything that shares its area): the stash (stride_r bytes per strand, the sequence's last base
// first), two candidate lists of cap entries per strand (listA: the walk's candidates; listB: scratch of get_nei), and the work lists of get_nei -- per strand
// the words of fmd_cls_part_off, and a header + reserve for each of the FMD_OVLP_MAX_PARTS parts a batch may be cut into.
struct BatchLayout { size_t srev, listA, listB, cls, total; uint32_t stride_r, cap; };
static BatchLayout batch_layout(size_t n, uint32_t max_len, int min_match)
{
    BatchLayout L;
    const size_t stride_r = align_up((size_t)max_len, 16), cap = fmd_ovlp_list_cap(max_len, min_match);
    L.stride_r = (uint32_t)stride_r; L.cap = (uint32_t)cap;
    size_t o = 0;
    L.srev = o; o += align_up(n * stride_r, 256);
    L.listA = o; o += align_up(n * cap * sizeof(fmd_intv_t), 256);
    L.listB = o; o += align_up(n * cap * sizeof(fmd_intv_t), 256);
    L.cls = o; o += align_up(4 * fmd_cls_part_off(FMD_OVLP_MAX_PARTS, n), 256) + 256;
    L.total = o;
    return L;
}
extern "C" size_t fmd_ovlp_work_bytes(size_t n, uint32_t max_len, int min_match) { return batch_layout(n, max_len, min_match).total; }

// The buffers of one fmd_ovlp_dev call; the two phases below work on the strands [b, b + np) of it.
struct OvlBatch {
    fmd_dev *h; FmdIndexView ix;
    const uint64_t *ids; int min_match; uint32_t max_len, max_nei, stride_r, cap, seq_stride;
    uint8_t *srev; fmd_intv_t *listA, *listB; uint32_t *cls;
    fmd_ovlp_rec_t *rec; fmd_intv_t *nei; uint8_t *seq;
    // a batch taken from the sorted order of a larger job (fmd_ovlp_sorted_dev): slot t of the batch is row gidx[t] of rec, nei, seq and of
    // park, where WALK_HEAD left it; nullptr: slot = row, the walk starts at the sentinel of ids[t]
    const uint32_t *gidx; FmdWalkPark *park;
    const uint32_t *keys;   // ... and, where the caller has them, the sort key of every slot (k_ovl_park_keys); nullptr otherwise
    // the work area of the batch: `area` laid out for `n_area` strands (the batch itself, or the largest batch of a sorted job)
    void carve(uint8_t *area, size_t n_area)
    {
        const BatchLayout L = batch_layout(n_area, max_len, min_match);
        stride_r = L.stride_r; cap = L.cap;
        srev = area + L.srev; listA = (fmd_intv_t *)(area + L.listA); listB = (fmd_intv_t *)(area + L.listB); cls = (uint32_t *)(area + L.cls);
    }
};

// The second pass of a sorted job through k_ovl_walk<WALK_TAIL2> (rows written by the walk, FMD_WALK_TAIL2=0: the A/B switch), and with the work
// lists of get_nei made by the walk as well (FMD_WALK_CLS=0: k_ovl_classify behind it as before)?
static bool ovl_tail2(const OvlBatch &o)
{
    const char *e = getenv("FMD_WALK_TAIL2");
    return o.gidx && fmd_walk_tail2_fits(o.stride_r, o.seq_stride) && !(e && atoi(e) == 0);
}
static bool ovl_tail2_cls(const OvlBatch &o)
{
    const char *e = getenv("FMD_WALK_CLS");
    return ovl_tail2(o) && !(e && atoi(e) == 0);
}
static int ovl_use_fast(void) { const char *ef = getenv("FMD_OVLP_FAST"); return fmd_nei_fast_available() && !(ef && atoi(ef) == 0); }   // FMD_OVLP_FAST=0: A/B switch, every strand through the general group kernels
static int ovl_grp_down(void) { const char *e = getenv("FMD_GRP_DOWN"); return !(e && atoi(e) == 0); }
static int ovl_walk_phase(void) { const char *e = getenv("FMD_WALK_PHASE"); return !(e && atoi(e) == 0); }
static int ovl_min_cls(void) { const char *e = getenv("FMD_GRP4"); return e && atoi(e) == 0 ? 1 : 0; }                                  // the smallest group class in use; FMD_GRP4=0: A/B knob, no groups of 4 (round 3's classes)

// phase A: LF-walk + overlap_intv + fm6_is_contained, then the read-order copy.  per_cu > 0 bounds the
// resident waves per CU (pipelined batches leave room for phase B of the previous part).
static void ovl_phase_a(const OvlBatch &o, hipStream_t st, size_t b, size_t np, int per_cu)
{
    WalkArgs a;
    a.ix = o.ix; a.n = np; a.min_match = o.min_match; a.stride_r = o.stride_r;
    a.listA = o.listA + b * (size_t)o.cap; a.cap = o.cap;
    uint8_t *srev = o.srev + b * (size_t)o.stride_r;
    if (!o.gidx) {   // the one-pass walk from the sentinel of ids[t], rows in batch order
        a.ids = o.ids + b; a.rec = o.rec + b; a.srev = srev;
        fmd_launch_walk_whole(o.h, st, a, o.max_len, o.seq + b * (size_t)o.seq_stride, o.seq_stride, per_cu, 64);
        return;
    }
    // the second pass of a sorted job: every strand of the batch from where WALK_HEAD parked it
    a.rec = o.rec; a.park = o.park; a.gidx = o.gidx + b;
    if (!ovl_tail2(o)) {
        a.srev = srev;
        fmd_launch_walk_tail(o.h, st, a, o.max_len, o.seq, o.seq_stride, per_cu);
        return;
    }
    // sequences of at most WALK_LS_BASES bases: the rows in read order come from the walk itself (bases in LDS, no stash in HBM, no k_ovl_seq_out).
    // The stash area, idle then, holds the list of the strands with an N.
    a.seq_out = o.seq; a.seq_stride = o.seq_stride; a.redo = (uint32_t *)srev;
    if (ovl_tail2_cls(o)) {   // the work lists of phase B made here (part 0 of the batch: a sorted job's batches are not pipelined)
        a.cls = o.cls + fmd_cls_part_off(0, b); a.use_fast = ovl_use_fast(); a.min_cls = ovl_min_cls();
    }
    // the strands of one minimizer in phase on the genome (k_ovl_walk<WALK_TAIL2>; FMD_WALK_PHASE=0: the A/B switch, free-running admission)
    if (o.keys && ovl_walk_phase()) a.keys = o.keys + b;
    fmd_launch_walk_tail2(o.h, st, a, per_cu);
}

// phase B: fm6_get_nei.  `part` selects the area of this part's work lists.
static int ovl_phase_b(const OvlBatch &o, hipStream_t st, size_t b, size_t np, int part, int per_cu, int fast_cu)
{
    NeiArgs a;
    a.ix = o.ix; a.n_cu = o.h->n_cu; a.grid = fmd_grid_for(o.h, np); a.np = np; a.min_match = o.min_match;
    a.srev = o.srev + b * (size_t)o.stride_r; a.stride_r = o.stride_r;
    a.listA = o.listA + b * (size_t)o.cap; a.listB = o.listB + b * (size_t)o.cap; a.cap = o.cap;
    a.gidx = o.gidx ? o.gidx + b : nullptr;
    a.rec = a.gidx ? o.rec : o.rec + b;
    a.nei = a.gidx ? o.nei : o.nei + b * (size_t)o.max_nei; a.max_nei = o.max_nei;
    a.seq = a.gidx ? o.seq : o.seq + b * (size_t)o.seq_stride; a.seq_stride = o.seq_stride;
    uint32_t *q2 = fmd_next_queue(o.h, st);
    uint32_t *cls = o.cls + fmd_cls_part_off(part, b);
    fmd_nei_lists_at(a, cls, np);
    const int use_fast = ovl_use_fast();
    if (!(part == 0 && ovl_tail2_cls(o))) {   // (else: k_ovl_walk<WALK_TAIL2> has zeroed the header and filled the lists)
        FMD_HIP_TRY(hipMemsetAsync(cls, 0, 4 * FMD_CLS_HEADER_U32, st));
        fmd_launch_classify(a, st, use_fast, ovl_min_cls());
    }
    // what classification sets aside (more than 32 candidates, a candidate wider than 63) goes through the lane-per-strand kernel NOW, on a
    // side stream beside the group kernels: it is a handful of long dependent chains (10 ms per 2*10^7 strands of raw reads for 1 % of
    // them), latency from end to end
    bool side = false;
    FmdSideStream &slow = o.h->slow;
    if (slow.acquire(2)) {
        side = hipEventRecord(slow.ev[0], st) == hipSuccess && hipStreamWaitEvent(slow.stream, slow.ev[0], 0) == hipSuccess;
        if (!side) { (void)hipGetLastError(); slow.release(); }
    }
    {
        hipStream_t ss = side ? slow.stream : st;
        fmd_launch_nei_slow(a, ss, fmd_next_queue(o.h, ss), 0);
    }
    // strands whose candidates the walk left in the narrow form: the unforked path (one lane per candidate, no x[0]-side fetch,
    // one shared window per strand and round); whatever turns out not to be that simple moves on to the general list of its class
    if (use_fast)
        for (int k = 0; k < 2 * FMD_GRP_CLASSES; ++k) {
            const int kg = k % FMD_GRP_CLASSES, wide = k >= FMD_GRP_CLASSES;
            // one lane per STRAND where its candidates fit a lane's registers (fmd_ovlp_lane.hip), one lane per candidate otherwise (FMD_NEI_LANE=0: always)
            if (fmd_nei_lane_enabled() && fmd_nei_lane_class_ok(kg, wide)) fmd_launch_nei_lane(a, kg, wide, fast_cu, st);
            else fmd_launch_nei_fast(a, kg, wide, fast_cu, st);
        }
    // one lane per candidate interval, 64 / G strands per wave
    // (second pass: the strands a group kernel moved to a smaller group when their candidates had died down to single reads -- reads with errors --, largest class first:
    // a strand may move again; their lists live where the fast lists were.  FMD_GRP_DOWN=0: the A/B switch, every strand stays in the group it was admitted to)
    const uint32_t down_cap = ovl_grp_down() && np > 2 * (size_t)FMD_FAST_CHUNK ? (uint32_t)np : 0u;
    for (int k = 0; k < FMD_GRP_CLASSES; ++k) fmd_launch_nei_grp(a, k, per_cu, st, down_cap, 0);
    if (down_cap)
        for (int k = FMD_GRP_CLASSES - 2; k >= 0; --k) fmd_launch_nei_grp(a, k, per_cu, st, down_cap, 1);
    // the rest (too many candidates, wide intervals, fake forks, neighbour overflow): lane per strand
    fmd_launch_nei_slow(a, st, q2, 1);
    // fake forks among the strands the group kernels finished: the fix-up alone
    fmd_launch_nei_fix(a, st, fmd_next_queue(o.h, st));
    if (side) {   // the caller's stream owns every row again (and the work area, which the next batch reuses)
        if (hipEventRecord(slow.ev[1], slow.stream) != hipSuccess || hipStreamWaitEvent(st, slow.ev[1], 0) != hipSuccess) { (void)hipGetLastError(); hipStreamSynchronize(slow.stream); }
        slow.release();
    }
    if (getenv("FMD_OVLP_STATS")) { // where the strands of this part went (synchronises: diagnostics only)
        uint32_t hs[FMD_CLS_HEADER_U32];
        hipStreamSynchronize(st);
        hipMemcpy(hs, cls, sizeof(hs), hipMemcpyDeviceToHost);
        const auto word = [&hs](int c, int w) { return hs[fmd_cls_cnt_off(c) + w]; };
        uint32_t nf = 0, nb = 0, ng = 0;
        for (int k = 0; k < 2 * FMD_GRP_CLASSES; ++k) { nf += word(fmd_cls_fast(k), FMD_CW_COUNT); nb += word(fmd_cls_fast(k), FMD_CW_HANDED); }
        for (int k = 0; k < FMD_GRP_CLASSES; ++k) ng += word(k, FMD_CW_COUNT);
        fprintf(stderr, "[M::fmd_ovlp] part of %zu strands: %u to the unforked path (%u of them handed on), %u slots of the general group kernels' lists (holes of the hand-over included), %u through the lane-per-strand kernel at once + %u handed back to it, %u fake forks fixed up\n",
                np, nf, nb, ng, word(FMD_CLS_SLOW, FMD_CW_COUNT), word(FMD_CLS_SLOW, FMD_CW_LATE), word(FMD_CLS_SLOW, FMD_CW_FIX));
        // The slots above depend on which waves handed strands on (a wave's last chunk keeps its unused slots as holes); what the general lists
        // CONTAIN does not: the entries that are no hole, per group class
        uint32_t ne[FMD_GRP_CLASSES];
        for (int k = 0; k < FMD_GRP_CLASSES; ++k) {
            const size_t slots = word(k, FMD_CW_COUNT);
            uint32_t *e = (uint32_t *)malloc(8 * slots + 8);
            ne[k] = 0;
            if (e && hipMemcpy(e, a.cl.lst[k], 8 * slots, hipMemcpyDeviceToHost) == hipSuccess)
                for (size_t i = 0; i < slots; ++i) ne[k] += e[2 * i] != FMD_LIST_HOLE;
            free(e);
        }
        static_assert(FMD_GRP_CLASSES == 6, "one %u per general class");
        fprintf(stderr, "[M::fmd_ovlp] ... of those slots %u %u %u %u %u %u hold a strand (general lists of the group classes, smallest first)\n", ne[0], ne[1], ne[2], ne[3], ne[4], ne[5]);
        // what the lanes of k_ovl_nei_lane did with them (its counting instantiations run under this switch), all classes together
        uint32_t ln[6] = {0, 0, 0, 0, 0, 0}, adm64 = 0;
        for (int k = 0; k < 2 * FMD_GRP_CLASSES; ++k) {
            for (int i = 0; i < 6; ++i) ln[i] += word(fmd_cls_fast(k), FMD_CW_LANE_ADM + i);
            if (k >= FMD_GRP_CLASSES) adm64 += word(fmd_cls_fast(k), FMD_CW_LANE_ADM);
        }
        fprintf(stderr, "[M::fmd_ovlp] ... one lane per strand: %u strands admitted (%u with 64-bit masks), lane rounds: %u quiet, %u self-end inline, %u closing past the loops, %u through the loops of the full round (%u of them applied a pending self-end round first)\n",
                ln[0], adm64, ln[1], ln[2], ln[3], ln[4], ln[5]);
    }
#ifdef GRP_STATS
    {
        uint32_t hs[FMD_CLS_HEADER_U32];
        hipStreamSynchronize(st);
        hipMemcpy(hs, cls, sizeof(hs), hipMemcpyDeviceToHost);
        const auto word = [&hs](int c, int w) { return hs[fmd_cls_cnt_off(c) + w]; };
        const uint32_t gr = word(FMD_CLS_SLOW, FMD_CW_GRP_ROUNDS), gl = word(FMD_CLS_SLOW, FMD_CW_GRP_LIVE), gh = word(FMD_CLS_SLOW, FMD_CW_GRP_HELD);
        static_assert(FMD_GRP_CLASSES == 6, "one %u per general class");
        fprintf(stderr, "[grp stats] classes %u %u %u %u %u %u slow %u | wave rounds %u, live lanes %u (%.1f %%), lanes of groups holding a strand %u (%.1f %%)\n",
                word(0, FMD_CW_COUNT), word(1, FMD_CW_COUNT), word(2, FMD_CW_COUNT), word(3, FMD_CW_COUNT), word(4, FMD_CW_COUNT), word(5, FMD_CW_COUNT), word(FMD_CLS_SLOW, FMD_CW_COUNT),
                gr, gl, 100.0 * gl / (64.0 * gr), gh, 100.0 * gh / (64.0 * gr));
        for (int k = 0; k < 2 * FMD_GRP_CLASSES; ++k) {
            const int f = fmd_cls_fast(k);
            const uint32_t fr = word(f, FMD_CW_FAST_ROUNDS);
            if (word(f, FMD_CW_COUNT)) fprintf(stderr, "[fast stats] G=%d %s: %u strands, %u handed on (%u) | wave rounds %u (%u with a second base), live lanes %.1f %%, lanes of groups holding a strand %.1f %%\n",
                              fmd_grp_size(k % FMD_GRP_CLASSES), k >= FMD_GRP_CLASSES ? "64-bit" : "32-bit", word(f, FMD_CW_COUNT), word(f, FMD_CW_HANDED), word(f, FMD_CW_HANDED_AT0), fr,
                              word(f, FMD_CW_FAST_ROUNDS2), 100.0 * word(f, FMD_CW_FAST_LIVE) / (64.0 * fr), 100.0 * word(f, FMD_CW_FAST_HELD) / (64.0 * fr));
        }
    }
#endif
    return FMD_OK;
}

// Pipelined batches (FMD_OVLP_PIPE="parts,walk_per_cu,grp_per_cu,fast_per_cu"; not the default any more).  A batch can be cut
// into parts with phase B of part p on a second stream beside phase A of part p+1, each with a share of the CU's wave slots.  That
// paid while get_nei was the general group kernel alone (92 ms of serial work in 82 on error-free reads).  With the unforked fast
// path phase B is a quarter of a part and bound by instruction issue, the walk wants every wave slot it can get (it runs at the
// memory system's rate of random lines), and the two side by side finish no sooner than one after the other -- 71 against 75 ms on
// error-free reads with "4,8,8,8", 147 against 117 ms on reads with 1 % errors, whose long get_nei phase then starves the walk
// (profiles/r2_ab/ab_fast_pipe.txt).  Default: the serial order.
static void ovl_pipe_config(size_t n, int &parts, int &walk_cu, int &grp_cu, int &fast_cu)
{
    parts = 1; walk_cu = 8; grp_cu = 8; fast_cu = 8;
    const char *e = getenv("FMD_OVLP_PIPE");
    if (e) {
        int a = 0, b = 0, c = 0, d = 0;
        const int k = sscanf(e, "%d,%d,%d,%d", &a, &b, &c, &d);
        if (k >= 1 && a >= 1) parts = a < FMD_OVLP_MAX_PARTS ? a : FMD_OVLP_MAX_PARTS;
        if (k >= 2 && b >= 1) walk_cu = b;
        if (k >= 3 && c >= 1) grp_cu = c;
        if (k >= 4 && d >= 1) fast_cu = d;
    }
}
extern "C" int fmd_ovlp_dev(fmd_dev_t *h, void *stream_, size_t n, const uint64_t *d_ids, int min_match, uint32_t max_len,
                            uint32_t max_nei, fmd_ovlp_rec_t *d_rec, fmd_intv_t *d_nei, uint8_t *d_seq, uint32_t seq_stride,
                            void *d_work, size_t work_bytes)
{
    if (!h || (n && (!d_ids || !d_rec || !d_nei || !d_seq || !d_work)) || max_len == 0 || max_nei == 0 || min_match < 0) return FMD_E_ARG;
    if (n == 0) return FMD_OK;
    if (n >= 0xffffff00ull || work_bytes < fmd_ovlp_work_bytes(n, max_len, min_match)) return FMD_E_ARG;
    if (fmd_ovlp_list_cap(max_len, min_match) >= 4096) return FMD_E_ARG; // category index is packed in 12 bits
    FMD_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream_;
    OvlBatch o;
    o.h = h; o.ix = fmd_view(h);
    o.ids = d_ids; o.min_match = min_match; o.max_len = max_len; o.max_nei = max_nei; o.seq_stride = seq_stride;
    o.carve((uint8_t *)d_work, n);
    o.rec = d_rec; o.nei = d_nei; o.seq = d_seq; o.gidx = nullptr; o.park = nullptr; o.keys = nullptr;

    int parts, walk_cu, grp_cu, fast_cu;
    ovl_pipe_config(n, parts, walk_cu, grp_cu, fast_cu);
    if (parts > 1 && !h->aux.acquire(FMD_OVLP_MAX_PARTS + 1)) parts = 1;   // the second stream is in use by another call: serial order
    int rc = FMD_OK;
    if (parts == 1) {
        ovl_phase_a(o, st, 0, n, 0);
        rc = ovl_phase_b(o, st, 0, n, 0, 0, 0);
    } else {
        hipStream_t s2 = h->aux.stream;
        // Equal parts: get_nei is the slower phase while the two run side by side, so the last part --
        // whose get_nei has the GPU to itself -- should not be smaller than the others.
        const size_t per = ((n + parts - 1) / parts + 63) & ~(size_t)63;
        int p = 0;
        bool join_ok = true;
        for (size_t b = 0; b < n && rc == FMD_OK; b += per, ++p) {
            const size_t np = n - b < per ? n - b : per;
            const bool last = b + per >= n;
            ovl_phase_a(o, st, b, np, p == 0 ? 0 : walk_cu);         // the first part has the GPU to itself
            if (hipEventRecord(h->aux.ev[p], st) != hipSuccess || hipStreamWaitEvent(s2, h->aux.ev[p], 0) != hipSuccess) { join_ok = false; break; }
            rc = ovl_phase_b(o, s2, b, np, p, last ? 0 : grp_cu, last ? 0 : fast_cu);      // so has the last phase B
        }
        // the caller's stream owns the results again; if the hand-over itself failed, wait on the host
        if (!join_ok || hipEventRecord(h->aux.ev[FMD_OVLP_MAX_PARTS], s2) != hipSuccess ||
            hipStreamWaitEvent(st, h->aux.ev[FMD_OVLP_MAX_PARTS], 0) != hipSuccess) {
            hipStreamSynchronize(s2);
            if (!join_ok) { fmd_set_hip_error(hipGetLastError(), "overlap batch: event hand-over"); rc = FMD_E_HIP; }
        }
        h->aux.release();
    }
    if (rc != FMD_OK) return rc;
    FMD_CHECK_LAUNCH("overlap kernels");
    return FMD_OK;
}

// ---- the whole job in an order that keeps neighbours on the genome in flight together ---------------------------------------------
// Work area of fmd_ovlp_sorted_dev: the parked strands (64 bytes each), two (key, row) arrays for the sort, the sort's own
// temporary storage, and the work area of ONE batch of fmd_ovlp_dev.
struct SortedLayout { size_t park, keys_a, keys_b, vals_a, vals_b, tmp, tmp_bytes, batch_area, total; };
static SortedLayout sorted_layout(size_t n, size_t batch, uint32_t max_len, int min_match)
{
    SortedLayout L;
    size_t o = 0;
    L.park = o; o += align_up(n * sizeof(FmdWalkPark), 256);
    L.keys_a = o; o += align_up(n * 4, 256);
    L.keys_b = o; o += align_up(n * 4, 256);
    L.vals_a = o; o += align_up(n * 4, 256);
    L.vals_b = o; o += align_up(n * 4, 256);
    L.tmp_bytes = fmd_park_sort_temp_bytes(n);
    L.tmp = o; o += align_up(L.tmp_bytes, 256);
    L.batch_area = o;   // (also the head's admission records, 32 bytes per strand of the job, while pass 1 runs)
    { const size_t ba = fmd_ovlp_work_bytes(batch, max_len, min_match), ad = align_up(n * 32, 256); o += ba > ad ? ba : ad; }
    L.total = o;
    return L;
}
extern "C" size_t fmd_ovlp_sorted_work_bytes(size_t n, size_t batch, uint32_t max_len, int min_match)
{
    if (batch == 0 || batch > n) batch = n;
    return sorted_layout(n, batch, max_len, min_match).total;
}
// can the two-pass form be used at all?  (nothing may be pushed inside the head; a parked stash is two 16-byte groups of the row)
static bool sorted_eligible(const fmd_dev *h, size_t n, int min_match, uint32_t max_len)
{
    const char *e = getenv("FMD_OVLP_SORT");   // A/B switch: 0 = batches in id order through the one-pass walk
    if (e && atoi(e) == 0) return false;
    return n < 0xffffff00ull && min_match >= (int)FMD_WALK_SPLIT && max_len >= FMD_WALK_SPLIT && h->ptab_d < (int)FMD_WALK_SPLIT;
}

// ---- the two halves of the sorted job as entry points of their own: a caller may do something between them (hand finished rows on
// while the rest is being computed; exchange the parked strands between GPUs by key: fmd_ovlp_dist.hip) --------------------------------
extern "C" int fmd_ovlp_two_pass_ok(const fmd_dev_t *h, size_t n, int min_match, uint32_t max_len)
{
    return h && sorted_eligible(h, n, min_match, max_len) && fmd_ovlp_list_cap(max_len, min_match) < 4096 ? 1 : 0;
}
// work area of the head: the admission records (32 bytes per strand), the unsorted (key, row) arrays, the sort's temporary storage
struct HeadLayout { size_t adm, keys_a, vals_a, tmp, tmp_bytes, total; };
static HeadLayout head_layout(size_t n)
{
    HeadLayout L;
    size_t o = 0;
    L.keys_a = o; o += align_up(n * 4, 256);
    L.vals_a = o; o += align_up(n * 4, 256);
    L.tmp_bytes = fmd_park_sort_temp_bytes(n);
    L.tmp = o; o += align_up(L.tmp_bytes, 256);
    L.adm = o; o += align_up(n * 32, 256);
    L.total = o;
    return L;
}
extern "C" size_t fmd_ovlp_head_work_bytes(size_t n) { return head_layout(n).total; }

extern "C" int fmd_ovlp_head_dev(fmd_dev_t *h, void *stream_, size_t n, const uint64_t *d_ids, int min_match, uint32_t max_len, fmd_ovlp_rec_t *d_rec,
                                 void *d_park, uint32_t *d_keys, uint32_t *d_order, void *d_work, size_t work_bytes)
{
    if (!h || (n && (!d_ids || !d_rec || !d_park || !d_keys || !d_order || !d_work)) || max_len == 0 || min_match < 0) return FMD_E_ARG;
    if (n == 0) return FMD_OK;
    if (!fmd_ovlp_two_pass_ok(h, n, min_match, max_len)) return FMD_E_ARG;
    const HeadLayout L = head_layout(n);
    if (work_bytes < L.total) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h->device));
    uint8_t *w = (uint8_t *)d_work;
    const int rc = fmd_ovlp_head(h, (hipStream_t)stream_, n, d_ids, min_match, d_rec, (FmdWalkPark *)d_park, (uint32_t *)(w + L.keys_a), (uint32_t *)(w + L.vals_a),
                            d_keys, d_order, w + L.tmp, L.tmp_bytes, (uint4 *)(w + L.adm));
    if (rc != FMD_OK) return rc;
    FMD_CHECK_LAUNCH("sorted overlap job: head");
    return FMD_OK;
}

// pass 2 + fm6_get_nei for np parked strands: slot t of the call = row d_rows[t] of d_park, d_rec, d_nei and d_seq
static int ovl_tail(fmd_dev *h, hipStream_t st, size_t np, const uint32_t *rows, const uint32_t *keys, FmdWalkPark *park, const uint64_t *d_ids, int min_match, uint32_t max_len, uint32_t max_nei,
                    fmd_ovlp_rec_t *d_rec, fmd_intv_t *d_nei, uint8_t *d_seq, uint32_t seq_stride, uint8_t *area, size_t area_strands)
{
    OvlBatch o;
    o.h = h; o.ix = fmd_view(h); o.ids = d_ids; o.min_match = min_match; o.max_len = max_len; o.max_nei = max_nei; o.seq_stride = seq_stride;
    o.carve(area, area_strands);
    o.rec = d_rec; o.nei = d_nei; o.seq = d_seq; o.park = park;
    o.gidx = rows; o.keys = keys;
    ovl_phase_a(o, st, 0, np, 0);
    return ovl_phase_b(o, st, 0, np, 0, 0, 0);
}

extern "C" int fmd_ovlp_tail_dev(fmd_dev_t *h, void *stream_, size_t np, const uint32_t *d_rows, void *d_park, int min_match, uint32_t max_len, uint32_t max_nei,
                                 fmd_ovlp_rec_t *d_rec, fmd_intv_t *d_nei, uint8_t *d_seq, uint32_t seq_stride, void *d_work, size_t work_bytes)
{
    if (!h || (np && (!d_rows || !d_park || !d_rec || !d_nei || !d_seq || !d_work)) || max_len == 0 || max_nei == 0 || min_match < 0) return FMD_E_ARG;
    if (np == 0) return FMD_OK;
    if (np >= 0xffffff00ull || !fmd_ovlp_two_pass_ok(h, np, min_match, max_len) || work_bytes < fmd_ovlp_work_bytes(np, max_len, min_match)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h->device));
    const int rc = ovl_tail(h, (hipStream_t)stream_, np, d_rows, nullptr, (FmdWalkPark *)d_park, nullptr, min_match, max_len, max_nei, d_rec, d_nei, d_seq, seq_stride, (uint8_t *)d_work, np);
    if (rc != FMD_OK) return rc;
    FMD_CHECK_LAUNCH("sorted overlap job: tail");
    return FMD_OK;
}

extern "C" int fmd_ovlp_sorted_dev(fmd_dev_t *h, void *stream_, size_t n, const uint64_t *d_ids, int min_match, uint32_t max_len,
                                   uint32_t max_nei, fmd_ovlp_rec_t *d_rec, fmd_intv_t *d_nei, uint8_t *d_seq, uint32_t seq_stride,
                                   void *d_work, size_t work_bytes, size_t batch)
{
    if (!h || (n && (!d_ids || !d_rec || !d_nei || !d_seq || !d_work)) || max_len == 0 || max_nei == 0 || min_match < 0) return FMD_E_ARG;
    if (n == 0) return FMD_OK;
    if (n >= 0xffffff00ull || fmd_ovlp_list_cap(max_len, min_match) >= 4096) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream_;
    if (batch == 0 || batch > n) batch = n;
    if (!sorted_eligible(h, n, min_match, max_len)) {   // the same strands in id order, batch by batch
        if (work_bytes < fmd_ovlp_work_bytes(batch, max_len, min_match)) return FMD_E_ARG;
        for (size_t b = 0; b < n; b += batch) {
            const size_t np = n - b < batch ? n - b : batch;
            const int rc = fmd_ovlp_dev(h, stream_, np, d_ids + b, min_match, max_len, max_nei, d_rec + b, d_nei + b * (size_t)max_nei,
                                        d_seq + b * (size_t)seq_stride, seq_stride, d_work, work_bytes);
            if (rc != FMD_OK) return rc;
        }
        return FMD_OK;
    }
    const SortedLayout L = sorted_layout(n, batch, max_len, min_match);
    if (work_bytes < L.total) return FMD_E_ARG;
    uint8_t *w = (uint8_t *)d_work;
    FmdWalkPark *park = (FmdWalkPark *)(w + L.park);
    uint32_t *sorted = (uint32_t *)(w + L.vals_b);
    // (the admission records live in the batch area, which is idle until pass 2; 32 bytes per strand of the job)
    {
        const int rc = fmd_ovlp_head(h, st, n, d_ids, min_match, d_rec, park, (uint32_t *)(w + L.keys_a), (uint32_t *)(w + L.vals_a), (uint32_t *)(w + L.keys_b), sorted,
                                w + L.tmp, L.tmp_bytes, (uint4 *)(w + L.batch_area));
        if (rc != FMD_OK) return rc;
    }
    // pass 2 + fm6_get_nei, batch by batch in that order
    for (size_t b = 0; b < n; b += batch) {
        const size_t np = n - b < batch ? n - b : batch;
        const int rc = ovl_tail(h, st, np, sorted + b, (const uint32_t *)(w + L.keys_b) + b, park, d_ids, min_match, max_len, max_nei, d_rec, d_nei, d_seq, seq_stride, w + L.batch_area, batch);
        if (rc != FMD_OK) return rc;
    }
    FMD_CHECK_LAUNCH("sorted overlap job");
    return FMD_OK;
}

// ---- rows that exceeded a capacity: again, alone, larger -------------------------------------------------------------------------
// fm6_get_nei has no capacities (kvec grows, unitig.c:93-179); here a row that needs more neighbours than max_nei, a longer candidate
// list or more bases than max_len is flagged (FMD_OVLP_F_OVERFLOW) instead of answered.  This collects the ids of the flagged rows of
// a finished job on the device and runs them through fmd_ovlp_dev with the capacities the caller names, into a side table; rows of
// the side table that are still flagged are counted so that the caller can go one size up.
__global__ void k_ovl_collect_overflow(size_t n, const fmd_ovlp_rec_t *__restrict__ rec, const uint64_t *__restrict__ ids, uint64_t cap,
                                       uint64_t *__restrict__ out_ids, uint32_t *__restrict__ out_rows, unsigned long long *__restrict__ counter)
{
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i0 = (size_t)blockIdx.x * blockDim.x; i0 < n; i0 += step) {
        const size_t i = i0 + threadIdx.x;
        const bool hit = i < n && (rec[i].flags & FMD_OVLP_F_OVERFLOW) != 0;
        const unsigned long long m = __ballot(hit);
        if (m == 0) continue;
        const int lane = threadIdx.x & 63;
        unsigned long long base = 0;
        if (lane == __ffsll((long long)m) - 1) base = atomicAdd(counter, (unsigned long long)__popcll(m));   // one atomic per wave that has any
        base = __shfl(base, __ffsll((long long)m) - 1);
        if (hit) {
            const unsigned long long slot = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
            if (slot < cap) { out_ids[slot] = ids ? ids[i] : (uint64_t)i; if (out_rows) out_rows[slot] = (uint32_t)i; }
        }
    }
}
__global__ void k_ovl_count_overflow(size_t n, const fmd_ovlp_rec_t *__restrict__ rec, unsigned long long *__restrict__ counter)
{
    const size_t step = (size_t)gridDim.x * blockDim.x;
    unsigned long long c = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) c += (rec[i].flags & FMD_OVLP_F_OVERFLOW) != 0;
    if (c) atomicAdd(counter, c);
}
extern "C" size_t fmd_ovlp_side_work_bytes(size_t side_cap, uint32_t max_len, int min_match)
{
    return 256 + fmd_ovlp_work_bytes(side_cap, max_len, min_match);
}
extern "C" int fmd_ovlp_rerun_overflow_dev(fmd_dev_t *h, void *stream_, size_t n, const uint64_t *d_ids, const fmd_ovlp_rec_t *d_rec, int min_match, uint32_t max_len,
                                           uint32_t max_nei, uint64_t side_cap, uint64_t *d_side_ids, uint32_t *d_side_rows, fmd_ovlp_rec_t *d_side_rec, fmd_intv_t *d_side_nei,
                                           uint8_t *d_side_seq, uint32_t side_stride, void *d_work, size_t work_bytes, uint64_t *n_side, uint64_t *n_still)
{
    if (!h || !n_side || !n_still || (n && !d_rec) || (side_cap && (!d_side_ids || !d_side_rec || !d_side_nei || !d_side_seq || !d_work)) || max_len == 0 || max_nei == 0) return FMD_E_ARG;
    *n_side = 0; *n_still = 0;
    if (n == 0) return FMD_OK;
    if (work_bytes < fmd_ovlp_side_work_bytes(side_cap, max_len, min_match)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream_;
    unsigned long long *ctr = (unsigned long long *)d_work;   // [0] flagged rows of the job, [1] rows of the side table still flagged
    FMD_HIP_TRY(hipMemsetAsync(ctr, 0, 16, st));
    size_t blocks = (n + 255) / 256;
    if (blocks > (1u << 16)) blocks = 1u << 16;
    k_ovl_collect_overflow<<<(unsigned)blocks, 256, 0, st>>>(n, d_rec, d_ids, side_cap, d_side_ids, d_side_rows, ctr);
    unsigned long long hc[2] = {0, 0};
    FMD_HIP_TRY(hipMemcpyAsync(hc, ctr, 8, hipMemcpyDeviceToHost, st));
    FMD_HIP_TRY(hipStreamSynchronize(st));
    *n_side = hc[0];
    if (hc[0] == 0) return FMD_OK;
    if (hc[0] > side_cap) return FMD_E_OVERFLOW;    // (the caller's side table is too small: *n_side says how many rows there are)
    const size_t k = (size_t)hc[0];
    FMD_HIP_TRY(hipMemsetAsync(d_side_seq, 0, k * (size_t)side_stride, st));
    const int rc = fmd_ovlp_dev(h, stream_, k, d_side_ids, min_match, max_len, max_nei, d_side_rec, d_side_nei, d_side_seq, side_stride, (uint8_t *)d_work + 256, work_bytes - 256);
    if (rc != FMD_OK) return rc;
    k_ovl_count_overflow<<<(unsigned)((k + 255) / 256 > 4096 ? 4096 : (k + 255) / 256), 256, 0, st>>>(k, d_side_rec, ctr + 1);
    FMD_HIP_TRY(hipMemcpyAsync(hc + 1, ctr + 1, 8, hipMemcpyDeviceToHost, st));
    FMD_HIP_TRY(hipStreamSynchronize(st));
    *n_still = hc[1];
    return FMD_OK;
}

// check_left_simple (unitig.c:186-204) for every strand of a finished fmd_ovlp_dev batch that has a
// unique neighbour; writes rec.reserved.  Same buffers and work area as the fmd_ovlp_dev call.
extern "C" int fmd_ovlp_check_left_dev(fmd_dev_t *h, void *stream_, size_t n, int min_match, uint32_t max_len, fmd_ovlp_rec_t *d_rec,
                                       const uint8_t *d_seq, uint32_t seq_stride, void *d_work, size_t work_bytes)
{
    if (!h || (n && (!d_rec || !d_seq || !d_work)) || max_len == 0) return FMD_E_ARG;
    if (n == 0) return FMD_OK;
    if (work_bytes < fmd_ovlp_work_bytes(n, max_len, min_match)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream_;
    const BatchLayout L = batch_layout(n, max_len, min_match);
    NeiArgs a;   // (the two candidate lists of the batch's area are its scratch; rows in batch order)
    a.ix = fmd_view(h); a.grid = fmd_grid_for(h, n); a.np = n; a.min_match = min_match; a.cap = L.cap;
    a.listA = (fmd_intv_t *)((uint8_t *)d_work + L.listA); a.listB = (fmd_intv_t *)((uint8_t *)d_work + L.listB);
    a.rec = d_rec; a.seq = const_cast<uint8_t *>(d_seq); a.seq_stride = seq_stride;
    fmd_launch_check_left(a, st, fmd_next_queue(h, st));
    FMD_CHECK_LAUNCH("k_ovl_cls");
    return FMD_OK;
}

// fm6_retrieve (exact.c:100-127) for a batch of sequence ids: rank, `$read$` bi-interval and
// containment of each sequence, i.e. the walk phase alone with no length threshold.  What
// fm6_seqsort (seqsort.c:12-35) needs.  rec.status = -3 when contained on either side.
extern "C" int fmd_seqinfo_dev(fmd_dev_t *h, void *stream_, size_t n, const uint64_t *d_ids, uint32_t max_len, fmd_ovlp_rec_t *d_rec,
                               uint8_t *d_seq, uint32_t seq_stride, void *d_work, size_t work_bytes)
{
    if (!h || (n && (!d_ids || !d_rec || !d_seq || !d_work)) || max_len == 0) return FMD_E_ARG;
    if (n == 0) return FMD_OK;
    if (n >= 0xffffff00ull || work_bytes < fmd_ovlp_work_bytes(n, max_len, (int)max_len - 1)) return FMD_E_ARG;
    FMD_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream_;
    const BatchLayout L = batch_layout(n, max_len, (int)max_len - 1);
    WalkArgs a;   // the one-pass walk with no threshold: records and the stash, no candidates
    a.ix = fmd_view(h); a.n = n; a.ids = d_ids; a.info_only = 1; a.rec = d_rec; a.srev = (uint8_t *)d_work + L.srev; a.stride_r = L.stride_r;
    a.listA = (fmd_intv_t *)((uint8_t *)d_work + L.listA); a.cap = L.cap;
    fmd_launch_walk_whole(h, st, a, max_len, d_seq, seq_stride, 0, FMD_TICKET_CHUNK);
    FMD_CHECK_LAUNCH("k_ovl_walk");
    return FMD_OK;
}

extern "C" int fmd_ovlp_batch(fmd_dev_t *h, size_t n, const uint64_t *ids, int min_match, uint32_t max_len, uint32_t max_nei,
                              fmd_ovlp_rec_t *rec, fmd_intv_t *nei, uint8_t *seq, uint32_t seq_stride, int with_check_left)
{
    if (!h || (n && (!ids || !rec || !nei || !seq))) return FMD_E_ARG;
    if (n == 0) return FMD_OK;
    FMD_HIP_TRY(hipSetDevice(h->device));
    // strands per pass: as many as keep the HBM work area (two candidate lists per strand: 6.4 kB at 100 bp,
    // -l50) around 32 GB, between 2^16 and 2^22
    const size_t per_strand = fmd_ovlp_work_bytes(1u << 16, max_len, min_match) >> 16;
    size_t chunk = ((size_t)32 << 30) / (per_strand ? per_strand : 1);
    if (chunk > (4u << 20)) chunk = 4u << 20;
    if (chunk < (1u << 16)) chunk = 1u << 16;
    const size_t m = n < chunk ? n : chunk;
    const size_t wb = fmd_ovlp_work_bytes(m, max_len, min_match);
    FmdDevBuf di, dr, dn, ds, dw;
    if (di.alloc(m * 8) || dr.alloc(m * sizeof(fmd_ovlp_rec_t)) || dn.alloc(m * max_nei * sizeof(fmd_intv_t)) ||
        ds.alloc(m * (size_t)seq_stride) || dw.alloc(wb)) return FMD_E_NOMEM;
    // Gigabytes come back per call: pin the caller's arrays for its duration so the copies run at link speed
    // instead of through the runtime's staging buffers (best effort; pageable copies otherwise).
    const size_t pin_min = (size_t)64 << 20;
    FmdHostPin pin_rec(rec, n * sizeof(fmd_ovlp_rec_t), pin_min), pin_nei(nei, n * max_nei * sizeof(fmd_intv_t), pin_min), pin_seq(seq, n * (size_t)seq_stride, pin_min);
    for (size_t o = 0; o < n; o += m) {
        const size_t c = n - o < m ? n - o : m;
        FMD_HIP_TRY(hipMemcpy(di.p, ids + o, c * 8, hipMemcpyHostToDevice));
        FMD_HIP_TRY(hipMemset(ds.p, 0, c * (size_t)seq_stride));
        FMD_HIP_TRY(hipMemset(dn.p, 0, c * max_nei * sizeof(fmd_intv_t)));
        int rc = fmd_ovlp_dev(h, nullptr, c, (uint64_t *)di.p, min_match, max_len, max_nei, (fmd_ovlp_rec_t *)dr.p,
                              (fmd_intv_t *)dn.p, (uint8_t *)ds.p, seq_stride, dw.p, wb);
        if (rc) return rc;
        if (with_check_left) {
            rc = fmd_ovlp_check_left_dev(h, nullptr, c, min_match, max_len, (fmd_ovlp_rec_t *)dr.p, (uint8_t *)ds.p, seq_stride, dw.p, wb);
            if (rc) return rc;
        }
        FMD_HIP_TRY(hipMemcpy(rec + o, dr.p, c * sizeof(fmd_ovlp_rec_t), hipMemcpyDeviceToHost));
        FMD_HIP_TRY(hipMemcpy(nei + o * max_nei, dn.p, c * max_nei * sizeof(fmd_intv_t), hipMemcpyDeviceToHost));
        FMD_HIP_TRY(hipMemcpy(seq + o * (size_t)seq_stride, ds.p, c * (size_t)seq_stride, hipMemcpyDeviceToHost));
    }
    return FMD_OK;
}

extern "C" int fmd_seqinfo_batch(fmd_dev_t *h, size_t n, const uint64_t *ids, uint32_t max_len, fmd_ovlp_rec_t *rec)
{
    if (!h || (n && (!ids || !rec))) return FMD_E_ARG;
    if (n == 0) return FMD_OK;
    FMD_HIP_TRY(hipSetDevice(h->device));
    const size_t chunk = 1u << 21;
    const size_t m = n < chunk ? n : chunk;
    const uint32_t stride = (uint32_t)align_up(max_len, 4);
    const size_t wb = fmd_ovlp_work_bytes(m, max_len, (int)max_len - 1);
    FmdDevBuf di, dr, ds, dw;
    if (di.alloc(m * 8) || dr.alloc(m * sizeof(fmd_ovlp_rec_t)) || ds.alloc(m * (size_t)stride) || dw.alloc(wb)) return FMD_E_NOMEM;
    for (size_t o = 0; o < n; o += m) {
        const size_t c = n - o < m ? n - o : m;
        FMD_HIP_TRY(hipMemcpy(di.p, ids + o, c * 8, hipMemcpyHostToDevice));
        int rc = fmd_seqinfo_dev(h, nullptr, c, (uint64_t *)di.p, max_len, (fmd_ovlp_rec_t *)dr.p, (uint8_t *)ds.p, stride, dw.p, wb);
        if (rc) return rc;
        FMD_HIP_TRY(hipMemcpy(rec + o, dr.p, c * sizeof(fmd_ovlp_rec_t), hipMemcpyDeviceToHost));
    }
    return FMD_OK;
}
