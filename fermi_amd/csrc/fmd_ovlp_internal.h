// fmd_ovlp_internal.h -- what the translation units of overlap discovery (fmd_ovlp*.hip) call in each other: host-side launchers only;
// no kernel is launched across files.  The walk's arguments are WalkArgs, phase B's are NeiArgs; where the work lists between the two lie in a batch's work
// area, and what the words of their counter lines mean, is written down once, in fmd_kernel_common.h (fmd_cls_list, fmd_cls_cnt_off, FmdClsWord).
#pragma once
#include "fmd_kernel_common.h"

// ---- fmd_ovlp_walk.hip: the fused LF-walk + overlap_intv
// The arguments of k_ovl_walk<MODE>.  A launch site fills what its mode reads; the rest stays null.
struct WalkArgs {
    FmdIndexView ix;
    size_t n = 0;                       // items of the launch: strands (WALK_WHOLE), admission records (WALK_HEAD), slots of the batch (WALK_TAIL, WALK_TAIL2)
    const uint64_t *ids = nullptr;      // WALK_WHOLE, WALK_HEAD: the sequence id of row r
    int min_match = 0;
    int info_only = 0;                  // WALK_WHOLE: no length threshold and no candidates (fmd_seqinfo_dev)
    fmd_ovlp_rec_t *rec = nullptr;
    uint8_t *srev = nullptr;            // WALK_WHOLE, WALK_TAIL: the stash, one row of stride_r bytes per item, last base first
    uint32_t stride_r = 0;              // ... and the longest sequence that gets a complete record (every mode)
    fmd_intv_t *listA = nullptr;        // all but WALK_HEAD: cap candidates per item
    uint32_t cap = 0;
    uint32_t *queue = nullptr;          // the launch's ticket counter and its largest chunk (FmdTickets)
    uint32_t tickets = 0;
    FmdWalkPark *park = nullptr;        // WALK_HEAD writes row gs, the two tails read it
    const uint4 *adm = nullptr;         // WALK_HEAD: two words per item (k_ovl_head_adm)
    int pair_from = 0;                  // WALK_HEAD: the depth below FMD_WALK_SPLIT at which a narrow strand is handed to k_ovl_pair; 0 = none is
    const uint32_t *gidx = nullptr;     // the two tails: slot of the batch -> row of park, rec (and seq_out)
    const uint32_t *keys = nullptr;     // WALK_TAIL2: the sort key of every slot (k_ovl_park_keys), strands of one key in phase on the genome; null = free-running admission
    uint8_t *seq_out = nullptr;         // WALK_TAIL2: the caller's rows in read order
    uint32_t seq_stride = 0;
    uint32_t *redo = nullptr;           // WALK_TAIL2: [0] number, [1 ..] slots of the strands with an N (k_ovl_seq_redo)
    uint32_t *cls = nullptr;            // WALK_TAIL2: the area of the part's work lists of get_nei (fmd_cls_list, fmd_kernel_common.h); null = k_ovl_classify makes them
    int use_fast = 0, min_cls = 0;      // ... as fmd_launch_classify takes them: narrow strands to the fast lists, the smallest group class in use
};
// Each launcher sizes the grid (per_cu > 0: at most that many waves per CU), takes a queue and sets n's share of tickets, and runs what belongs behind the walk:
// the read-order copy (whole, tail) or the rows of the strands with an N (tail2, which also zeroes redo[0] and the header of cls).
void fmd_launch_walk_whole(fmd_dev *h, hipStream_t st, WalkArgs a, uint32_t max_len, uint8_t *seq_out, uint32_t seq_stride, int per_cu, uint32_t tickets);
void fmd_launch_walk_tail(fmd_dev *h, hipStream_t st, WalkArgs a, uint32_t max_len, uint8_t *seq_out, uint32_t seq_stride, int per_cu);
void fmd_launch_walk_tail2(fmd_dev *h, hipStream_t st, WalkArgs a, int per_cu);
bool fmd_walk_tail2_fits(uint32_t stride_r, uint32_t seq_stride);   // can WALK_TAIL2 hold a batch's sequences in LDS and write rows of this stride?
// pass 1 of a sorted job with the arrays where the caller wants them: park[n], the sorted keys and the order (row of the t-th strand in key order)
int fmd_ovlp_head(fmd_dev *h, hipStream_t st, size_t n, const uint64_t *d_ids, int min_match, fmd_ovlp_rec_t *d_rec, FmdWalkPark *park,
                  uint32_t *keys_a, uint32_t *vals_a, uint32_t *keys_sorted, uint32_t *order, void *tmp, size_t tmp_bytes, uint4 *adm);

// ---- phase B: fm6_get_nei over the work lists of one part of a batch (their layout: fmd_cls_list and the functions beside it, fmd_kernel_common.h)
// What the kernels of phase B share, for the strands [b, b + np) of a batch.  Host code only: a launcher unpacks it into the kernel's own __restrict__ parameters
// (walk_run, fmd_ovlp_walk.hip, says why the kernels do not take a struct).
struct NeiArgs {
    FmdIndexView ix;
    int n_cu = 0, grid = 0;             // CUs of the device (the group kernels size their grids from it); waves of a lane-per-strand launch over np items (fmd_grid_for)
    size_t np = 0;                      // strands of the part
    int min_match = 0;
    const uint8_t *srev = nullptr;      // the part's rows of the stash, the candidate lists and their scratch: slot t of the part = row t
    uint32_t stride_r = 0;
    fmd_intv_t *listA = nullptr, *listB = nullptr;
    uint32_t cap = 0;
    const uint32_t *gidx = nullptr;     // slot of a sorted batch -> row of rec / nei / seq (fmd_ovlp_sorted_dev); nullptr = the slot is the row
    fmd_ovlp_rec_t *rec = nullptr;
    fmd_intv_t *nei = nullptr;          // max_nei entries per row
    uint32_t max_nei = 0;
    uint8_t *seq = nullptr;             // (fmd_launch_check_left only reads the rows: its caller's const pointer comes in through a const_cast)
    uint32_t seq_stride = 0;
    FmdOvlClasses cl;                   // the lists classification fills and their counter lines,
    uint32_t *late = nullptr, *fix = nullptr;   // ... the late list and the fix-up list (counters: words of the slow list's line)
    uint32_t *cnt(int c, int word = FMD_CW_COUNT) const { return cl.cnt + fmd_cls_cnt_off(c) + word; }
};
// the lists of a part of np strands laid over `area` (fmd_cls_part_off picks the area of a part out of a batch's)
inline void fmd_nei_lists_at(NeiArgs &a, uint32_t *area, size_t np)
{
    a.cl.cnt = area;
    for (int k = 0; k < FMD_GRP_CLASSES; ++k) a.cl.lst[k] = fmd_cls_list(area, k, np);
    a.cl.lslow = fmd_cls_list(area, FMD_CLS_SLOW, np);
    for (int k = 0; k < 2 * FMD_GRP_CLASSES; ++k) a.cl.fast[k] = fmd_cls_list(area, fmd_cls_fast(k), np);
    a.late = fmd_cls_late(area, np); a.fix = fmd_cls_fix(area, np);
}
// Each launcher finds its list, the counters and the hand-over targets in `a` from what is particular to the launch.
// fmd_ovlp_grp.hip: the lists from the records and listA (where the walk has not made them; min_cls: the smallest group class in use)
void fmd_launch_classify(const NeiArgs &a, hipStream_t st, int use_fast, int min_cls);
// fmd_ovlp_nei.hip: one lane per strand, over the slow list (late = 0) or the late list; the fix-up list; check_left_simple over all np strands (a.seq is read only)
void fmd_launch_nei_slow(const NeiArgs &a, hipStream_t st, uint32_t *queue, int late);
void fmd_launch_nei_fix(const NeiArgs &a, hipStream_t st, uint32_t *queue);
void fmd_launch_check_left(const NeiArgs &a, hipStream_t st, uint32_t *queue);
// fmd_ovlp_grp.hip, fmd_ovlp_lane.hip: by groups of lanes, by one lane per strand with the candidates in registers.  cls: the group class; wide: the list
// with 64-bit masks; per_cu_cap > 0: at most that many waves per CU.  The fast forms read fast list cls (+ FMD_GRP_CLASSES: wide) and hand on to general list cls;
// the group form reads general list cls, or in the second pass the list that strands moved down to class cls are on (down_cap: entries such a list holds, 0 = nobody moves)
int fmd_nei_fast_available(void);
int fmd_nei_lane_enabled(void);
int fmd_nei_lane_class_ok(int cls, int wide);
void fmd_launch_nei_lane(const NeiArgs &a, int cls, int wide, int per_cu_cap, hipStream_t st);
void fmd_launch_nei_fast(const NeiArgs &a, int cls, int wide, int per_cu_cap, hipStream_t st);
void fmd_launch_nei_grp(const NeiArgs &a, int cls, int per_cu_cap, hipStream_t st, uint32_t down_cap, int second_pass);

// ---- fmd_ovlp_sort.hip: minimizer keys of the parked strands, then their rows sorted by key (-> vals_b)
size_t fmd_park_sort_temp_bytes(size_t n);
int fmd_park_sort(hipStream_t st, size_t n, const FmdWalkPark *park, uint32_t *keys_a, uint32_t *keys_b, uint32_t *vals_a, uint32_t *vals_b, void *tmp, size_t tmp_bytes);
