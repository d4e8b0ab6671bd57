// fmd_ovlp_internal.h -- what the translation units of overlap discovery (fmd_ovlp*.hip) call in each other: host-side launchers only;
// no kernel is launched across files.
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
    uint32_t *cls = nullptr;            // WALK_TAIL2: the work lists of get_nei (FmdOvlClasses laid over it); null = k_ovl_classify makes them
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

// ---- fmd_ovlp_nei.hip: fm6_get_nei and check_left_simple, one lane per strand
// (gidx: slot of a sorted batch -> row of rec / nei_out / seq_out, fmd_ovlp_sorted_dev; nullptr = the slot is the row)
// work_list == nullptr: all n strands; otherwise the *work_n strands of the list
void fmd_launch_nei_slow(int grid, hipStream_t st, uint32_t *queue, const FmdIndexView &ix, size_t n, int min_match, const uint8_t *srev, uint32_t stride_r, uint32_t cap,
                         fmd_intv_t *listA, fmd_intv_t *listB, fmd_ovlp_rec_t *rec, fmd_intv_t *nei_out, uint32_t max_nei, uint8_t *seq_out, uint32_t seq_stride,
                         const uint32_t *work_list, const uint32_t *work_n, const uint32_t *gidx);
void fmd_launch_nei_fix(int grid, hipStream_t st, uint32_t *queue, const FmdIndexView &ix, const uint32_t *list, const uint32_t *list_n, const uint8_t *srev, uint32_t stride_r,
                        fmd_ovlp_rec_t *rec, const fmd_intv_t *nei_out, uint32_t max_nei, uint8_t *seq_out, uint32_t seq_stride, const uint32_t *gidx);
void fmd_launch_check_left(int grid, hipStream_t st, uint32_t *queue, const FmdIndexView &ix, size_t n, int min_match, uint32_t cap, fmd_intv_t *listA, fmd_intv_t *listB,
                           fmd_ovlp_rec_t *rec, const uint8_t *seq, uint32_t seq_stride);

// ---- fmd_ovlp_grp.hip, fmd_ovlp_lane.hip: fm6_get_nei by groups of lanes, by one lane per strand with the candidates in registers
void fmd_launch_nei_grp(int cls, int n_cu, int per_cu_cap, hipStream_t st, const FmdIndexView &ix, const uint32_t *list, const uint32_t *list_n, uint32_t cap,
                        const fmd_intv_t *listA, fmd_intv_t *listB, const FmdOvlClasses &cl, fmd_ovlp_rec_t *rec, fmd_intv_t *nei_out, uint32_t max_nei, uint8_t *seq_out,
                        uint32_t seq_stride, uint32_t *slow_list, uint32_t *slow_n, const uint32_t *gidx, size_t fix_off, uint32_t down_cap, int second_pass);
int fmd_nei_fast_available(void);
int fmd_nei_lane_enabled(void);
int fmd_nei_lane_class_ok(int cls, int wide);
void fmd_launch_nei_lane(int cls, int wide, int n_cu, int per_cu_cap, hipStream_t st, const FmdIndexView &ix, const uint32_t *list, const uint32_t *list_n, uint32_t cap,
                         const fmd_intv_t *listA, fmd_intv_t *listB, fmd_ovlp_rec_t *rec, fmd_intv_t *nei_out, uint32_t max_nei, uint8_t *seq_out,
                         uint32_t seq_stride, uint32_t *gen_list, uint32_t *gen_n, uint32_t *bail_n, const uint32_t *gidx);
void fmd_launch_nei_fast(int cls, int wide, int n_cu, int per_cu_cap, hipStream_t st, const FmdIndexView &ix, const uint32_t *list, const uint32_t *list_n, uint32_t cap,
                         const fmd_intv_t *listA, fmd_intv_t *listB, fmd_ovlp_rec_t *rec, fmd_intv_t *nei_out, uint32_t max_nei, uint8_t *seq_out,
                         uint32_t seq_stride, uint32_t *gen_list, uint32_t *gen_n, uint32_t *bail_n, uint32_t *slow_list, uint32_t *slow_n, const uint32_t *gidx);
void fmd_launch_classify(hipStream_t st, size_t n, const fmd_ovlp_rec_t *rec, const fmd_intv_t *listA, uint32_t cap, FmdOvlClasses cl, int use_fast, const uint32_t *gidx);

// ---- fmd_ovlp_sort.hip: minimizer keys of the parked strands, then their rows sorted by key (-> vals_b)
size_t fmd_park_sort_temp_bytes(size_t n);
int fmd_park_sort(hipStream_t st, size_t n, const FmdWalkPark *park, uint32_t *keys_a, uint32_t *keys_b, uint32_t *vals_a, uint32_t *vals_b, void *tmp, size_t tmp_bytes);
