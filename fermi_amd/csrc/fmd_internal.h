// fmd_internal.h -- host-side internals shared by the .hip translation units of libfmdhip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/fmd_hip.h"
#include "fmd_wave.h"

#define FMD_OVLP_MAX_PARTS 8

void fmd_set_hip_error(hipError_t e, const char *what);
// A device buffer of at least `bytes` from the handle's cache (hipMalloc when none fits); give it back with
// fmd_scratch_release.  Thread-safe; nullptr when the device is out of memory.
void *fmd_scratch_acquire(fmd_dev *h, size_t bytes);
void fmd_scratch_release(fmd_dev *h, void *p);

// the owning host-side resources (device / pinned buffers, streams, events, scratch leases): a .hip file uses these and defines none
#include <stdlib.h>
#include "fmd_hostres.h"

struct fmd_dev {
    int device;
    int n_cu;                 // compute units on this GPU
    uint64_t n_blocks;        // rank blocks incl. one trailing pad block
    uint64_t bytes;           // HBM bytes held
    uint4 *blocks;            // device
    uint64_t cnt[7], mcnt[7];
    uint4 *ptab;              // device: intervals of all strings of ptab_d bases (FmdIndexView)
    int ptab_d;
    unsigned long long *tail;  // device: FmdIndexView::tail
    uint4 *pair;               // device: two-base blocks (fmd_pair.hip), built on first use by the sorted overlap job; nullptr = none
    unsigned long long *pair_tab;
    uint64_t pair_bytes;
    int pair_tried;
    uint32_t *queues;         // device ring of work-queue heads for the persistent kernels
    uint32_t queue_next;      // host-side ring cursor (atomic)
    unsigned long long *stat; // device: FMD_STAT_SLOTS x FMD_STAT_STRIDE line counters (written by the instrumented build only)
    // device buffers kept between host-form calls (fmd_scratch_*): hipFree + hipMalloc of tens of GB per call cost
    // 1-2 s (`unitig` on 10 M reads: 1.05 s of a 1.2 s table pass); released by fmd_dev_close
    struct { void *p; size_t bytes; int busy; } scratch[24];
    int scratch_lock;
    // second stream + events of the pipelined overlap batch (fmd_ovlp_dev), and the side stream of fm6_get_nei's lane-per-strand kernel
    // (k_ovl_nei on the strands k_ovl_classify sets aside runs beside the group kernels: a few long dependent chains, nothing to gain
    // from having the GPU to itself).  Made on first use; one call at a time uses each, a concurrent call takes the serial path.
    FmdSideStream aux, slow;
};
#define FMD_N_QUEUES 256

#define FMD_HIP_TRY(expr)                                       \
    do {                                                        \
        hipError_t e__ = (expr);                                \
        if (e__ != hipSuccess) {                                \
            fmd_set_hip_error(e__, #expr);                      \
            return e__ == hipErrorOutOfMemory ? FMD_E_NOMEM : FMD_E_HIP; \
        }                                                       \
    } while (0)

#define FMD_TRY(expr) do { int rc__ = (expr); if (rc__) return rc__; } while (0)   // an FMD_* code

// after kernel launches: what the runtime says of them, recorded under `what`; FMD_E_HIP whatever the error (FMD_HIP_TRY maps out-of-memory)
#define FMD_CHECK_LAUNCH(what)                                  \
    do {                                                        \
        hipError_t e__ = hipGetLastError();                     \
        if (e__ != hipSuccess) { fmd_set_hip_error(e__, what); return FMD_E_HIP; } \
    } while (0)

static inline FmdIndexView fmd_view(const fmd_dev *h)
{
    FmdIndexView v;
    v.blocks = h->blocks;
    for (int i = 0; i < 7; ++i) v.cnt[i] = h->cnt[i];
    v.n_sym = h->mcnt[0];
    v.n_seq = h->mcnt[1];
    v.ptab = h->ptab; v.ptab_d = h->ptab_d; v.tail = h->tail;
    v.pair = h->pair; v.pair_tab = h->pair_tab;
    v.stat = h->stat;
    return v;
}

// the in-place index builder's hooks into fmd_index.hip
int fmd_index_alloc(int device, uint64_t n_sym, fmd_dev **out);
int fmd_index_put_slice(fmd_dev *h, hipStream_t st, const uint8_t *d_slice, uint64_t first, uint64_t m);
int fmd_index_finish(fmd_dev *h, int tables = 1);   // tables = 0: no prefix / tail table (FMD_OPEN_NO_TABLES)

// the two-base blocks (fmd_pair.hip): built when forced (fmd_dev_build_pairs) or FMD_PAIR asks, and they fit; FMD_OK either way (h->pair says)
int fmd_pairs_ensure(fmd_dev *h, int force);

// kcount's walk without its end (fmd_kcount.hip), for a walk that ends differently (kgraph, fmd_kgraph.hip): on a work area of fmd_kcount_work_bytes(cap),
// from n_roots <= cap roots of one length (fmd_kcount_part_dev's), the levels root_len .. depth - 1 (depth <= 31).  *d_frontier = the nodes at `depth`, both
// orientations of every k-mer with min_occ occurrences and more, size 0 = a hole; the u64 counters at the head of d_work: [depth] = the entries of that
// frontier (more than cap when it overflowed), [FMD_KCOUNT_CTR_OVF] != 0 when an entry did not fit, [FMD_KCOUNT_CTR_EXT] = the extensions done.
// *level_grid (may be NULL) = the waves a level ran on.  Enqueues on st; checks nothing.
#define FMD_KCOUNT_CTR_OVF 41
#define FMD_KCOUNT_CTR_EXT 44
int fmd_kcount_levels(fmd_dev *h, hipStream_t st, int depth, int min_occ, int root_len, size_t n_roots, const fmd_intv_t *d_roots, uint64_t cap, void *d_work,
                      const fmd_intv_t **d_frontier, int *level_grid);

// kgraph's compaction (fmd_kgraph.hip: link resolution, pointer doubling, cut, final) on the sorted nodes of ANY de Bruijn graph held on the device --
// kgraph's own and the union graph of kcgraph (fmd_kcgraph.hip).  d_kmer ascending, d_arcs the arc bytes, d_pat NULL or a byte per node: a link is then
// compactable only between nodes with equal bytes (FMD_KCGRAPH_SPLIT).  d_work = fmd_kgraph_compact_bytes(n) bytes and more; d_ctr = 128 u64 words whose
// words 4, 5 and 16.. are zero.  Null stream; returns after the device is done.  The labels stay in d_work: label = the smallest node id of the chain,
// off, oc = orient | 2 on a cycle.  fmd_kgraph_number_host turns downloaded labels into unitig ids and fills the per-unitig arrays (malloc'ed).
// st = the settled doubling state of the 2 n ports, in d_work too (k_kgraph_round: x = the free port at the chain's end, y = the steps there, w = 1), and
// st_spare = the doubling's other buffer, 32 n bytes that nobody reads any more: what the bubble stage (fmd_kbubble.hip) takes.
struct FmdKgLabels { uint32_t *label, *off; uint8_t *oc; uint64_t n_links, n_cycles, n_rounds; double ms_links, ms_label; const uint4 *st; void *st_spare; };
size_t fmd_kgraph_compact_bytes(uint64_t n);
int fmd_kgraph_compact_dev(int k, uint64_t n, const uint64_t *d_kmer, const uint8_t *d_arcs, const uint8_t *d_pat, void *d_work, size_t work_bytes,
                           unsigned long long *d_ctr, FmdKgLabels *out);
int fmd_kgraph_number_host(uint64_t n, uint32_t *unitig, const uint32_t *offset, uint8_t *orient, uint64_t *n_unitigs, uint32_t **u_nodes, uint32_t **u_first,
                           uint8_t **u_flags);

// kbubble's stage (fmd_kbubble.hip) on a graph that fmd_kgraph_compact_dev has just compacted WITHOUT the split rule (d_pat == NULL) and whose work area is
// still there: the simple bubbles of include/fmd_hip.h, ascending by src, in *bubble (malloc'ed; NULL when there are none).  grid = the blocks of 256
// threads (0: as the link kernel's).  Scratch comes from h's cache.  Null stream; returns after the device is done; *ms = its host wall time.
int fmd_kbubble_stage_dev(fmd_dev *h, int k, uint64_t n, const uint64_t *d_kmer, const uint8_t *d_arcs, const FmdKgLabels *lb, uint32_t max_len, int grid,
                          uint64_t *n_forks, uint64_t *n_bubbles, fmd_kbubble_t **bubble, double *ms);

// next zeroed work-queue head for a persistent launch on `stream`
uint32_t *fmd_next_queue(fmd_dev *h, hipStream_t stream);

// persistent-grid size: waves (= 64-thread workgroups) to launch for n items
int fmd_grid_for(const fmd_dev *h, size_t n_items);
// same for a kernel that uses lds_bytes of LDS per 64-thread workgroup (160 KiB per CU)
int fmd_grid_for_lds(const fmd_dev *h, size_t n_items, size_t lds_bytes);

// Resident 64-thread workgroups per CU of `kernel` with lds_bytes of static LDS, for kernels that deal
// their work statically (round-robin or by ranges): a workgroup beyond the resident set would start when
// the others are done and then work through a full share alone.  The runtime's occupancy query, bounded by
// the LDS granule (1280 bytes on gfx950: 160 KiB / 128) and by `cap`.
template <typename K>
static inline int fmd_resident_per_cu(K kernel, size_t lds_bytes, int cap, const char *name)
{
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 64, 0) != hipSuccess || nb < 1) nb = 1;
    const int by_lds = lds_bytes ? (int)((160 * 1024) / (((lds_bytes + 1279) / 1280) * 1280)) : nb;
    if (nb > by_lds) nb = by_lds;
    if (nb > cap) nb = cap;
    if (getenv("FMD_DEBUG_OCC")) fprintf(stderr, "[occupancy] %s: %d workgroups per CU\n", name, nb);
    return nb;
}
