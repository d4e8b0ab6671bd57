/* include/fmd_hip.h -- C ABI of libfmdhip.so, the MI355X (gfx950) implementation of fermi's
 * FMD-index hot path.  Plain pointers and sizes only; no C++ or torch types.
 *
 * This is the drop-in boundary: each entry point is the batched, device-side
 * replacement of one function of the reference's internal C API (rld.h:45-58, fermi.h:61-103,
 * unitig.c:77/93, correct.c:35), cited per declaration.  A reference maintainer binds these
 * from cmd.c / unitig.c / correct.c exactly as shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 (FMD_OK) or a negative FMD_E_* code; fmd_strerror() names it.
 *   - fmd_dev_t is an opaque handle to an index resident in one GPU's HBM (read-only after
 *     open, like the reference's `const rld_t*`; safe to share between host threads).
 *   - `*_dev` entry points take DEVICE pointers and a hipStream_t (as void*; NULL = default
 *     stream), enqueue work and return without synchronising.  They allocate nothing.
 *   - `*_batch` entry points take HOST pointers: copy in, run the `_dev` path, copy out, sync.
 *   - nt6 alphabet everywhere: $=0 A=1 C=2 G=3 T=4 N=5 (seq.c:12-21).
 *   - There is NO CPU fallback behind these symbols: without a GPU they return FMD_E_NODEV.
 */
#ifndef FMD_HIP_H
#define FMD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMD_OK          0
#define FMD_E_NODEV    (-1)  /* no usable HIP device */
#define FMD_E_ARG      (-2)  /* bad argument */
#define FMD_E_FORMAT   (-3)  /* not an RLD\2 (asize 6, sbits 3) or RLE\6 file */
#define FMD_E_IO       (-4)  /* file could not be read/written */
#define FMD_E_NOMEM    (-5)  /* host or device allocation failed */
#define FMD_E_HIP      (-6)  /* a HIP runtime call failed; see fmd_last_hip_error() */
#define FMD_E_OVERFLOW (-7)  /* a fixed-capacity device list overflowed for some item */

/* bi-interval; identical layout to fmintv_t (fermi.h:13-16) */
typedef struct {
    uint64_t x[3]; /* [0] SA start of W, [1] SA start of revcomp(W), [2] size */
    uint64_t info;
} fmd_intv_t;

typedef struct fmd_dev fmd_dev_t;

typedef struct {
    uint64_t cnt[7];     /* cnt[c] = # symbols < c, cnt[6] = total      (rld.c:282-284) */
    uint64_t mcnt[7];    /* mcnt[0] = total, mcnt[1..6] = # of $ACGTN   (rld.c:233)     */
    uint64_t n_blocks;   /* 128-byte device blocks                                      */
    uint64_t hbm_bytes;  /* device bytes held by the index                              */
    int device;
} fmd_info_t;

const char *fmd_strerror(int code);
const char *fmd_last_hip_error(void);
int fmd_device_count(void);

/* ---- index residency: replaces rld_restore / rld_restore_mmap / rld_destroy -------------
 * (rld.c:288, :327, :81).  The on-disk .fmd is unchanged; the GPU transcodes it at upload
 * into fixed-stride 128-byte rank blocks (DESIGN.md "HBM layout"). */
int fmd_dev_open_file(int device, const char *fn, fmd_dev_t **out);            /* RLD\2 or RLE\6 */
int fmd_dev_open_rld(int device, const uint64_t *payload, uint64_t n_words,
                     const uint64_t mcnt[7], fmd_dev_t **out);                  /* RLD\2 payload words (rld.c:242-263) */
int fmd_dev_open_rle6(int device, const uint8_t *runs, uint64_t n_bytes, fmd_dev_t **out); /* len<<3|sym bytes (ropebwt.c:132) */
int fmd_dev_open_bwt(int device, const uint8_t *bwt, uint64_t n, fmd_dev_t **out);          /* plain nt6 BWT string, host */
int fmd_dev_open_bwt_dev(int device, const uint8_t *d_bwt, uint64_t n, fmd_dev_t **out);    /* same, already in HBM */
/* the same without the prefix and tail tables (FMD_OPEN_NO_TABLES; flags = 0: what the entries above build): an index that is
 * only ranked and decoded -- the inputs of fmd_dev_merge -- needs neither, and at 2^31 symbols and more they are 4.3 GB + 8 bytes
 * per sequence.  Every entry point works on such a handle; the overlap and search jobs take the steps the tables would save. */
#define FMD_OPEN_NO_TABLES 1u
/* FMD_OPEN_EMPTY_OK: an RLD\2 file of no symbols (the 216 bytes `sub` writes when nothing is kept; rld_restore reads it) is opened as a
 * handle of no rows, all counts 0, instead of FMD_E_ARG.  Such a handle is a part for fmd_multi_bsearch_* -- a lane of the driver that got
 * no reads -- and for fmd_dev_info / fmd_dev_close; every other job assumes at least one sequence and must not be given it.  (2u is no flag.) */
#define FMD_OPEN_EMPTY_OK 4u
int fmd_dev_open_file_ex(int device, const char *fn, unsigned flags, fmd_dev_t **out);
int fmd_dev_open_bwt_ex(int device, const uint8_t *bwt, uint64_t n, unsigned flags, fmd_dev_t **out);
void fmd_dev_close(fmd_dev_t *h);
/* the work areas the handle keeps between calls of the host-buffer entries (fmd_*_batch, the table jobs) back to the device; -> bytes released.
 * (The reference's per-call vectors are freed per call, e.g. unitig.c:321-325; the handle keeps them because allocating 10-100 GB per call costs more than the call.) */
uint64_t fmd_dev_trim(fmd_dev_t *h);
int fmd_dev_info(const fmd_dev_t *h, fmd_info_t *info);
int fmd_dev_sync(const fmd_dev_t *h, void *stream);
/* measurement aid (no reference counterpart): lines[0] = 64-byte rank blocks, lines[1] = other random lines
 * (prefix-table look-ups) that the kernels launched on this handle have requested since the last reset.  Only
 * libfmdhip_count.so -- the same sources built with -DFMD_COUNT_LINES=1 -- counts (*counting = 1); the shipped
 * library returns zeros and *counting = 0.  Synchronises the device. */
int fmd_dev_line_count(fmd_dev_t *h, uint64_t lines[2], int reset, int *counting);
int fmd_dev_line_count3(fmd_dev_t *h, uint64_t lines[3], int reset, int *counting);   /* ... and lines[2] = 128-byte two-base blocks requested (fmd_dev_build_pairs) */

/* ---- rank: rld_rank1a (rld.c:424) / rld_rank2a (rld.c:457) -------------------------------
 * ok/ol: n rows of 6 counts ($ACGTN) of BWT[0..k] inclusive; k == UINT64_MAX gives zeros.
 * sym (may be NULL): BWT[k], -1 for k == UINT64_MAX. */
int fmd_rank1a_dev(fmd_dev_t *h, void *stream, size_t n, const uint64_t *d_k, uint64_t *d_ok, int8_t *d_sym);
int fmd_rank2a_dev(fmd_dev_t *h, void *stream, size_t n, const uint64_t *d_k, const uint64_t *d_l,
                   uint64_t *d_ok, uint64_t *d_ol);
int fmd_rank1a_batch(fmd_dev_t *h, size_t n, const uint64_t *k, uint64_t *ok, int8_t *sym);
int fmd_rank2a_batch(fmd_dev_t *h, size_t n, const uint64_t *k, const uint64_t *l, uint64_t *ok, uint64_t *ol);

/* ---- fm6_extend (exact.c:72-88): n bi-intervals -> n x 6 bi-intervals (info = 0) --------- */
int fmd_extend_dev(fmd_dev_t *h, void *stream, size_t n, const fmd_intv_t *d_ik, const uint8_t *d_is_back,
                   fmd_intv_t *d_ok);
int fmd_extend_batch(fmd_dev_t *h, size_t n, const fmd_intv_t *ik, const uint8_t *is_back, fmd_intv_t *ok);

/* ---- fm_backward_search (exact.c:7-23) ---------------------------------------------------
 * Read i is seqs[off[i] .. off[i+1]) in nt6.  cnt[i] = occurrences (0 = miss; beg/end are then
 * written as 0, where the reference leaves them untouched). */
int fmd_bsearch_dev(fmd_dev_t *h, void *stream, size_t n, const uint8_t *d_seqs, const uint64_t *d_off,
                    uint64_t *d_cnt, uint64_t *d_beg, uint64_t *d_end);
int fmd_bsearch_batch(fmd_dev_t *h, size_t n, const uint8_t *seqs, const uint64_t *off,
                      uint64_t *cnt, uint64_t *beg, uint64_t *end);

/* ---- fm_multi_backward_search (exact.c:25-57): backward search over n_idx indexes at once ---------
 * The SA interval each read has in the MERGED index of h[0], h[1], .. (fm_merge, in that order), from the parts alone: nothing is merged, no
 * second copy is held.  Reads and results as fmd_bsearch_dev (cnt[i] = 0: a miss, beg/end written as 0; the read bytes 4-byte aligned and
 * readable to the next multiple of 4).  All handles on one device; the same handle may be given twice; at most FMD_MULTI_MAX of them.
 * Two-base blocks on a handle are not used.  The _dev form enqueues on `stream` and returns: it neither allocates nor synchronises, and takes
 * a work area of fmd_multi_bsearch_work_bytes(n_idx, n) bytes, 16-byte aligned (0 for an n_idx out of range).
 * FMD_E_ARG: n_idx < 1, n_idx > FMD_MULTI_MAX, a null handle, handles on different devices, a work area too small.  n = 0 is a no-op. */
#define FMD_MULTI_MAX 16
size_t fmd_multi_bsearch_work_bytes(int n_idx, size_t n);
int fmd_multi_bsearch_dev(int n_idx, fmd_dev_t *const *h, void *stream, size_t n, const uint8_t *d_seqs, const uint64_t *d_off,
                          uint64_t *d_cnt, uint64_t *d_beg, uint64_t *d_end, void *d_work, size_t work_bytes);
int fmd_multi_bsearch_batch(int n_idx, fmd_dev_t *const *h, size_t n, const uint8_t *seqs, const uint64_t *off,
                            uint64_t *cnt, uint64_t *beg, uint64_t *end);

/* ---- fm_retrieve (exact.c:59-70): LF-walk from row x[i] until '$' --------------------------
 * Row i of seqs (stride bytes) receives the sequence REVERSED, exactly as fm_retrieve emits it
 * (callers seq_reverse it, unitig.c:285); len[i] = its length (bases beyond `stride` are
 * dropped, len still counts them); rank[i] = the returned sentinel rank. */
int fmd_retrieve_dev(fmd_dev_t *h, void *stream, size_t n, const uint64_t *d_x, uint8_t *d_seqs, uint32_t stride,
                     uint32_t *d_len, uint64_t *d_rank);
int fmd_retrieve_batch(fmd_dev_t *h, size_t n, const uint64_t *x, uint8_t *seqs, uint32_t stride,
                       uint32_t *len, uint64_t *rank);

/* ---- locate (no reference counterpart: the FMD-index keeps no suffix-array samples) ------------------
 * Which sequences hold the rows [beg[i], beg[i] + cnt[i]) -- the SA interval of a search -- and at which offset: the LF-walk of a row ends at
 * its sequence's '$' after `off` steps, on the sentinel rank fm_retrieve returns (the index into seqsort's map), and the rows of an interval are
 * walked TOGETHER, as intervals that split by the preceding symbol, one level per base.  A run = the sentinel ranks
 * rank .. rank + n - 1 of query `query`, all at offset `off` (0-based, in the strand's sequence as indexed); runs come in no particular order from
 * the _dev form and sorted by (query, off, rank) from the _batch form.  cnt[i] = 0 gives nothing; an interval with cnt[i] > max_occ, or one that does
 * not lie inside the index, is left out whole and counted in n_skipped.
 * stat: n_runs = runs stored, n_rows = the rows in them, n_unfinished = rows still walking after the last level, n_ext = backward extensions done,
 * overflow = 1 when a run did not fit run_cap or an item did not fit the work area (nothing is written past either; the result is incomplete).
 * The _dev form enqueues exactly `levels` levels on `stream` and returns: it neither allocates nor synchronises.  total_rows = the sum of the
 * cnt[i] <= max_occ; that many runs always suffice for run_cap; the work area is 16-byte aligned.  FMD_E_ARG: a null pointer with n > 0, a work
 * area smaller than fmd_locate_work_bytes(n, 0) -- one sized for fewer rows than there are sets `overflow` --, n >= 2^32.  n = 0 is a no-op.
 * The _batch form sizes everything from the counts, runs levels in groups of at most 64 until the frontier is empty (max_len = 0) or max_len levels
 * are done, and returns FMD_E_OVERFLOW if the flag is set.  Handles opened with FMD_OPEN_NO_TABLES work; two-base blocks are not used. */
typedef struct { uint64_t rank; uint32_t n, off, query, reserved; } fmd_locate_run_t;   /* ranks rank .. rank+n-1, all at offset off */
typedef struct { uint64_t n_runs, n_rows, n_skipped, n_unfinished, overflow, n_ext; } fmd_locate_stat_t;
size_t fmd_locate_work_bytes(size_t n, uint64_t total_rows);
int fmd_locate_dev(fmd_dev_t *h, void *stream, size_t n, const uint64_t *d_beg, const uint64_t *d_cnt, uint32_t max_occ, uint32_t levels,
                   fmd_locate_run_t *d_runs, uint64_t run_cap, fmd_locate_stat_t *d_stat, void *d_work, size_t work_bytes);
int fmd_locate_batch(fmd_dev_t *h, size_t n, const uint64_t *beg, const uint64_t *cnt, uint32_t max_occ, uint32_t max_len,
                     fmd_locate_run_t **runs, uint64_t *n_runs, fmd_locate_stat_t *stat);      /* runs freed with fmd_host_free */

/* ---- kcount (no reference counterpart; fermi2 has `count`): k-mer spectrum and counted k-mers from the index ----------------------
 * A k-mer is k bases of A < C < G < T, 1 <= k <= 32, no N, no sentinel; occ(W) = the positions of the indexed sequences, both strands, where W
 * occurs.  On an index of both strands occ(W) = occ(rc(W)); the canonical k-mer of W is min(W, rc(W)) and its COUNT is occ(W), or occ(W) / 2
 * when W = rc(W) (even k only; occ is even then): the number of N-free k-windows of the forward sequences as indexed whose canonical form it is.
 * Only k-mers with count >= min_occ (>= 1) are reported.  Packed form: uint64_t, 2 bits per base, A=0 C=1 G=2 T=3, the first base in the highest
 * of the low 2k bits: numeric order is lexicographic order.  Counts are uint32_t and SATURATE at 2^32 - 1; the histogram and n_total use the
 * exact count.  Histogram of n_bins >= 2 bins: hist[0] = 0, hist[i] = the k-mers with count i for 0 < i < n_bins - 1, hist[n_bins - 1] = those
 * with count >= n_bins - 1.  stat: n_kmers = k-mers reported, n_total = the sum of their counts (min_occ = 1: the N-free k-windows of the forward
 * sequences), n_ext = backward extensions done (discarded parts included), overflow (the _dev form), widest_level = the most frontier slots a
 * level reserved (holes included), n_parts = parts run, n_retries = parts discarded because they did not fit.
 *
 * fmd_kcount_part_dev: one part.  d_roots = n_roots <= cap bi-intervals, 16-byte aligned, of suffixes of ONE length root_len (1 <= root_len <
 * k, so k >= 2; info = the packed suffix; size 0 = skipped); every k-mer W that ends in one of them is walked, kept iff rc(W) <= W, ADDED to
 * d_hist (n_bins words the caller zeroes) and -- d_kmer != NULL -- stored as (rc(W), count) in d_kmer / d_count, in no particular order, dense,
 * out_cap entries at most.  cap = the entries of each of the two frontiers the work area (fmd_kcount_work_bytes(cap), 16-byte aligned) holds,
 * FMD_KCOUNT_MIN_CAP <= cap <= FMD_KCOUNT_MAX_CAP (work_bytes returns 0 outside); chunk and grid shrink with it.  When a frontier entry or a pair
 * does not fit, d_stat->overflow = 1, nothing is written past either, and histogram, list and sums are incomplete: discard them.  Enqueues on
 * `stream` and returns: it neither allocates nor synchronises.
 * fmd_kcount: the whole index.  Parts start from the four single-base roots in the order of rc(suffix); one that overflows is discarded whole and
 * its run of roots cut in two, a single root replaced by its children one base deeper.  sink == NULL: the spectrum only.  Otherwise every part's
 * pairs are sorted on the device and handed to sink(ctx, n, kmer, count) -- host arrays that live until it returns -- as consecutive slices,
 * ascending over the whole run, no k-mer twice; a non-zero return stops the run (FMD_E_IO).  cap = 0: sized from the index and the free device
 * memory, grown after an overflow while it fits; the list of a part has room for cap pairs.  The large buffers stay in the handle's cache between calls
 * (fmd_dev_trim).  Histogram, list, n_kmers and n_total are the same for every cap.  k = 1 is answered from the
 * marginal counts.  FMD_E_ARG: k outside 1..32 (the part entry: 2..32), min_occ < 1, n_bins < 2, a cap outside the range, or an index with
 * mcnt[A] != mcnt[T], mcnt[C] != mcnt[G] or an odd number of sentinels -- a necessary sign of an index of both strands, NOT a sufficient one: a
 * one-strand index (fmd_build_bwt_strands, `ropebwt -F/-R`) that passes it gets counts that mean nothing.  FMD_OPEN_NO_TABLES handles work. */
#define FMD_KCOUNT_MIN_CAP 4096u
#define FMD_KCOUNT_MAX_CAP (1u << 30)
typedef struct { uint64_t n_kmers, n_total, n_ext, overflow, widest_level, n_parts, n_retries; } fmd_kcount_stat_t;
typedef int (*fmd_kcount_sink_fn)(void *ctx, uint64_t n, const uint64_t *kmer, const uint32_t *count);
size_t fmd_kcount_work_bytes(uint64_t cap);
int fmd_kcount_part_dev(fmd_dev_t *h, void *stream, int k, int min_occ, int root_len, size_t n_roots, const fmd_intv_t *d_roots, uint64_t cap,
                        uint32_t n_bins, uint64_t *d_hist, uint64_t *d_kmer, uint32_t *d_count, uint64_t out_cap, fmd_kcount_stat_t *d_stat,
                        void *d_work, size_t work_bytes);
int fmd_kcount(fmd_dev_t *h, int k, int min_occ, uint32_t n_bins, uint64_t *hist, uint64_t cap, fmd_kcount_sink_fn sink, void *ctx,
               fmd_kcount_stat_t *stat);

/* ---- kcmp (no reference counterpart): the joint k-mer counts of TWO indexes of both strands ---------------------------------------
 * k, a k-mer, its packed and its canonical form are kcount's (above), 1 <= k <= 32.  c_i(W) = kcount's COUNT of W in index i: occ_i(W), halved
 * when W = rc(W).  A selection is four bounds, min <= max on each side, a max of 0xffffffff = no upper bound; a canonical k-mer is REPORTED iff
 * c0 + c1 >= 1, min0 <= c0 <= max0 and min1 <= c1 <= max1, tested on the exact counts.  Histogram, list and sums cover the reported k-mers and
 * nothing else.  The walk is the trie of the k-mers of both indexes, level by level, a node = one suffix's interval (start, size) in each
 * index; an inner node is DROPPED iff occ0 < min0, or occ1 < min1, or occ0 = occ1 = 0.  That is exact: a count never exceeds the occ of a
 * suffix of the k-mer, and a palindrome's occ is at least its count.  Upper bounds prune nothing.  A side whose interval is empty is never
 * fetched again: from there the node walks in the other index alone.
 * Histogram: n_bins per axis, 2 <= n_bins <= 1024, row-major: hist[min(c0, n_bins - 1) * n_bins + min(c1, n_bins - 1)] = the reported k-mers
 * there; hist[0] = 0.  List: (kmer, c0, c1), both counts uint32_t that SATURATE at 2^32 - 1 (histogram and sums use the exact counts),
 * ascending by k-mer over the whole run, no k-mer twice.  stat: n_kmers = k-mers reported, n_total0 / n_total1 = the sums of their counts
 * (the selection of everything: the N-free k-windows of each set), n_only0 = those with c1 = 0, n_only1 = those with c0 = 0, n_shared = those
 * with both >= 1, n_ext = backward extensions done, one per (node, non-empty side), discarded parts included, overflow (the _dev form),
 * widest_level = the most frontier slots a level reserved (holes included), n_parts = parts run, n_retries = parts discarded.
 * Handles: both on one device; each passes kcount's test of both strands; the same handle may be given twice; FMD_OPEN_NO_TABLES handles
 * work; a handle of an empty index (FMD_OPEN_EMPTY_OK) is a side on which every count is 0.  Two-base blocks are not used.
 *
 * fmd_kcmp_part_dev: one part, for k >= 2.  d_roots = n_roots <= cap nodes, 16-byte aligned, of suffixes of ONE length root_len (1 <= root_len <
 * k; kmer = the packed suffix; size 0 on both sides = skipped); every k-mer W that ends in one of them is walked, kept iff rc(W) <= W and the
 * selection holds, ADDED to d_hist (n_bins x n_bins words the caller zeroes) and -- d_kmer != NULL -- stored as rc(W) in d_kmer and c0 | c1 << 32
 * (saturated) in d_c01, dense, in no particular order, out_cap entries at most (d_kmer == NULL: no list, out_cap is ignored).  cap = the
 * entries of each of the two frontiers the work area (fmd_kcmp_work_bytes(cap), 16-byte aligned) holds, FMD_KCMP_MIN_CAP <= cap <=
 * FMD_KCMP_MAX_CAP (work_bytes returns 0 outside).  When a frontier entry or a list entry does not fit, d_stat->overflow = 1, nothing is
 * written past either, and histogram, list and sums are incomplete: discard them.  Enqueues on `stream` and returns: it neither allocates
 * nor synchronises.
 * fmd_kcmp: both indexes whole.  Parts start from the single-base roots in the order of rc(suffix); one that overflows is discarded whole and
 * its run of roots cut in two, a single root replaced by its children one base deeper (fmd_extend_batch on each index; those the pruning rule
 * drops are dropped).  sink == NULL: the histogram and the sums only.  Otherwise every part's list is sorted on the device and handed to
 * sink(ctx, n, kmer, c0, c1) -- host arrays that live until it returns -- as consecutive slices; a non-zero return stops the run (FMD_E_IO).
 * cap = 0: sized from the indexes and the free device memory, grown after an overflow while it fits; the list of a part has room for cap
 * entries.  The large buffers stay in h0's cache between calls (fmd_dev_trim).  Histogram, list and sums are the same for every cap.  k = 1 is
 * answered from the marginal counts.  FMD_E_ARG: k outside 1..32 (the part entry: 2..32), n_bins outside 2..1024, min > max, a cap outside the
 * range, a null handle, handles on different devices, a handle that fails the strand test, a work area that is too small. */
#define FMD_KCMP_MIN_CAP 4096u
#define FMD_KCMP_MAX_CAP (1u << 30)
#define FMD_KCMP_NO_MAX 0xffffffffu
typedef struct { uint32_t min0, max0, min1, max1; } fmd_kcmp_sel_t;
typedef struct { uint64_t x0[2], size[2], kmer, reserved; } fmd_kcmp_node_t;   /* 48 bytes: one suffix's interval start and size in each index; size 0 on both = skipped */
typedef struct { uint64_t n_kmers, n_total0, n_total1, n_only0, n_only1, n_shared, n_ext, overflow, widest_level, n_parts, n_retries; } fmd_kcmp_stat_t;
typedef int (*fmd_kcmp_sink_fn)(void *ctx, uint64_t n, const uint64_t *kmer, const uint32_t *c0, const uint32_t *c1);
size_t fmd_kcmp_work_bytes(uint64_t cap);                     /* 0 outside FMD_KCMP_MIN_CAP..FMD_KCMP_MAX_CAP */
int fmd_kcmp_part_dev(fmd_dev_t *h0, fmd_dev_t *h1, void *stream, int k, const fmd_kcmp_sel_t *sel, int root_len, size_t n_roots,
                      const fmd_kcmp_node_t *d_roots, uint64_t cap, uint32_t n_bins, uint64_t *d_hist, uint64_t *d_kmer, uint64_t *d_c01,
                      uint64_t out_cap, fmd_kcmp_stat_t *d_stat, void *d_work, size_t work_bytes);
int fmd_kcmp(fmd_dev_t *h0, fmd_dev_t *h1, int k, const fmd_kcmp_sel_t *sel, uint32_t n_bins, uint64_t *hist, uint64_t cap,
             fmd_kcmp_sink_fn sink, void *ctx, fmd_kcmp_stat_t *stat);

/* ---- kmat (no reference counterpart): the joint k-mer counts of UP TO EIGHT indexes of both strands, unmerged ------------------------------
 * The "k-mer matrix": rows are canonical k-mers, columns are the n_idx indexes h[0 .. n_idx - 1], 1 <= n_idx <= FMD_KMAT_MAX_IDX.  k, a k-mer,
 * its packed and its canonical form are kcount's (above), 1 <= k <= 32.  c_i(W) = kcount's COUNT of W in index i: occ_i(W), halved when W =
 * rc(W), each side on its own.  A selection is one pair (min[i], max[i]) per index, min <= max, a max of FMD_KMAT_NO_MAX = no upper bound (the
 * entries from n_idx on are ignored), and a presence threshold `present` >= 1.  A canonical k-mer is REPORTED iff the sum of its c_i is >= 1 and
 * min[i] <= c_i <= max[i] for every i, tested on the exact counts; its PATTERN is the n_idx-bit number with bit i set iff c_i >= present.
 * Histogram, list and sums cover the reported k-mers and nothing else.  The walk is the trie of the k-mers of all the indexes, level by level, a
 * node = one suffix's interval (start, size) in each index; an inner node is DROPPED iff occ_i < min[i] for some i, or occ_i = 0 for all i.
 * That is exact (kcmp's argument, side by side): a count never exceeds the occ of a suffix of the k-mer, and a palindrome's occ is at least its
 * count.  Upper bounds and `present` prune nothing.  A side whose interval is empty is never fetched again.
 * Pattern spectrum: hist = 1 << n_idx words, hist[pattern] = the reported k-mers with that pattern; with present = 1, hist[0] = 0.  List: (kmer,
 * c_0 .. c_{n_idx - 1}), the counts uint32_t that SATURATE at 2^32 - 1 (pattern and sums use the exact counts), ascending by k-mer over the whole
 * run, no k-mer twice.  stat: n_kmers = k-mers reported, n_total[i] = the sum of their c_i (the selection of everything: the N-free k-windows of
 * set i), n_present[i] = those with c_i >= present, n_ext = backward extensions done, one per (node, non-empty side), discarded parts included,
 * overflow (the _dev form), widest_level = the most frontier slots a level reserved (holes included), n_parts = parts run, n_retries = parts
 * discarded.  The entries of n_total and n_present from n_idx on are 0.
 * Handles: all on one device; each passes kcount's test of both strands; the same handle may be given several times; FMD_OPEN_NO_TABLES
 * handles work; a handle of an empty index (FMD_OPEN_EMPTY_OK) is a side on which every count is 0.
 *
 * A frontier entry (a root) is fmd_kmat_node_bytes(n_idx) = 16 (n_idx + 1) bytes of uint64_t: the packed suffix, a reserved 0, x0[n_idx] (the
 * interval start in each index; 0 where the size is 0), size[n_idx]; all sizes 0 = skipped.  The stride depends on n_idx on purpose: three
 * indexes do not move the bytes of eight.
 * fmd_kmat_part_dev: one part, for k >= 2.  d_roots = n_roots <= cap entries, 16-byte aligned, of suffixes of ONE length root_len (1 <= root_len
 * < k); every k-mer W that ends in one of them is walked, kept iff rc(W) <= W and the selection holds, its pattern ADDED to d_hist (1 << n_idx
 * words the caller zeroes) and -- d_kmer != NULL -- stored as rc(W) in d_kmer[j] and c_i (saturated) in d_count[i * out_cap + j], dense, in no
 * particular order, out_cap entries at most (d_kmer == NULL: no list, out_cap is ignored).  cap = the entries of each of the two frontiers the
 * work area (fmd_kmat_work_bytes(n_idx, cap), 16-byte aligned) holds, FMD_KMAT_MIN_CAP <= cap <= FMD_KMAT_MAX_CAP (work_bytes returns 0
 * outside, and for an n_idx outside 1..8).  When a frontier entry or a list entry does not fit, d_stat->overflow = 1, nothing is written past
 * either, and histogram, list and sums are incomplete: discard them.  Enqueues on `stream` and returns: it neither allocates nor synchronises.
 * fmd_kmat: all indexes whole.  Parts start from the single-base roots in the order of rc(suffix); one that overflows is discarded whole and
 * its run of roots cut in two, a single root replaced by its children one base deeper (fmd_extend_batch on each index with a non-empty side;
 * those the pruning rule drops are dropped).  sink == NULL: the spectrum and the sums only.  Otherwise every part's k-mers are sorted on the
 * device, the count columns gathered in their order, and handed to sink(ctx, n, kmer, count) -- count[i][j] = c_i of kmer[j]; host arrays that
 * live until it returns -- as consecutive slices; a non-zero return stops the run (FMD_E_IO).  cap = 0: sized from the indexes and the free
 * device memory, grown after an overflow while it fits; the list of a part has room for cap entries.  The large buffers stay in h[0]'s cache
 * between calls (fmd_dev_trim).  Spectrum, list and sums are the same for every cap.  k = 1 is answered from the marginal counts.
 * FMD_E_ARG: n_idx outside 1..8, k outside 1..32 (the part entry: 2..32), min > max, present < 1, a cap outside the range, a null handle,
 * handles on different devices, a handle that fails the strand test, a work area that is too small or not 16-byte aligned. */
#define FMD_KMAT_MAX_IDX 8
#define FMD_KMAT_MIN_CAP 4096u
#define FMD_KMAT_MAX_CAP (1u << 30)
#define FMD_KMAT_NO_MAX 0xffffffffu
typedef struct { uint32_t min[8], max[8], present, reserved; } fmd_kmat_sel_t;
typedef struct { uint64_t n_kmers, n_total[8], n_present[8], n_ext, overflow, widest_level, n_parts, n_retries; } fmd_kmat_stat_t;
typedef int (*fmd_kmat_sink_fn)(void *ctx, uint64_t n, const uint64_t *kmer, const uint32_t *const *count);   /* count[i][j] */
size_t fmd_kmat_node_bytes(int n_idx);                        /* 16 (n_idx + 1); 0 outside 1..FMD_KMAT_MAX_IDX */
size_t fmd_kmat_work_bytes(int n_idx, uint64_t cap);          /* 0 outside the ranges */
int fmd_kmat_part_dev(int n_idx, fmd_dev_t *const *h, void *stream, int k, const fmd_kmat_sel_t *sel, int root_len, size_t n_roots,
                      const void *d_roots, uint64_t cap, uint64_t *d_hist, uint64_t *d_kmer, uint32_t *d_count, uint64_t out_cap,
                      fmd_kmat_stat_t *d_stat, void *d_work, size_t work_bytes);
int fmd_kmat(int n_idx, fmd_dev_t *const *h, int k, const fmd_kmat_sel_t *sel, uint64_t *hist, uint64_t cap, fmd_kmat_sink_fn sink, void *ctx,
             fmd_kmat_stat_t *stat);

/* ---- kprofile (no reference counterpart): kcount's COUNT of every k-window of the query sequences -------------------------------------
 * Sequence i is seqs[off[i] .. off[i+1]) in nt6 (the contract of fmd_bsearch_dev: the bytes 4-byte aligned and readable to the next multiple
 * of 4).  Window j of sequence i is its bases [j, j + k), 0 <= j <= len_i - k: nw_i = max(0, len_i - k + 1) windows, woff[0] = 0, woff[i+1] =
 * woff[i] + nw_i, and window j of sequence i writes count[woff[i] + j].  count = kcount's COUNT of the window's k-mer (above): occ(W) on the
 * index of both strands, halved when W = rc(W) -- which is seen from the window's bases --, uint32_t, SATURATED at 2^32 - 1; 0 for a window
 * with any base outside A/C/G/T, for which no search is made (an N never matches an N).  For k <= 32 it is the number `kcount -d -o1` prints
 * for that k-mer, or 0 when kcount does not list it.  1 <= k <= FMD_KPROFILE_MAX_K: nothing is packed, so k > 32 is ordinary; the bound is the
 * bytes one sequence's windows in a wave may take in that wave's LDS.  flags: 0 = the library chooses the path, FMD_KPROFILE_PLAIN = one lane per
 * window, one rank pair per base behind the prefix table.  That is the only path: a second one, which searched the bases that G consecutive
 * windows share once and grew that bi-interval at both ends, was built, measured and lost everywhere -- it is not in
 * the library, and its flag (2u) is refused like every other bit.
 * stat (ADDED to: the caller zeroes it): n_windows = windows written, n_valid = those free of N, n_hit = those with count >= 1, n_ext = rank
 * pairs requested, n_table = windows that started from the prefix table.
 * fmd_kprofile_dev enqueues on `stream` and returns: it neither allocates nor synchronises, and it does not validate d_woff (n + 1 words, as
 * defined above for this k; d_count has room for d_woff[n] words).  d_stat may be NULL.  fmd_kprofile_batch writes woff (n + 1 words) itself
 * and returns the counts in *count (malloc'ed: fmd_host_free); with n = 0 or no window at all woff is still written and *count is NULL.
 * FMD_E_ARG: k out of range, unknown flags, a null pointer with n > 0, n >= 2^32, or a handle that fails kcount's test of both strands (a
 * necessary sign, NOT a sufficient one: a one-strand index that passes it gets counts that mean nothing).  FMD_OPEN_NO_TABLES handles work
 * (every search starts from its last base); a handle of an empty index (FMD_OPEN_EMPTY_OK) gives all zeros.  Two-base blocks are not used. */
#define FMD_KPROFILE_MAX_K 255
#define FMD_KPROFILE_PLAIN  1u
typedef struct { uint64_t n_windows, n_valid, n_hit, n_ext, n_table; } fmd_kprofile_stat_t;
int fmd_kprofile_dev(fmd_dev_t *h, void *stream, size_t n, const uint8_t *d_seqs, const uint64_t *d_off, const uint64_t *d_woff,
                     int k, unsigned flags, uint32_t *d_count, fmd_kprofile_stat_t *d_stat /* may be NULL; the caller zeroes it */);
int fmd_kprofile_batch(fmd_dev_t *h, size_t n, const uint8_t *seqs, const uint64_t *off, int k, unsigned flags,
                       uint64_t *woff /* n + 1, written */, uint32_t **count /* fmd_host_free */, fmd_kprofile_stat_t *stat);

/* ---- kgraph (no reference counterpart): the de Bruijn graph of kcount's k-mers, and its unitigs ------------------------------------------
 * k is ODD, 3 <= k <= 31 (no k-mer is its own reverse complement, so every node has two distinct sides); min_occ >= 1.  COUNT(W) is kcount's
 * (above) for W of k and of k + 1 bases: occ(W) on the index of both strands, halved when W = rc(W) -- which a (k+1)-mer can be.
 * NODES: the canonical k-mers with COUNT >= min_occ: exactly the list of fmd_kcount(k, min_occ), packed and counted (saturating) as there.  A
 * node's id is its position in that ascending list; its FORWARD orientation is its canonical string x.
 * ARCS: one byte per node: bit c (c = 0..3 for A, C, G, T) is set iff COUNT(x.c) >= min_occ, bit 4 + c iff COUNT(c.x) >= min_occ: what
 * fmd_kcount(k + 1, min_occ) lists, seen from its nodes.  Arcs are symmetric: x.c and rc(x.c) have the same COUNT.
 * LINK: for oriented nodes u and v = the last k - 1 bases of u followed by c, the arc u -> v is COMPACTABLE iff u has exactly one right arc, v
 * has exactly one left arc, and u and v are different nodes (a loop A^k -> A^k, and a hairpin u -> rc(u) through a (k+1)-mer that is its own
 * reverse complement, always end a unitig).
 * UNITIGS: the maximal chains of compactable links; every node is in exactly one, and a unitig of n nodes spells n + k - 1 bases.  A chain with
 * two ends is printed as the lexicographically smaller of its string and that string's reverse complement.  A chain that closes on itself (an
 * isolated cycle; flag FMD_KGRAPH_CYCLE) is opened at its smallest node id and printed from that node in forward orientation, n + k - 1 bases.
 * Unitig ids ascend by the smallest node id contained.  Per node: unitig = its unitig's id, offset = its position in the printed string (the
 * node's k bases are [offset, offset + k) there), orient = 0 when the node reads forward in the printed string, 1 when reversed.  Per unitig:
 * u_nodes = its nodes, u_first = the node at offset 0, u_flags.
 * stat: n_nodes; n_arcs = the (k+1)-mers up to reverse complement behind the arc bits (= the length of kcount's list for k + 1); n_links =
 * compactable links, a link and its reverse-complement twin counted once; n_unitigs = n_nodes - n_links + n_cycles; n_ext = backward extensions
 * done (discarded tries included); n_rounds = doubling rounds run; ms_arcs / ms_links / ms_label = host wall time of the three stages (the walk,
 * the sort and the arc kernel; link resolution; labelling), each ended by a wait for the device.
 * fmd_karcs: sink(ctx, n, kmer, count, arcs) gets the nodes ascending in consecutive slices -- host arrays that live until it returns; a non-zero
 * return stops the run (FMD_E_IO); sink == NULL: stat only.  fmd_kunitig: *out is written whole; its nine arrays are malloc'ed, each released
 * with fmd_host_free (all NULL, and the counts 0, for an empty graph and after an error).  Both allocate device memory from the handle's cache
 * (fmd_dev_trim), run on the null stream and return after the device is done.  cap = the most nodes the graph may have, 0 = no limit but
 * FMD_KGRAPH_MAX_NODES (node ids and ports are 32-bit words); the frontiers of the walk are sized from the index and the free device memory as
 * fmd_kcount sizes them and grown after an overflow.  FMD_E_NOMEM, with nothing kept, when the graph has more nodes than cap or the frontiers do
 * not fit; the handle stays usable.  FMD_E_ARG: k even or outside 3..31, min_occ < 1, cap > FMD_KGRAPH_MAX_NODES, a null pointer, or a handle that
 * fails kcount's test of both strands (necessary, NOT sufficient).  A handle of an empty index (FMD_OPEN_EMPTY_OK) gives an empty graph;
 * FMD_OPEN_NO_TABLES handles work. */
#define FMD_KGRAPH_MAX_NODES 0x7ffffffeu
#define FMD_KGRAPH_CYCLE 1u
typedef struct { uint64_t n_nodes, n_arcs, n_links, n_unitigs, n_cycles, n_ext, n_rounds; double ms_arcs, ms_links, ms_label; } fmd_kgraph_stat_t;
typedef int (*fmd_karcs_sink_fn)(void *ctx, uint64_t n, const uint64_t *kmer, const uint32_t *count, const uint8_t *arcs);
typedef struct {
    uint64_t n_nodes, n_unitigs;
    uint64_t *kmer; uint32_t *count; uint8_t *arcs;        /* per node */
    uint32_t *unitig, *offset; uint8_t *orient;            /* per node */
    uint32_t *u_nodes, *u_first; uint8_t *u_flags;         /* per unitig */
    fmd_kgraph_stat_t stat;
} fmd_kunitig_t;
int fmd_karcs(fmd_dev_t *h, int k, int min_occ, uint64_t cap, fmd_karcs_sink_fn sink, void *ctx, fmd_kgraph_stat_t *stat);
int fmd_kunitig(fmd_dev_t *h, int k, int min_occ, uint64_t cap, fmd_kunitig_t *out);

/* ---- kcgraph (no reference counterpart): the COLOURED de Bruijn graph of up to eight indexes of both strands, unmerged, and its unitigs -------
 * The inputs are n_idx handles h[0 .. n_idx - 1], 1 <= n_idx <= FMD_KMAT_MAX_IDX, the COLOURS, all on one device; each passes kcount's test of
 * both strands; the same handle may be given several times; FMD_OPEN_NO_TABLES handles work; a handle of an empty index (FMD_OPEN_EMPTY_OK) is a
 * colour in which every count is 0.  k is ODD, 3 <= k <= 31, and min_occ >= 1, as for kgraph.  c_i(W) = kcount's COUNT of W in index i: occ_i(W)
 * on both strands, halved when W = rc(W) -- which only a (k+1)-mer can be here.
 * NODES: a canonical k-mer x is a node iff c_i(x) >= min_occ for SOME i (a sum over the colours that reaches min_occ makes no node when no single
 * colour does); ids run along the ascending list.  count[i] = c_i(x), exact even below min_occ, saturated to uint32_t.  The node's PATTERN has
 * bit i set iff c_i(x) >= min_occ; it is never 0.
 * ARCS: one byte per node AND colour in kgraph's layout: in arcs[i], bit c is set iff c_i(x.c) >= min_occ, bit 4 + c iff c_i(c.x) >= min_occ.
 * The UNION byte (uarcs) is the OR over i; it is symmetric like kgraph's.  Hence: with n_idx = 1 everything equals fmd_karcs / fmd_kunitig; the
 * nodes with pattern bit i, with count[i] and arcs[i], are exactly the answer of fmd_karcs(h[i], k, min_occ); an arc bit in colour i implies
 * pattern bit i at both of its nodes.
 * WALK: the trie of the k-mers of all the colours (kmat's, one level further); an inner node is DROPPED iff occ_i < min_occ for ALL i, which is
 * exact by kcmp's argument (NOT kmat's predicate, an AND of per-index minima).
 * COMPACTION: kgraph's LINK and UNITIGS rules on the union byte, word for word: cycles opened at the smallest node id, the smaller of string and
 * reverse complement printed, ids by smallest node.  With FMD_KCGRAPH_SPLIT a link is compactable only if, in addition, both nodes have the same
 * pattern: every unitig then has one pattern, and a chain that closes on itself is a cycle only if all its nodes agree.
 * Per unitig, besides kgraph's three arrays: u_count[u * n_idx + i] = the uint64_t sum of the listed count[i] of its nodes, u_present[u * n_idx +
 * i] = its nodes with pattern bit i, u_pattern[u] = the OR of its nodes' patterns.
 * stat: g = kgraph's fields on the union graph (ms_label includes the per-unitig sums); n_nodes_in[i] = nodes with pattern bit i, n_arcs_in[i] =
 * the (k+1)-mers up to reverse complement behind colour i's bits (= the length of fmd_kcount(h[i], k + 1, min_occ)'s list); 0 from n_idx on.
 * fmd_kcarcs: sink(ctx, n, kmer, count, arcs, uarcs) gets the nodes ascending in consecutive slices, count[i][j] and arcs[i][j] of kmer[j] --
 * host arrays that live until it returns; a non-zero return stops the run (FMD_E_IO); sink == NULL: stat only.  fmd_kcunitig: *out is written
 * whole; count and arcs are n_idx columns of n_nodes entries (count[i * n_nodes + j]); its arrays are malloc'ed, each released with fmd_host_free
 * (all NULL, and the counts 0, for an empty graph and after an error).  Device buffers come from h[0]'s cache (fmd_dev_trim); null stream; both
 * return after the device is done.  cap = the most nodes the graph may have, 0 = no limit but FMD_KGRAPH_MAX_NODES; the frontiers are sized from
 * the distinct indexes and the free device memory as fmd_kmat sizes them and grown after an overflow; the graph is held whole.  FMD_E_NOMEM, with
 * nothing kept, when the graph has more nodes than cap or the frontiers do not fit; the handles stay usable.  FMD_E_ARG: k even or outside 3..31,
 * min_occ < 1, n_idx outside 1..8, cap > FMD_KGRAPH_MAX_NODES, unknown flag bits, a null pointer, handles on different devices, or a handle that
 * fails kcount's test of both strands (necessary, NOT sufficient; indexes whose depth-k frontier is not pairs of orientations are refused too). */
#define FMD_KCGRAPH_SPLIT 1u
typedef struct { fmd_kgraph_stat_t g; uint64_t n_nodes_in[8], n_arcs_in[8]; } fmd_kcgraph_stat_t;
typedef int (*fmd_kcarcs_sink_fn)(void *ctx, uint64_t n, const uint64_t *kmer, const uint32_t *const *count, const uint8_t *const *arcs,
                                  const uint8_t *uarcs);
typedef struct {
    uint64_t n_nodes, n_unitigs;
    int32_t n_idx, reserved;
    uint64_t *kmer; uint32_t *count; uint8_t *arcs, *uarcs, *pattern;   /* per node; count and arcs: n_idx columns */
    uint32_t *unitig, *offset; uint8_t *orient;                         /* per node */
    uint32_t *u_nodes, *u_first; uint8_t *u_flags;                      /* per unitig */
    uint64_t *u_count; uint32_t *u_present; uint8_t *u_pattern;         /* per unitig; u_count and u_present: n_idx per unitig */
    fmd_kcgraph_stat_t stat;
} fmd_kcunitig_t;
int fmd_kcarcs(int n_idx, fmd_dev_t *const *h, int k, int min_occ, uint64_t cap, fmd_kcarcs_sink_fn sink, void *ctx, fmd_kcgraph_stat_t *stat);
int fmd_kcunitig(int n_idx, fmd_dev_t *const *h, int k, int min_occ, unsigned flags, uint64_t cap, fmd_kcunitig_t *out);

/* ---- kbubble (no reference counterpart): the simple variant bubbles of kcgraph's graph ------------------------------------------------------
 * Everything is defined on the node graph of kcgraph: its nodes, its UNION arc byte, k odd in 3..31, min_occ >= 1, 1 <= n_idx <= 8 as there.
 * ORIENTED NODES: 2 * id + o; o = 0 is the canonical k-mer x, o = 1 is rc(x) -- the port numbering of the compaction: port p leaves that oriented
 * node through its right end.  The right arcs of (id, 0) are uarcs & 15, those of (id, 1) the high nibble with its bits reversed; the left degree
 * of u is the right degree of u ^ 1; follow(u, c) is the oriented node of text(u)[1:] + c.
 * SIMPLE BUBBLE (s, t, A, B): s is an oriented node with exactly two right arcs, bases c0 < c1.  Branch A starts at a_0 = follow(s, c0), branch B
 * at b_0 = follow(s, c1).  A branch is a chain v_0 .. v_{m-1}, m >= 1: every v_j has left degree 1 and right degree 1, and v_{j+1} is v_j's only
 * successor; it ends at the first successor whose left degree is not 1, its TARGET (a first node whose left degree is not 1 makes no branch: there
 * are no empty branches).  Both branches have the same oriented target t, t has exactly two left arcs, id(t) != id(s), and with max_len > 0 both
 * branches have at most max_len nodes.  Hence: neither s nor t lies in a branch, the branches share no node, and in the UNSPLIT compaction each
 * branch is exactly one whole unitig.  Every bubble is met twice -- from s, and from t ^ 1 with the branches reversed -- and REPORTED once, from the
 * side with id(s) < id(t).
 * RECORD: src = s, dst = t, first[b] = the oriented first node of branch b, len[b] = its nodes; branch 0 leaves s by the smaller base in s's
 * orientation.  Records ascend by src (a port is the source of at most one bubble).
 * HELD: colour i holds branch b iff every node of it has pattern bit i: u_present[u * n_idx + i] == u_nodes[u] for its unitig u = unitig[first[b]
 * >> 1]; the branch's count sum in colour i is u_count[u * n_idx + i].
 * NOT LOOKED FOR: a bubble with an empty branch (s -> t directly), branches that branch themselves (a tip on an allele, nested variants,
 * superbubbles); the graph is not cleaned.
 * fmd_kcbubble: g = exactly what fmd_kcunitig(n_idx, h, k, min_occ, 0, cap, &g) returns; n_forks = the ports with exactly two right arcs; bubble
 * is malloc'ed (fmd_host_free), NULL with n_bubbles = 0 when there are none and after an error; ms_bubble = the host wall time of the stage, ended
 * by a wait for the device.  Errors and argument rules are fmd_kcunitig's (flags = 0).  The stage runs on the graph while it is still on the
 * device, one thread per port, and reads a branch's far end and length from the settled pointer-doubling state of the compaction: it does not walk.
 * fmd_kcbubble_dev: the same stage for a graph already on h's device -- d_kmer the n ascending canonical k-mers, d_uarcs their arc bytes; link
 * resolution and doubling are run first (scratch from h's cache) -- on `grid` blocks of 256 threads, 0 = fmd_kcbubble's choice.  n = 0 gives no
 * bubble; FMD_E_ARG for a null pointer, k even or outside 3..31, n > FMD_KGRAPH_MAX_NODES or grid < 0. */
typedef struct { uint32_t src, dst, first[2], len[2]; } fmd_kbubble_t;
typedef struct { fmd_kcunitig_t g; uint64_t n_forks, n_bubbles; fmd_kbubble_t *bubble; double ms_bubble; } fmd_kcbubble_t;
int fmd_kcbubble(int n_idx, fmd_dev_t *const *h, int k, int min_occ, uint32_t max_len, uint64_t cap, fmd_kcbubble_t *out);
int fmd_kcbubble_dev(fmd_dev_t *h, int k, uint64_t n, const uint64_t *d_kmer, const uint8_t *d_uarcs, uint32_t max_len, int grid, uint64_t *n_forks,
                     uint64_t *n_bubbles, fmd_kbubble_t **bubble);

/* ---- asearch (no reference counterpart): search with up to max_sub substitutions ---------------------------------------------------
 * Query i is seqs[off[i] .. off[i+1]) in nt6, L bases (the contract of fmd_bsearch_dev: the bytes 4-byte aligned and readable to the next
 * multiple of 4).  A PATTERN P is a string over A/C/G/T of length L; it is a HIT of the query when occ(P) > 0 and P differs from the query in
 * at most max_sub positions, 0 <= max_sub <= FMD_ASEARCH_MAX_SUB.  A query base outside A/C/G/T (N) equals no pattern base: every pattern pays
 * one substitution there.  N and '$' of the index match nothing, so a hit never spans two sequences.  ONLY SUBSTITUTIONS: insertions and
 * deletions are not looked for.  A hit: beg, cnt = the SA interval of P (the beg fmd_bsearch gives for P); query; n_sub; sub[j] = pos << 2 |
 * (base - 1) of each substitution (base = the pattern's, nt6), by DESCENDING pos, unused entries 0xffff -- hence L <= FMD_ASEARCH_MAX_LEN.
 * Distinct hits of one query have disjoint intervals.  Per query i and stratum j = 0 .. max_sub two exact counters,
 * strata[(i * (max_sub + 1) + j) * 2 + {0, 1}] = the hits with j substitutions and the sum of their cnt; they are kept whether or not hits are
 * listed (d_hits == NULL, hit_cap == 0: count-only).  A query with more than max_hits hits is TRUNCATED: none of its hits is listed (as locate does
 * with max_occ), its strata stay exact.  A query that is empty or longer than FMD_ASEARCH_MAX_LEN gives nothing and is counted in n_skipped.
 * stat: n_hits, n_occ = the hits of the queries that are not truncated and the sum of their cnt; n_skipped; n_truncated; n_unfinished = items
 * still walking after the last level; overflow != 0: a frontier entry (bit 0) or a hit (bit 1) did not fit -- it was written nowhere, the result
 * is incomplete; n_ext = backward extensions done; widest_level = the most frontier slots a level reserved (holes included).
 *
 * The walk: the trie of the patterns, rooted at the LAST base, level by level -- level 0 takes the last base from the
 * marginal counts, an item of level t >= 1 stands before position L - 1 - t and takes one backward extension --, each item with the number of
 * substitutions spent so far.  fmd_asearch_bound_dev gives the bound that prunes it: lb[off[i] + p] = min(255, the number of disjoint substrings
 * of q[0 .. p] that do not occur, found greedily from the left), a lower bound of the substitutions any hit spends in q[0 .. p] (what BWA calls
 * D); an N costs one.  It relies on occ(W) > 0 <=> occ(rc(W)) > 0: on an index that fails kcount's necessary test of both strands (mcnt[A] !=
 * mcnt[T], mcnt[C] != mcnt[G] or an odd number of sentinels) lb is all zero -- no pruning.  lb of a skipped query is not written.
 * fmd_asearch_dev: d_lb = NULL walks without the bound.  It zeroes d_strata (n * (max_sub + 1) * 2 words), enqueues level 0 and exactly `levels`
 * levels (L - 1 finish a query of L bases) on `stream` and returns: it neither allocates nor synchronises.  d_hits receives hits in no
 * particular order, dense: those of the queries that are not truncated and max_hits of every truncated one -- n_hits + n_truncated * max_hits
 * entries, which the caller sorts out by the strata -- never more than hit_cap.  The work area is fmd_asearch_work_bytes(n, cap) bytes, 16-byte
 * aligned; cap = the entries of each of the two frontiers, FMD_ASEARCH_MIN_CAP <= cap <= FMD_ASEARCH_MAX_CAP (0 outside); the capacity follows
 * from work_bytes.
 * fmd_asearch_batch: host arrays.  The bound, then parts of the query range, levels in groups until the frontier is empty; a part that overflows
 * is discarded and its range cut in two; a single query that does not fit is retried in twice the capacity while cap = 0 allows (cap = 0: sized
 * from the batch and the free device memory), FMD_E_OVERFLOW otherwise.  hits (may be NULL: count only; else freed with fmd_host_free): those of
 * the queries that are not truncated, sorted by (query, n_sub, beg).  strata: n * (max_sub + 1) * 2 words.  The result is the same for every
 * cap.  FMD_ASEARCH_NO_PRUNE: without the bound.  FMD_ASEARCH_BEST: only the lowest stratum of every query that has a hit -- budgets 0, 1, .. over
 * the queries still without one; the strata above it are reported as zero.
 * FMD_E_ARG: max_sub outside 0 .. FMD_ASEARCH_MAX_SUB, a null pointer with n > 0, n >= 2^32, a work area too small or misaligned, a cap out of
 * range, unknown flags.  n = 0 is a no-op.  FMD_OPEN_NO_TABLES handles work; two-base blocks are not used. */
#define FMD_ASEARCH_MAX_SUB 4
#define FMD_ASEARCH_MAX_LEN 16383u
#define FMD_ASEARCH_MIN_CAP 4096u
#define FMD_ASEARCH_MAX_CAP (1u << 28)
#define FMD_ASEARCH_NO_PRUNE 1u
#define FMD_ASEARCH_BEST 2u
typedef struct { uint64_t beg, cnt; uint32_t query, n_sub; uint16_t sub[4]; } fmd_asearch_hit_t;
typedef struct { uint64_t n_hits, n_occ, n_skipped, n_truncated, n_unfinished, overflow, n_ext, widest_level; } fmd_asearch_stat_t;
size_t fmd_asearch_work_bytes(size_t n, uint64_t cap);
int fmd_asearch_bound_dev(fmd_dev_t *h, void *stream, size_t n, const uint8_t *d_seqs, const uint64_t *d_off, uint8_t *d_lb);
int fmd_asearch_dev(fmd_dev_t *h, void *stream, size_t n, const uint8_t *d_seqs, const uint64_t *d_off, const uint8_t *d_lb, int max_sub,
                    uint32_t max_hits, uint32_t levels, fmd_asearch_hit_t *d_hits, uint64_t hit_cap, uint64_t *d_strata,
                    fmd_asearch_stat_t *d_stat, void *d_work, size_t work_bytes);
int fmd_asearch_batch(fmd_dev_t *h, size_t n, const uint8_t *seqs, const uint64_t *off, int max_sub, uint32_t max_hits, unsigned flags,
                      uint64_t cap, fmd_asearch_hit_t **hits, uint64_t *n_hits, uint64_t *strata, fmd_asearch_stat_t *stat);

/* ---- esearch (no reference counterpart): search within max_edit edits, insertions and deletions included -------------------------------
 * Query i is seqs[off[i] .. off[i+1]) in nt6, L bases (read byte by byte: no alignment is asked for).  A PATTERN P is a non-empty string over
 * A/C/G/T that occurs in the index; N and '$' of the index match nothing, so a pattern never spans two sequences.  P is a HIT of the query Q at
 * budget max_edit when the global (Levenshtein) edit distance ed(P, Q) <= max_edit, 0 <= max_edit <= FMD_ESEARCH_MAX_EDIT: a substitution, an
 * insertion and a deletion cost 1 each, so the length of P lies in [max(1, L - max_edit), L + max_edit].  A query base outside A/C/G/T (N) equals no
 * pattern base: it costs 1, substituted or skipped.  Every distinct pattern is ONE hit with its exact distance n_edit, however many alignments
 * reach it.  A hit: beg, cnt = the SA interval of P (what fmd_bsearch gives for P); query; n_edit = ed(P, Q); len = the length of P; reserved = 0.
 * The hit does not carry P: it is the first len symbols of the suffix of row beg (fmdh_esearch_patterns reads it back).  A pattern and its only
 * extension to the left share beg and cnt and differ in len.  Per query i and stratum j = 0 .. max_edit two exact counters,
 * strata[(i * (max_edit + 1) + j) * 2 + {0, 1}] = the hits at distance j and the sum of their cnt; they are kept whether or not hits are listed
 * (d_hits == NULL, hit_cap == 0: count-only).  A query with more than max_hits hits is TRUNCATED: none of its hits is listed, its strata stay
 * exact.  A query that is empty or longer than FMD_ESEARCH_MAX_LEN gives nothing and is counted in n_skipped.  stat: the fields of asearch's --
 * n_hits, n_occ = the hits of the queries that are not truncated and the sum of their cnt; n_skipped; n_truncated; n_unfinished = items still
 * walking after the last level; overflow != 0: a frontier entry (bit 0) or a hit (bit 1) did not fit -- it was written nowhere, the result is
 * incomplete; n_ext = backward extensions done; widest_level = the most frontier slots a level reserved (holes included).
 *
 * The walk: the trie of the index rooted at the END of the pattern, level by level; level t holds the nodes of pattern
 * length t, each with the band of the edit-distance column of its t bases against the query's suffixes of t - max_edit .. t + max_edit bases.
 * Level 0 takes the four one-base patterns from the marginal counts.  d_lb = the bound fmd_asearch_bound_dev gives (it holds with insertions and
 * deletions: an edit breaks at most one of the disjoint substrings that do not occur): a cell is dropped when its value + the bound of the part
 * of the query still ahead exceeds max_edit.  Pruning changes no result; d_lb = NULL walks without it.
 * fmd_esearch_dev: zeroes d_strata (n * (max_edit + 1) * 2 words), enqueues level 0 and exactly `levels` levels (L + max_edit - 1 finish a query
 * of L bases: patterns of up to L + max_edit bases) on `stream` and returns: it neither allocates nor synchronises.  d_hits receives hits in
 * no particular order, dense: those of the queries that are not truncated and max_hits of every truncated one -- n_hits + n_truncated * max_hits
 * entries -- never more than hit_cap.  The work area is fmd_esearch_work_bytes(n, cap) bytes, 16-byte aligned; cap = the entries of each of the
 * two frontiers, FMD_ESEARCH_MIN_CAP <= cap <= FMD_ESEARCH_MAX_CAP (0 outside); the capacity follows from work_bytes.
 * fmd_esearch_batch: host arrays.  The bound, then parts of the query range, levels in groups until the frontier is empty; a part that overflows
 * is discarded and its range cut in two; a single query that does not fit is retried in twice the capacity while cap = 0 allows (cap = 0: sized
 * from the batch and the free device memory), FMD_E_OVERFLOW otherwise.  hits (may be NULL: count only; else freed with fmd_host_free): those of
 * the queries that are not truncated, sorted by (query, n_edit, beg, len).  strata: n * (max_edit + 1) * 2 words.  The result is the same for
 * every cap.  FMD_ESEARCH_NO_PRUNE: without the bound.  FMD_ESEARCH_BEST: only the lowest stratum of every query that has a hit -- budgets 0, 1,
 * .. over the queries still without one; the strata above it are reported as zero.
 * FMD_E_ARG: max_edit outside 0 .. FMD_ESEARCH_MAX_EDIT, a null pointer with n > 0, n >= 2^32, a work area too small or misaligned, a cap out of
 * range, unknown flags.  n = 0 is a no-op.  FMD_OPEN_NO_TABLES handles work; two-base blocks are not used. */
#define FMD_ESEARCH_MAX_EDIT 4
#define FMD_ESEARCH_MAX_LEN 16383u
#define FMD_ESEARCH_MIN_CAP 4096u
#define FMD_ESEARCH_MAX_CAP (1u << 28)
#define FMD_ESEARCH_NO_PRUNE 1u
#define FMD_ESEARCH_BEST 2u
typedef struct { uint64_t beg, cnt; uint32_t query, n_edit, len, reserved; } fmd_esearch_hit_t;
typedef struct { uint64_t n_hits, n_occ, n_skipped, n_truncated, n_unfinished, overflow, n_ext, widest_level; } fmd_esearch_stat_t;
size_t fmd_esearch_work_bytes(size_t n, uint64_t cap);
int fmd_esearch_dev(fmd_dev_t *h, void *stream, size_t n, const uint8_t *d_seqs, const uint64_t *d_off, const uint8_t *d_lb, int max_edit,
                    uint32_t max_hits, uint32_t levels, fmd_esearch_hit_t *d_hits, uint64_t hit_cap, uint64_t *d_strata,
                    fmd_esearch_stat_t *d_stat, void *d_work, size_t work_bytes);
int fmd_esearch_batch(fmd_dev_t *h, size_t n, const uint8_t *seqs, const uint64_t *off, int max_edit, uint32_t max_hits, unsigned flags,
                      uint64_t cap, fmd_esearch_hit_t **hits, uint64_t *n_hits, uint64_t *strata, fmd_esearch_stat_t *stat);

/* ---- inspection (`fermi chkbwt`, cmd.c:47-130) ------------------------------------------------
 * export: BWT[first, first+n) as nt6 bytes, decoded from the device layout (chkbwt -p).
 * check_rank: the device layout's rank of every position against the symbols themselves (chkbwt -r):
 * n_bad = positions whose six counts are not those of the previous position plus the symbol there (or,
 * at the last position, not the marginal counts); first_bad = the smallest of them. */
int fmd_dev_export_bwt(fmd_dev_t *h, uint64_t first, uint64_t n, uint8_t *bwt);
int fmd_dev_check_rank(fmd_dev_t *h, uint64_t *n_bad, uint64_t *first_bad);
/* The two-base blocks (32 bits per symbol beside the 8 of the rank blocks; fmd_pair.hip): what the sorted overlap job reads below min_match, two bases per
 * 128-byte line where the rank blocks give one per 64-byte line -- same results, fewer requests.  The job builds them on first use where they fit
 * (FMD_PAIR=0: never, FMD_PAIR=1: whenever the allocation succeeds); this call builds them now (*built = 1 when the handle has them).  The
 * reference has nothing like it: rld_rank2a (rld.c:457) is asked once per base (unitig.c:47-59, exact.c:59-70).
 * fmd_dev_check_pairs: every row's pair step against two single LF steps (FMD_E_ARG when the handle has no two-base blocks). */
int fmd_dev_build_pairs(fmd_dev_t *h, int *built);
int fmd_dev_check_pairs(fmd_dev_t *h, uint64_t *n_bad, uint64_t *first_bad);

/* ---- forward reach ("matching statistics") --------------------------------------------------
 * seqs: n_bytes of nt6 sequences, each followed by at least one 0 byte (the _dev form: 4-byte
 * aligned, a 0 byte at or after seqs[n_bytes - 1], readable to the next multiple of 4).  len[p] = length of
 * the longest prefix of seqs[p ..] (up to its terminator) that occurs in the index; 0 at terminators and
 * at bases the index does not contain.  x -> x + len[x] is the chain of start positions that
 * fm6_miter_next / fm6_smem walk (smem.c:46, :96-102, :404-409): with it, every fm6_smem1_core call
 * of a long sequence is known up front and independent (fmd_smem_win_* with stop = start + 1). */
int fmd_reach_dev(fmd_dev_t *h, void *stream, size_t n_bytes, const uint8_t *d_seqs, uint32_t *d_len);
int fmd_reach_batch(fmd_dev_t *h, size_t n_bytes, const uint8_t *seqs, uint32_t *len);

/* ---- super-maximal exact matches: fm6_smem (smem.c:397-410) = repeated fm6_smem1_core
 * (smem.c:13-80); what `fermi exact [-s]` prints (cmd.c:319-327, smem.c:412-418).
 * mem: n rows of max_mem intervals in the reference's order; info = leftclosed<<63 | beg<<32 | end
 * (FM_MASK30 fields, smem.c:63).  n_mem[i] = number of SMEMs of read i; bit 31 set = the read was
 * longer than max_len or produced more than max_mem SMEMs (row invalid: re-run larger).  The low 31
 * bits: 0 for a read longer than max_len (nothing was computed, its row is not touched); else, when
 * only max_mem was too small, the TRUE number of SMEMs of the read, so the caller knows the max_mem that
 * fits.  (Windows: a candidate list that outgrew 2 * max_len + 2 entries also sets bit 31, and the low
 * bits then count what an incomplete list gave: meaningless.)  An overflowing read writes nothing outside
 * its own row and its lane's part of the work area; the other reads of the launch are unaffected.
 * A start the reference leaves undefined -- a base q[x] the index does not hold, or (self_match) a forward
 * sweep that pushes no interval because every occurrence of q[x] ends its sequence, where fm6_smem1_core
 * reads a[0] of an empty vector -- ends the read: n_mem = the SMEMs found before it, bit 31 clear.
 * d_seqs: 4-byte aligned and readable up to the next multiple of 4 past off[n] (the kernels read
 * the sequences one aligned word at a time); same for fmd_bsearch_dev. */
size_t fmd_smem_work_bytes(size_t n, uint32_t max_len);
int fmd_smem_dev(fmd_dev_t *h, void *stream, size_t n, const uint8_t *d_seqs, const uint64_t *d_off, int self_match,
                 uint32_t max_len, uint32_t max_mem, fmd_intv_t *d_mem, uint32_t *d_n_mem, void *d_work, size_t work_bytes);
/* The same chain over WINDOWS of long sequences (what fm6_miter_next does over a contig in `fermi
 * remap`, smem.c:96-102, :151): item i = start positions [start, stop) of the sequence of seq_len
 * bases at seqs + seq_off.  The union over a partition of a sequence into windows is its SMEM set;
 * an SMEM covering a window boundary may be reported by both windows.  max_len = longest match
 * possible (longest sequence in the index + 1). */
typedef struct { uint64_t seq_off; uint32_t seq_len, start, stop, reserved /* flags */; } fmd_smem_win_t;
#define FMD_SMEM_WIN_F_FULL 1u   /* keep only matches closed by a sentinel on both sides (what remap consumes) */
int fmd_smem_win_dev(fmd_dev_t *h, void *stream, size_t n, const uint8_t *d_seqs, const fmd_smem_win_t *d_wins, int self_match,
                     uint32_t max_len, uint32_t max_mem, fmd_intv_t *d_mem, uint32_t *d_n_mem, void *d_work, size_t work_bytes);
int fmd_smem_win_batch(fmd_dev_t *h, size_t n, const uint8_t *seqs, uint64_t seq_bytes, const fmd_smem_win_t *wins, int self_match,
                       uint32_t max_len, uint32_t max_mem, fmd_intv_t *mem, uint32_t *n_mem);
int fmd_smem_batch(fmd_dev_t *h, size_t n, const uint8_t *seqs, const uint64_t *off, int self_match, uint32_t max_len,
                   uint32_t max_mem, fmd_intv_t *mem, uint32_t *n_mem);

/* ---- overlap discovery for unitig construction --------------------------------------------
 * One record per sequence id: the read-only front half of unitig1 (unitig.c:274-300), i.e.
 *   fm_retrieve (exact.c:59) + seq_reverse + fm6_is_contained (unitig.c:77) +
 *   fm6_get_nei(beg = 0, used = NULL, sorted = NULL) (unitig.c:93)
 * which SURVEY.md (fact 3) shows is a pure function of (index, id) and is exactly what the
 * deterministic `fermi unitig -t1` walk consumes.  `rank`, k[0] and k[1] are in the coordinate
 * system of the reference's used/bend/visited bitmaps (unitig.c:289, 299). */
#define FMD_OVLP_SHORT      (-1)  /* len <= min_match (unitig.c:288) */
#define FMD_OVLP_CONTAINED  (-3)  /* fm6_is_contained < 0 (unitig.c:292) */
#define FMD_OVLP_F_FORKED   1u    /* more than one category survived a round (unitig.c:152) */
#define FMD_OVLP_F_OVERFLOW 2u    /* a capacity (max_len, list, max_nei) was exceeded: record invalid, re-run larger */
#define FMD_OVLP_F_FIXED    4u    /* the fake-fork fix-up of unitig.c:158-176 ran */
#define FMD_OVLP_F_PACK4    8u    /* packed rows only (fmd_ovlp_pack_dev): the bases are stored 2 per byte, not 4 */
typedef struct {
    uint64_t rank;     /* fm_retrieve's return value */
    uint64_t k[3];     /* *intv of fm6_is_contained: bi-interval of `$read$` */
    int32_t len;       /* sequence length */
    int32_t status;    /* 0, FMD_OVLP_SHORT or FMD_OVLP_CONTAINED */
    int32_t n_ovlp;    /* candidate intervals from overlap_intv (unitig.c:47-58) */
    int32_t rbeg;      /* fm6_get_nei's return value; -1 = no overlap */
    int32_t ext_len;   /* bases fm6_get_nei appended to the sequence */
    int32_t n_nei;     /* irreducible neighbours found */
    uint32_t flags;    /* FMD_OVLP_F_* */
    uint16_t reserved; /* check_left_simple (unitig.c:186) for the edge to the unique neighbour, when it was computed
                          for this row (fmd_ovlp_check_left_dev): 0 = passes, 1 = potential backward bifurcation (-1);
                          2 = not computed / not applicable */
    uint16_t lfork;    /* what fm6_get_nei's rounds on THIS strand X say about check_left_simple on any edge S -> N whose
                          neighbour N is the reverse complement of X (FMD_LFORK_*): the reads check_left_simple collects on
                          N and pulls back over S are the candidates of X extended forward, round for round */
} fmd_ovlp_rec_t;      /* 64 bytes */
/* lfork = D << 15 | R:  rounds 0 .. R-1 saw every read that starts inside X with >= min_match bases either end or go on
 * with one and the same base (R = FMD_LFORK_ALL: all of them ended, nothing can ever disagree); D = 1: round R has two
 * different bases.  For an edge S -> N with rbeg = fm6_get_nei's return value on S (the walk's check_left_simple(beg = 0,
 * rbeg), unitig.c:186-204 visits rounds 0 .. rbeg-1):   rbeg <= R  => 0;   D && R < rbeg  => -1;   otherwise not
 * decided by this row (lfork = 0 decides nothing) and fmd_ovlp_check_left_dev has to be run on S. */
#define FMD_LFORK_ALL 0x7fffu
static inline int fmd_lfork_decide(uint16_t lfork, int rbeg) /* 0 / -1 as check_left_simple, 1 = undecided */
{
    const int r = lfork & 0x7fff;
    if (rbeg <= r || r == (int)FMD_LFORK_ALL) return 0;
    return (lfork & 0x8000) ? -1 : 1;
}
/* capacity of the per-strand candidate lists kept in the work area: overlap_intv (unitig.c:47-58) pushes at most one
 * interval per suffix longer than min_match, and a round of fm6_get_nei keeps more children than it had parents only
 * where the read set forks -- a strand that needs more sets FMD_OVLP_F_OVERFLOW and is re-run with larger capacities */
static inline uint32_t fmd_ovlp_list_cap(uint32_t max_len, int min_match)
{
    uint32_t d = max_len > (uint32_t)min_match ? max_len - (uint32_t)min_match : 1;
    return d + 8 < 16 ? 16 : d + 8;
}
size_t fmd_ovlp_work_bytes(size_t n, uint32_t max_len, int min_match);
/* d_nei: n x max_nei neighbours {x[0], x[1], x[2] of `$neighbour$`, info = overlap length};
 * d_seq: n rows of seq_stride bytes = the sequence in read order followed by the ext_len appended
 * bases (seq_stride >= 2*max_len is always enough).
 * Stream order is the caller's: the call starts after the work already queued on `stream` and its results
 * belong to `stream` when it returns, although a batch of 2^21 strands or more also runs kernels on a
 * second, library-owned stream in between (joined by events, no host synchronisation). */
int fmd_ovlp_dev(fmd_dev_t *h, void *stream, size_t n, const uint64_t *d_ids, int min_match, uint32_t max_len,
                 uint32_t max_nei, fmd_ovlp_rec_t *d_rec, fmd_intv_t *d_nei, uint8_t *d_seq, uint32_t seq_stride,
                 void *d_work, size_t work_bytes);
/* The same records for ALL n ids in one call, computed in an order that keeps neighbours on the genome in flight together
 * (fm6_unitig hands its workers the ids in input order, unitig.c:394-404; any order gives the same records, and the order decides
 * how often a rank block is found in cache).  Two strands whose last bases lie d positions apart on the genome visit the same rank
 * blocks d steps apart; in input order each such visit is a DRAM miss.  Pass 1 takes every strand 32 bases in and parks it (64 bytes
 * per strand); the strands are sorted by the minimizer of those 32 bases; pass 2 + fm6_get_nei then run batch by batch in that
 * order and write row i of d_rec / d_nei / d_seq for ids[i] with the contents fmd_ovlp_dev gives them: the record in full, the first
 * min(n_nei, max_nei) neighbours, the first len + ext_len bytes of the sequence row (bytes of a row beyond those are unspecified in both).  `batch` strands share the work
 * area of one fmd_ovlp_dev call (0 = n); work_bytes >= fmd_ovlp_sorted_work_bytes(n, batch, ..).  Where the two-pass form does not
 * apply (min_match < 32, FMD_OVLP_SORT=0) the batches are taken in id order. */
size_t fmd_ovlp_sorted_work_bytes(size_t n, size_t batch, uint32_t max_len, int min_match);
int fmd_ovlp_sorted_dev(fmd_dev_t *h, void *stream, size_t n, const uint64_t *d_ids, int min_match, uint32_t max_len,
                        uint32_t max_nei, fmd_ovlp_rec_t *d_rec, fmd_intv_t *d_nei, uint8_t *d_seq, uint32_t seq_stride,
                        void *d_work, size_t work_bytes, size_t batch);
/* Rows that exceeded a capacity, again, alone, larger.  fm6_get_nei has no capacities (its vectors grow, unitig.c:93-179); a row of the calls above
 * that needs more than max_nei neighbours, a longer candidate list or more bases than max_len carries FMD_OVLP_F_OVERFLOW instead of a
 * result.  This entry collects the flagged rows of a finished job on the device (d_side_ids[k] = their ids -- d_ids[i], or i when d_ids is
 * NULL --, d_side_rows[k] = their rows, any order; d_side_rows may be NULL) and runs them through fmd_ovlp_dev with the capacities named
 * here into the side arrays (row k of d_side_rec / d_side_nei [max_nei per row] / d_side_seq [side_stride per row]).  *n_side = rows
 * collected (FMD_E_OVERFLOW when they exceed side_cap: nothing was run), *n_still = rows of the side table that are flagged again
 * (call again on the side table with larger capacities).  Synchronises the stream twice (the counts come back to the host). */
size_t fmd_ovlp_side_work_bytes(size_t side_cap, uint32_t max_len, int min_match);
int fmd_ovlp_rerun_overflow_dev(fmd_dev_t *h, void *stream, size_t n, const uint64_t *d_ids, const fmd_ovlp_rec_t *d_rec, int min_match, uint32_t max_len,
                                uint32_t max_nei, uint64_t side_cap, uint64_t *d_side_ids, uint32_t *d_side_rows, fmd_ovlp_rec_t *d_side_rec, fmd_intv_t *d_side_nei,
                                uint8_t *d_side_seq, uint32_t side_stride, void *d_work, size_t work_bytes, uint64_t *n_side, uint64_t *n_still);
/* Optional second step over the same buffers: check_left_simple (unitig.c:186-204) for every
 * strand with a unique neighbour -> rec.reserved (the unitig walk needs it; plain overlap
 * discovery does not, and records of fmd_ovlp_dev alone carry reserved = 2). */
int fmd_ovlp_check_left_dev(fmd_dev_t *h, void *stream, size_t n, int min_match, uint32_t max_len, fmd_ovlp_rec_t *d_rec,
                            const uint8_t *d_seq, uint32_t seq_stride, void *d_work, size_t work_bytes);
int fmd_ovlp_batch(fmd_dev_t *h, size_t n, const uint64_t *ids, int min_match, uint32_t max_len, uint32_t max_nei,
                   fmd_ovlp_rec_t *rec, fmd_intv_t *nei, uint8_t *seq, uint32_t seq_stride, int with_check_left);

/* ---- compact form of a finished batch: what leaves the GPU (PCIe to the host walk, xGMI to rank 0) ----------
 * The walk (unitig.c:227-317) reads from a row its record, its n_nei neighbours and len + ext_len bases.  Row i becomes
 *   d_prec[i]          the record (flags gains FMD_OVLP_F_PACK4 when the row holds a base other than A/C/G/T)
 *   d_var + d_off[i]   min(n_nei, max_nei) neighbours (32 bytes each), then len + ext_len bases, 4 per byte as
 *                      (base - 1) in 2 bits, first base in the low bits -- or nt6 codes 2 per byte with PACK4 --
 *                      padded to 8 bytes; empty for rows with status != 0 or FMD_OVLP_F_OVERFLOW
 * d_off has n + 1 entries; rows that would end past var_cap are not written (compare d_off[n] with var_cap;
 * fmd_ovlp_pack_max_bytes is always enough).  seq_stride must be a multiple of 8 (FMD_E_ARG otherwise). */
size_t fmd_ovlp_pack_max_bytes(size_t n, uint32_t max_nei, uint32_t seq_stride);
size_t fmd_ovlp_pack_work_bytes(size_t n);
int fmd_ovlp_pack_dev(fmd_dev_t *h, void *stream, size_t n, const fmd_ovlp_rec_t *d_rec, const fmd_intv_t *d_nei, uint32_t max_nei,
                      const uint8_t *d_seq, uint32_t seq_stride, fmd_ovlp_rec_t *d_prec, uint64_t *d_off, uint8_t *d_var, uint64_t var_cap,
                      void *d_work, size_t work_bytes);

/* The link pass over a COMPLETE table on one device (rows = sequence ids 0 .. n-1, fixed-stride records): row_of[k] = the
 * smallest id whose `$read$` interval starts at k; link[i] = rows of the unique neighbour of i and of its reverse strand
 * (what the walk's `cur = neighbour` and check_left's second look need, unitig.c:206-262); rec[i].reserved = 0 / 1 where
 * the lfork of the neighbour's reverse strand decides check_left_simple, left at 2 elsewhere -- those ids are appended
 * to d_undecided (any order; n capacity) for fmd_ovlp_check_left_dev, which only looks at rows still at 2.
 * d_nei_x01: x[0], x[1] of each row's first neighbour at d_nei_x01[i * nei_stride_u64] (a fmd_intv_t array: stride
 * 4 * max_nei; a compact copy: 2). */
typedef struct { uint32_t nxt, rev; } fmd_ovlp_link_t;
int fmd_ovlp_link_dev(fmd_dev_t *h, void *stream, size_t n, fmd_ovlp_rec_t *d_rec, const uint64_t *d_nei_x01, uint32_t nei_stride_u64,
                      uint32_t *d_row_of, fmd_ovlp_link_t *d_link, uint64_t *d_undecided, uint64_t *d_n_undecided);

/* Host form, pipelined: the packed table of one shard of sequence ids -- ids[0..n) when ids != NULL, else
 * first, first + step, ... (the reference's worker interleave, unitig.c:333, 398-399).  Chunks of 2^chunk_shift rows
 * are computed (fmd_ovlp_dev, fmd_ovlp_check_left_dev when asked, fmd_ovlp_pack_dev) while the previous chunk crosses
 * PCIe.  rec[n], off[n] (byte offset of row i inside chunks[i >> chunk_shift]); chunks[] receives
 * ceil(n / 2^chunk_shift) buffers the caller releases with fmd_ovlp_packed_free().  The end of row i's variable part
 * follows from its record (fmd_ovlp_row_bytes). */
int fmd_ovlp_packed_batch(fmd_dev_t *h, const uint64_t *ids, uint64_t first, uint64_t step, size_t n, int min_match, uint32_t max_len,
                          uint32_t max_nei, int with_check_left, fmd_ovlp_rec_t *rec, uint64_t *off, uint32_t chunk_shift, uint8_t **chunks);
void fmd_ovlp_packed_free(uint8_t **chunks, size_t n_chunks);
/* Host memory for tables that are filled once and then read at random -- the chunks above come from here, and a caller that keeps
 * rec / off / row_of / link for a whole .fmd (the reference keeps nothing of the kind: it recomputes, unitig.c:274-300) should too.
 * Default: malloc; large blocks 2 MiB-aligned with transparent huge pages on request.  With FMD_TABLE_DIR=<dir> in the environment,
 * blocks of FMD_TABLE_DIR_MIN bytes (default 32 MiB) and more are pages of unlinked files in <dir> (mmap, MAP_SHARED): the table of a
 * large .fmd then lives in the page cache and on <dir>'s device instead of in anonymous memory, and `unitig` of BASELINE's 7*10^8
 * reads (~ 190 GB of table) runs in whatever RAM the host has, at the speed of that device once the table no longer fits.
 * fmd_table_free() accepts any pointer fmd_table_alloc() returned (and, like free(), NULL). */
void *fmd_table_alloc(size_t bytes);
void fmd_table_free(void *p);
/* The whole table (ids 0 .. n-1) on ONE device: the packed rows as above (no per-row check_left), then fmd_ovlp_link_dev on
 * the device: row_of[n], link[n], rec[i].reserved = check_left_simple's verdict wherever lfork decides it; the ids it leaves
 * open come back in *undecided (malloc'ed: fmd_host_free; ascending) for a fmd_ovlp_packed_batch(ids, with_check_left = 1). */
int fmd_ovlp_packed_table(fmd_dev_t *h, size_t n, int min_match, uint32_t max_len, uint32_t max_nei, fmd_ovlp_rec_t *rec, uint64_t *off,
                          uint32_t chunk_shift, uint8_t **chunks, uint32_t *row_of, fmd_ovlp_link_t *link, uint64_t **undecided, uint64_t *n_undecided);
/* Streamed forms of the two entries above: the packed chunks (2^chunk_shift rows each, in the order of the ids) are handed to fn from
 * pinned staging buffers -- first_row = the chunk's first row of the call, rec[n_rows], off[n_rows] (offsets into var), var_bytes of var --
 * and are the library's again when fn returns (non-zero: the call stops and returns it).  fn runs on the calling thread while the next
 * chunk is computed and the one after crosses PCIe.  Nothing of the table stays in host memory unless fn keeps it: `unitig` keeps
 * ~58 bytes per row (host/slim_table.c) where the reference keeps three bitmaps (unitig.c:390-392) and recomputes. */
typedef int (*fmd_ovlp_rows_fn)(void *ctx, uint64_t first_row, size_t n_rows, const fmd_ovlp_rec_t *rec, const uint64_t *off, const uint8_t *var, uint64_t var_bytes);
int fmd_ovlp_packed_stream(fmd_dev_t *h, const uint64_t *ids, uint64_t first, uint64_t step, size_t n, int min_match, uint32_t max_len,
                           uint32_t max_nei, int with_check_left, uint32_t chunk_shift, fmd_ovlp_rows_fn fn, void *ctx);
/* fmd_ovlp_packed_table as a job in three steps, so that the link pass sees the rows as they are in the END:
 *   rows   ids 0 .. n-1 streamed to fn; the job keeps the fixed-stride records and the first neighbour's coordinates on the device
 *   patch  rows the caller has computed again since (flagged FMD_OVLP_F_OVERFLOW by the first step): rec[m], nei01[2 m] = x[0], x[1] of each
 *          row's first neighbour, replace the job's copies at ids[m]
 *   link   fmd_ovlp_link_dev over the job's records; link[n_rows] and reserved[n_rows] (0 / 1 / 2 as rec.reserved) go to fn in pieces of
 *          2^22 rows; *undecided as fmd_ovlp_packed_table returns it */
typedef struct fmd_ovlp_tabjob fmd_ovlp_tabjob_t;
typedef int (*fmd_ovlp_links_fn)(void *ctx, uint64_t first_row, size_t n_rows, const fmd_ovlp_link_t *link, const uint8_t *reserved);
int fmd_ovlp_tabjob_rows(fmd_dev_t *h, size_t n, int min_match, uint32_t max_len, uint32_t max_nei, uint32_t chunk_shift,
                         fmd_ovlp_rows_fn fn, void *ctx, fmd_ovlp_tabjob_t **job);
int fmd_ovlp_tabjob_patch(fmd_ovlp_tabjob_t *job, size_t m, const uint64_t *ids, const fmd_ovlp_rec_t *rec, const uint64_t *nei01);
int fmd_ovlp_tabjob_link(fmd_ovlp_tabjob_t *job, fmd_ovlp_links_fn fn, void *ctx, uint64_t **undecided, uint64_t *n_undecided);
void fmd_ovlp_tabjob_free(fmd_ovlp_tabjob_t *job);
/* layout of a packed row's variable part, from its (packed) record */
static inline uint32_t fmd_ovlp_row_nei(const fmd_ovlp_rec_t *r, uint32_t max_nei)
{
    if (r->status != 0 || (r->flags & FMD_OVLP_F_OVERFLOW)) return 0;
    return (uint32_t)r->n_nei < max_nei ? (uint32_t)r->n_nei : max_nei;
}
static inline uint32_t fmd_ovlp_row_bytes(const fmd_ovlp_rec_t *r, uint32_t max_nei, uint32_t seq_stride)
{
    uint32_t nb, sb;
    if (r->status != 0 || (r->flags & FMD_OVLP_F_OVERFLOW)) return 0;
    nb = (uint32_t)r->len + (uint32_t)r->ext_len;
    if (nb > seq_stride) nb = seq_stride;
    sb = (r->flags & FMD_OVLP_F_PACK4) ? (nb + 1) / 2 : (nb + 3) / 4;
    return fmd_ovlp_row_nei(r, max_nei) * 32 + ((sb + 7) & ~7u);
}
/* base j of a packed row (nt6 code) */
static inline int fmd_ovlp_row_base(const fmd_ovlp_rec_t *r, uint32_t max_nei, const uint8_t *var, uint32_t j)
{
    const uint8_t *s = var + fmd_ovlp_row_nei(r, max_nei) * 32;
    return (r->flags & FMD_OVLP_F_PACK4) ? (s[j >> 1] >> (4 * (j & 1))) & 15 : ((s[j >> 2] >> (2 * (j & 3))) & 3) + 1;
}

/* ---- the sorted job in its two halves ----------------------------------------------------------------------------
 * fmd_ovlp_sorted_dev = fmd_ovlp_head_dev, then fmd_ovlp_tail_dev over slices of d_order.  A caller that wants to do something
 * between the two -- hand finished rows on while the rest is being computed, exchange the parked strands between GPUs by key
 * (fmd_ovlp_dist_*) -- calls them itself.  fmd_ovlp_two_pass_ok: can this index / these parameters use the two-pass form at all
 * (min_match >= 32, ...)?
 * head: pass 1 of every strand (32 bases in), d_park[n] = 64 bytes per strand, d_keys[n] = the minimizer keys ascending,
 *       d_order[n] = row of the t-th strand in that order; d_rec receives the final record of strands that end inside the head
 *       (shorter than 32 bases: status FMD_OVLP_SHORT; their key is 0xffffffff).
 * tail: pass 2 + fm6_get_nei for np parked strands, slot t of the call = row d_rows[t] of d_park, d_rec, d_nei, d_seq;
 *       work_bytes >= fmd_ovlp_work_bytes(np, ..). */
int fmd_ovlp_two_pass_ok(const fmd_dev_t *h, size_t n, int min_match, uint32_t max_len);
size_t fmd_ovlp_head_work_bytes(size_t n);
int fmd_ovlp_head_dev(fmd_dev_t *h, void *stream, size_t n, const uint64_t *d_ids, int min_match, uint32_t max_len, fmd_ovlp_rec_t *d_rec,
                      void *d_park, uint32_t *d_keys, uint32_t *d_order, void *d_work, size_t work_bytes);
int fmd_ovlp_tail_dev(fmd_dev_t *h, void *stream, size_t np, const uint32_t *d_rows, void *d_park, int min_match, uint32_t max_len, uint32_t max_nei,
                      fmd_ovlp_rec_t *d_rec, fmd_intv_t *d_nei, uint8_t *d_seq, uint32_t seq_stride, void *d_work, size_t work_bytes);
/* fmd_ovlp_pack_dev for the rows d_rows[0..n) of the fixed-stride arrays, in that order ("a piece"): output row t is row d_rows[t];
 * d_pid[t] = its sequence id: d_row_ids[d_rows[t]] when d_row_ids != NULL, else id_first + id_step * d_rows[t]. */
int fmd_ovlp_pack_rows_dev(fmd_dev_t *h, void *stream, size_t n, const uint32_t *d_rows, const uint64_t *d_row_ids, uint64_t id_first, uint64_t id_step,
                           const fmd_ovlp_rec_t *d_rec, const fmd_intv_t *d_nei, uint32_t max_nei, const uint8_t *d_seq, uint32_t seq_stride,
                           uint32_t *d_pid, fmd_ovlp_rec_t *d_prec, uint64_t *d_off, uint8_t *d_var, uint64_t var_cap, void *d_work, size_t work_bytes);

/* ---- N GPUs: the exchange steps of the overlap path behind the C ABI ---------------------------------------------
 * The reference joins N workers over one shared index at no cost (pthreads, unitig.c:394-404); N GPUs hold N replicas of the index
 * and the only data that has to move is (a) the finished rows, to the rank that runs the walk, and (b) -- optional -- the parked
 * strands between pass 1 and pass 2, so that every GPU runs pass 2 on ONE RANGE OF MINIMIZER KEYS of the whole read set instead of on
 * 1/N of the coverage everywhere (strands of one genomic window meet on one GPU and share rank blocks in cache).
 *
 * fmd_comm_t is the transport: two collective calls on DEVICE buffers, enqueued on a HIP stream.  fmd_comm_rccl_* is the one that
 * ships (RCCL over xGMI: ncclAllGather; ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd -- direct, every peer on its own link to
 * the root, no ring); a host may plug in its own (MPI, sockets; the tests plug in torch.distributed/gloo). */
typedef struct { int is_recv, peer; void *d_ptr; size_t bytes; } fmd_comm_op_t;
typedef struct fmd_comm {
    int rank, world;
    void *ctx;
    /* every rank contributes `bytes` from d_send; d_recv receives world x bytes in rank order */
    int (*allgather)(void *ctx, void *stream, const void *d_send, void *d_recv, size_t bytes);
    /* one group of point-to-point transfers (matching sends and receives are posted by the peers in the same call) */
    int (*exchange)(void *ctx, void *stream, int n_ops, const fmd_comm_op_t *ops);
    void (*destroy)(void *ctx);
} fmd_comm_t;
#define FMD_COMM_ID_BYTES 128
int fmd_comm_rccl_unique_id(uint8_t id[FMD_COMM_ID_BYTES]);                       /* ncclGetUniqueId: rank 0 calls, the host carries it to the others */
int fmd_comm_rccl_init(int device, int rank, int world, const uint8_t id[FMD_COMM_ID_BYTES], fmd_comm_t **out);   /* ncclCommInitRank */
int fmd_comm_rccl_version(void);                                                 /* ncclGetVersion; 0 = librccl not loadable */
int fmd_comm_rccl_count(const fmd_comm_t *c);                                    /* ncclCommCount of a communicator made by fmd_comm_rccl_init; -1 otherwise */
void fmd_comm_free(fmd_comm_t *c);                                               /* calls destroy(ctx) and frees c if fmd_comm_rccl_init made it */

/* One pass of overlap discovery over the sequence ids 0 .. n_ids-1 on `world` GPUs, rank r on its own replica of the index:
 *   pass 1 on the ids r, r + world, ... (the reference's worker interleave, unitig.c:333, 398-399);
 *   key_shard: one all-to-all of the parked strands (64 bytes each) by minimizer key range;
 *   pass 2 + fm6_get_nei in `pieces` batches of the sorted order; while batch p + 1 is computed, the rows of batch p are packed
 *   on a second stream and sent to `root` (fmd_ovlp_pack_rows_dev; ids, records, offsets, variable parts).
 * On return (stream-ordered on `stream` for the caller's later work; the call itself synchronises with the host between pieces)
 * the root holds all n_ids rows: fmd_ovlp_dist_table().  The object keeps every buffer between steps. */
typedef struct fmd_ovlp_dist fmd_ovlp_dist_t;
typedef struct {
    uint64_t n_ids;
    int min_match;
    uint32_t max_len, max_nei;
    uint32_t pieces;        /* 0 = default (4, fewer for small shards) */
    int key_shard;          /* 0 / 1; where the two-pass form does not apply (fmd_ovlp_two_pass_ok) the shard is computed in id order */
    int root;
    int host_table;         /* root: 0 = the table stays in HBM, 1 = in pinned host memory (pieces staged through HBM), -1 = by free HBM, 2 = no table: row_sink below */
    size_t batch;           /* 0 = a piece is one batch; else pieces are cut further so that no batch exceeds this many strands */
    /* host_table = 2 (the same on every rank): the root keeps NO table.  Every piece of every peer, once it has landed in pinned host memory, is handed to
     * row_sink -- n_rows packed rows as fmd_ovlp_pack_rows_dev writes them: ids[n_rows], prec[n_rows], off[n_rows + 1] into var -- on the thread that runs the
     * step, while the GPUs compute and pack the next piece; the buffers are reused two pieces later.  What unitig.c:394-404 does by joining its workers into
     * one graph: here the consumer (fmdh_dist_root_sink, fermi_amd/host/ovlp_table.c, folds the rows into the 44.5-byte rows `unitig` walks) takes them as they arrive, and the
     * root's memory is what the consumer keeps.  A non-zero return fails the step on every rank (FMD_E_IO).  Only the root's row_sink / sink_ctx are read.
     * A step that fails (any rank, any reason) has handed the sink SOME of its pieces: what the consumer holds then is incomplete -- it starts over. */
    int (*row_sink)(void *ctx, uint64_t n_rows, const uint32_t *ids, const fmd_ovlp_rec_t *prec, const uint64_t *off, const uint8_t *var, uint32_t max_nei);
    void *sink_ctx;
} fmd_ovlp_dist_cfg_t;
typedef struct {            /* of the last step, this rank; milliseconds from HIP events / the host clock */
    double head_ms, key_exchange_ms, tail_ms;      /* compute stream: pass 1 + sort; the all-to-all and the re-sort; all pieces of pass 2 */
    double last_piece_pack_send_ms;                /* comm stream: pack + transfer of the LAST piece (what cannot hide under compute) */
    double gather_exposed_ms;                      /* HIP events: end of this rank's last compute kernel -> end of its part in the gather */
    double step_ms;                                /* host clock, whole step */
    uint64_t rows_computed, rows_sent, bytes_sent, bytes_received, key_rows_sent;
    int pieces, on_host /* 2: rows went to cfg.row_sink */, key_shard, two_pass;
} fmd_ovlp_dist_stats_t;
typedef struct {            /* root only: the table of the last step */
    int on_host;                  /* the arrays below are device (0) or pinned host (1) memory */
    uint64_t n_rows;              /* = n_ids when the step is complete */
    const fmd_ovlp_rec_t *prec;   /* records in arrival order (packed form: fmd_ovlp_pack_dev) */
    const uint32_t *ids;          /* sequence id of each row */
    const uint64_t *vaddr;        /* address of each row's variable part (same memory kind) */
    const uint32_t *row_of_id;    /* n_ids entries: the row that holds sequence id i */
} fmd_ovlp_dist_table_t;
int fmd_ovlp_dist_new(fmd_dev_t *h, fmd_comm_t *comm, const fmd_ovlp_dist_cfg_t *cfg, fmd_ovlp_dist_t **out);
int fmd_ovlp_dist_step(fmd_ovlp_dist_t *d, void *stream, fmd_ovlp_dist_stats_t *stats);
int fmd_ovlp_dist_table(fmd_ovlp_dist_t *d, fmd_ovlp_dist_table_t *t);     /* FMD_E_ARG on a job whose rows went to a sink */
/* this rank's own fixed-stride rows of the last step (tests, parity samples): row j describes sequence id ids[j] */
int fmd_ovlp_dist_local(fmd_ovlp_dist_t *d, uint64_t *n_rows, const uint64_t **d_ids, const fmd_ovlp_rec_t **d_rec, const fmd_intv_t **d_nei, const uint8_t **d_seq, uint32_t *seq_stride);
void fmd_ovlp_dist_free(fmd_ovlp_dist_t *d);

/* ---- k-mer harvest of `fermi correct`: fm6_traverse (exact.c:141) + ec_collect (correct.c:35-87)
 * over ALL 4^suf_len suffix buckets (what worker1 does, correct.c:272-279).  Emits one
 * (bucket, key, val) triple per solid k-mer: bucket = index into `solid[]` (correct.c:346-349),
 * key/val exactly what kh_put/kh_val store (correct.c:71-75).  The order of triples is
 * unspecified for the _dev form (the reference's own order is hash-table iteration order); the host
 * form returns them sorted by (bucket, key), or -- for an index whose frontiers do not fit beside it -- as four sorted parts.  w <= 27, w - suf_len <= 15,
 * suf_len <= 16 (a bucket is 32 bits; fmd_ectab_build* asks the same): anything else is FMD_E_ARG.  FMD_KMER_CAP0 (read per call, at least 1 << 16;
 * default 1 << 22) is the capacity the host forms start from before they grow it.
 * d_status (4 x u64): [0] #triples, [1] non-zero = cap overflowed (re-run larger), [2] cnt[0],
 * [3] cnt[1] (correct.c:64-69). */
size_t fmd_kmer_work_bytes(uint64_t cap);
int fmd_kmer_collect_dev(fmd_dev_t *h, void *stream, int w, int min_occ, int suf_len, void *d_work, size_t work_bytes,
                         uint64_t cap, uint32_t *d_bucket, uint32_t *d_key, uint8_t *d_val, uint64_t *d_status);
/* the part of the harvest whose k-mers end in a base of seed_mask (bit c-1 = nt6 base c; 0xf = all): the trie is a forest
 * rooted at the last base, the parts are disjoint and each needs about a quarter of the frontier */
int fmd_kmer_collect_part_dev(fmd_dev_t *h, void *stream, int w, int min_occ, int suf_len, int seed_mask, void *d_work, size_t work_bytes,
                              uint64_t cap, uint32_t *d_bucket, uint32_t *d_key, uint8_t *d_val, uint64_t *d_status);
int fmd_kmer_collect(fmd_dev_t *h, int w, int min_occ, int suf_len, uint32_t **bucket, uint32_t **key, uint8_t **val,
                     uint64_t *n, int64_t cnt[2]);
/* The same for the k-mers that END in one of the bases of seed_mask (bit c-1 = base c): one GPU's shard of a harvest spread over
 * several (`fermi-amd correct -g`; the reference shards ec_collect over its threads by suffix bucket, correct.c:346-356).  Disjoint
 * masks covering 0xf give, together, exactly the triples of fmd_kmer_collect. */
int fmd_kmer_collect_seeds(fmd_dev_t *h, int w, int min_occ, int suf_len, int seed_mask, uint32_t **bucket, uint32_t **key, uint8_t **val,
                           uint64_t *n, int64_t cnt[2]);   /* outputs malloc'ed: fmd_host_free() */

/* ---- the correction pass of `fermi correct`: ec_fix1 / ec_fix (correct.c:121-256) ------------------------------
 * The table is what fmd_kmer_collect* returns (one triple per solid k-mer, any order), loaded into a device hash
 * table: a look-up kh_get(solid[x & (SUF_NUM-1)], x >> 2*SUF_LEN << 2) (correct.c:156-157) is one 8-byte load.
 * fmd_ecfix_*: read i = bytes [off[i], off[i+1]) of seqs (nt6 codes) and quals (phred + 33).  Both are rewritten in
 * place exactly as ec_fix leaves str.s and qual[i] after its two ec_fix1 passes (correct.c:237-243); info[i] = the
 * value ec_fix holds at correct.c:246, before the lower-case count (correct.c:247-252, host).  A lane keeps its best-
 * first queue (<= 256 paths, correct.c:114) and its trace in d_work; a read whose trace exceeds trace_cap gets
 * info = FMD_ECFIX_TRACE_FULL and must be run again FROM ITS ORIGINAL BYTES with a larger cap (the host form does). */
typedef struct fmd_ectab fmd_ectab_t;
#define FMD_ECFIX_TRACE_FULL ((int32_t)0x80000000)
int fmd_ectab_build_dev(int device, void *stream, int w, int suf_len, uint64_t n, const uint32_t *d_bucket, const uint32_t *d_key,
                        const uint8_t *d_val, fmd_ectab_t **out);
int fmd_ectab_build(int device, int w, int suf_len, uint64_t n, const uint32_t *bucket, const uint32_t *key, const uint8_t *val, fmd_ectab_t **out);
void fmd_ectab_free(fmd_ectab_t *t);
size_t fmd_ecfix_work_bytes(const fmd_ectab_t *t, size_t n, uint32_t trace_cap);
int fmd_ecfix_dev(fmd_ectab_t *t, void *stream, size_t n, uint8_t *d_seqs, uint8_t *d_quals, const uint64_t *d_off, int step, uint32_t trace_cap,
                  int32_t *d_info, void *d_work, size_t work_bytes);
int fmd_ecfix_batch(fmd_ectab_t *t, size_t n, uint8_t *seqs, uint8_t *quals, const uint64_t *off, int step, int32_t *info);
/* what the kernels launched on the table requested since the last reset: {table slots probed (8 B each), queue entries moved (16 B), trace entries
 * moved (8 B)} -- counted by the instrumented build only (*counting = 1; the shipped library answers zeros and *counting = 0), like fmd_dev_line_count */
int fmd_ectab_line_count(fmd_ectab_t *t, uint64_t counts[3], int reset, int *counting);

/* ---- fm6_retrieve (exact.c:100-127) in bulk: rank, `$read$` bi-interval and containment of each
 * sequence id (rec.rank, rec.k[], rec.status = -3 when contained, rec.len); no length threshold,
 * no overlap search.  This is what fm6_seqsort (seqsort.c:12-35) consumes. */
int fmd_seqinfo_dev(fmd_dev_t *h, void *stream, size_t n, const uint64_t *d_ids, uint32_t max_len, fmd_ovlp_rec_t *d_rec,
                    uint8_t *d_seq, uint32_t seq_stride, void *d_work, size_t work_bytes); /* work: fmd_ovlp_work_bytes(n, max_len, max_len-1) */
int fmd_seqinfo_batch(fmd_dev_t *h, size_t n, const uint64_t *ids, uint32_t max_len, fmd_ovlp_rec_t *rec);

/* ---- index construction: the BWT `fermi build` computes (cmd.c:378-484, build.c:11-50) ------
 * reads: nt6 bases of all reads back to back, NO sentinels; read i = reads[off[i], off[i+1]).
 * The text indexed is  read $ revcomp(read) $  per read in input order, sentinels ordered by
 * sequence id (ksa.c:54).  Palindrome trimming (cmd.c:457-463) is the caller's job
 * (fermi_amd/host).  bwt (host) must hold 2*(off[n]+n) bytes.  The _dev form returns a device
 * buffer the caller releases with fmd_dev_free(); uniform_len != 0 asserts all reads have
 * max_len bases. */
int fmd_build_bwt(int device, size_t n_reads, const uint8_t *reads, const uint64_t *off, uint8_t *bwt, uint64_t *n_sym);
int fmd_build_bwt_dev(int device, void *stream, size_t n_reads, const uint8_t *d_reads, const uint64_t *d_off,
                      uint64_t total_bases, uint32_t max_len, int uniform_len, uint8_t **d_bwt, uint64_t *n_sym);
/* The BWT of a chosen set of strands: what `fermi ropebwt [-F] [-R]` inserts per read (insert1, ropebwt.c:22-45) -- the forward
 * strand, then the reverse complement, each a sequence of its own closed by its '$'; `strands` takes ropebwt.c's flag values.
 *   FMD_STRAND_BOTH   read $ revcomp $   n_sym = 2 * (total_bases + n_reads)   (= fmd_build_bwt, byte for byte)
 *   FMD_STRAND_FWD    read $             n_sym = total_bases + n_reads
 *   FMD_STRAND_REV    revcomp $          n_sym = total_bases + n_reads
 * Any other value is FMD_E_ARG.  Sentinels are ordered by insertion order, symbol 5 (N) is its own complement.  Unlike
 * fmd_build_bwt, a read of no bases is legal: a sequence of its '$' alone (bpr_insert_string with l = 0, bprope6.c:218-224).
 * bwt (host) must hold n_sym bytes.  Reads and arguments otherwise as above. */
#define FMD_STRAND_FWD  1u
#define FMD_STRAND_REV  2u
#define FMD_STRAND_BOTH 3u
int fmd_build_bwt_strands(int device, size_t n_reads, const uint8_t *reads, const uint64_t *off, unsigned strands, uint8_t *bwt, uint64_t *n_sym);
int fmd_build_bwt_strands_dev(int device, void *stream, size_t n_reads, const uint8_t *d_reads, const uint64_t *d_off,
                              uint64_t total_bases, uint32_t max_len, int uniform_len, unsigned strands, uint8_t **d_bwt, uint64_t *n_sym);
void fmd_dev_free(void *d_ptr);
/* The same index without the byte BWT, for read sets whose text + BWT do not fit next to the index (7*10^8 x 100 bp:
 * 1.4*10^11 symbols): reads of ONE length appended in any number of calls (n x read_len nt6 bytes on the device, no
 * sentinels; they need not stay resident), text kept 4 bits per symbol, BWT slices written straight into the device
 * layout.  fmd_builder_finish releases the builder and returns the index fmd_dev_open_bwt_dev(fmd_build_bwt_dev(..))
 * would return. */
typedef struct fmd_builder fmd_builder_t;
int fmd_builder_new(int device, uint64_t n_reads, uint32_t read_len, fmd_builder_t **out);
int fmd_builder_add_dev(fmd_builder_t *b, void *stream, uint64_t n, const uint8_t *d_reads);
int fmd_builder_finish(fmd_builder_t *b, fmd_dev_t **out);
void fmd_builder_free(fmd_builder_t *b);
/* ---- merging two indexes: fm_merge (merge.c:100-134), fm_compute_gap_bits (merge.c:33-96) ------------------------------
 * The merged index holds the sequences of h0 followed by those of h1 (what `fermi merge h0 h1`, `fermi build -i h0` and
 * `fermi build` of the concatenated reads write).  Both handles on one device (FMD_E_ARG otherwise); neither is changed.
 * n_tot = n0 + n1 symbols.  The smaller index (h1 on a tie) is the WALKED one: every sequence of it is LF-walked beside
 * its insertion row in the other, and the rows it lands on are set in d_bits.
 * walk: d_bits = (n_tot + 63) / 64 words, zeroed by the caller; bit p set = merged row p comes from the walked index
 *       (*walked = 0: h0, 1: h1; may be NULL).  It also leaves the prefix counts of d_bits in d_work (work_bytes >=
 *       fmd_merge_work_bytes(n_tot)), which the interleave reads.
 * interleave: merged BWT[first, first + n) as nt6 bytes into d_out, from d_bits / d_work of a walk of the same two handles.
 * Both enqueue on `stream` and return; they allocate nothing.  fmd_dev_merge: the whole merge into a new resident index
 * (FMD_E_NOMEM when the inputs, the merged index and the bit array do not fit together); fmd_dev_merge_ex with
 * FMD_OPEN_NO_TABLES: the same without the prefix and tail tables (a result that is only merged again or decoded). */
size_t fmd_merge_work_bytes(uint64_t n_tot);
int fmd_merge_walk_dev(fmd_dev_t *h0, fmd_dev_t *h1, void *stream, uint64_t *d_bits, void *d_work, size_t work_bytes, int *walked);
int fmd_merge_interleave_dev(fmd_dev_t *h0, fmd_dev_t *h1, void *stream, const uint64_t *d_bits, const void *d_work,
                             uint64_t first, uint64_t n, uint8_t *d_out);
int fmd_dev_merge(fmd_dev_t *h0, fmd_dev_t *h1, fmd_dev_t **out);
int fmd_dev_merge_ex(fmd_dev_t *h0, fmd_dev_t *h1, unsigned flags, fmd_dev_t **out);

/* ---- contrast assembly: fm6_contrast (cmp.c:94-126: contrast_core cmp.c:45-76, descend cmp.c:10-20, collect_tips cmp.c:22-43) --------
 * The reads of each index that carry a string of up to k bases which the other index lacks, as one bit per sequence IN SORTED ORDER:
 * bit i = the sequence whose '$' is the i-th of the BWT (the rows ok[0].x[0] .. of a backward extension, cmp.c:32-39) -- the array before
 * fm6_sub_conv (cmp.c:128-144), which the caller applies with the .rank file (`seqsort`): bit i -> bit rank[i] >> 2, the sequence's number.  A string counts as present in an index
 * only while it or the other side has >= min_occ occurrences on the way down (cmp.c:68).  Both handles on one device; the same
 * handle twice is legal (all-zero arrays).  k <= 4 (cmp.c:101), min_occ < 1 and a null handle are FMD_E_ARG.
 * fmd_contrast_dev: enqueues on `stream` and returns; allocates nothing.  d_sub0 / d_sub1: (n_seq + 63) / 64 words each, zeroed by
 *   the caller, OR-ed into.  The trie is walked level by level through lists of `cap` entries each (>= 1024) in d_work
 *   (work_bytes >= fmd_contrast_work_bytes(cap)); seed_mask (bit c-1 = base c, 0xf = all) restricts the walk to the strings that END
 *   in one of those bases: the parts are disjoint and the union of their bits is the whole result.  d_status (device, 4 x u64):
 *   [0] pair nodes expanded, [1] overflow flag -- a list was full: every bit set is right but some are missing, call again with a
 *   larger cap or part by part into the same arrays --, [2] / [3] tip nodes expanded in h0 / h1.
 * fmd_contrast: the host form; runs again with larger lists, or in four parts, until nothing overflows.  *sub0 / *sub1 are
 *   malloc'ed (fmd_host_free). */
size_t fmd_contrast_work_bytes(uint64_t cap);
int fmd_contrast_dev(fmd_dev_t *h0, fmd_dev_t *h1, void *stream, int k, int min_occ, int seed_mask, uint64_t *d_sub0, uint64_t *d_sub1,
                     void *d_work, size_t work_bytes, uint64_t cap, uint64_t *d_status);
int fmd_contrast(fmd_dev_t *h0, fmd_dev_t *h1, int k, int min_occ, uint64_t **sub0, uint64_t **sub1);
/* ---- the sub-index of selected sequences: fm_sub (sub.c:71-97: set_bits sub.c:14-28, gen_idx sub.c:30-55) -------------------------
 * d_sub: one bit per sequence of h by its NUMBER, which is its sentinel's row ((n_seq + 63) / 64 words: what `fermi contrast` /
 * `bitand` write behind their 8-byte length, i.e. after fm6_sub_conv).  Both strands of a read must be selected together for the result to be an FMD index (the reference does not check).
 * mark: every selected sequence is LF-walked and the rows it visits are set in d_bits ((n_sym + 63) / 64 words, zeroed by the
 *       caller); it leaves the prefix counts of d_bits in d_work (work_bytes >= fmd_sub_work_bytes(n_sym)) and the number of set
 *       bits in *d_n_kept (device; may be NULL) -- the symbols of the sub-index; of its complement: n_sym minus that.
 * select: rows [first, first + n) of the sub-index (is_comp: of the index of the sequences NOT selected, `fermi sub -c`) as nt6 bytes
 *       into d_out, from d_bits / d_work of a mark of the same handle.
 * Both enqueue on `stream` and return; they allocate nothing.  fmd_dev_sub: the whole of it, from a host bit array into a new
 * resident index (flags as fmd_dev_merge_ex; FMD_E_ARG when no sequence is kept). */
size_t fmd_sub_work_bytes(uint64_t n_sym);
int fmd_sub_mark_dev(fmd_dev_t *h, void *stream, const uint64_t *d_sub, uint64_t *d_bits, void *d_work, size_t work_bytes, uint64_t *d_n_kept);
int fmd_sub_select_dev(fmd_dev_t *h, void *stream, const uint64_t *d_bits, const void *d_work, int is_comp, uint64_t first, uint64_t n, uint8_t *d_out);
int fmd_dev_sub(fmd_dev_t *h, const uint64_t *sub, int is_comp, unsigned flags, fmd_dev_t **out);

/* ---- `fermi fltuniq`: the k-mer table and the verdict per read (main_fltuniq, seq.c:122-210) ---------------------------------------
 * Reads as fmd_ecfix_* takes them: read i = bytes [off[i], off[i+1]) of seqs, nt6 codes (1..4 = A C G T; every other byte is a non-base:
 * the reference indexes seq_nt6_table with bytes >= 128 out of range, seq.c:168 -- undefined there).  Forward strand only.
 * The table is the reference's flags[] (seq.c:161, :172) word for word: 2 bits per k-mer, k-mer z (first base most significant) at bits
 * [(z & 31) << 1, +2) of 64-bit word z >> 5; 0 = absent, 1 = seen once, 3 = seen more than once.  fmd_fltuniq_table_bytes(k) = 4^k / 4
 * bytes (16 GiB at k = 18), 0 for a k outside 3..20 (below 3 the reference's table has no word).
 * count (seq.c:164-175): every window of k bases of every read raises its state; any number of calls on one table zeroed by the caller
 *   (fmd_memset_dev) -- a state depends only on how often its k-mer occurs in all of them, not on the order or on where the batches were
 *   cut (DESIGN.md "fltuniq").
 * test (seq.c:192-199): d_pass[i] = 1 when read i holds no non-base and every window of k bases has state 3 (reads shorter than k: when
 *   they hold no non-base), else 0.  The table is only read.
 * Both enqueue on `stream` and return; they allocate nothing.  A k outside the range and null pointers are FMD_E_ARG.
 * fmd_fltuniq / fmd_fltuniq_table: the host forms -- both passes over reads in host memory (pass[n_reads]), or pass 1 and the table
 *   copied out (table_bytes(k) / 8 words); FMD_E_NOMEM when the table does not fit the device.
 * fmd_fltuniq_t: a streamed run for input larger than memory (what `fermi-amd fltuniq` uses).  open allocates and zeroes the table and
 *   two staging slots of max_bytes bases and max_reads reads in pinned host memory; slot hands out the next one (off[0] must be 0;
 *   waits until its previous work is done); count / test upload the slot last handed out and enqueue its kernel -- the caller fills the
 *   next slot meanwhile; the first test waits for every count.  pass[] of a test is filled when its slot comes round again or at
 *   sync; sync also reports the milliseconds the count and the test kernels took so far.  export copies table words out.
 * fmd_fltuniq_batch_limits: the most bases and reads the host forms and the command put into one batch (64 MiB, 2^20).  A test aid that
 *   changes no result: with FMD_FLTUNIQ_TEST_HOOKS=1 in the environment, FMD_FLTUNIQ_TEST_BATCH_BYTES / FMD_FLTUNIQ_TEST_BATCH_READS
 *   (each >= 1) replace them, so that a small input runs in many batches; without the gate both are ignored.  Read on every call. */
typedef struct fmd_fltuniq_run fmd_fltuniq_t;
size_t fmd_fltuniq_table_bytes(int k);
int fmd_fltuniq_count_dev(int device, void *stream, int k, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t n_reads, uint64_t *d_table);
int fmd_fltuniq_test_dev(int device, void *stream, int k, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t n_reads, const uint64_t *d_table,
                         uint8_t *d_pass);
int fmd_fltuniq(int device, int k, const uint8_t *seqs, const uint64_t *off, uint64_t n_reads, uint8_t *pass);
int fmd_fltuniq_table(int device, int k, const uint8_t *seqs, const uint64_t *off, uint64_t n_reads, uint64_t *table);
int fmd_fltuniq_open(int device, int k, uint64_t max_bytes, uint64_t max_reads, fmd_fltuniq_t **out);
int fmd_fltuniq_slot(fmd_fltuniq_t *f, uint8_t **seqs, uint64_t **off);
int fmd_fltuniq_count(fmd_fltuniq_t *f, uint64_t n_reads);
int fmd_fltuniq_test(fmd_fltuniq_t *f, uint64_t n_reads, uint8_t *pass);
int fmd_fltuniq_sync(fmd_fltuniq_t *f, double kernel_ms[2]);
int fmd_fltuniq_export(fmd_fltuniq_t *f, uint64_t first_word, uint64_t n_words, uint64_t *table);
void fmd_fltuniq_close(fmd_fltuniq_t *f);
void fmd_fltuniq_batch_limits(uint64_t *max_bytes, uint64_t *max_reads);

/* ---- `fermi scaf`: the link stage, collect_nei (scaf.c:189-254) -- from the unpaired-read lists of a remapped MAG to links between unitig ends ----
 * Entry i of the UR lists of all unitigs: x[i] = read id << 1 | strand, span[i] = b << 32 | e (already shifted and clipped to the trimmed
 * unitig, scaf.c:107), utig[i] = its unitig (< n_utig < 2^31); per unitig len[] and excluded[] (A < a_thres, scaf.c:649-650).
 * The end of an entry is idd = utig << 1 | ((x & 1) ^ 1), its distance to that end dist = (x & 1) ? e : len - b, its value idd << 32 | dist.
 * The dictionary (the reference's hash `h`, scaf.c:195-211): read id -> value over the entries of unitigs that are not excluded with
 * dist <= max_dist, for the ids that occur ONCE among them and whose value is not 0 (0 is the reference's "deleted" mark, scaf.c:207).
 *   self[i], mate[i]   dictionary[x >> 1] and dictionary[(x >> 1) ^ 1], FMD_SCAF_NONE where absent -- for every entry, dropped ones included:
 *                      the reference looks a read up by id alone (scaf.c:223, :356-360, :390-394), and so do add_seq and compute_t on these words.
 *   gkey / gval        the links grouped (the table `t`, scaf.c:221-234): entry i contributes when self and mate are there and the mate's unitig is
 *                      not utig[i]; key = (utig[i] << 1 | end bit of self) << 32 | the mate's idd, value = count << 40 | sum of both distances.
 *                      *n_groups of them (<= n), ascending by key.
 *   n_nei[2 n_utig]    per end, the number of its groups: what the reference's table held when it picked the best two (its bucket count carries
 *                      over from end to end while it stays below 32, scaf.c:217-220, and decides the order of equal values).
 * The _dev form enqueues on `stream` and returns; it allocates nothing (work_bytes >= fmd_scaf_links_work_bytes(n): six arrays of n words
 * and rocPRIM's temporary storage).  The host form copies in, runs, copies out. */
#define FMD_SCAF_NONE (~0ull)
size_t fmd_scaf_links_work_bytes(uint64_t n);
int fmd_scaf_links_dev(int device, void *stream, uint64_t n, const uint64_t *d_x, const uint64_t *d_span, const uint32_t *d_utig, uint64_t n_utig,
                       const int32_t *d_len, const uint8_t *d_excluded, int max_dist, uint64_t *d_self, uint64_t *d_mate, uint64_t *d_gkey,
                       uint64_t *d_gval, uint32_t *d_n_nei, uint64_t *d_n_groups, void *d_work, size_t work_bytes);
int fmd_scaf_links(int device, uint64_t n, const uint64_t *x, const uint64_t *span, const uint32_t *utig, uint64_t n_utig, const int32_t *len,
                   const uint8_t *excluded, int max_dist, uint64_t *self, uint64_t *mate, uint64_t *gkey, uint64_t *gval, uint32_t *n_nei,
                   uint64_t *n_groups);

/* device memory for C hosts (the reference has no device; these are what a cgo/C caller uses to
 * stage batches): plain hipMalloc / hipMemcpyAsync behind the ABI. */
int fmd_dev_malloc(int device, size_t bytes, void **d_ptr);
int fmd_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream);
int fmd_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream);
int fmd_memset_dev(void *d_dst, int value, size_t bytes, void *stream);   /* hipMemsetAsync: enqueued, not synchronised (the zeroed bit array of fmd_merge_walk_dev) */
/* device BWT -> host RLE\6 byte stream (`len<<3|sym`, ropebwt.c:132-136); *h_rle6 is malloc'ed,
 * release with fmd_host_free().  Prefix it with "RLE\6" and it is a .fmd the reference loads. */
int fmd_bwt_to_rle6(int device, const uint8_t *d_bwt, uint64_t n, uint8_t **h_rle6, uint64_t *n_bytes);
void fmd_host_free(void *p);

/* ---- diagnostics: random-gather ceiling of this GPU (DESIGN.md "practical roofline") -----
 * Reads n_access random aligned lines of `line_bytes` (64/128/256) from a working set of
 * ws_bytes with the same LDS-DMA gather the rank kernels use; returns milliseconds. */
int fmd_probe_gather(int device, uint64_t ws_bytes, uint32_t line_bytes, uint64_t n_access, int iters, float *ms);

#ifdef __cplusplus
}
#endif
#endif
