/* scaf.h -- what scaf_cmd.c (the command: GPU calls and their order) and scaf_core.c (everything that needs no device: reading the
 * remapped MAG, the statistics per unitig, the choice of links, the verdict on an assembled gap, the joiner) share.  mag_scaf_core and
 * what it calls (scaf.c) restated; every output byte is the reference's. */
#ifndef FMDH_SCAF_H
#define FMDH_SCAF_H
#include <stdint.h>
#include <stdio.h>
#include "mag.h"

/* The local alignment WITH coordinates, as ksw_align returns it under KSW_XSTART to scaf.c:504 (scaf_stat.c): match +1, mismatch -3, a gap of
 * k bases 5 + 2k, codes 0..4.  score, the last aligned position of the target (te) and of the query (qe), and -- when the pass over the
 * reversed prefixes reaches the same score -- the first ones (tb, qb; -1 otherwise).  Equal cells are resolved as the reference's striped
 * 16-bit kernel resolves them.  -1: out of memory. */
typedef struct { int score, te, qe, tb, qb; } fmdh_swaln_t;
int fmdh_sw_align(int ql, const uint8_t *q, int tl, const uint8_t *t, fmdh_swaln_t *r);
/* the statistics of `scaf` (scaf.c:290-335, :371-378, :400-405), in double and in the reference's order of operations */
double fmdh_kf_lgamma(double z);
double fmdh_kf_betai(double a, double b, double x);
double fmdh_scaf_correct_mean(double l, double mu, double sigma);
double fmdh_scaf_pvalue(int n, int64_t sum, int64_t sum2, double mu);

typedef struct { int l, patched; double t; char *s; } fmdh_scaf_ext_t;      /* a link's gap: l > 0 bases to insert (s), l < 0 bases of overlap */
typedef struct {
    uint64_t k[2];                        /* the ids of its two ends */
    fmdh_scaf_ext_t ext[2];
    double A;
    int len, nsr, maxo;
    uint8_t deleted, excluded;
    uint8_t *seq;                         /* nt6 codes, trimmed */
    uint64_t first, n_reads;              /* its UR entries: [first, first + n_reads) of the flat arrays */
    uint64_t dist[2], dist2[2];           /* best and second-best neighbour of each end: count << 40 | distance */
    int64_t nei[2], nei2[2];              /* their ends, -1 = none */
} fmdh_scaf_utig_t;

typedef struct fmdh_scaf {
    size_t n, m;
    fmdh_scaf_utig_t *u;
    /* the UR entries of all unitigs, in file order (the input of fmd_scaf_links) */
    uint64_t n_ent, m_ent;
    uint64_t *x, *span;
    uint32_t *utig;
    /* per entry, from the link stage */
    uint64_t *self, *mate;
    double rdist;
    int err;                              /* 1: the input names a read the index does not hold, or a link has fewer than two pairs behind it */
} fmdh_scaf_t;

typedef struct { int min_supp, pr_links, n_threads; double a_thres, p_thres, avg, std; } fmdh_scafopt_t;

fmdh_scaf_t *fmdh_scaf_read(const char *fn);                                  /* read_utig, scaf.c:47-115; NULL: cannot open */
void fmdh_scaf_free(fmdh_scaf_t *s);
/* for bindings: the number of unitigs; one unitig's ids, {len, nsr, maxo}, A and number of UR entries; the flat entry arrays (and who is excluded);
 * the link stage's per-entry words copied in */
size_t fmdh_scaf_count(const fmdh_scaf_t *s);
void fmdh_scaf_unitig_info(const fmdh_scaf_t *s, size_t i, uint64_t k[2], int32_t len_nsr_maxo[3], double *A, uint64_t *n_reads);
uint64_t fmdh_scaf_entries(const fmdh_scaf_t *s, const uint64_t **x, const uint64_t **span, const uint32_t **utig, uint8_t *excluded);
int fmdh_scaf_set_links(fmdh_scaf_t *s, const uint64_t *self, const uint64_t *mate);
double fmdh_scaf_cal_rdist(fmdh_scaf_t *s);                                   /* cal_rdist, scaf.c:152-187: rdist, and A of every unitig */
void fmdh_scaf_exclude(fmdh_scaf_t *s, double a_thres);
/* the second half of collect_nei (scaf.c:213-252) from the link stage's output: best and second-best neighbour of every end */
int fmdh_scaf_choose(fmdh_scaf_t *s, uint64_t n_groups, const uint64_t *gkey, const uint64_t *gval, const uint32_t *n_nei);
void fmdh_scaf_resolve_contained(fmdh_scaf_t *s, uint32_t id, double avg, double std, int pr_link, FILE *err);   /* scaf.c:256-284 */
/* is the link at end iddp one to patch (scaf.c:468-478)?  *iddq = the other end */
int fmdh_scaf_candidate(const fmdh_scaf_t *s, uint32_t iddp, int min_supp, uint32_t *iddq);
/* the rows whose mates add_seq fetches at end idd (scaf.c:352-369): entries whose own value names idd and -- idd_mate >= 0 -- whose mate's names idd_mate */
int fmdh_scaf_keeps(const fmdh_scaf_t *s, uint64_t entry, uint32_t idd, int64_t idd_mate);
void fmdh_scaf_end_seq(const fmdh_scaf_utig_t *p, int is3, int is_2nd, int max_dist, uint8_t *dst, int *l);   /* end_seq, scaf.c:341-350; dst: max_dist + 1 bytes */
/* what assemble does with the graph of the local assembly (scaf.c:419-451); g may be NULL (no unitig at all) */
fmdh_scaf_ext_t fmdh_scaf_gap_from_graph(fmdh_mag_t *g, int max_len, const char *t0, const char *t1);
int fmdh_scaf_compute_t(fmdh_scaf_t *s, uint32_t idd, int l, double mu, double sigma, int max_len, double *t);   /* compute_t, scaf.c:380-406; -1: fewer than two pairs */
/* the two rounds' verdict and the fallback (scaf.c:489-520): call with each round's gap in turn (returns 1 when the second round is not needed),
 * then fmdh_scaf_fallback with the last round's gap */
int fmdh_scaf_accept(fmdh_scaf_t *s, uint32_t iddp, uint32_t iddq, int round, fmdh_scaf_ext_t *ext, double avg, double std, int max_len);
void fmdh_scaf_fallback(fmdh_scaf_t *s, uint32_t iddp, uint32_t iddq, const fmdh_scaf_ext_t *last, const char *t0, int pl, const char *t1, int ql, double avg,
                        double std, int max_len, FILE *err);
void fmdh_scaf_print_links(const fmdh_scaf_t *s, FILE *err);                  /* debug_utig over every end, scaf.c:129-146 */
void fmdh_scaf_join(fmdh_scaf_t *s, double a_thres, double p_thres, FILE *out);   /* make_scaftigs, scaf.c:528-603 */
#endif
