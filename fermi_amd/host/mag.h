/* mag.h -- fermi's unitig graph (MAG) on the host: reading, printing and cleaning (mag.c, mag_bubble.c, swscore.c).
 * Plain C, no GPU and nothing of libfmdhip: `clean` is one thread chasing pointers over a graph 10^3 - 10^5 times smaller than
 * the reads it came from.  The output of every operation is, byte for byte, what the reference's operation of the same name
 * leaves behind (mag.c, bubble.c); each entry names the function it stands for.  The layout is this module's own.  Where the reference asserts on an
 * inconsistent graph, the operation sets g->err and returns; nothing here aborts. */
#ifndef FMDH_MAG_H
#define FMDH_MAG_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#ifdef __cplusplus
extern "C" {
#endif

/* mag.h:8-14 */
#define FMDH_MAG_F_READ_ORI   0x1    /* -O: take the file as it is (no filtering of arcs, no tip cut at read time) */
#define FMDH_MAG_F_READ_MERGE 0x4    /* merge(1) after reading; set by init_opt and never cleared by `clean` */
#define FMDH_MAG_F_CLEAN      0x10   /* -C */
#define FMDH_MAG_F_AGGRESSIVE 0x20   /* -A */
#define FMDH_MAG_F_NO_AMEND   0x40   /* -F */
#define FMDH_MAG_F_NO_SIMPL   0x80   /* -S */

typedef struct {                     /* = magopt_t; the four ratios are float there and so here: they enter float arithmetic */
    int flag, max_arc, n_iter, min_ovlp, min_elen, min_ensr, min_insr, max_bdist, max_bvtx;
    float min_dratio0, min_dratio1, max_bcov, max_bfrac;
} fmdh_magopt_t;

/* An end's arcs.  a[0 .. n) are the LIVE arcs in the order they arrived; an arc that is deleted leaves the array at once and is counted
 * in n_gone until the list is compacted or sorted: the reference keeps a deleted arc in its slot until then, and several of its tests
 * count slots, so `slots` below is what those tests see while nothing else has to step over dead entries. */
typedef struct { uint64_t to; int64_t ovlp; } fmdh_arc_t;                /* to: the id of the neighbour's end */
typedef struct { fmdh_arc_t *a; uint32_t n, room, n_gone; } fmdh_arcs_t;
typedef struct { uint64_t id; fmdh_arcs_t arcs; } fmdh_magend_t;
typedef struct {
    int len, nsr;                    /* bases (-1: the slot is empty), reads */
    uint32_t cap;                    /* bytes behind seq and cov, > len: both end in a NUL */
    int32_t aux;                     /* the bubble walk's record of this vertex + 1, 0 outside of it */
    fmdh_magend_t end[2];            /* left, right */
    char *seq, *cov;                 /* nt6 codes; coverage + 33 */
} fmdh_magv_t;
typedef struct fmdh_mag {
    size_t n, m;
    fmdh_magv_t *v;
    float rdist;
    int min_ovlp;
    int err;                         /* set once an operation met an inconsistent graph or ran out of memory; every operation returns at once then */
    struct fmdh_magdict *h;          /* end id -> vertex << 1 | side */
} fmdh_mag_t;
static inline uint32_t fmdh_arcs_slots(const fmdh_arcs_t *r) { return r->n + r->n_gone; }

void fmdh_mag_init_opt(fmdh_magopt_t *o);                                   /* mag_init_opt, mag.c:592-613 */
/* mag_g_read, mag.c:190-285 ("-" = stdin; plain or gzip).  NULL: the file cannot be opened or a record cannot be parsed (a message on stderr) */
fmdh_mag_t *fmdh_mag_read(const char *fn, const fmdh_magopt_t *opt);
/* the same over records held in memory.  flag = READ_ORI | NO_AMEND without READ_MERGE gives the graph as fm6_api_unitig returns it
 * (unitig.c:413-434): the dictionary built, nothing filtered, amended or merged */
fmdh_mag_t *fmdh_mag_read_mem(const void *p, size_t n, const fmdh_magopt_t *opt);
void fmdh_mag_destroy(fmdh_mag_t *g);                                        /* mag_g_destroy */
void fmdh_mag_print(const fmdh_mag_t *g, FILE *out);                         /* mag_g_print + mag_v_write, mag.c:149-188 */
int fmdh_mag_build_hash(fmdh_mag_t *g);                                      /* mag_g_build_hash, mag.c:87-105 */
void fmdh_mag_amend(fmdh_mag_t *g);                                          /* mag_amend, mag.c:119-143 */
double fmdh_mag_cal_rdist(const fmdh_mag_t *g);                              /* mag_cal_rdist, mag.c:544-586 */
void fmdh_mag_merge(fmdh_mag_t *g, int rmdup);                               /* mag_g_merge, mag.c:461-480 */
void fmdh_mag_rm_vext(fmdh_mag_t *g, int min_len, int min_nsr);              /* mag_g_rm_vext, mag.c:486-494 */
void fmdh_mag_rm_vint(fmdh_mag_t *g, int min_len, int min_nsr, int min_ovlp);/* mag_g_rm_vint, mag.c:496-504 */
void fmdh_mag_rm_edge(fmdh_mag_t *g, int min_ovlp, double min_ratio, int min_len, int min_nsr);   /* mag_g_rm_edge, mag.c:506-535 */
void fmdh_mag_simplify_bubble(fmdh_mag_t *g, int max_vtx, int max_dist);     /* mag_g_simplify_bubble, bubble.c:165-176 */
void fmdh_mag_pop_simple(fmdh_mag_t *g, float max_cov, float max_frac, int aggressive);   /* mag_g_pop_simple, bubble.c:250-258 */
void fmdh_mag_pop_open(fmdh_mag_t *g, int min_elen);                         /* mag_g_pop_open, bubble.c:344-350 */
void fmdh_mag_clean(fmdh_mag_t *g, const fmdh_magopt_t *opt);                /* mag_g_clean, mag.c:615-673 */

/* what mag.c and mag_bubble.c share */
int fmdh_mag_end(fmdh_mag_t *g, uint64_t end_id, uint64_t *where);          /* vertex << 1 | side of an end: 0, or -1 with g->err set (the reference asserts) */
void fmdh_mag_arcs_compact(fmdh_arcs_t *r);                                  /* mag_v128_clean: the deleted arcs stop counting */
void fmdh_mag_arc_drop(fmdh_arcs_t *r, uint32_t at);                         /* arc `at` is deleted */
uint32_t fmdh_mag_arcs_unlink(fmdh_mag_t *g, uint64_t end_id, uint64_t to);  /* every arc of end `end_id` that leads to `to` is deleted; how many */
void fmdh_mag_v_del(fmdh_mag_t *g, fmdh_magv_t *p);                          /* mag_v_del, mag.c:346-362 */

/* The score of the local alignment ksw_align returns to bubble.c:233 and :319 (xtra = 0: the 16-bit kernel, no coordinates, no second
 * best): match +5, mismatch -4, a gap of k bases 5 + 2k, never above 32767 where the 16-bit additions saturate.  Bases are codes 0..3;
 * any other code matches nothing.  -1: out of memory (rows longer than 512 cells are allocated). */
int fmdh_sw_score(int la, const uint8_t *a, int lb, const uint8_t *b);

/* `fermi clean` (cmd.c:508-558); argv[0] = the command's name */
int fmdh_main_clean(int argc, char *argv[]);

#ifdef __cplusplus
}
#endif
#endif
