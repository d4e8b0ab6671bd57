/* mag.c -- the unitig graph of fermi (MAG) on the host: the reader, the printer, the dictionary of end ids and the plain graph
 * operations of `fermi clean` (mag.c of the reference); the bubble operations are in mag_bubble.c.
 *
 * A vertex is a unitig with two ends; an end has an id and a list of arcs (id of the neighbour's end, overlap length).  The
 * dictionary maps an end id to vertex << 1 | side.  What the output depends on, and what therefore is kept exactly:
 *   - vertices keep their slot: a merged vertex stays in the slot of its left partner, printing goes over the slots in order;
 *   - a new arc goes to the END of a list; rmdup sorts a list by (id ascending, overlap descending) and keeps the first arc of
 *     every id, compaction keeps the order -- two arcs equal in both keys cannot be told apart, so any sort will do;
 *   - a deleted arc still COUNTS in its list until the list is compacted or sorted (the reference leaves it in its slot and tests
 *     the number of slots): a list here holds the live arcs only, and a count of the ones that went (mag.h);
 *   - the integer and float conversions of the thresholds (see fmdh_mag_clean and read_arcs).
 * Where the reference asserts, g->err is set and the operation returns. */
#include <ctype.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "fmd_host.h"
#include "mag.h"

/* ---- the dictionary: open addressing, linear probing, tombstones ---- */
typedef struct fmdh_magdict {
    uint64_t mask;
    uint64_t *key, *val;
    uint8_t *st;             /* 0 empty, 1 full, 2 tombstone */
} dict_t;

static inline uint64_t dict_mix(uint64_t k) { k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33; return k; }

static dict_t *dict_new(uint64_t n_keys)
{
    dict_t *d = (dict_t *)calloc(1, sizeof(*d));
    uint64_t cap = 16;
    if (!d) return 0;
    while (cap < n_keys * 2 + 2) cap <<= 1;
    d->mask = cap - 1;
    d->key = (uint64_t *)malloc(cap * 8); d->val = (uint64_t *)malloc(cap * 8); d->st = (uint8_t *)calloc(cap, 1);
    if (!d->key || !d->val || !d->st) { free(d->key); free(d->val); free(d->st); free(d); return 0; }
    return d;
}
static void dict_free(dict_t *d) { if (d) { free(d->key); free(d->val); free(d->st); free(d); } }
static inline int64_t dict_find(const dict_t *d, uint64_t key)
{
    uint64_t i = dict_mix(key) & d->mask;
    for (; d->st[i]; i = (i + 1) & d->mask)
        if (d->st[i] == 1 && d->key[i] == key) return (int64_t)i;
    return -1;
}
/* 1: inserted, 0: the key was there (*slot says where).  The table never grows: the graph only loses ends after it was built. */
static int dict_put(dict_t *d, uint64_t key, uint64_t val, int64_t *slot)
{
    uint64_t i = dict_mix(key) & d->mask;
    int64_t tomb = -1;
    for (; d->st[i]; i = (i + 1) & d->mask) {
        if (d->st[i] == 1 && d->key[i] == key) { *slot = (int64_t)i; return 0; }
        if (d->st[i] == 2 && tomb < 0) tomb = (int64_t)i;
    }
    if (tomb >= 0) i = (uint64_t)tomb;
    d->st[i] = 1; d->key[i] = key; d->val[i] = val; *slot = (int64_t)i;
    return 1;
}
static inline void dict_del(dict_t *d, uint64_t key) { const int64_t i = dict_find(d, key); if (i >= 0) d->st[i] = 2; }

int fmdh_mag_end(fmdh_mag_t *g, uint64_t end_id, uint64_t *where)
{
    const int64_t i = g->h ? dict_find(g->h, end_id) : -1;
    if (i < 0 || (g->h->val[i] >> 1) >= g->n) { g->err = 1; return -1; }   /* (an end id that two vertices claim maps to -1: mag.c:100) */
    *where = g->h->val[i];
    return 0;
}
static inline fmdh_arcs_t *arcs_at(fmdh_mag_t *g, uint64_t where) { return &g->v[where >> 1].end[where & 1].arcs; }

int fmdh_mag_build_hash(fmdh_mag_t *g)
{
    size_t i;
    int j;
    dict_free(g->h);
    g->h = dict_new(2 * (uint64_t)g->n);
    if (!g->h) { g->err = 1; return -1; }
    for (i = 0; i < g->n; ++i)
        for (j = 0; j < 2; ++j) {
            int64_t s;
            if (!dict_put(g->h, g->v[i].end[j].id, (uint64_t)i << 1 | (uint64_t)j, &s)) g->h->val[s] = (uint64_t)-1;   /* a duplicated terminal */
        }
    return 0;
}

/* ---- arc lists: the live arcs in order, and how many went since the list was last compacted (mag.h) ---- */
void fmdh_mag_arcs_compact(fmdh_arcs_t *r) { r->n_gone = 0; }

void fmdh_mag_arc_drop(fmdh_arcs_t *r, uint32_t at)
{
    memmove(r->a + at, r->a + at + 1, (size_t)(r->n - at - 1) * sizeof(fmdh_arc_t));
    --r->n; ++r->n_gone;
}

uint32_t fmdh_mag_arcs_unlink(fmdh_mag_t *g, uint64_t end_id, uint64_t to)
{
    uint64_t where;
    fmdh_arcs_t *r;
    uint32_t i, kept = 0, went;
    if ((int64_t)end_id < 0 || fmdh_mag_end(g, end_id, &where)) return 0;   /* (a negative id names no end of this graph) */
    r = arcs_at(g, where);
    for (i = 0; i < r->n; ++i)
        if (r->a[i].to != to) r->a[kept++] = r->a[i];
    went = r->n - kept;
    r->n = kept; r->n_gone += went;
    return went;
}

static int arcs_append(fmdh_arcs_t *r, uint64_t to, int64_t ovlp)
{
    if (r->n == r->room) {
        const uint32_t room = r->room ? r->room * 2 : 2;
        fmdh_arc_t *a = (fmdh_arc_t *)realloc(r->a, (size_t)room * sizeof(fmdh_arc_t));
        if (!a) return -1;
        r->a = a; r->room = room;
    }
    r->a[r->n].to = to; r->a[r->n].ovlp = ovlp; ++r->n;
    return 0;
}
/* an arc from end `end_id` to `to`, unless there is one */
static void arcs_link(fmdh_mag_t *g, uint64_t end_id, uint64_t to, int ovlp)
{
    uint64_t where;
    fmdh_arcs_t *r;
    uint32_t i;
    if ((int64_t)end_id < 0 || fmdh_mag_end(g, end_id, &where)) return;
    r = arcs_at(g, where);
    for (i = 0; i < r->n; ++i)
        if (r->a[i].to == to) return;
    if (arcs_append(r, to, ovlp)) g->err = 1;
}

static inline int by_end_then_longer(const fmdh_arc_t *a, const fmdh_arc_t *b) { return a->to < b->to || (a->to == b->to && (uint64_t)a->ovlp > (uint64_t)b->ovlp); }
static int cmp_end_then_longer(const void *a, const void *b)
{
    return by_end_then_longer((const fmdh_arc_t *)a, (const fmdh_arc_t *)b) ? -1 : by_end_then_longer((const fmdh_arc_t *)b, (const fmdh_arc_t *)a);
}
static int cmp_longer(const void *a, const void *b)
{
    const int64_t x = ((const fmdh_arc_t *)a)->ovlp, y = ((const fmdh_arc_t *)b)->ovlp;
    return x > y ? -1 : x < y;
}
/* one arc per neighbour, the one with the longest overlap, in the order of the ids; nothing gone is counted any more (v128_rmdup) */
static void arcs_one_per_end(fmdh_arcs_t *r)
{
    uint32_t i, kept = 0;
    r->n_gone = 0;
    if (r->n < 2) return;
    if (r->n <= 24) {   /* nearly every list is a handful of arcs */
        for (i = 1; i < r->n; ++i) {
            const fmdh_arc_t t = r->a[i];
            uint32_t j = i;
            for (; j > 0 && by_end_then_longer(&t, &r->a[j - 1]); --j) r->a[j] = r->a[j - 1];
            r->a[j] = t;
        }
    } else qsort(r->a, r->n, sizeof(fmdh_arc_t), cmp_end_then_longer);
    for (i = 0; i < r->n; ++i)
        if (kept == 0 || r->a[kept - 1].to != r->a[i].to) r->a[kept++] = r->a[i];
    r->n = kept;
}
/* longer than `max`: only the arcs strictly above the overlap of the one that would be number max + 1 stay (v128_cap) */
static void arcs_keep_longest(fmdh_arcs_t *r, int max)
{
    uint32_t i;
    int cut;
    if (max < 0 || r->n <= (uint32_t)max) return;
    qsort(r->a, r->n, sizeof(fmdh_arc_t), cmp_longer);
    cut = (int)r->a[max].ovlp;
    for (i = 0; i < r->n && (int)r->a[i].ovlp != cut; ++i) {}
    r->n = i;
}

/* ---- vertices ---- */
static void v_release(fmdh_magv_t *v)
{
    free(v->end[0].arcs.a); free(v->end[1].arcs.a); free(v->seq); free(v->cov);
    memset(v, 0, sizeof(*v));
    v->len = -1;
}

void fmdh_mag_destroy(fmdh_mag_t *g)
{
    size_t i;
    if (!g) return;
    dict_free(g->h);
    for (i = 0; i < g->n; ++i) v_release(&g->v[i]);
    free(g->v);
    free(g);
}

static inline int own_end(const fmdh_magv_t *p, uint64_t id) { return id == p->end[0].id || id == p->end[1].id; }

/* the vertex goes: its neighbours lose their arcs to it, the dictionary its two ends */
void fmdh_mag_v_del(fmdh_mag_t *g, fmdh_magv_t *p)
{
    int side;
    uint32_t i;
    if (p->len < 0) return;
    for (side = 0; side < 2; ++side)
        for (i = 0; i < p->end[side].arcs.n; ++i) {
            const uint64_t to = p->end[side].arcs.a[i].to;
            if (!own_end(p, to)) fmdh_mag_arcs_unlink(g, to, p->end[side].id);
            if (g->err) return;
        }
    dict_del(g->h, p->end[0].id); dict_del(g->h, p->end[1].id);
    v_release(p);
}

/* the vertex goes, and its left and right neighbours are joined wherever their overlaps with it reach across it by min_ovlp or more */
static void v_bridge_and_del(fmdh_mag_t *g, fmdh_magv_t *p, int min_ovlp)
{
    const fmdh_arcs_t *lt = &p->end[0].arcs, *rt = &p->end[1].arcs;
    uint32_t i, j;
    if (fmdh_arcs_slots(lt) && fmdh_arcs_slots(rt))
        for (i = 0; i < lt->n; ++i) {
            if (own_end(p, lt->a[i].to)) continue;
            for (j = 0; j < rt->n; ++j) {
                const int across = (int)(lt->a[i].ovlp + rt->a[j].ovlp) - p->len;
                if (own_end(p, rt->a[j].to) || across < min_ovlp) continue;
                arcs_link(g, lt->a[i].to, rt->a[j].to, across);
                arcs_link(g, rt->a[j].to, lt->a[i].to, across);
                if (g->err) return;
            }
        }
    fmdh_mag_v_del(g, p);
}

/* the vertex turned round: the other strand, read from the other end */
static void v_turn(fmdh_mag_t *g, fmdh_magv_t *p)
{
    char *lo = p->seq, *hi = p->seq + p->len - 1, *clo = p->cov, *chi = p->cov + p->len - 1;
    int side;
    for (; lo < hi; ++lo, --hi, ++clo, --chi) {
        const char b = *lo, c = *clo;
        *lo = (char)(*hi >= 1 && *hi <= 4 ? 5 - *hi : *hi); *hi = (char)(b >= 1 && b <= 4 ? 5 - b : b);
        *clo = *chi; *chi = c;
    }
    if (lo == hi && *lo >= 1 && *lo <= 4) *lo = (char)(5 - *lo);
    { const fmdh_magend_t t = p->end[0]; p->end[0] = p->end[1]; p->end[1] = t; }
    for (side = 0; side < 2; ++side) {          /* (an end id the vertex has twice is toggled twice) */
        const int64_t s = dict_find(g->h, p->end[side].id);
        if (s < 0) { g->err = 1; return; }
        g->h->val[s] ^= 1;
    }
}

/* ---- merge: while the right end of a vertex has one arc, and the end it leads to has one arc (back), the two vertices are one ---- */
static int v_room(fmdh_magv_t *p, uint32_t need)
{
    uint32_t cap = p->cap ? p->cap : 1;
    char *a, *b;
    if (need <= p->cap) return 0;
    while (cap < need) cap <<= 1;
    if ((a = (char *)realloc(p->seq, cap))) p->seq = a;
    if ((b = (char *)realloc(p->cov, cap))) p->cov = b;
    if (!a || !b) return -1;
    p->cap = cap;
    return 0;
}
/* q, whose LEFT end is the one p's right end leads to, becomes the tail of p; q's slot is empty afterwards */
static int v_swallow(fmdh_mag_t *g, fmdh_magv_t *p, fmdh_magv_t *q)
{
    const fmdh_arc_t out = p->end[1].arcs.a[0];
    const fmdh_arcs_t *back = &q->end[0].arcs;
    int shared, k;
    int64_t s;
    /* the arc, its twin and the two vertices must agree (the reference asserts all of it) */
    if (back->n != 1 || back->a[0].to != p->end[1].id || q->end[0].id != out.to || back->a[0].ovlp != out.ovlp
        || out.ovlp < 0 || out.ovlp > p->len || out.ovlp > q->len || dict_find(g->h, p->end[1].id) < 0) return -1;
    shared = (int)out.ovlp;
    dict_del(g->h, p->end[1].id); dict_del(g->h, q->end[0].id);
    if (v_room(p, (uint32_t)(p->len + q->len - shared) + 1)) return -1;
    for (k = 0; k < shared; ++k) {                       /* over the overlap the coverage adds up, to '~' at the most */
        const int c = (int)p->cov[p->len - shared + k] + (q->cov[k] - 33);
        p->cov[p->len - shared + k] = (char)(c > 126 ? 126 : c);
    }
    memcpy(p->seq + p->len - shared, q->seq, (size_t)q->len);             /* (the shared bases are q's afterwards) */
    memcpy(p->cov + p->len, q->cov + shared, (size_t)(q->len - shared));
    p->len += q->len - shared;
    p->seq[p->len] = p->cov[p->len] = 0;
    p->nsr += q->nsr;
    free(p->end[1].arcs.a);
    p->end[1] = q->end[1];                               /* q's right end, id and arcs, is p's now */
    memset(&q->end[1].arcs, 0, sizeof(fmdh_arcs_t));
    if ((s = dict_find(g->h, p->end[1].id)) < 0) return -1;
    g->h->val[s] = (uint64_t)(p - g->v) << 1 | 1;
    v_release(q);
    return 0;
}
/* grow p to the right as far as it goes without a choice */
static void v_grow_right(fmdh_mag_t *g, fmdh_magv_t *p)
{
    while (!g->err) {
        const fmdh_arcs_t *r = &p->end[1].arcs;
        uint64_t where;
        fmdh_magv_t *q;
        if (fmdh_arcs_slots(r) != 1 || r->n != 1 || (int64_t)r->a[0].to < 0) return;   /* none, several, or one that leads out of the graph */
        if (fmdh_mag_end(g, r->a[0].to, &where)) return;
        q = &g->v[where >> 1];
        if (q == p || fmdh_arcs_slots(&q->end[where & 1].arcs) != 1) return;             /* a loop; a neighbour that has a choice */
        if (where & 1) v_turn(g, q);                                                     /* "><": the neighbour is met at its right end */
        if (g->err || v_swallow(g, p, q)) { g->err = 1; return; }
    }
}

void fmdh_mag_merge(fmdh_mag_t *g, int rmdup)
{
    size_t i;
    int side;
    if (g->err) return;
    for (i = 0; i < g->n; ++i)
        for (side = 0; side < 2; ++side) {
            if (rmdup) arcs_one_per_end(&g->v[i].end[side].arcs);
            else fmdh_mag_arcs_compact(&g->v[i].end[side].arcs);
        }
    for (i = 0; i < g->n && !g->err; ++i) {      /* to the right, then -- turned round, and left that way -- to what was the left */
        if (g->v[i].len < 0) continue;
        v_grow_right(g, &g->v[i]);
        if (!g->err) v_turn(g, &g->v[i]);
        v_grow_right(g, &g->v[i]);
    }
}

/* ---- the easy simplifications ---- */
/* short, few reads, and nothing on one side */
static inline int weak_tip(const fmdh_magv_t *p, int min_len, int min_nsr)
{
    return p->len >= 0 && p->len < min_len && p->nsr < min_nsr && (fmdh_arcs_slots(&p->end[0].arcs) == 0 || fmdh_arcs_slots(&p->end[1].arcs) == 0);
}

void fmdh_mag_rm_vext(fmdh_mag_t *g, int min_len, int min_nsr)
{
    size_t i;
    for (i = 0; i < g->n && !g->err; ++i)
        if (weak_tip(&g->v[i], min_len, min_nsr)) fmdh_mag_v_del(g, &g->v[i]);
}

void fmdh_mag_rm_vint(fmdh_mag_t *g, int min_len, int min_nsr, int min_ovlp)
{
    size_t i;
    for (i = 0; i < g->n && !g->err; ++i)
        if (g->v[i].len >= 0 && g->v[i].len < min_len && g->v[i].nsr < min_nsr) v_bridge_and_del(g, &g->v[i], min_ovlp);
}

/* the arcs of one end that are short, or short beside the longest of that end, go together with their twins.  The yardstick is the
 * longest overlap of the end if it is above min_ovlp and does not lead to a weak tip, else min_ovlp itself. */
static void end_drop_short_arcs(fmdh_mag_t *g, fmdh_magv_t *p, int side, int min_ovlp, double min_ratio, int min_len, int min_nsr)
{
    fmdh_arcs_t *r = &p->end[side].arcs;
    int64_t longest = min_ovlp;
    int has_longest = 0;
    uint32_t i, at = 0;
    for (i = 0; i < r->n; ++i)
        if (r->a[i].ovlp > longest) { longest = r->a[i].ovlp; at = i; has_longest = 1; }   /* the first of equals */
    if (has_longest) {
        uint64_t where;
        if (fmdh_mag_end(g, r->a[at].to, &where)) return;
        if (weak_tip(&g->v[where >> 1], min_len, min_nsr)) longest = min_ovlp;
    }
    for (i = 0; i < r->n && !g->err;) {
        const fmdh_arc_t arc = r->a[i];
        if (!(arc.ovlp < min_ovlp || (double)arc.ovlp / (double)(int)longest < min_ratio)) { ++i; continue; }
        fmdh_mag_arcs_unlink(g, arc.to, p->end[side].id);
        /* (an arc of this end to itself went with its twin: it IS its twin) */
        if (i < r->n && r->a[i].to == arc.to && r->a[i].ovlp == arc.ovlp) fmdh_mag_arc_drop(r, i);
    }
}

void fmdh_mag_rm_edge(fmdh_mag_t *g, int min_ovlp, double min_ratio, int min_len, int min_nsr)
{
    size_t i;
    for (i = 0; i < g->n && !g->err; ++i) {
        fmdh_magv_t *p = &g->v[i];
        if (weak_tip(p, min_len, min_nsr)) continue;       /* they go as a whole or not at all */
        end_drop_short_arcs(g, p, 0, min_ovlp, min_ratio, min_len, min_nsr);
        if (!g->err) end_drop_short_arcs(g, p, 1, min_ovlp, min_ratio, min_len, min_nsr);
    }
}

/* ---- amend: an arc stays only if the end it leads to exists and has the arc back; then one arc per neighbour ---- */
void fmdh_mag_amend(fmdh_mag_t *g)
{
    size_t i;
    int side;
    if (g->err || !g->h) return;
    for (i = 0; i < g->n; ++i)
        for (side = 0; side < 2; ++side) {
            fmdh_magend_t *e = &g->v[i].end[side];
            uint32_t k, kept = 0;
            for (k = 0; k < e->arcs.n; ++k) {
                const int64_t s = dict_find(g->h, e->arcs.a[k].to);
                const fmdh_arcs_t *back;
                uint32_t b;
                if (s < 0) continue;                                   /* e.g. to a tip that was cut while reading */
                if ((g->h->val[s] >> 1) >= g->n) { g->err = 1; return; }
                back = arcs_at(g, g->h->val[s]);
                for (b = 0; b < back->n && back->a[b].to != e->id; ++b) {}
                if (b < back->n) e->arcs.a[kept++] = e->arcs.a[k];
            }
            e->arcs.n = kept;
            arcs_one_per_end(&e->arcs);
        }
}

/* ---- the read-distance estimate: bases per read start over the vertices that hold the better half of the reads, taken from the
 * vertex with the most reads down (of equals, the later one first); a second round leaves out what looks like a repeat by the
 * A-statistic of the first ---- */
typedef struct { int nsr; uint32_t at; } by_reads_t;
static int cmp_more_reads(const void *a, const void *b)
{
    const by_reads_t *x = (const by_reads_t *)a, *y = (const by_reads_t *)b;
    if (x->nsr != y->nsr) return x->nsr > y->nsr ? -1 : 1;
    return x->at > y->at ? -1 : x->at < y->at;
}

double fmdh_mag_cal_rdist(const fmdh_mag_t *g)
{
    by_reads_t *order = (by_reads_t *)malloc((g->n ? g->n : 1) * sizeof(by_reads_t));
    double per_read = -1.;
    int64_t all_reads = 0;
    size_t i;
    int round;
    if (!order) return per_read;
    for (i = 0; i < g->n; ++i) { order[i].nsr = g->v[i].nsr; order[i].at = (uint32_t)i; all_reads += g->v[i].nsr; }
    qsort(order, g->n, sizeof(by_reads_t), cmp_more_reads);
    for (round = 0; round < 2; ++round) {
        int64_t reads = 0, bases = 0;
        for (i = 0; i < g->n; ++i) {
            const fmdh_magv_t *p = &g->v[order[i].at];
            const int span = p->len - (fmdh_arcs_slots(&p->end[0].arcs) != 0) - (fmdh_arcs_slots(&p->end[1].arcs) != 0);
            if (per_read > 0. && span / per_read - p->nsr * M_LN2 < 20.) continue;
            reads += p->nsr; bases += span;
            if ((double)reads >= (double)all_reads * 0.5) break;
        }
        per_read = (double)bases / (double)reads;
    }
    free(order);
    return per_read;
}

/* ---- printing ---- */
typedef struct { char *s; size_t l, m; } sbuf_t;
static int sb_room(sbuf_t *b, size_t extra)
{
    if (b->l + extra + 1 > b->m) {
        size_t m = b->m ? b->m : 256;
        char *s;
        while (m < b->l + extra + 1) m <<= 1;
        if (!(s = (char *)realloc(b->s, m))) return -1;
        b->s = s; b->m = m;
    }
    return 0;
}
static void sb_i64(sbuf_t *b, int64_t v)
{
    char t[24];
    int n = 0;
    uint64_t u = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    if (sb_room(b, 24)) return;
    do { t[n++] = (char)('0' + u % 10); u /= 10; } while (u);
    if (v < 0) t[n++] = '-';
    while (n) b->s[b->l++] = t[--n];
}
static inline void sb_c(sbuf_t *b, int c) { if (!sb_room(b, 1)) b->s[b->l++] = (char)c; }

static void v_write(const fmdh_magv_t *p, sbuf_t *b)   /* mag_v_write, mag.c:149-174 */
{
    int j;
    size_t k;
    if (p->len <= 0) return;   /* (a vertex of no bases leaves the buffer as it was: the caller writes the previous record again) */
    b->l = 0;
    sb_c(b, '@'); sb_i64(b, (int64_t)p->end[0].id); sb_c(b, ':'); sb_i64(b, (int64_t)p->end[1].id);
    sb_c(b, '\t'); sb_i64(b, p->nsr);
    for (j = 0; j < 2; ++j) {
        const fmdh_arcs_t *r = &p->end[j].arcs;
        sb_c(b, '\t');
        for (k = 0; k < r->n; ++k) { sb_i64(b, (int64_t)r->a[k].to); sb_c(b, ','); sb_i64(b, (int32_t)r->a[k].ovlp); sb_c(b, ';'); }
        if (fmdh_arcs_slots(r) == 0) sb_c(b, '.');            /* (a list whose arcs have all gone but still count is an empty field) */
    }
    sb_c(b, '\n');
    if (sb_room(b, 2 * (size_t)p->len + 5)) return;
    for (j = 0; j < p->len; ++j) b->s[b->l++] = (p->seq[j] >= 1 && p->seq[j] <= 4) ? "ACGT"[p->seq[j] - 1] : 0;   /* a base that is none of the four: a NUL */
    memcpy(b->s + b->l, "\n+\n", 3); b->l += 3;
    memcpy(b->s + b->l, p->cov, (size_t)p->len); b->l += (size_t)p->len;
    b->s[b->l++] = '\n';
}

void fmdh_mag_print(const fmdh_mag_t *g, FILE *out)
{
    size_t i;
    sbuf_t b = {0, 0, 0};
    for (i = 0; i < g->n; ++i) {
        if (g->v[i].len < 0) continue;
        v_write(&g->v[i], &b);
        fwrite(b.s, 1, b.l, out);
    }
    free(b.s);
    fflush(out);
}

/* ---- reading ---- */
void fmdh_mag_init_opt(fmdh_magopt_t *o)
{
    memset(o, 0, sizeof(*o));
    o->flag = FMDH_MAG_F_READ_MERGE;
    o->max_arc = 512; o->min_dratio0 = 0.7f;
    o->n_iter = 3; o->min_elen = 300; o->min_ovlp = 60; o->min_ensr = 4; o->min_insr = 3; o->min_dratio1 = 0.8f;
    o->max_bcov = 10.f; o->max_bfrac = 0.15f; o->max_bvtx = 64; o->max_bdist = 512;
}

static int parse_i64(const char **q, int64_t *v)   /* [-]digits */
{
    const char *p = *q;
    int neg = 0;
    uint64_t u = 0;
    if (*p == '-') { neg = 1; ++p; }
    if (!isdigit((unsigned char)*p)) return -1;
    for (; isdigit((unsigned char)*p); ++p) {
        if (u > (UINT64_MAX - 9) / 10) return -1;
        u = u * 10 + (uint64_t)(*p - '0');
    }
    if (u > (uint64_t)INT64_MAX) return -1;
    *v = neg ? -(int64_t)u : (int64_t)u;
    *q = p;
    return 0;
}

/* one side of the header: "." or "id,ovlp;id,ovlp;..."; then the filtering of mag.c:226-245 unless -O.  *q ends behind the field's tab */
static int read_arcs(const char **q, fmdh_arcs_t *nei, const fmdh_magopt_t *opt, int *is_mod)
{
    const char *p = *q;
    int64_t max = 0, max2 = 0;
    uint32_t i, kept = 0;
    nei->n = nei->n_gone = 0;
    if (*p == '.') { *q = p[1] ? p + 2 : p + 1; return 0; }
    while (isdigit((unsigned char)*p) || *p == '-') {
        int64_t x, y;
        if (parse_i64(&p, &x) || *p++ != ',' || parse_i64(&p, &y) || *p++ != ';' || y < 0 || y > INT_MAX) return -1;
        if (arcs_append(nei, (uint64_t)x, y)) return -1;
        /* the largest overlap and what the reference keeps as the second largest: a value that replaces the largest does NOT hand the
         * old one down (mag.c:232-233), so this is the largest of the values that arrived at or below the maximum of their time */
        if (max < y) max = y;
        else if (max2 < y) max2 = y;
    }
    if (*p == '\t') ++p;
    else if (*p) return -1;
    *q = p;
    if (!(opt->flag & FMDH_MAG_F_READ_ORI)) {
        const double thres = (int)((float)max2 * opt->min_dratio0 + .499);   /* int * float is float arithmetic */
        for (i = 0; i < nei->n; ++i) {
            if ((double)nei->a[i].ovlp < thres) *is_mod = 1;
            if ((double)nei->a[i].ovlp >= thres && nei->a[i].ovlp != 0) nei->a[kept++] = nei->a[i];
        }
        nei->n = kept;
        arcs_one_per_end(nei);
        if (opt->max_arc >= 0 && nei->n > (uint32_t)opt->max_arc) { *is_mod = 1; arcs_keep_longest(nei, opt->max_arc); }
    } else {                                            /* as it is: an arc of overlap 0 is a deleted arc that still counts */
        for (i = 0; i < nei->n; ++i)
            if (nei->a[i].ovlp != 0) nei->a[kept++] = nei->a[i];
        nei->n_gone = nei->n - kept; nei->n = kept;
    }
    return 0;
}

static fmdh_mag_t *read_io(fmdh_seqio_t *io, const fmdh_magopt_t *opt)
{
    fmdh_mag_t *g = (fmdh_mag_t *)calloc(1, sizeof(*g));
    fmdh_arcs_t nei = {0, 0, 0, 0};
    int is_mod = 0, len, j;
    uint64_t n_rec = 0;
    const char *why = "out of memory";
    if (!g) return 0;
    while ((len = fmdh_seq_read(io)) >= 0) {
        fmdh_magv_t *p;
        const char *q = fmdh_seq_name(io), *c = fmdh_seq_comment(io), *qual = fmdh_seq_qual(io);
        const char *s = fmdh_seq_bases(io);
        int64_t k0, k1, nsr;
        ++n_rec;
        if (g->n == g->m) {
            const size_t m = g->m ? g->m << 1 : 256;
            fmdh_magv_t *v = (fmdh_magv_t *)realloc(g->v, m * sizeof(*v));
            if (!v) goto fail;
            g->v = v; g->m = m;
        }
        p = &g->v[g->n];
        memset(p, 0, sizeof(*p));
        p->len = -1;
        why = "the name is not <int>:<int>";
        if (parse_i64(&q, &k0) || *q++ != ':' || parse_i64(&q, &k1) || *q) goto fail;
        why = "the header does not hold <#reads> <left arcs> <right arcs>";
        if (!c || parse_i64(&c, &nsr) || nsr < INT_MIN || nsr > INT_MAX || *c++ != '\t') goto fail;
        p->end[0].id = (uint64_t)k0; p->end[1].id = (uint64_t)k1; p->nsr = (int)nsr;
        for (j = 0; j < 2; ++j) {
            fmdh_arcs_t *r = &p->end[j].arcs;
            if (read_arcs(&c, &nei, opt, &is_mod)) { free(p->end[0].arcs.a); goto fail; }
            r->n_gone = nei.n_gone;
            if (nei.n) {
                r->a = (fmdh_arc_t *)malloc(nei.n * sizeof(fmdh_arc_t));
                if (!r->a) { why = "out of memory"; free(p->end[0].arcs.a); goto fail; }
                memcpy(r->a, nei.a, nei.n * sizeof(fmdh_arc_t));
                r->n = r->room = nei.n;
            }
        }
        /* a short tip of one read is cut here, before the dictionary exists (mag.c:250) */
        if (!(opt->flag & FMDH_MAG_F_READ_ORI) && (fmdh_arcs_slots(&p->end[0].arcs) == 0 || fmdh_arcs_slots(&p->end[1].arcs) == 0) && len < opt->min_elen && p->nsr == 1) {
            free(p->end[0].arcs.a); free(p->end[1].arcs.a);
            is_mod = 1;
            continue;
        }
        p->len = len;
        for (p->cap = 1; p->cap < (uint32_t)len + 1;) p->cap <<= 1;
        p->seq = (char *)malloc(p->cap); p->cov = (char *)malloc(p->cap);
        ++g->n;                                       /* from here on fmdh_mag_destroy releases it */
        if (!p->seq || !p->cov) { why = "out of memory"; goto fail; }
        for (j = 0; j < len; ++j) p->seq[j] = (char)fmdh_nt6[(unsigned char)s[j]];
        if (qual) memcpy(p->cov, qual, (size_t)len);
        else memset(p->cov, 34, (size_t)len);         /* a record without qualities: every base seen once */
        p->seq[len] = p->cov[len] = 0;
    }
    /* a quality string that is not as long as its sequence ends the reading as the end of the file does (mag.c:205: the loop runs while the
     * reader returns a length); special.mag.gz of the fixtures is such a file from its first record on.  Not silently, though. */
    if (len == -2) fprintf(stderr, "[W::fmdh_mag_read] record %llu: the quality string is not as long as the sequence; the graph ends before it\n", (unsigned long long)n_rec + 1);
    free(nei.a); nei.a = 0;
    why = "out of memory";
    if (fmdh_mag_build_hash(g)) goto fail;
    if (is_mod || !(opt->flag & FMDH_MAG_F_NO_AMEND)) fmdh_mag_amend(g);
    g->rdist = (float)fmdh_mag_cal_rdist(g);
    if (opt->flag & FMDH_MAG_F_READ_MERGE) fmdh_mag_merge(g, 1);
    return g;
fail:
    fprintf(stderr, "[E::fmdh_mag_read] record %llu: %s\n", (unsigned long long)n_rec, why);
    free(nei.a);
    fmdh_mag_destroy(g);
    return 0;
}

fmdh_mag_t *fmdh_mag_read(const char *fn, const fmdh_magopt_t *opt)
{
    fmdh_seqio_t *io = fmdh_seq_open(fn);
    fmdh_mag_t *g;
    if (!io) { fprintf(stderr, "[E::%s] cannot open `%s'\n", __func__, fn); return 0; }
    g = read_io(io, opt);
    fmdh_seq_close(io);
    return g;
}

fmdh_mag_t *fmdh_mag_read_mem(const void *p, size_t n, const fmdh_magopt_t *opt)
{
    fmdh_seqio_t *io = fmdh_seq_open_mem(p, n);
    fmdh_mag_t *g;
    if (!io) return 0;
    g = read_io(io, opt);
    fmdh_seq_close(io);
    return g;
}

/* ---- clean ---- */
static void tips_then_merge(fmdh_mag_t *g, const fmdh_magopt_t *opt) { fmdh_mag_rm_vext(g, opt->min_elen, opt->min_ensr); fmdh_mag_merge(g, 0); }

void fmdh_mag_clean(fmdh_mag_t *g, const fmdh_magopt_t *opt)
{
    const int aggressive = (opt->flag & FMDH_MAG_F_AGGRESSIVE) != 0;
    int round;
    if (!(opt->flag & FMDH_MAG_F_CLEAN) || g->err) return;
    if (g->min_ovlp < opt->min_ovlp) g->min_ovlp = opt->min_ovlp;
    /* 1. tips and weak arcs, the thresholds rising from a half to the whole over the rounds.  Where the callee takes an int the product is cut
     *    to one; the read count of the tip removal inside the round is, in the reference, the VALUE of its comparison (mag.c:628): 1 where
     *    min_ensr * scale exceeds 2, else 2 */
    fmdh_mag_rm_vext(g, opt->min_elen, opt->min_ensr < 3 ? opt->min_ensr : 3);
    for (round = 0; round < opt->n_iter; ++round) {
        const double scale = opt->n_iter == 1 ? 1. : .5 + .5 * round / (opt->n_iter - 1);
        fmdh_mag_rm_edge(g, (int)(opt->min_ovlp * scale), opt->min_dratio1 * scale, opt->min_elen, opt->min_ensr);
        fmdh_mag_rm_vext(g, (int)(opt->min_elen * scale), opt->min_ensr * scale > 2. ? 1 : 2);
        fmdh_mag_merge(g, 1);
    }
    for (round = 0; round < opt->n_iter; ++round) tips_then_merge(g, opt);
    /* 2. bubbles */
    if (aggressive) fmdh_mag_pop_open(g, opt->min_elen);
    if (!(opt->flag & FMDH_MAG_F_NO_SIMPL)) fmdh_mag_simplify_bubble(g, opt->max_bvtx, opt->max_bdist);
    fmdh_mag_pop_simple(g, opt->max_bcov, opt->max_bfrac, aggressive);
    /* 3. inner vertices of few reads, and what that leaves behind */
    if (opt->min_insr >= 2) {
        fmdh_mag_rm_vint(g, opt->min_elen, opt->min_insr, g->min_ovlp);
        fmdh_mag_rm_edge(g, opt->min_ovlp, opt->min_dratio1, opt->min_elen, opt->min_ensr);
        fmdh_mag_rm_vext(g, opt->min_elen, opt->min_ensr);
        fmdh_mag_merge(g, 1);
    }
    if (aggressive) fmdh_mag_pop_open(g, opt->min_elen);
    else tips_then_merge(g, opt);
}
