/* mag_bubble.c -- the bubble operations of `fermi clean` over the graph of mag.c; what each leaves behind is what the reference's
 * operation of that name leaves behind (bubble.c):
 *   simplify_bubble  from every end with two or more arcs, a walk in topological order to the end where all the ways meet again;
 *                    every vertex inside that is on neither of the two ways with the most reads goes;
 *   pop_simple       an end with exactly two arcs whose two neighbours lead on to one and the same end: the arm with the lower coverage
 *                    goes when the two arms say nearly the same (or, with `aggressive`, whenever they do and whatever its coverage);
 *   pop_open         a short vertex that hangs on one arc and says what another arc of the end it hangs on leads into loses that arc.
 * All three end with merge(0). */
#include <limits.h>
#include <stdlib.h>
#include <string.h>
#include "mag.h"

/* two stretches say "nearly the same" when their alignment shows fewer differences than this, or fewer per base than that */
#define FEW_DIFFS 2.01
#define FEW_DIFFS_PER_BASE 0.1
#define DIFFS_PER_BASE_OF_LENGTH 0.2   /* no alignment to be had (an arm without bases of its own): the difference in length stands in */

/* ---- simplify_bubble ---- */
#define NO_WAY INT_MIN                 /* reads of a way that does not exist; it still takes part in the sums below, as in the reference */
#define NOWHERE 0xffffffffu
typedef struct {
    int reads, bases;                  /* on the way from the start to here; the start's own are taken off first */
    uint32_t left_through;             /* the end (vertex << 1 | side) the way left the vertex before through */
    int rank_there;                    /* and which of that vertex's two ways it continues */
} way_t;
typedef struct {
    uint32_t vertex;
    int arcs_walked[2];                /* per end: arcs into it the walk has come over */
    way_t best[2][2];                  /* per end: the way with the most reads and the runner-up */
    int on_a_best_way;
} visit_t;
typedef struct {
    visit_t *visit; size_t n_visit, m_visit;
    uint64_t *ready; size_t n_ready, m_ready;     /* ends all of whose arcs have been walked, last in first out */
} walk_t;

static visit_t *visit_new(walk_t *w, fmdh_magv_t *v, uint32_t vertex)
{
    static const way_t none = {NO_WAY, NO_WAY, NOWHERE, 0};
    visit_t *t;
    if (w->n_visit == w->m_visit) {
        const size_t m = w->m_visit ? w->m_visit * 2 : 256;
        if (!(t = (visit_t *)realloc(w->visit, m * sizeof(visit_t)))) return 0;
        w->visit = t; w->m_visit = m;
    }
    t = &w->visit[w->n_visit++];
    memset(t, 0, sizeof(*t));
    t->vertex = vertex;
    t->best[0][0] = t->best[0][1] = t->best[1][0] = t->best[1][1] = none;
    v->aux = (int32_t)w->n_visit;
    return t;
}
static inline visit_t *visit_of(walk_t *w, const fmdh_mag_t *g, uint64_t vertex) { return &w->visit[g->v[vertex].aux - 1]; }
static int ready_push(walk_t *w, uint64_t end)
{
    if (w->n_ready == w->m_ready) {
        const size_t m = w->m_ready ? w->m_ready * 2 : 64;
        uint64_t *s = (uint64_t *)realloc(w->ready, m * 8);
        if (!s) return -1;
        w->ready = s; w->m_ready = m;
    }
    w->ready[w->n_ready++] = end;
    return 0;
}
static inline int clamp_int(int64_t x) { return x < INT_MIN ? INT_MIN : x > INT_MAX ? INT_MAX : (int)x; }

/* way `rank` into end `in` of vertex p, carried on over p and an arc of overlap `ovlp` that leaves p through `out` */
static way_t way_across(const visit_t *at, int in, int rank, const fmdh_magv_t *p, int64_t ovlp, uint32_t out)
{
    way_t w;
    w.reads = clamp_int((int64_t)at->best[in][rank].reads + p->nsr);
    w.bases = clamp_int((int64_t)at->best[in][rank].bases + p->len - (int32_t)ovlp);
    w.left_through = out; w.rank_there = rank;
    return w;
}
/* two ways arrive over one arc, the best and the second best of the vertex before: where the first becomes the new best here, the old best
 * moves down and the second competes for runner-up; else the first competes for runner-up itself */
static void ways_offer(way_t top[2], way_t first, way_t second)
{
    way_t c = first;
    if (c.reads > top[0].reads) { top[1] = top[0]; top[0] = c; c = second; }
    if (c.reads > top[1].reads) top[1] = c;
}
/* back along a way to the start, marking the vertices it crosses; 1 if any */
static int way_mark(fmdh_mag_t *g, walk_t *w, way_t way, uint64_t start)
{
    int any = 0;
    size_t steps = 0;
    while (way.left_through != start) {
        const uint64_t vertex = way.left_through >> 1;
        visit_t *t;
        if (way.left_through == NOWHERE || vertex >= g->n || g->v[vertex].aux == 0 || ++steps > 4 * w->n_visit + 4) { g->err = 1; return any; }
        t = visit_of(w, g, vertex);
        t->on_a_best_way = 1; any = 1;
        way = t->best[(way.left_through & 1) ^ 1][way.rank_there];      /* it had come in at the other end */
    }
    return any;
}

static void simplify_from(fmdh_mag_t *g, uint64_t start, int max_vtx, int max_dist, walk_t *w)   /* start: the end the bubble opens at */
{
    const uint64_t entry = start ^ 1;          /* the walk "arrives" at the start vertex's other end */
    fmdh_magv_t *p = &g->v[start >> 1];
    visit_t *t;
    size_t i;
    int waiting = 0, closed = 0;               /* waiting: vertices seen whose arcs have not all been walked */
    if (p->len < 0 || fmdh_arcs_slots(&p->end[start & 1].arcs) < 2) return;
    w->n_ready = w->n_visit = 0;
    if (!(t = visit_new(w, p, (uint32_t)(start >> 1))) || ready_push(w, entry)) { g->err = 1; goto done; }
    t->best[entry & 1][0].reads = -p->nsr;     /* so that a way's sums start behind the start vertex */
    t->best[entry & 1][0].bases = -p->len;
    while (w->n_ready) {
        uint64_t in;
        const fmdh_arcs_t *out;
        uint32_t k;
        if (w->n_ready == 1 && w->ready[0] != entry && waiting == 0) break;                 /* everything has met again in one end */
        in = w->ready[--w->n_ready];
        p = &g->v[in >> 1];
        out = &p->end[(in & 1) ^ 1].arcs;
        t = visit_of(w, g, in >> 1);
        if ((int64_t)w->n_visit > max_vtx || t->best[in & 1][0].bases > max_dist || t->best[in & 1][1].bases > max_dist || fmdh_arcs_slots(out) == 0)
            break;                                                                          /* too many vertices, too far, or a dead end */
        for (k = 0; k < out->n; ++k) {
            uint64_t to;
            fmdh_magv_t *q;
            visit_t *u;
            if ((int64_t)out->a[k].to < 0) continue;
            if (fmdh_mag_end(g, out->a[k].to, &to)) goto done;
            if (to == entry) { w->n_ready = 0; break; }                                     /* round to the start: no bubble */
            q = &g->v[to >> 1];
            if (q->aux == 0) {
                if (!visit_new(w, q, (uint32_t)(to >> 1))) { g->err = 1; goto done; }
                ++waiting;
                fmdh_mag_arcs_compact(&q->end[to & 1].arcs);                                /* its arcs are counted below */
            }
            t = visit_of(w, g, in >> 1); u = visit_of(w, g, to >> 1);                       /* (the records may have moved) */
            ways_offer(u->best[to & 1], way_across(t, (int)(in & 1), 0, p, out->a[k].ovlp, (uint32_t)(in ^ 1)),
                       way_across(t, (int)(in & 1), 1, p, out->a[k].ovlp, (uint32_t)(in ^ 1)));
            if ((uint32_t)++u->arcs_walked[to & 1] == fmdh_arcs_slots(&q->end[to & 1].arcs)) {
                if (ready_push(w, to)) { g->err = 1; goto done; }
                --waiting;
            }
        }
    }
    if (waiting == 0 && w->n_ready == 1) {     /* (also when the walk gave up with exactly one end left ready: the reference's test is this one) */
        const uint64_t last = w->ready[0];
        const way_t a = visit_of(w, g, last >> 1)->best[last & 1][0], b = visit_of(w, g, last >> 1)->best[last & 1][1];
        closed = way_mark(g, w, a, start);
        if (!g->err) closed |= way_mark(g, w, b, start);
    }
done:
    for (i = 0; i < w->n_visit; ++i) g->v[w->visit[i].vertex].aux = 0;
    if (closed && !g->err)
        for (i = 1; i < w->n_visit && !g->err; ++i)                                         /* (0 is the start) */
            if (w->visit[i].vertex != w->ready[0] >> 1 && !w->visit[i].on_a_best_way) fmdh_mag_v_del(g, &g->v[w->visit[i].vertex]);
}

void fmdh_mag_simplify_bubble(fmdh_mag_t *g, int max_vtx, int max_dist)
{
    walk_t w;
    size_t i;
    if (g->err) return;
    memset(&w, 0, sizeof(w));
    for (i = 0; i < 2 * g->n && !g->err; ++i) simplify_from(g, i, max_vtx, max_dist, &w);
    free(w.visit); free(w.ready);
    fmdh_mag_merge(g, 0);
}

/* ---- pop_simple ---- */
typedef struct {
    fmdh_magv_t *v;
    int entered;               /* the end of v the bubble's opening leads into */
    int own;                   /* bases between its two overlaps; <= 0 where they meet or cross (around a tandem repeat) */
    float cover;               /* mean coverage of those bases (of what lies between the overlaps' edges where there are none) */
    uint8_t *bases;            /* own > 0: the bases, codes 0..3, in the direction the bubble is crossed */
} arm_t;

/* 0: this is an arm; 1: it is not; -1: error */
static int arm_take(fmdh_mag_t *g, const fmdh_arc_t *arc, arm_t *m)
{
    uint64_t where;
    const fmdh_arcs_t *lt, *rt;
    if ((int64_t)arc->to < 0) return 1;
    if (fmdh_mag_end(g, arc->to, &where)) return -1;
    m->v = &g->v[where >> 1]; m->entered = (int)(where & 1); m->bases = 0;
    lt = &m->v->end[0].arcs; rt = &m->v->end[1].arcs;
    if (fmdh_arcs_slots(lt) != 1 || fmdh_arcs_slots(rt) != 1 || lt->n != 1 || rt->n != 1) return 1;   /* an arm has one way in and one way out */
    if (lt->a[0].ovlp < 0 || rt->a[0].ovlp < 0 || lt->a[0].ovlp > m->v->len || rt->a[0].ovlp > m->v->len) { g->err = 1; return -1; }
    m->own = m->v->len - (int)(lt->a[0].ovlp + rt->a[0].ovlp);
    return 0;
}
static int arm_measure(arm_t *m)
{
    const fmdh_magv_t *v = m->v;
    const int from = (int)v->end[0].arcs.a[0].ovlp, to = v->len - (int)v->end[1].arcs.a[0].ovlp;   /* own > 0: [from, to) are the arm's own */
    int i;
    m->cover = 0.;
    if (m->own > 0) {
        if (!(m->bases = (uint8_t *)malloc((size_t)m->own))) return -1;
        for (i = 0; i < m->own; ++i) {          /* entered at the right end: crossed from `to` down, on the other strand */
            const int at = m->entered ? to - 1 - i : from + i;
            const uint8_t c = (uint8_t)(v->seq[at] - 1);
            m->bases[i] = (uint8_t)(m->entered && c < 4 ? 3 - c : c);
            m->cover += v->cov[at] - 33;
        }
        m->cover /= m->own;
    } else if (from != to) {
        const int lo = from < to ? from : to, hi = from < to ? to : from;
        for (i = lo; i < hi; ++i) m->cover += v->cov[i] - 33;
        m->cover /= hi - lo;
    } else m->cover = v->cov[from] - 33;
    return 0;
}

static void pop_simple_at(fmdh_mag_t *g, uint64_t opening, float max_cov, float max_frac, int aggressive)
{
    const fmdh_magv_t *p = &g->v[opening >> 1];
    const fmdh_arcs_t *r = &p->end[opening & 1].arcs;
    const float few = aggressive ? FEW_DIFFS * 2. : FEW_DIFFS;
    arm_t arm[2];
    float diffs, per_base;
    int j;
    if (p->len < 0 || fmdh_arcs_slots(r) != 2 || r->n != 2) return;
    for (j = 0; j < 2; ++j)
        if (arm_take(g, &r->a[j], &arm[j])) return;
    if (arm[0].v->end[arm[0].entered ^ 1].arcs.a[0].to != arm[1].v->end[arm[1].entered ^ 1].arcs.a[0].to) return;   /* they do not lead on to the same end */
    if (arm_measure(&arm[0]) || arm_measure(&arm[1])) { g->err = 1; goto done; }
    if (arm[0].own > 0 && arm[1].own > 0) {
        const int shorter = arm[0].own < arm[1].own ? arm[0].own : arm[1].own;
        const int score = fmdh_sw_score(arm[0].own, arm[0].bases, arm[1].own, arm[1].bases);
        if (score < 0) { g->err = 1; goto done; }
        diffs = (shorter * 5. - score) / (5. + 4.);          /* what is missing from a full score, in mismatches (+5 against -4) */
        per_base = diffs / ((arm[0].own + arm[1].own) / 2.);
    } else {
        diffs = abs(arm[0].own - arm[1].own) * DIFFS_PER_BASE_OF_LENGTH;
        per_base = 1.;
    }
    if (diffs < few || per_base < FEW_DIFFS_PER_BASE) {
        const arm_t *weak = arm[0].cover < arm[1].cover ? &arm[0] : &arm[1], *strong = weak == &arm[0] ? &arm[1] : &arm[0];
        if (aggressive || (weak->cover < max_cov && weak->cover / (strong->cover + weak->cover) < max_frac)) fmdh_mag_v_del(g, weak->v);
    }
done:
    free(arm[0].bases); free(arm[1].bases);
}

void fmdh_mag_pop_simple(fmdh_mag_t *g, float max_cov, float max_frac, int aggressive)
{
    size_t i;
    if (g->err) return;
    for (i = 0; i < 2 * g->n && !g->err; ++i) pop_simple_at(g, i, max_cov, max_frac, aggressive);
    fmdh_mag_merge(g, 0);
}

/* ---- pop_open ---- */
/* what a vertex holds beyond an overlap of `ovlp` bases at its end `side`, read away from that end, at most `most` bases, as codes 0..3 */
static int beyond_overlap(const fmdh_magv_t *t, int side, int ovlp, int most, uint8_t *dst)
{
    int j, k = 0;
    if (side == 0) for (j = ovlp; j < t->len && k < most; ++j) dst[k++] = (uint8_t)(t->seq[j] - 1);
    else for (j = t->len - ovlp - 1; j >= 0 && k < most; --j) dst[k++] = (uint8_t)(4 - t->seq[j]);
    return k;
}
/* does one of the OTHER arcs of this end lead into something that says what `hang` (n_hang bases) says?  1 / 0 / -1 */
static int a_sibling_says_it(fmdh_mag_t *g, const fmdh_arcs_t *siblings, uint64_t not_to, const uint8_t *hang, int n_hang, int most, uint8_t *room)
{
    uint32_t i;
    for (i = 0; i < siblings->n; ++i) {
        uint64_t where;
        const fmdh_magv_t *t;
        int n, score;
        if (siblings->a[i].to == not_to || (int64_t)siblings->a[i].to < 0) continue;
        if (fmdh_mag_end(g, siblings->a[i].to, &where)) return -1;
        t = &g->v[where >> 1];
        if (siblings->a[i].ovlp < 0 || siblings->a[i].ovlp > t->len) { g->err = 1; return -1; }
        n = beyond_overlap(t, (int)(where & 1), (int)siblings->a[i].ovlp, most, room);
        if ((score = fmdh_sw_score(n_hang, hang, n, room)) < 0) { g->err = 1; return -1; }
        if (score >= n_hang * 5 / 2) {                       /* at least half of a full score, and then few differences */
            const double diffs = (n_hang * 5. - score) / (5. + 4.);
            if (diffs < FEW_DIFFS || diffs / n_hang < FEW_DIFFS_PER_BASE) return 1;
        }
    }
    return 0;
}

static void pop_open_at(fmdh_mag_t *g, fmdh_magv_t *p, int min_elen)
{
    fmdh_arcs_t *mine;
    int side;
    uint32_t l;
    if (p->len < 0 || p->len >= min_elen) return;
    if (fmdh_arcs_slots(&p->end[0].arcs) + fmdh_arcs_slots(&p->end[1].arcs) != 1) return;   /* it hangs on ONE arc */
    side = fmdh_arcs_slots(&p->end[0].arcs) ? 0 : 1;
    mine = &p->end[side].arcs;
    for (l = 0; l < mine->n && !g->err;) {
        const fmdh_arc_t arc = mine->a[l];
        uint64_t where;
        fmdh_arcs_t *theirs;
        uint8_t *buf;
        int most, n_hang, same;
        ++l;
        if ((int64_t)arc.to < 0) continue;
        if (fmdh_mag_end(g, arc.to, &where)) return;
        theirs = &g->v[where >> 1].end[where & 1].arcs;
        if (&g->v[where >> 1] == p || fmdh_arcs_slots(theirs) == 1) continue;                 /* nothing else leaves that end */
        if (arc.ovlp < 0 || arc.ovlp > p->len) { g->err = 1; return; }
        most = (p->len - (int)arc.ovlp) * 2;
        if (!(buf = (uint8_t *)malloc(2 * (size_t)most + 2))) { g->err = 1; return; }
        n_hang = beyond_overlap(p, side, (int)arc.ovlp, most, buf);
        same = a_sibling_says_it(g, theirs, p->end[side].id, buf, n_hang, most, buf + most + 1);
        free(buf);
        if (same > 0) {                                       /* the arc and its twin go */
            uint32_t k;
            for (k = 0; k < theirs->n;)
                if (theirs->a[k].to == p->end[side].id) fmdh_mag_arc_drop(theirs, k); else ++k;
            fmdh_mag_arc_drop(mine, --l);
        }
    }
    if (!g->err && mine->n == 0) fmdh_mag_v_del(g, p);        /* nothing holds it any more */
}

void fmdh_mag_pop_open(fmdh_mag_t *g, int min_elen)
{
    size_t i;
    if (g->err) return;
    for (i = 0; i < g->n && !g->err; ++i) pop_open_at(g, &g->v[i], min_elen);
    fmdh_mag_merge(g, 0);
}
