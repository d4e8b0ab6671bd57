/* scaf_core.c -- the host side of `scaf` that needs no device (scaf.h): the remapped MAG, rdist and A, the choice of the best two
 * neighbours of every end from the link stage's groups, contained unitigs, the verdict on a locally assembled gap, the alignment fallback for
 * overlapping ends, and the joiner.  mag_scaf_core and what it calls (scaf.c), restated; each function names the lines it stands for. */
#include <ctype.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fmd_host.h"
#include "scaf.h"

#define NONE64 (~0ull)
#define LOW40(v) ((int64_t)((v) << 24 >> 24))

/* ---- reading (read_utig, scaf.c:47-115) ---- */
static int ent_push(fmdh_scaf_t *s, uint64_t x, uint64_t span, uint32_t u)
{
    if (s->n_ent == s->m_ent) {
        const uint64_t m = s->m_ent ? s->m_ent << 1 : 1024;
        uint64_t *nx = (uint64_t *)realloc(s->x, m * 8), *ns;
        uint32_t *nu;
        if (!nx) return -1;
        s->x = nx;
        if (!(ns = (uint64_t *)realloc(s->span, m * 8))) return -1;
        s->span = ns;
        if (!(nu = (uint32_t *)realloc(s->utig, m * 4))) return -1;
        s->utig = nu; s->m_ent = m;
    }
    s->x[s->n_ent] = x; s->span[s->n_ent] = span; s->utig[s->n_ent++] = u;
    return 0;
}

void fmdh_scaf_free(fmdh_scaf_t *s)
{
    size_t i;
    int a;
    if (!s) return;
    for (i = 0; i < s->n; ++i) {
        fmdh_scaf_utig_t *p = &s->u[i];
        free(p->seq);
        for (a = 0; a < 2; ++a)                       /* both ends of a link share one string: the lower end frees it */
            if ((int64_t)(i << 1) < p->nei[a]) free(p->ext[a].s);
    }
    free(s->u); free(s->x); free(s->span); free(s->utig); free(s->self); free(s->mate); free(s);
}

fmdh_scaf_t *fmdh_scaf_read(const char *fn)
{
    fmdh_seqio_t *io = fmdh_seq_open(fn);
    fmdh_scaf_t *s;
    int l;
    if (!io) return 0;
    s = (fmdh_scaf_t *)calloc(1, sizeof(*s));
    while (s && (l = fmdh_seq_read(io)) >= 0) {
        const char *comment = fmdh_seq_comment(io), *name = fmdh_seq_name(io), *bases = fmdh_seq_bases(io), *qual = fmdh_seq_qual(io), *ur, *qq;
        char *end;
        long k[2] = {0, 0};
        int i, j, beg = 0, stop = l;
        fmdh_scaf_utig_t *p;
        if (!comment || !*comment) continue;
        if (!(ur = strstr(comment, "UR:Z:"))) continue;
        ur += 5;
        if (s->n == s->m) {
            const size_t m = s->m ? s->m << 1 : 64;
            fmdh_scaf_utig_t *nu = (fmdh_scaf_utig_t *)realloc(s->u, m * sizeof(*nu));
            if (!nu) { s->err = 2; break; }
            s->u = nu; s->m = m;
        }
        p = &s->u[s->n];
        memset(p, 0, sizeof(*p));
        p->nei[0] = p->nei[1] = p->nei2[0] = p->nei2[1] = -1;
        p->nsr = (int)strtol(comment, &end, 10);
        qq = end;
        sscanf(name, "%ld:%ld", &k[0], &k[1]);
        p->k[0] = (uint64_t)k[0]; p->k[1] = (uint64_t)k[1];
        if (qual) {                                   /* the ends covered by a single read go (quality '"') */
            for (i = 0; i < l && qual[i] == 34; ++i) {}
            beg = i;
            for (i = l - 1; i >= 0 && qual[i] == 34; --i) {}
            stop = i + 1;
            if (beg >= stop) { beg = 0; stop = l; }
        }
        p->len = stop - beg;
        if (!(p->seq = (uint8_t *)calloc(1, (size_t)p->len + 1))) { s->err = 2; break; }
        for (i = 0; i < p->len; ++i) p->seq[i] = fmdh_nt6[(unsigned char)bases[beg + i]];
        /* maxo: the reference means to scan both neighbour lists, but its first round only steps over the blank behind the read count
         * (scaf.c:89-99), so the overlaps of the FIRST list are the ones that count */
        for (j = p->maxo = 0; j < 2 && *qq; ++j) {
            if (*qq != '.') {
                while (isdigit((unsigned char)*qq) || *qq == '-') {
                    long o;
                    strtol(qq, &end, 10); qq = end; if (*qq) ++qq;
                    o = strtol(qq, &end, 10); qq = end; if (*qq) ++qq;
                    if (o > p->maxo) p->maxo = (int)o;
                }
                if (*qq) ++qq;
            } else qq += qq[1] ? 2 : 1;
        }
        p->first = s->n_ent;
        while (isdigit((unsigned char)*ur)) {
            long x, b, e;
            int lo, hi;
            x = strtol(ur, &end, 10); ur = *end ? end + 1 : end;
            b = strtol(ur, &end, 10); ur = *end ? end + 1 : end;
            e = strtol(ur, &end, 10); ur = end;
            lo = (int)e - beg < p->len ? (int)e - beg : p->len;
            if (lo < 0) lo = 0;                       /* (a span that ends before the trimmed unitig begins) */
            hi = (int)b > beg ? (int)b - beg : 0;
            if (hi > p->len) hi = p->len;             /* (a span that begins behind the trimmed unitig: the reference's distance goes negative there and spills into the end's id) */
            if (ent_push(s, (uint64_t)x, (uint64_t)hi << 32 | (uint32_t)lo, (uint32_t)s->n)) { s->err = 2; break; }
            if (*ur++ == 0) break;
        }
        p->n_reads = s->n_ent - p->first;
        ++s->n;
        if (s->err) break;
    }
    fmdh_seq_close(io);
    if (s && s->err) { fmdh_scaf_free(s); return 0; }
    return s;
}

/* ---- what a binding reads and sets without knowing the structs' layout ---- */
size_t fmdh_scaf_count(const fmdh_scaf_t *s) { return s->n; }
void fmdh_scaf_unitig_info(const fmdh_scaf_t *s, size_t i, uint64_t k[2], int32_t len_nsr_maxo[3], double *A, uint64_t *n_reads)
{
    const fmdh_scaf_utig_t *p = &s->u[i];
    k[0] = p->k[0]; k[1] = p->k[1]; len_nsr_maxo[0] = p->len; len_nsr_maxo[1] = p->nsr; len_nsr_maxo[2] = p->maxo; *A = p->A; *n_reads = p->n_reads;
}
uint64_t fmdh_scaf_entries(const fmdh_scaf_t *s, const uint64_t **x, const uint64_t **span, const uint32_t **utig, uint8_t *excluded /* n unitigs */)
{
    size_t i;
    *x = s->x; *span = s->span; *utig = s->utig;
    for (i = 0; excluded && i < s->n; ++i) excluded[i] = s->u[i].excluded;
    return s->n_ent;
}
int fmdh_scaf_set_links(fmdh_scaf_t *s, const uint64_t *self, const uint64_t *mate)
{
    const size_t bytes = (size_t)(s->n_ent ? s->n_ent : 1) * 8;
    free(s->self); free(s->mate);
    s->self = (uint64_t *)malloc(bytes); s->mate = (uint64_t *)malloc(bytes);
    if (!s->self || !s->mate) return -1;
    if (s->n_ent) { memcpy(s->self, self, (size_t)s->n_ent * 8); memcpy(s->mate, mate, (size_t)s->n_ent * 8); }
    return 0;
}

/* ---- rdist and A (cal_rdist, scaf.c:152-187) ---- */
static int cmp_u64(const void *a, const void *b) { const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b; return x < y ? -1 : x > y; }

double fmdh_scaf_cal_rdist(fmdh_scaf_t *s)
{
    const double a_thres = 20.;                        /* A_THRES of scaf.c:17, whatever -a says */
    uint64_t *srt = (uint64_t *)calloc(s->n ? s->n : 1, 8);
    double rdist = -1.;
    int64_t i, sum_n_all = 0, sum_n, sum_l, sum_ovlp = 0;
    int j, n_ovlp = 0, avg_ovlp;
    if (!srt) return rdist;
    for (i = 0; i < (int64_t)s->n; ++i) { srt[i] = (uint64_t)(uint32_t)s->u[i].nsr << 32 | (uint64_t)i; sum_n_all += s->u[i].nsr; }
    qsort(srt, s->n, 8, cmp_u64);
    for (j = 0; j < 2; ++j) {                          /* the unitigs with the most reads, down to half of all reads; the second time without those of low A */
        sum_n = sum_l = 0;
        for (i = (int64_t)s->n - 1; i >= 0; --i) {
            const fmdh_scaf_utig_t *p = &s->u[srt[i] & 0xffffffffu];
            if (rdist > 0. && (p->len - p->maxo) / rdist - p->nsr * M_LN2 < a_thres) continue;
            sum_n += p->nsr; sum_l += p->len - p->maxo;
            if (sum_n >= sum_n_all * 0.5) break;
        }
        rdist = (double)sum_l / sum_n;
    }
    free(srt);
    for (i = 0; i < (int64_t)s->n; ++i) if (s->u[i].maxo) { ++n_ovlp; sum_ovlp += s->u[i].maxo; }
    { const double v = (double)sum_ovlp / n_ovlp + .499; avg_ovlp = v == v && v < 2147483647. && v > -2147483648. ? (int)v : INT_MIN; }   /* no overlap anywhere: what the conversion gives on x86 */
    for (i = 0; i < (int64_t)s->n; ++i) {
        fmdh_scaf_utig_t *p = &s->u[i];
        p->A = (int)((uint32_t)p->len - (uint32_t)(p->maxo ? p->maxo : avg_ovlp)) / rdist - p->nsr * M_LN2;
    }
    s->rdist = rdist;
    return rdist;
}

void fmdh_scaf_exclude(fmdh_scaf_t *s, double a_thres)
{
    size_t i;
    for (i = 0; i < s->n; ++i) if (s->u[i].A < a_thres) s->u[i].excluded = 1;
}

/* ---- the best two neighbours of every end (scaf.c:213-252).  The reference collects an end's neighbours in a small hash table and walks
 * its buckets choosing with >=, so among neighbours of equal weight the bucket order decides; the table is emptied from end to end but keeps its
 * size while that is below 32 buckets.  The table is replayed here -- same hash, probing and growth (khash 0.2.6), keys put in the order
 * of the end's reads -- and takes each neighbour's weight from the link stage's groups. ---- */
/* The table as this loop needs it: keys are only ever added, and the whole table is emptied between ends, so a slot is free or taken and
 * nothing else.  What must be the reference's is WHERE a key lands: slot hash & mask first, then steps of ((hash >> 3 ^ hash << 3) | 1) & mask,
 * hash = the low word of key >> 33 ^ key ^ key << 11; the table doubles (from 0 to 4) when a put finds it 77 % full -- a put of a key that is
 * already there included.  Growing rehashes in place there; seen from outside that is an ORDER in which the old keys enter the empty
 * larger table: old slot 0, 1, 2, ... in turn, except that a key which lands on the number of an old slot whose key has not moved yet is
 * followed at once by that key.  tab_grow replays that order with two tables instead of one. */
typedef struct { uint32_t slots, used, full_at; uint8_t *taken; uint64_t *key, *val; } nbr_tab_t;

static inline uint32_t tab_hash(uint64_t k) { return (uint32_t)(k >> 33 ^ k ^ k << 11); }
static void tab_drop(nbr_tab_t *t) { free(t->taken); free(t->key); free(t->val); memset(t, 0, sizeof(*t)); }
static void tab_empty(nbr_tab_t *t) { if (t->slots) memset(t->taken, 0, t->slots); t->used = 0; }
/* the slot of k in a table without holes: where it is, or the first free slot of its probe sequence */
static uint32_t tab_slot(const uint8_t *taken, const uint64_t *key, uint32_t slots, uint64_t k)
{
    const uint32_t h = tab_hash(k), mask = slots - 1, step = ((h >> 3 ^ h << 3) | 1) & mask;
    uint32_t at = h & mask;
    while (taken[at] && key[at] != k) at = (at + step) & mask;
    return at;
}
static int tab_grow(nbr_tab_t *t)
{
    const uint32_t bigger = t->slots ? t->slots << 1 : 4;
    uint8_t *taken = (uint8_t *)calloc(bigger, 1), *moved = (uint8_t *)calloc(t->slots ? t->slots : 1, 1);
    uint64_t *key = (uint64_t *)malloc((size_t)bigger * 8), *val = (uint64_t *)malloc((size_t)bigger * 8);
    uint32_t j;
    if (!taken || !moved || !key || !val) { free(taken); free(moved); free(key); free(val); return -1; }
    for (j = 0; j < t->slots; ++j) {
        uint32_t from = j;
        while (t->taken[from] && !moved[from]) {       /* this key, then whichever unmoved key sat under the number it lands on */
            const uint32_t to = tab_slot(taken, key, bigger, t->key[from]);
            taken[to] = 1; key[to] = t->key[from]; val[to] = t->val[from];
            moved[from] = 1;
            if (to >= t->slots) break;
            from = to;
        }
    }
    free(moved); free(t->taken); free(t->key); free(t->val);
    t->taken = taken; t->key = key; t->val = val; t->slots = bigger;
    t->full_at = (uint32_t)(bigger * 0.77 + 0.5);
    return 0;
}
/* *at = the slot of k, *fresh = 1 when it was not there before */
static int tab_put(nbr_tab_t *t, uint64_t k, uint32_t *at, int *fresh)
{
    if (t->used >= t->full_at && tab_grow(t)) return -1;
    *at = tab_slot(t->taken, t->key, t->slots, k);
    *fresh = !t->taken[*at];
    if (*fresh) { t->taken[*at] = 1; t->key[*at] = k; ++t->used; }
    return 0;
}

static inline uint64_t to_avg(uint64_t v) { return v ? v >> 40 << 40 | (uint64_t)(int)((double)LOW40(v) / (double)(v >> 40) + .499) : 0; }

int fmdh_scaf_choose(fmdh_scaf_t *s, uint64_t n_groups, const uint64_t *gkey, const uint64_t *gval, const uint32_t *n_nei)
{
    uint64_t *goff = (uint64_t *)calloc(2 * s->n + 1, 8), e;
    nbr_tab_t t;
    size_t i;
    int a, rc = 0;
    memset(&t, 0, sizeof(t));
    if (!goff) return -1;
    for (e = 0; e < 2 * s->n; ++e) goff[e + 1] = goff[e] + n_nei[e];
    if (goff[2 * s->n] != n_groups) { free(goff); return -1; }
    for (i = 0; i < s->n && !rc; ++i) {
        fmdh_scaf_utig_t *p = &s->u[i];
        for (a = 0; a < 2 && !rc; ++a) {
            const uint64_t own = (uint64_t)i << 1 | (uint64_t)a;
            uint64_t j;
            uint32_t k;
            if (t.slots >= 32) tab_drop(&t); else tab_empty(&t);
            for (j = p->first; j < p->first + p->n_reads; ++j) {
                const uint64_t sv = s->self[j], mv = s->mate[j];
                int absent;
                if (sv == NONE64 || ((sv >> 32) & 1) != (uint64_t)a || mv == NONE64 || (mv >> 33) == i) continue;
                if (tab_put(&t, mv >> 32, &k, &absent)) { rc = -1; break; }
                if (absent) {                          /* its weight: the group (own end, this neighbour) */
                    uint64_t lo = goff[own], hi = goff[own + 1];
                    const uint64_t want = own << 32 | (mv >> 32);
                    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (gkey[mid] < want) lo = mid + 1; else hi = mid; }
                    if (lo >= goff[own + 1] || gkey[lo] != want) { rc = -1; break; }   /* the link stage and this loop disagree */
                    t.val[k] = gval[lo];
                }
            }
            for (k = 0; k != t.slots && !rc; ++k) {
                uint64_t v;
                if (!t.taken[k] || (v = t.val[k]) >> 40 < 1) continue;
                if (v >= p->dist[a]) { p->dist2[a] = p->dist[a]; p->nei2[a] = p->nei[a]; p->dist[a] = v; p->nei[a] = (int64_t)t.key[k]; }
                else if (v >= p->dist2[a]) { p->dist2[a] = v; p->nei2[a] = (int64_t)t.key[k]; }
            }
        }
    }
    tab_drop(&t); free(goff);
    for (i = 0; i < s->n; ++i)                          /* sums become averages */
        for (a = 0; a < 2; ++a) { s->u[i].dist[a] = to_avg(s->u[i].dist[a]); s->u[i].dist2[a] = to_avg(s->u[i].dist2[a]); }
    return rc;
}

/* ---- a unitig that sits between two others which are also linked to each other (resolve_contained, scaf.c:256-284) ---- */
void fmdh_scaf_resolve_contained(fmdh_scaf_t *s, uint32_t id, double avg, double std, int pr_link, FILE *err)
{
    fmdh_scaf_utig_t *p = &s->u[id], *q[2];
    int d_long, d_short, a, e0, e1;
    if (p->excluded || p->nei[0] < 0 || p->nei[1] < 0 || p->nei2[0] >= 0 || p->nei2[1] >= 0) return;
    q[0] = &s->u[p->nei[0] >> 1]; q[1] = &s->u[p->nei[1] >> 1];
    e0 = (int)(p->nei[0] & 1); e1 = (int)(p->nei[1] & 1);
    if (q[0]->nei2[e0] < 0 || q[1]->nei2[e1] < 0) return;
    if (q[1]->nei[e1] != p->nei[0] && q[1]->nei2[e1] != p->nei[0]) return;
    if (q[0]->nei[e0] == p->nei[1]) d_long = (int)(avg - LOW40(q[0]->dist[e0]) + .499);
    else if (q[0]->nei2[e0] == p->nei[1]) d_long = (int)(avg - LOW40(q[0]->dist2[e0]) + .499);
    else return;
    d_short = (int)(2 * avg - LOW40(p->dist[0]) - LOW40(p->dist[1]) + p->len + .499);
    if (abs(d_long - d_short) < std && pr_link) {       /* (the reference breaks the outer link only when it prints: scaf.c:271) */
        fprintf(err, "CT\t%ld:%ld\t%d\t%d\n", (long)p->k[0], (long)p->k[1], d_long, d_short);
        for (a = 0; a < 2; ++a) {
            const int e = (int)(p->nei[a] & 1);
            if (q[a]->nei[e] == p->nei[a ^ 1]) { q[a]->nei[e] = q[a]->nei2[e]; q[a]->dist[e] = q[a]->dist2[e]; }
            q[a]->nei2[e] = -4; q[a]->dist2[e] = 0;
        }
    }
}

/* ---- gaps ---- */
int fmdh_scaf_candidate(const fmdh_scaf_t *s, uint32_t iddp, int min_supp, uint32_t *iddq_out)
{
    const fmdh_scaf_utig_t *p = &s->u[iddp >> 1], *q;
    const int a = (int)(iddp & 1);
    uint32_t iddq;
    int b, dist1, dist2 = 0;
    if (p->nei[a] < 0 || (int64_t)(p->dist[a] >> 40) < min_supp) return 0;
    iddq = (uint32_t)p->nei[a];
    if (iddp >= iddq) return 0;                         /* each link once */
    q = &s->u[iddq >> 1]; b = (int)(iddq & 1);
    if (q->nei[b] != (int64_t)iddp) return 0;           /* not each other's best */
    dist1 = (int)(p->dist[a] >> 40);
    if (p->nei2[a] >= 0) dist2 = (int)(p->dist2[a] >> 40);
    if (q->nei2[b] >= 0 && dist2 < (int)(q->dist2[b] >> 40)) dist2 = (int)(q->dist2[b] >> 40);
    if (dist2 >= min_supp || (double)dist2 / dist1 >= 1. / min_supp) return 0;
    *iddq_out = iddq;
    return 1;
}

int fmdh_scaf_keeps(const fmdh_scaf_t *s, uint64_t j, uint32_t idd, int64_t idd_mate)
{
    if (s->self[j] == NONE64 || s->self[j] >> 32 != idd) return 0;
    if (idd_mate >= 0 && (s->mate[j] == NONE64 || (int64_t)(s->mate[j] >> 32) != idd_mate)) return 0;
    return 1;
}

static void revcomp6(int l, uint8_t *s)
{
    int i;
    for (i = 0; i < l >> 1; ++i) {
        const uint8_t x = s[i], y = s[l - 1 - i];
        s[i] = y >= 1 && y <= 4 ? 5 - y : y; s[l - 1 - i] = x >= 1 && x <= 4 ? 5 - x : x;
    }
    if (l & 1) s[i] = s[i] >= 1 && s[i] <= 4 ? 5 - s[i] : s[i];
}

void fmdh_scaf_end_seq(const fmdh_scaf_utig_t *p, int is3, int is_2nd, int max_dist, uint8_t *dst, int *l)
{
    const int n = p->len > max_dist ? max_dist : p->len;
    memcpy(dst, p->len > max_dist && is3 ? p->seq + (p->len - max_dist) : p->seq, (size_t)n);
    if ((!is3) ^ (!!is_2nd)) revcomp6(n, dst);
    dst[n] = 0;
    *l = n;
}

fmdh_scaf_ext_t fmdh_scaf_gap_from_graph(fmdh_mag_t *g, int max_len, const char *t0, const char *t1)
{
    fmdh_scaf_ext_t e;
    const int tip = (int)(max_len * 1.1);
    size_t j;
    int best = 0;
    int64_t at = -1;
    memset(&e, 0, sizeof(e));
    if (!g) return e;
    fmdh_mag_merge(g, 1);
    fmdh_mag_rm_vext(g, tip, 4);
    fmdh_mag_simplify_bubble(g, 25, max_len * 2);
    fmdh_mag_pop_simple(g, 10.f, 0.15f, 1);
    fmdh_mag_rm_edge(g, 0, 0.8, tip, 5);
    fmdh_mag_merge(g, 1);
    fmdh_mag_rm_vext(g, tip, 100);
    fmdh_mag_merge(g, 0);
    fmdh_mag_simplify_bubble(g, 25, max_len * 2);
    fmdh_mag_pop_simple(g, 10.f, 0.15f, 1);
    if (g->err) return e;
    for (j = 0; j < g->n; ++j) if (g->v[j].len > best) { best = g->v[j].len; at = (int64_t)j; }
    if (at >= 0) {                                     /* both ends in the longest vertex, the second after the first: the gap is what lies between */
        fmdh_magv_t *p = &g->v[at];
        char *q = strstr(p->seq, t0), *r;
        if (!q) { revcomp6(p->len, (uint8_t *)p->seq); q = strstr(p->seq, t0); }
        if (q && (r = strstr(p->seq, t1)) > q) {
            const int l0 = (int)strlen(t0);
            e.patched = 1;
            e.l = (int)(r - (q + l0));
            if (e.l > 0 && (e.s = (char *)calloc(1, (size_t)e.l + 1))) strncpy(e.s, p->seq + l0, (size_t)e.l);   /* from the vertex's start + |t0|, wherever t0 was found (scaf.c:447) */
        }
    }
    return e;
}

int fmdh_scaf_compute_t(fmdh_scaf_t *s, uint32_t idd, int l, double mu, double sigma, int max_len, double *t)
{
    const fmdh_scaf_utig_t *p = &s->u[idd >> 1];
    int64_t sum = 0, sum2 = 0;
    uint64_t j;
    int n = 0;
    *t = 0.0;
    if (p->nei[idd & 1] < 0) return 0;
    for (j = p->first; j < p->first + p->n_reads; ++j) {
        int dist;
        if (s->self[j] == NONE64 || s->mate[j] == NONE64 || (int64_t)(s->mate[j] >> 32) != p->nei[idd & 1]) continue;
        dist = (int)(uint32_t)s->self[j] + (int)(uint32_t)s->mate[j] + l;
        ++n; sum += dist; sum2 += (int64_t)(int)((uint32_t)dist * (uint32_t)dist);
    }
    if (n < 2) { s->err = 1; return -1; }
    *t = fmdh_scaf_pvalue(n, sum, sum2, fmdh_scaf_correct_mean(2 * max_len + l, mu, sigma));
    return 0;
}

int fmdh_scaf_accept(fmdh_scaf_t *s, uint32_t iddp, uint32_t iddq, int round, fmdh_scaf_ext_t *ext, double avg, double std, int max_len)
{
    fmdh_scaf_utig_t *p = &s->u[iddp >> 1], *q = &s->u[iddq >> 1];
    if (ext->patched && ext->l + p->len > 0 && ext->l + q->len > 0) {
        if (fmdh_scaf_compute_t(s, iddp, ext->l, avg, std, max_len, &ext->t)) return 1;
        if ((round == 0 && ext->t > 1e-5) || (round == 1 && ext->t > 1e-10)) {
            p->ext[iddp & 1] = q->ext[iddq & 1] = *ext;
            return round == 0 ? 3 : 2;                 /* bit 1: the link keeps ext->s */
        }
    }
    return 0;
}

#define MAX_DROP 7
#define SCORE_THRES 13
void fmdh_scaf_fallback(fmdh_scaf_t *s, uint32_t iddp, uint32_t iddq, const fmdh_scaf_ext_t *last, const char *t0, int pl, const char *t1, int ql, double avg,
                        double std, int max_len, FILE *err)
{
    fmdh_scaf_utig_t *p = &s->u[iddp >> 1], *q = &s->u[iddq >> 1];
    const int a = (int)(iddp & 1), b = (int)(iddq & 1);
    fmdh_swaln_t r;
    int drop[2], max_drop, min_drop;
    if (last->patched != 0 || !((double)LOW40(p->dist[a]) > avg)) return;   /* ends that may overlap: the links say they lie closer than a read pair spans */
    if (fmdh_sw_align(ql - 1, (const uint8_t *)t1, pl - 1, (const uint8_t *)t0, &r)) { s->err = 2; return; }
    drop[0] = r.qb; drop[1] = (pl - 1) - (r.te + 1);
    max_drop = drop[0] > drop[1] ? drop[0] : drop[1];
    min_drop = drop[0] < drop[1] ? drop[0] : drop[1];
    if (min_drop == 0 && max_drop < MAX_DROP && r.score >= SCORE_THRES + max_drop) {   /* end to end */
        const int lp = r.te + 1 - r.tb + drop[0] + drop[1], lq = r.qe + 1 + drop[0] + drop[1];
        if (lp < p->len && lq < q->len) {
            double t;
            p->ext[a].l = -lp; q->ext[b].l = -lq;
            p->ext[a].patched = q->ext[b].patched = 1;
            if (fmdh_scaf_compute_t(s, iddp, p->ext[a].l, avg, std, max_len, &t)) return;
            p->ext[a].t = q->ext[b].t = t;
        }
    }
    if (!p->ext[a].patched) fprintf(err, "SW\t%ld\t%ld\t%d\t%d\t%d\n", (long)p->k[a], (long)q->k[b], drop[0], drop[1], r.score);
}

void fmdh_scaf_print_links(const fmdh_scaf_t *s, FILE *err)
{
    uint64_t idd;
    for (idd = 0; idd < 2 * s->n; ++idd) {
        const int a = (int)(idd & 1);
        const fmdh_scaf_utig_t *p = &s->u[idd >> 1], *q;
        fprintf(err, "LK\t%u:%d\t%ld\t%d\t%d\t%.2f", (unsigned)(idd >> 1), a, (long)p->k[a], p->len, p->nsr, p->A);
        if (p->nei[a] >= 0) {
            q = &s->u[p->nei[a] >> 1];
            fprintf(err, "\t%ld\t%d:%d", (long)q->k[p->nei[a] & 1], (int)(p->dist[a] >> 40), (int)LOW40(p->dist[a]));
            fprintf(err, "\t%d:%d:%.1e", p->ext[a].patched, p->ext[a].l, p->ext[a].t);
        }
        if (p->nei2[a] >= 0) {
            q = &s->u[p->nei2[a] >> 1];
            fprintf(err, "\t%ld\t%d:%d", (long)q->k[p->nei2[a] & 1], (int)(p->dist2[a] >> 40), (int)LOW40(p->dist2[a]));
        }
        fputc('\n', err);
    }
}

/* ---- joining (find_path, make_scaftigs: scaf.c:528-603) ---- */
typedef struct { uint64_t *a; size_t n, m; } path_t;
static int path_push(path_t *p, uint64_t v)
{
    if (p->n == p->m) { const size_t m = p->m ? p->m << 1 : 16; uint64_t *na = (uint64_t *)realloc(p->a, m * 8); if (!na) return -1; p->a = na; p->m = m; }
    p->a[p->n++] = v;
    return 0;
}
static void extend(fmdh_scaf_t *s, path_t *path, double a_thres, double p_thres)
{
    while (path->n) {
        const uint32_t idd = (uint32_t)path->a[path->n - 1];
        const fmdh_scaf_utig_t *p = &s->u[idd >> 1];
        fmdh_scaf_utig_t *q;
        uint32_t iddq;
        if (p->nei[idd & 1] < 0 || p->ext[idd & 1].patched == 0 || p->ext[idd & 1].t < p_thres) break;
        iddq = (uint32_t)p->nei[idd & 1];
        q = &s->u[iddq >> 1];
        if (q->deleted || q->A < a_thres) break;
        if (path_push(path, iddq) || path_push(path, iddq ^ 1)) { s->err = 2; break; }
        q->deleted = 1;
    }
}

void fmdh_scaf_join(fmdh_scaf_t *s, double a_thres, double p_thres, FILE *out)
{
    path_t path = {0, 0, 0};
    char *ctg = 0;
    size_t m_ctg = 0, i, j;
    for (i = 0; i < s->n && s->err != 2; ++i) {
        fmdh_scaf_utig_t *p0 = &s->u[i], *beg, *end;
        int64_t l = 0;
        int nsr = 0;
        path.n = 0;
        if (p0->deleted) continue;
        if (path_push(&path, (uint64_t)i << 1) || path_push(&path, (uint64_t)i << 1 | 1)) { s->err = 2; break; }
        p0->deleted = 1;
        if (p0->A >= a_thres) {                        /* to the right, then -- the path turned round -- to the left */
            extend(s, &path, a_thres, p_thres);
            for (j = 0; j < path.n >> 1; ++j) { const uint64_t t = path.a[j]; path.a[j] = path.a[path.n - 1 - j]; path.a[path.n - 1 - j] = t; }
            extend(s, &path, a_thres, p_thres);
        }
        for (j = 0; j < path.n; j += 2) {
            const uint32_t idd = (uint32_t)path.a[j], ndir = (idd & 1) ^ 1;
            const fmdh_scaf_utig_t *p = &s->u[idd >> 1];
            const size_t need = (size_t)(l > 0 ? l : 0) + (size_t)p->len + (size_t)(p->ext[ndir].l > 0 ? p->ext[ndir].l : 0) + 2;
            if (need > m_ctg) { char *nc = (char *)realloc(ctg, need * 2); if (!nc) { s->err = 2; break; } ctg = nc; m_ctg = need * 2; }
            if (l < 0) l = 0;                          /* (an overlap longer than everything before it) */
            nsr += p->nsr;
            memcpy(ctg + l, p->seq, (size_t)p->len);
            if (idd & 1) revcomp6(p->len, (uint8_t *)ctg + l);
            l += p->len;
            if (j == path.n - 2) break;
            if (p->ext[ndir].l > 0 && p->ext[ndir].s) {
                memcpy(ctg + l, p->ext[ndir].s, (size_t)p->ext[ndir].l);
                if (path.a[j + 2] < path.a[j]) revcomp6(p->ext[ndir].l, (uint8_t *)ctg + l);
                l += p->ext[ndir].l;
            } else l += p->ext[ndir].l;                /* overlapping ends: the next unitig starts that far back */
        }
        if (s->err == 2) break;
        for (j = 0; (int64_t)j < l; ++j) ctg[j] = "$ACGTN"[(uint8_t)ctg[j] < 6 ? (uint8_t)ctg[j] : 5];
        ctg[l > 0 ? l : 0] = 0;
        beg = &s->u[path.a[0] >> 1]; end = &s->u[path.a[path.n - 1] >> 1];
        fprintf(out, ">%ld:%ld\t%ld\t%d\t%.2f\n", (long)beg->k[path.a[0] & 1], (long)end->k[path.a[path.n - 1] & 1], (long)(path.n / 2), nsr, path.n > 2 ? 100.0 : beg->A);
        fputs(ctg ? ctg : "", out); fputc('\n', out);
    }
    free(path.a); free(ctg);
}
