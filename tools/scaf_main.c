/* scaf_main.c -- the host side of `scaf` alone, without the GPU library: what `make asan-scaf` builds with -fsanitize=address,undefined to run
 * the reader, the statistics, the alignment, the choice of links with its table replay and the joiner (host/scaf_core.c, scaf_stat.c and the
 * reader they use) over the fixtures and over truncated and malformed MAGs.  The link stage, which the command runs on the GPU, is restated
 * here with two sorts on the host.  The local assemblies need the device; in their place the program takes the gaps the reference found
 * (tests/golden/scafN.ext.tsv: lower end, upper end, patched, l, t, inserted bases), sets every filled gap with its P-value computed here,
 * and sends every other candidate link through the alignment fallback.  With that file its stdout is the FASTA of `fermi scaf` and its LK / CT /
 * SW lines are the reference's; without it only overlapping ends are joined.
 *   scaf_main <in.remapped.mag> <avg> <std> [a_thres [gaps.tsv]]      LK / CT / SW lines on stderr, scaftigs on stdout
 *   scaf_main --sw <query> <target>                        the alignment of two ACGT strings: score te qe tb qb
 *   scaf_main --stat <n> <t>                               the incomplete beta function behind a P-value */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fmd_host.h"
#include "scaf.h"

static const uint64_t *g_key;
static int by_key(const void *a, const void *b)
{
    const uint64_t x = g_key[*(const uint64_t *)a], y = g_key[*(const uint64_t *)b];
    return x < y ? -1 : x > y ? 1 : *(const uint64_t *)a < *(const uint64_t *)b ? -1 : 1;
}
static int by_u64(const void *a, const void *b) { const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b; return x < y ? -1 : x > y; }

static uint64_t lookup(uint64_t nd, const uint64_t *dk, const uint64_t *dv, uint64_t r)
{
    uint64_t lo = 0, hi = nd;
    while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (dk[mid] < r) lo = mid + 1; else hi = mid; }
    return lo < nd && dk[lo] == r ? dv[lo] : ~0ull;
}

/* fmd_scaf_links (include/fmd_hip.h) on the host */
static int links_host(fmdh_scaf_t *s, int max_dist, uint64_t **gkey, uint64_t **gval, uint32_t **n_nei, uint64_t *n_groups)
{
    const uint64_t n = s->n_ent;
    uint64_t *key = (uint64_t *)malloc((n + 1) * 8), *val = (uint64_t *)malloc((n + 1) * 8), *ord = (uint64_t *)malloc((n + 1) * 8), *dk = (uint64_t *)malloc((n + 1) * 8),
             *dv = (uint64_t *)malloc((n + 1) * 8), *lk = (uint64_t *)malloc((n + 1) * 16), nd = 0, nl = 0, i, ng = 0;
    *gkey = (uint64_t *)malloc((n + 1) * 8); *gval = (uint64_t *)malloc((n + 1) * 8); *n_nei = (uint32_t *)calloc(2 * s->n + 1, 4);
    s->self = (uint64_t *)malloc((n + 1) * 8); s->mate = (uint64_t *)malloc((n + 1) * 8);
    if (!key || !val || !ord || !dk || !dv || !lk || !*gkey || !*gval || !*n_nei || !s->self || !s->mate) return -1;
    for (i = 0; i < n; ++i) {
        const uint64_t x = s->x[i], u = s->utig[i];
        const int32_t dist = (x & 1) ? (int32_t)(uint32_t)s->span[i] : s->u[u].len - (int32_t)(uint32_t)(s->span[i] >> 32);
        key[i] = ~0ull; val[i] = 0; ord[i] = i;
        if (!s->u[u].excluded && dist <= max_dist) { key[i] = x >> 1; val[i] = (u << 1 | ((x & 1) ^ 1)) << 32 | (uint32_t)dist; }
    }
    g_key = key;
    qsort(ord, n, 8, by_key);
    for (i = 0; i < n; ++i) {
        const uint64_t k = key[ord[i]];
        if (k != ~0ull && (i == 0 || key[ord[i - 1]] != k) && (i + 1 == n || key[ord[i + 1]] != k) && val[ord[i]] != 0) { dk[nd] = k; dv[nd++] = val[ord[i]]; }
    }
    for (i = 0; i < n; ++i) {
        const uint64_t r = s->x[i] >> 1, u = s->utig[i], sv = lookup(nd, dk, dv, r), mv = lookup(nd, dk, dv, r ^ 1);
        s->self[i] = sv; s->mate[i] = mv;
        if (sv != ~0ull && mv != ~0ull && (mv >> 33) != u) {
            lk[2 * nl] = (u << 1 | ((sv >> 32) & 1)) << 32 | (mv >> 32);
            lk[2 * nl + 1] = (1ull << 40 | (uint64_t)(uint32_t)sv) + (uint64_t)(uint32_t)mv;
            ++nl;
        }
    }
    qsort(lk, nl, 16, by_u64);
    for (i = 0; i < nl; ++i) {
        if (i == 0 || lk[2 * i] != lk[2 * i - 2]) { (*gkey)[ng] = lk[2 * i]; (*gval)[ng] = 0; ++(*n_nei)[lk[2 * i] >> 32]; ++ng; }
        (*gval)[ng - 1] += lk[2 * i + 1];
    }
    *n_groups = ng;
    free(key); free(val); free(ord); free(dk); free(dv); free(lk);
    return 0;
}

/* the recorded gaps: rec[idd of the lower end] */
typedef struct { int have, l; char *s; } gap_t;
static gap_t *load_gaps(const char *fn, size_t n_ends, int *max_len)
{
    gap_t *g = (gap_t *)calloc(n_ends + 1, sizeof(*g));
    char *line = 0;
    size_t m = 0;
    FILE *f = fn ? fopen(fn, "r") : 0;
    *max_len = 0;
    if (!g || !f) return g;
    while (getline(&line, &m, f) > 0) {
        unsigned long p, q;
        int patched, l, used = 0;
        if (sscanf(line, "max_len %d", max_len) == 1) continue;
        if (sscanf(line, "%lu %lu %d %d %*s %n", &p, &q, &patched, &l, &used) < 4 || p >= n_ends || !used) continue;
        g[p].have = 1; g[p].l = l;
        if (l > 0) { char *e; g[p].s = strdup(line + used); if (g[p].s && (e = strpbrk(g[p].s, "\r\n"))) *e = 0; }
    }
    free(line); fclose(f);
    return g;
}

/* what the command does per candidate link, with the recorded gap in the place of the two local assemblies */
static void patch_from_record(fmdh_scaf_t *s, const gap_t *gap, int max_len, int max_dist, double avg, double std)
{
    uint8_t *e0 = (uint8_t *)malloc((size_t)max_dist + 2), *e1 = (uint8_t *)malloc((size_t)max_dist + 2);
    size_t i;
    for (i = 0; e0 && e1 && i < 2 * s->n && !s->err; ++i) {
        uint32_t iddq;
        fmdh_scaf_utig_t *p = &s->u[i >> 1], *q;
        fmdh_scaf_ext_t ext;
        int pl, ql;
        if (!fmdh_scaf_candidate(s, (uint32_t)i, 5, &iddq)) continue;
        q = &s->u[iddq >> 1];
        memset(&ext, 0, sizeof(ext));
        fmdh_scaf_end_seq(p, (int)(i & 1), 0, max_dist, e0, &pl);
        fmdh_scaf_end_seq(q, (int)(iddq & 1), 1, max_dist, e1, &ql);
        if (gap[i].have && gap[i].l > 0 && gap[i].s && (int)strlen(gap[i].s) == gap[i].l) {      /* a filled gap: nt6 codes, shared by both ends */
            int j;
            ext.patched = 1; ext.l = gap[i].l;
            if (!(ext.s = (char *)calloc(1, (size_t)ext.l + 1))) break;
            for (j = 0; j < ext.l; ++j) ext.s[j] = (char)fmdh_nt6[(unsigned char)gap[i].s[j]];
            {   /* the same gap once more the command's way: a local assembly of ONE vertex -- first end, gap, second end -- through the search for the
                 * ends and the verdict of the two rounds; it must find what was recorded */
                const size_t n = (size_t)pl + (size_t)ext.l + (size_t)ql;
                char *rec = (char *)malloc(2 * n + 64);
                fmdh_magopt_t mo;
                fmdh_mag_t *g = 0;
                fmdh_scaf_ext_t found;
                size_t at;
                int verdict = 0, round;
                if (!rec) { free(ext.s); break; }
                at = (size_t)sprintf(rec, "@1:2\t2\t.\t.\n");
                for (j = 0; j < pl; ++j) rec[at++] = "$ACGTN"[e0[j] < 6 ? e0[j] : 5];
                memcpy(rec + at, gap[i].s, (size_t)ext.l); at += (size_t)ext.l;
                for (j = 0; j < ql; ++j) rec[at++] = "$ACGTN"[e1[j] < 6 ? e1[j] : 5];
                at += (size_t)sprintf(rec + at, "\n+\n");
                memset(rec + at, '5', n); at += n; rec[at++] = '\n';
                fmdh_mag_init_opt(&mo);
                mo.flag = FMDH_MAG_F_READ_ORI | FMDH_MAG_F_NO_AMEND;
                g = fmdh_mag_read_mem(rec, at, &mo);
                free(rec);
                found = fmdh_scaf_gap_from_graph(g, max_len, (const char *)e0, (const char *)e1);
                if (g) fmdh_mag_destroy(g);
                if (!found.patched || found.l != ext.l || !found.s || memcmp(found.s, ext.s, (size_t)ext.l)) {
                    fprintf(stderr, "[E::%s] the gap of the link at end %zu was not found again in its own assembly\n", __func__, i);
                    free(found.s); free(ext.s); s->err = 2; break;
                }
                free(ext.s); ext = found;
                for (round = 0; round < 2 && !(verdict & 2) && !s->err; ++round) verdict = fmdh_scaf_accept(s, (uint32_t)i, iddq, round, &ext, avg, std, max_len);
                if (!(verdict & 2)) free(ext.s);       /* (a P-value below both rounds' thresholds: the link stays open, as in the command) */
            }
        } else if (gap[i].have && gap[i].l <= 0) {      /* ends that overlap: found by the fallback -- or, where that finds something else, by the assembly, with one l for both ends */
            char *text = 0;
            size_t n_text = 0;
            FILE *quiet = open_memstream(&text, &n_text);
            if (!quiet) break;
            fmdh_scaf_fallback(s, (uint32_t)i, iddq, &ext, (const char *)e0, pl + 1, (const char *)e1, ql + 1, avg, std, max_len, quiet);
            fclose(quiet); free(text);
            if (!p->ext[i & 1].patched || p->ext[i & 1].l != gap[i].l) {
                ext.patched = 1; ext.l = gap[i].l;
                if (fmdh_scaf_compute_t(s, (uint32_t)i, ext.l, avg, std, max_len, &ext.t)) break;
                p->ext[i & 1] = q->ext[iddq & 1] = ext;
            }
        } else fmdh_scaf_fallback(s, (uint32_t)i, iddq, &ext, (const char *)e0, pl + 1, (const char *)e1, ql + 1, avg, std, max_len, stderr);
    }
    free(e0); free(e1);
}

int main(int argc, char *argv[])
{
    if (argc == 4 && strcmp(argv[1], "--sw") == 0) {
        fmdh_swaln_t r;
        uint8_t *q = (uint8_t *)strdup(argv[2]), *t = (uint8_t *)strdup(argv[3]);
        size_t i, ql = strlen(argv[2]), tl = strlen(argv[3]);
        for (i = 0; i < ql; ++i) q[i] = fmdh_nt6[q[i]];
        for (i = 0; i < tl; ++i) t[i] = fmdh_nt6[t[i]];
        if (fmdh_sw_align((int)ql, q, (int)tl, t, &r)) return 1;
        printf("%d %d %d %d %d\n", r.score, r.te, r.qe, r.tb, r.qb);
        free(q); free(t);
        return 0;
    }
    if (argc == 4 && strcmp(argv[1], "--stat") == 0) {
        const double n = atof(argv[2]), t = atof(argv[3]);
        printf("%a\n", fmdh_kf_betai(.5 * n, .5, n / (n + t * t)));
        return 0;
    }
    if (argc < 4) { fprintf(stderr, "Usage: scaf_main <in.remapped.mag> <avg> <std> [a_thres [gaps.tsv]] | --sw <query> <target> | --stat <n> <t>\n"); return 1; }
    {
        const double avg = atof(argv[2]), std = atof(argv[3]), a_thres = argc > 4 ? atof(argv[4]) : 20.;
        const int max_dist = (int)(avg + 2. * std + .499);
        fmdh_scaf_t *s = fmdh_scaf_read(argv[1]);
        uint64_t *gkey = 0, *gval = 0, n_groups = 0;
        uint32_t *n_nei = 0;
        size_t i;
        int rc = 1;
        if (!s) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
        fmdh_scaf_cal_rdist(s);
        fmdh_scaf_exclude(s, a_thres);
        fprintf(stderr, "rdist\t%.3f\n", s->rdist);
        if (links_host(s, max_dist, &gkey, &gval, &n_nei, &n_groups) == 0 && fmdh_scaf_choose(s, n_groups, gkey, gval, n_nei) == 0) {
            int max_len = 0;
            gap_t *gap = load_gaps(argc > 5 ? argv[5] : 0, 2 * s->n, &max_len);
            for (i = 0; i < s->n; ++i) fmdh_scaf_resolve_contained(s, (uint32_t)i, avg, std, 1, stderr);
            if (gap) patch_from_record(s, gap, max_len, max_dist > 0 ? max_dist : 0, avg, std);
            for (i = 0; gap && i < 2 * s->n; ++i) free(gap[i].s);
            free(gap);
            fmdh_scaf_print_links(s, stderr);
            fmdh_scaf_join(s, a_thres, 1e-20, stdout);
            rc = s->err ? 1 : 0;
        }
        free(gkey); free(gval); free(n_nei);
        fmdh_scaf_free(s);
        return rc;
    }
}
