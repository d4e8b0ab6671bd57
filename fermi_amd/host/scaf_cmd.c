#define _GNU_SOURCE
/* scaf_cmd.c -- `fermi scaf [-t INT] [-m INT] [-P] [-a FLOAT] [-p FLOAT] <in.fmd> <in.remapped.mag> <avg> <std>` (cmd.c:560-587 -> mag_scaf_core,
 * scaf.c:632-690): unitigs joined into scaftigs by the read pairs that `remap` left unpaired at their ends.
 *
 * The order of work and what runs where:
 *   read     the remapped MAG (scaf_core.c)                                                     host
 *   rdist    rdist, A of every unitig, the excluded ones                                        host
 *   paired   the link stage over all UR entries: fmd_scaf_links (csrc/fmd_scaf.hip)             GPU
 *            then the best two neighbours of every end and the contained unitigs                host
 *   patched  every reciprocal-best link with enough support: the mates of the reads at both ends are fetched for ALL candidate links in one
 *            fmd_retrieve_batch (the reference calls fm_retrieve read by read, scaf.c:363); per link and round one local assembly through the
 *            in-memory path (fmdh_api_unitig_mag: index construction and overlap discovery on the GPU), its cleaning, the search for both ends in
 *            the longest vertex, the P-value; for ends that may overlap, the alignment fallback                                   GPU + host
 *   joined   the scaftigs (scaf_core.c)                                                          host
 * GPU calls stay on this one thread (the library documents no thread safety).  -t spreads the host part of the links -- cleaning, the search
 * for the ends, the alignment, the statistics -- over host threads, round by round: all local assemblies of a round first, then their verdicts
 * in parallel.  Links touch disjoint unitig ends, so the result does not depend on -t; only the SW lines may come in another order, as with
 * the reference's -tN. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include "fmd_host.h"
#include "scaf.h"

static double now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

typedef struct { uint32_t iddp, iddq; uint64_t row0[2], n_rows[2]; } cand_t;   /* a link to patch; the rows of the batch that hold the mates at its two ends */

/* the mates' rows at end idd: x ^ 3 of every read kept there (the other strand of the other read of the pair) */
static int collect_rows(fmdh_scaf_t *s, uint32_t idd, uint64_t n_seq, uint64_t **rows, uint64_t *n, uint64_t *m)
{
    const fmdh_scaf_utig_t *p = &s->u[idd >> 1];
    uint64_t j;
    for (j = p->first; j < p->first + p->n_reads; ++j) {
        if (!fmdh_scaf_keeps(s, j, idd, -1)) continue;
        if ((s->x[j] ^ 3) >= n_seq) {
            fprintf(stderr, "[E::%s] read %llu of unitig %ld:%ld is not in the index (it holds %llu sequences)\n", __func__, (unsigned long long)(s->x[j] >> 1),
                    (long)p->k[0], (long)p->k[1], (unsigned long long)n_seq);
            s->err = 1;
            return -1;
        }
        if (*n == *m) { const uint64_t nm = *m ? *m << 1 : 1024; uint64_t *nr = (uint64_t *)realloc(*rows, nm * 8); if (!nr) return -1; *rows = nr; *m = nm; }
        (*rows)[(*n)++] = s->x[j] ^ 3;
    }
    return 0;
}

/* the mates of the reads kept at end idd (all of them, or those whose mate lies at idd_mate) appended to buf, a NUL after each; -> the longest */
static int add_mates(const fmdh_scaf_t *s, uint32_t idd, int64_t idd_mate, uint64_t row0, const uint8_t *seqs, uint32_t stride, const uint32_t *len, char *buf, size_t *l)
{
    const fmdh_scaf_utig_t *p = &s->u[idd >> 1];
    uint64_t j, r = row0;
    int max_len = 0;
    for (j = p->first; j < p->first + p->n_reads; ++j) {
        uint32_t i, n;
        if (!fmdh_scaf_keeps(s, j, idd, -1)) continue;
        n = len[r];
        if (fmdh_scaf_keeps(s, j, idd, idd_mate)) {
            const uint8_t *row = seqs + r * stride;
            if ((int)n > max_len) max_len = (int)n;
            for (i = 0; i < n; ++i) buf[(*l)++] = (char)row[n - 1 - i];      /* the rows arrive reversed, as fm_retrieve emits them */
            buf[(*l)++] = 0;
        }
        ++r;
    }
    return max_len;
}

/* a link on its way through the two rounds: what the GPU part leaves for the host part */
typedef struct {
    uint32_t iddp, iddq;
    char *buf;                            /* both ends, then the mates: a NUL after each (the ends stay for the fallback) */
    int pl, ql, max_len, stop, err;
    fmdh_mag_t *g;                        /* the local assembly of the current round */
    fmdh_scaf_ext_t last;                 /* the last round's gap */
} job_t;
typedef struct { fmdh_scaf_t *s; const fmdh_scafopt_t *opt; job_t *jobs; size_t n; int round; } host_work_t;

/* the host part of one round (0, 1) or the fallback (2) for the links k = tid, tid + nt, ...; links touch disjoint unitig ends */
static void host_round(void *ctx, int tid, int nt)
{
    host_work_t *w = (host_work_t *)ctx;
    size_t k;
    for (k = (size_t)tid; k < w->n; k += (size_t)nt) {
        job_t *jb = &w->jobs[k];
        fmdh_scaf_t one = *w->s;                       /* (its own error flag) */
        one.err = 0;
        if (jb->err) continue;
        if (w->round < 2) {
            int verdict;
            if (jb->stop) continue;
            jb->last = fmdh_scaf_gap_from_graph(jb->g, jb->max_len, jb->buf, jb->buf + jb->pl);
            if (jb->g) { fmdh_mag_destroy(jb->g); jb->g = 0; }
            verdict = fmdh_scaf_accept(&one, jb->iddp, jb->iddq, w->round, &jb->last, w->opt->avg, w->opt->std, jb->max_len);
            if (!(verdict & 2)) { free(jb->last.s); jb->last.s = 0; }
            if (verdict & 1) jb->stop = 1;
        } else fmdh_scaf_fallback(&one, jb->iddp, jb->iddq, &jb->last, jb->buf, jb->pl, jb->buf + jb->pl, jb->ql, w->opt->avg, w->opt->std, jb->max_len, stderr);
        jb->err = one.err;
    }
}

static int patch_all(fmdh_scaf_t *s, fmd_dev_t *dev, int device, const fmdh_scafopt_t *opt, int max_dist)
{
    fmd_info_t info;
    cand_t *c = 0;
    size_t n_c = 0, m_c = 0, k, buf_m = 0;
    uint64_t *rows = 0, n_rows = 0, m_rows = 0, i;
    uint8_t *seqs = 0, *end0 = 0, *end1 = 0;
    uint32_t *len = 0, stride = 256;
    uint64_t *rank = 0;
    char *work = 0;
    job_t *jobs = 0;
    host_work_t hw;
    const int nt = opt->n_threads < 1 ? 1 : opt->n_threads > 64 ? 64 : opt->n_threads;
    int rc = 1, a, round;
    if (fmd_dev_info(dev, &info)) return 1;
    for (i = 0; i < 2 * s->n; ++i) {
        uint32_t iddq;
        if (!fmdh_scaf_candidate(s, (uint32_t)i, opt->min_supp, &iddq)) continue;
        if (n_c == m_c) { const size_t nm = m_c ? m_c << 1 : 64; cand_t *nc = (cand_t *)realloc(c, nm * sizeof(*c)); if (!nc) goto done; c = nc; m_c = nm; }
        c[n_c].iddp = (uint32_t)i; c[n_c].iddq = iddq;
        for (a = 0; a < 2; ++a) {
            c[n_c].row0[a] = n_rows;
            if (collect_rows(s, a ? iddq : (uint32_t)i, info.mcnt[1], &rows, &n_rows, &m_rows)) goto done;
            c[n_c].n_rows[a] = n_rows - c[n_c].row0[a];
        }
        ++n_c;
    }
    if (n_c == 0) { rc = 0; goto done; }
    for (;;) {                                         /* one batch for all links; again with wider rows should a read be longer */
        uint32_t longest = 0;
        int e;
        seqs = (uint8_t *)malloc((size_t)(n_rows ? n_rows : 1) * stride);
        len = (uint32_t *)malloc((size_t)(n_rows ? n_rows : 1) * 4);
        rank = (uint64_t *)malloc((size_t)(n_rows ? n_rows : 1) * 8);
        if (!seqs || !len || !rank) goto done;
        if (n_rows && (e = fmd_retrieve_batch(dev, n_rows, rows, seqs, stride, len, rank)) != 0) { fprintf(stderr, "[E::%s] fmd_retrieve_batch: %s\n", __func__, fmd_strerror(e)); goto done; }
        for (i = 0; i < n_rows; ++i) if (len[i] > longest) longest = len[i];
        if (longest <= stride) break;
        free(seqs); free(len); free(rank); seqs = 0; len = 0; rank = 0;
        stride = (longest + 63) & ~63u;
    }
    end0 = (uint8_t *)malloc((size_t)max_dist + 2); end1 = (uint8_t *)malloc((size_t)max_dist + 2);
    jobs = (job_t *)calloc(n_c, sizeof(*jobs));
    if (!end0 || !end1 || !jobs) goto done;
    hw.s = s; hw.opt = opt; hw.jobs = jobs; hw.n = n_c;
    for (round = 0; round < 2; ++round) {              /* first the mates must land on the other end; then any mate counts */
        for (k = 0; k < n_c; ++k) {                    /* the local assemblies of this round, one after the other on this thread: they use the GPU */
            const uint32_t iddp = c[k].iddp, iddq = c[k].iddq;
            const fmdh_scaf_utig_t *p = &s->u[iddp >> 1], *q = &s->u[iddq >> 1];
            job_t *jb = &jobs[k];
            size_t need = 2 * ((size_t)max_dist + 2), l = 0;
            int arc;
            if (jb->stop) continue;
            jb->iddp = iddp; jb->iddq = iddq;
            fmdh_scaf_end_seq(p, (int)(iddp & 1), 0, max_dist, end0, &jb->pl); ++jb->pl;       /* (lengths with the NUL, as the reference counts them) */
            fmdh_scaf_end_seq(q, (int)(iddq & 1), 1, max_dist, end1, &jb->ql); ++jb->ql;
            for (a = 0; a < 2; ++a) for (i = 0; i < c[k].n_rows[a]; ++i) need += (size_t)len[c[k].row0[a] + i] + 1;
            if (!jb->buf && !(jb->buf = (char *)malloc(need))) goto done;
            if (need > buf_m) { char *nw = (char *)realloc(work, need); if (!nw) goto done; work = nw; buf_m = need; }
            memcpy(jb->buf, end0, (size_t)jb->pl); l += (size_t)jb->pl;
            memcpy(jb->buf + l, end1, (size_t)jb->ql); l += (size_t)jb->ql;
            jb->max_len = add_mates(s, iddp, round ? -1 : (int64_t)iddq, c[k].row0[0], seqs, stride, len, jb->buf, &l);
            add_mates(s, iddq, round ? -1 : (int64_t)iddp, c[k].row0[1], seqs, stride, len, jb->buf, &l);
            memcpy(work, jb->buf, l);                  /* (the in-memory path may rewrite its input) */
            jb->g = fmdh_api_unitig_mag(device, (int)(jb->max_len / 3. < 17 ? jb->max_len / 3. : 17), (int64_t)l, work, &arc);
            if (arc) { fprintf(stderr, "[E::%s] the local assembly of the link %ld -> %ld failed\n", __func__, (long)p->k[iddp & 1], (long)q->k[iddq & 1]); goto done; }
        }
        hw.round = round;
        fmdh_par_for(nt, host_round, &hw);             /* cleaning, the search for both ends, the P-value: host only, link by link */
        for (k = 0; k < n_c; ++k) if (jobs[k].err) { s->err = jobs[k].err; goto fail_t; }
    }
    hw.round = 2;
    fmdh_par_for(nt, host_round, &hw);                 /* the alignment fallback; with one thread the SW lines come in the reference's order */
    for (k = 0; k < n_c; ++k) if (jobs[k].err) { s->err = jobs[k].err; goto fail_t; }
    rc = 0;
    goto done;
fail_t:
    if (s->err == 1) fprintf(stderr, "[E::%s] a link with fewer than two read pairs behind it: the input is not what `remap` wrote for this index\n", __func__);
done:
    if (jobs) for (k = 0; k < n_c; ++k) { free(jobs[k].buf); if (jobs[k].g) fmdh_mag_destroy(jobs[k].g); }
    free(jobs); free(c); free(rows); free(seqs); free(len); free(rank); free(end0); free(end1); free(work);
    return rc;
}

int fmdh_main_scaf(int argc, char *argv[])
{
    fmdh_scafopt_t opt;
    fmdh_scaf_t *s = 0;
    fmd_dev_t *dev = 0;
    int c, device = 0, max_dist, rc = 1, e;
    double t;
    size_t i;
    opt.min_supp = 5; opt.pr_links = 0; opt.a_thres = 20.; opt.p_thres = 1e-20; opt.n_threads = 1;
    while ((c = getopt(argc, argv, "m:t:Pea:p:g:")) >= 0) {
        switch (c) {
        case 't': opt.n_threads = atoi(optarg); break;
        case 'm': opt.min_supp = atoi(optarg); break;
        case 'P': opt.pr_links = 1; break;
        case 'a': opt.a_thres = atof(optarg); break;
        case 'p': opt.p_thres = atof(optarg); break;
        case 'g': device = atoi(optarg); break;
        }
    }
    if (optind + 4 > argc) {
        fprintf(stderr, "\nUsage:   fermi-amd scaf [options] <in.fmd> <in.remapped.mag> <avg> <std>\n\n");
        fprintf(stderr, "Options: -t INT     number of host threads; the GPU calls stay on one [1]\n");
        fprintf(stderr, "         -m INT     minimum number of supporting reads [%d]\n", opt.min_supp);
        fprintf(stderr, "         -a FLOAT   minimum A of a unitig that is joined [%g]\n", opt.a_thres);
        fprintf(stderr, "         -p FLOAT   minimum P-value of a gap that is joined [%g]\n", opt.p_thres);
        fprintf(stderr, "         -P         print the links between unitigs\n");
        fprintf(stderr, "         -g INT     GPU to use [0]\n\n");
        return 1;
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::%s] %s\n", __func__, fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::%s] GPU %d: this node has %d\n", __func__, device, fmd_device_count()); return 1; }
    opt.avg = atof(argv[optind + 2]); opt.std = atof(argv[optind + 3]);
    max_dist = (int)(opt.avg + 2. * opt.std + .499);
    if (max_dist < 0) max_dist = 0;
    if ((e = fmd_dev_open_file(device, argv[optind], &dev)) != 0) { fprintf(stderr, "[E::%s] cannot load `%s': %s\n", __func__, argv[optind], fmd_strerror(e)); return 1; }
    t = now();
    if (!(s = fmdh_scaf_read(argv[optind + 1]))) { fprintf(stderr, "[E::%s] cannot read `%s'\n", __func__, argv[optind + 1]); goto done; }
    fprintf(stderr, "[M::%s] read %zu unitigs in %.3f sec\n", __func__, s->n, now() - t);
    t = now();
    fmdh_scaf_cal_rdist(s);
    fmdh_scaf_exclude(s, opt.a_thres);
    fprintf(stderr, "[M::%s] rdist = %.3f, computed in %.3f sec\n", __func__, s->rdist, now() - t);
    t = now();
    {
        const uint64_t n = s->n_ent;
        int32_t *len = (int32_t *)malloc((s->n ? s->n : 1) * 4);
        uint8_t *exc = (uint8_t *)malloc(s->n ? s->n : 1);
        uint64_t *gkey = (uint64_t *)malloc((n ? n : 1) * 8), *gval = (uint64_t *)malloc((n ? n : 1) * 8), n_groups = 0;
        uint32_t *n_nei = (uint32_t *)calloc(2 * s->n + 1, 4);
        s->self = (uint64_t *)malloc((n ? n : 1) * 8); s->mate = (uint64_t *)malloc((n ? n : 1) * 8);
        e = len && exc && gkey && gval && n_nei && s->self && s->mate ? 0 : FMD_E_NOMEM;
        for (i = 0; !e && i < s->n; ++i) { len[i] = s->u[i].len; exc[i] = s->u[i].excluded; }
        if (!e) e = fmd_scaf_links(device, n, s->x, s->span, s->utig, s->n, len, exc, max_dist, s->self, s->mate, gkey, gval, n_nei, &n_groups);
        if (e) fprintf(stderr, "[E::%s] the link stage failed: %s\n", __func__, fmd_strerror(e));
        else if ((e = fmdh_scaf_choose(s, n_groups, gkey, gval, n_nei)) != 0) fprintf(stderr, "[E::%s] the links do not match the unitigs' read lists\n", __func__);
        free(len); free(exc); free(gkey); free(gval); free(n_nei);
        if (e) goto done;
        fprintf(stderr, "[M::%s] paired unitigs in %.3f sec (%llu entries, %llu links between ends)\n", __func__, now() - t, (unsigned long long)n, (unsigned long long)n_groups);
    }
    for (i = 0; i < s->n; ++i) fmdh_scaf_resolve_contained(s, (uint32_t)i, opt.avg, opt.std, opt.pr_links, stderr);
    t = now();
    if (patch_all(s, dev, device, &opt, max_dist)) goto done;
    fprintf(stderr, "[M::%s] patched gaps in %.3f sec\n", __func__, now() - t);
    if (opt.pr_links) fmdh_scaf_print_links(s, stderr);
    fmdh_scaf_join(s, opt.a_thres, opt.p_thres, stdout);
    rc = s->err ? 1 : 0;
done:
    if (s) fmdh_scaf_free(s);
    fmd_dev_close(dev);
    return rc;
}
