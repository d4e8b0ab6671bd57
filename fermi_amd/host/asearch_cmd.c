#define _GNU_SOURCE
/* asearch_cmd.c -- `fermi-amd asearch [-g GPU] [-d 1] [-b] [-m 1000] [-l] [-M 1000] [-r reads.rank] <reads.fmd> <query.fa>`: the patterns within -d
 * substitutions of every query that occur in the indexed reads (fmd_asearch_batch; only substitutions, no insertions or deletions), and with -l the
 * reads that hold each of them (fmd_locate_batch + fmdh_locate_hits, as `locate` does for an exact match).  The reference has no such command.  Per
 * query, in input order:
 *     SQ <tab> name <tab> length <tab> n_hits <tab> n_occ <tab> listed(1/0) <tab> h0,h1,..,hd     h_j = hits with j substitutions; listed = 0: more than -m hits, none listed
 *     AH <tab> n_sub <tab> pattern <tab> count <tab> pos:X>Y,..                                 by (n_sub, SA interval); pos 0-based, ascending; * = no substitution
 *     OC <tab> read <tab> +|- <tab> offset                                                      with -l, after each AH, as `locate` prints them (none above -M occurrences)
 *     //
 * Usage and unreadable-file errors return 1 before the device is looked for. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "fmd_host.h"

#define ASEARCH_BATCH 65536

int fmdh_asearch_pattern(const uint8_t *query, uint32_t len, const fmd_asearch_hit_t *hit, uint8_t *out)
{
    uint32_t prev = 0xffffffffu;
    if (!query || !hit || !out || hit->n_sub > FMD_ASEARCH_MAX_SUB) return 1;
    memcpy(out, query, len);
    for (uint32_t j = 0; j < FMD_ASEARCH_MAX_SUB; ++j) {
        const uint32_t v = hit->sub[j], pos = v >> 2;
        if (j >= hit->n_sub) { if (v != 0xffffu) return 1; continue; }
        if (v == 0xffffu || pos >= len || pos >= prev) return 1;
        out[pos] = (uint8_t)(1 + (v & 3));
        prev = pos;
    }
    return 0;
}

typedef struct {
    int max_sub, locate;
    uint32_t max_hits, max_occ;
    unsigned flags;
    const uint64_t *sorted;
    uint64_t n_seq;
} asearch_opt_t;

static int flush_batch(fmd_dev_t *d, const asearch_opt_t *o, size_t n, char **names, const uint8_t *bases, const uint64_t *off, FILE *out)
{
    const size_t cols = (size_t)o->max_sub + 1;
    uint64_t *strata = (uint64_t *)calloc(n * cols * 2, 8), n_hits = 0, n_runs = 0, n_oc = 0, k = 0, oc = 0, max_len = 1;
    fmd_asearch_hit_t *hits = 0;
    fmd_asearch_stat_t st;
    fmd_locate_run_t *runs = 0;
    fmd_locate_stat_t lst;
    fmdh_locate_hit_t *ocs = 0;
    uint8_t *pat = 0;
    int rc = 1;
    if (!strata) { fprintf(stderr, "[E::main_asearch] out of memory\n"); return 1; }
    const int e = fmd_asearch_batch(d, n, bases, off, o->max_sub, o->max_hits, o->flags, 0, &hits, &n_hits, strata, &st);
    if (e) { fprintf(stderr, "[E::main_asearch] %s\n", fmd_strerror(e)); goto done; }
    if (o->locate && n_hits) {
        uint64_t *beg = (uint64_t *)malloc(n_hits * 16), *cnt = beg ? beg + n_hits : 0;
        if (!beg) { fprintf(stderr, "[E::main_asearch] out of memory\n"); goto done; }
        for (uint64_t j = 0; j < n_hits; ++j) { beg[j] = hits[j].beg; cnt[j] = hits[j].cnt; }
        const int e2 = fmd_locate_batch(d, n_hits, beg, cnt, o->max_occ, 0, &runs, &n_runs, &lst);
        free(beg);
        if (e2) { fprintf(stderr, "[E::main_asearch] %s\n", fmd_strerror(e2)); goto done; }
        if (fmdh_locate_hits(runs, n_runs, o->sorted, o->n_seq, &ocs, &n_oc)) {
            fprintf(stderr, "[E::main_asearch] a sentinel rank beyond the index's %llu sequences, or out of memory\n", (unsigned long long)o->n_seq);
            goto done;
        }
    }
    for (size_t i = 0; i < n; ++i) if (off[i + 1] - off[i] > max_len) max_len = off[i + 1] - off[i];
    if (!(pat = (uint8_t *)malloc(max_len))) { fprintf(stderr, "[E::main_asearch] out of memory\n"); goto done; }
    for (size_t i = 0; i < n; ++i) {
        const uint64_t *w = strata + i * cols * 2;
        const uint32_t len = (uint32_t)(off[i + 1] - off[i]);
        uint64_t nh = 0, no = 0;
        for (size_t c = 0; c < cols; ++c) { nh += w[2 * c]; no += w[2 * c + 1]; }
        fprintf(out, "SQ\t%s\t%u\t%llu\t%llu\t%d\t", names[i], len, (unsigned long long)nh, (unsigned long long)no, nh <= o->max_hits);
        for (size_t c = 0; c < cols; ++c) fprintf(out, "%s%llu", c ? "," : "", (unsigned long long)w[2 * c]);
        fputc('\n', out);
        for (; k < n_hits && hits[k].query == i; ++k) {
            const fmd_asearch_hit_t *h = &hits[k];
            if (fmdh_asearch_pattern(bases + off[i], len, h, pat)) { fprintf(stderr, "[E::main_asearch] a hit of query %s with a substitution list that cannot be\n", names[i]); goto done; }
            fprintf(out, "AH\t%u\t", h->n_sub);
            for (uint32_t j = 0; j < len; ++j) fputc("$ACGTN"[pat[j] < 6 ? pat[j] : 5], out);
            fprintf(out, "\t%llu\t", (unsigned long long)h->cnt);
            if (h->n_sub == 0) fputc('*', out);
            for (int j = (int)h->n_sub - 1; j >= 0; --j) {          /* sub[] is by descending position */
                const uint32_t pos = h->sub[j] >> 2, q = bases[off[i] + pos];
                fprintf(out, "%u:%c>%c%s", pos, "$ACGTN"[q < 6 ? q : 5], "ACGT"[h->sub[j] & 3], j ? "," : "");
            }
            fputc('\n', out);
            for (; oc < n_oc && ocs[oc].query == k; ++oc)
                fprintf(out, "OC\t%llu\t%c\t%u\n", (unsigned long long)(ocs[oc].id >> 1), "+-"[ocs[oc].id & 1], ocs[oc].off);
        }
        fputs("//\n", out);
    }
    rc = 0;
done:
    free(pat); free(ocs); free(strata);
    fmd_host_free(runs); fmd_host_free(hits);
    return rc;
}

int fmdh_main_asearch(int argc, char *argv[])
{
    int c, device = 0, rc = 0, l, best = 0;
    long long max_hits = 1000, max_occ = 1000, max_sub = 1;
    const char *rank_fn = 0;
    fmd_dev_t *d = 0;
    uint64_t *sorted = 0, n_sorted = 0;
    fmd_info_t info;
    asearch_opt_t o;
    memset(&o, 0, sizeof(o));
    while ((c = getopt(argc, argv, "g:d:bm:lM:r:")) >= 0) {
        if (c == 'g') device = atoi(optarg);
        else if (c == 'd') max_sub = atoll(optarg);
        else if (c == 'b') best = 1;
        else if (c == 'm') max_hits = atoll(optarg);
        else if (c == 'l') o.locate = 1;
        else if (c == 'M') max_occ = atoll(optarg);
        else if (c == 'r') rank_fn = optarg;
    }
    if (optind + 2 > argc || max_sub < 0 || max_sub > FMD_ASEARCH_MAX_SUB || max_hits < 1 || max_occ < 1) {
        fprintf(stderr, "\nUsage:   fermi-amd asearch [-g GPU] [-d INT] [-b] [-m INT] [-l] [-M INT] [-r reads.rank] <reads.fmd> <query.fa>\n\n");
        fprintf(stderr, "Options: -d INT    substitutions allowed, 0 to %d (no insertions or deletions) [1]\n", FMD_ASEARCH_MAX_SUB);
        fprintf(stderr, "         -b        only the hits with the fewest substitutions of each query\n");
        fprintf(stderr, "         -m INT    list the hits of a query that has at most INT of them [1000]\n");
        fprintf(stderr, "         -l        locate every hit: the reads that hold it, strand and offset\n");
        fprintf(stderr, "         -M INT    with -l, list the occurrences of a hit that has at most INT of them [1000]\n");
        fprintf(stderr, "         -r FILE   with -l, the rank -> read map `seqsort` wrote for the index [computed]\n\n");
        fprintf(stderr, "Output:  SQ name length n_hits n_occ listed(1/0) h0,..,hd; AH n_sub pattern count pos:X>Y,.. per hit; OC read +|- offset per occurrence (-l); //\n\n");
        return 1;
    }
    if (max_hits > 0xffffffffll) max_hits = 0xffffffffll;
    if (max_occ > 0xffffffffll) max_occ = 0xffffffffll;
    {
        const char *fn[3] = { argv[optind], strcmp(argv[optind + 1], "-") == 0 ? 0 : argv[optind + 1], o.locate ? rank_fn : 0 };
        for (int j = 0; j < 3; ++j) {
            FILE *fp = fn[j] ? fopen(fn[j], "rb") : 0;
            if (fn[j] && !fp) { fprintf(stderr, "[E::main_asearch] fail to open file '%s'\n", fn[j]); return 1; }
            if (fp) fclose(fp);
        }
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_asearch] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    if (o.locate && rank_fn) {
        FILE *fp = fopen(rank_fn, "rb");
        long long bytes = -1;
        if (fp && fseek(fp, 0, SEEK_END) == 0) bytes = ftell(fp);
        if (fp && bytes >= 0 && bytes % 8 == 0 && (sorted = (uint64_t *)malloc(bytes ? (size_t)bytes : 8)) != 0) {
            rewind(fp);
            n_sorted = (uint64_t)bytes / 8;
            if (fread(sorted, 8, n_sorted, fp) != n_sorted) { free(sorted); sorted = 0; }
        }
        if (fp) fclose(fp);
        if (!sorted) { fprintf(stderr, "[E::main_asearch] cannot read the rank file '%s'\n", rank_fn); return 1; }
    } else if (o.locate && fmdh_seqsort(argv[optind], device, &sorted, &n_sorted)) return 1;
    rc = fmd_dev_open_file(device, argv[optind], &d);
    if (rc) { fprintf(stderr, "[E::main_asearch] cannot load `%s': %s\n", argv[optind], fmd_strerror(rc)); free(sorted); return 1; }
    fmd_dev_info(d, &info);
    if (o.locate && n_sorted != info.mcnt[1]) {
        fprintf(stderr, "[E::main_asearch] the rank file has %llu entries, the index %llu sequences\n", (unsigned long long)n_sorted, (unsigned long long)info.mcnt[1]);
        rc = 1;
    }
    o.max_sub = (int)max_sub; o.max_hits = (uint32_t)max_hits; o.max_occ = (uint32_t)max_occ; o.flags = best ? FMD_ASEARCH_BEST : 0;
    o.sorted = sorted; o.n_seq = info.mcnt[1];
    fmdh_seqio_t *io = rc ? 0 : fmdh_seq_open(argv[optind + 1]);
    if (!rc && !io) { fprintf(stderr, "[E::main_asearch] fail to open file '%s'\n", argv[optind + 1]); rc = 1; }
    if (rc == 0) {
        char **names = (char **)calloc(ASEARCH_BATCH, sizeof(char *));
        uint64_t *off = (uint64_t *)malloc((ASEARCH_BATCH + 1) * 8);
        size_t n = 0, cap = 1 << 20, tot = 0;
        uint8_t *bases = (uint8_t *)malloc(cap);
        if (!names || !off || !bases) { fprintf(stderr, "[E::main_asearch] out of memory\n"); rc = 1; }
        else off[0] = 0;
        while (rc == 0) {
            l = fmdh_seq_read(io);
            if (l < 0 || n == ASEARCH_BATCH) {
                if (n) rc = flush_batch(d, &o, n, names, bases, off, stdout);
                for (size_t i = 0; i < n; ++i) free(names[i]);
                n = 0; tot = 0;
                if (rc || l < 0) break;
            }
            if (tot + (size_t)l + 8 > cap) {
                while (tot + (size_t)l + 8 > cap) cap <<= 1;
                if ((bases = (uint8_t *)realloc(bases, cap)) == 0) { fprintf(stderr, "[E::main_asearch] out of memory\n"); rc = 1; break; }
            }
            const char *s = fmdh_seq_bases(io);
            for (int i = 0; i < l; ++i) bases[tot + i] = fmdh_nt6[(unsigned char)s[i]];
            names[n] = strdup(fmdh_seq_name(io));
            tot += (size_t)l; off[++n] = tot;
        }
        free(names); free(off); free(bases);
    }
    if (io) fmdh_seq_close(io);
    fmd_dev_close(d);
    free(sorted);
    return rc ? 1 : 0;
}
