#define _GNU_SOURCE
/* locate_cmd.c -- `fermi-amd locate [-g GPU] [-m INT] [-r reads.rank] <reads.fmd> <query.fa>`: which reads hold every query, on which strand and at
 * which offset.  Backward search (fmd_bsearch_batch) gives the query's SA interval; fmd_locate_batch walks its rows to their sentinels -- runs of sentinel
 * ranks at one offset -- and fmdh_locate_hits turns the runs into hits through the rank -> read map `seqsort` writes (-r; computed here the way seqsort
 * does when the option is absent).  The reference has no such command: its index keeps no suffix-array samples.  Per query, in input order:
 *     SQ <tab> name <tab> length <tab> count <tab> located(1/0)       located = 0: more than -m occurrences, none listed
 *     OC <tab> read <tab> +|- <tab> offset                           read = id >> 1, strand = id & 1; offset 0-based in the strand's sequence as indexed
 *     //
 * Usage and unreadable-file errors return 1 before the device is looked for. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "fmd_host.h"

#define LOCATE_BATCH 262144

static int hit_cmp(const void *pa, const void *pb)
{
    const fmdh_locate_hit_t *a = (const fmdh_locate_hit_t *)pa, *b = (const fmdh_locate_hit_t *)pb;
    if (a->query != b->query) return a->query < b->query ? -1 : 1;
    if (a->id != b->id) return a->id < b->id ? -1 : 1;
    return a->off < b->off ? -1 : a->off > b->off;
}

/* runs -> hits {query, id, off} sorted by (query, id, off); id = sorted[rank] >> 2 with a map, the rank itself without one.  *hits is malloc'ed.
 * 1 (and no hits) when a run reaches a rank >= n_seq -- the map is never read past its end -- or memory runs out. */
int fmdh_locate_hits(const fmd_locate_run_t *runs, uint64_t n_runs, const uint64_t *sorted, uint64_t n_seq, fmdh_locate_hit_t **hits, uint64_t *n_hits)
{
    uint64_t total = 0, k = 0;
    if (!hits || !n_hits || (n_runs && !runs)) return 1;
    *hits = 0; *n_hits = 0;
    for (uint64_t i = 0; i < n_runs; ++i) {
        if (runs[i].rank >= n_seq || runs[i].n > n_seq - runs[i].rank) return 1;
        total += runs[i].n;
    }
    fmdh_locate_hit_t *h = (fmdh_locate_hit_t *)malloc((total ? total : 1) * sizeof(*h));
    if (!h) return 1;
    for (uint64_t i = 0; i < n_runs; ++i)
        for (uint32_t j = 0; j < runs[i].n; ++j, ++k) {
            const uint64_t rank = runs[i].rank + j;
            h[k].id = sorted ? sorted[rank] >> 2 : rank; h[k].query = runs[i].query; h[k].off = runs[i].off;
        }
    qsort(h, total, sizeof(*h), hit_cmp);
    *hits = h; *n_hits = total;
    return 0;
}

static int flush_batch(fmd_dev_t *d, const uint64_t *sorted, uint64_t n_seq, uint32_t max_occ, size_t n, char **names, const uint8_t *bases, const uint64_t *off,
                       uint64_t *res, FILE *out)
{
    uint64_t *cnt = res, *beg = res + n, *end = res + 2 * n, n_runs = 0, n_hits = 0, k = 0;
    fmd_locate_run_t *runs = 0;
    fmd_locate_stat_t st;
    fmdh_locate_hit_t *hits = 0;
    int rc = fmd_bsearch_batch(d, n, bases, off, cnt, beg, end);
    if (rc == 0) rc = fmd_locate_batch(d, n, beg, cnt, max_occ, 0, &runs, &n_runs, &st);
    if (rc) { fprintf(stderr, "[E::main_locate] %s\n", fmd_strerror(rc)); return 1; }
    rc = fmdh_locate_hits(runs, n_runs, sorted, n_seq, &hits, &n_hits);
    fmd_host_free(runs);
    if (rc) { fprintf(stderr, "[E::main_locate] a sentinel rank beyond the index's %llu sequences, or out of memory\n", (unsigned long long)n_seq); return 1; }
    for (size_t i = 0; i < n; ++i) {
        fprintf(out, "SQ\t%s\t%llu\t%llu\t%d\n", names[i], (unsigned long long)(off[i + 1] - off[i]), (unsigned long long)cnt[i], cnt[i] <= max_occ);
        for (; k < n_hits && hits[k].query == i; ++k)
            fprintf(out, "OC\t%llu\t%c\t%u\n", (unsigned long long)(hits[k].id >> 1), "+-"[hits[k].id & 1], hits[k].off);
        fputs("//\n", out);
    }
    free(hits);
    return 0;
}

int fmdh_main_locate(int argc, char *argv[])
{
    int c, device = 0, rc = 0, l;
    long long max_occ = 1000;
    const char *rank_fn = 0;
    fmd_dev_t *d = 0;
    uint64_t *sorted = 0, n_sorted = 0;
    fmd_info_t info;
    while ((c = getopt(argc, argv, "g:m:r:")) >= 0) {
        if (c == 'g') device = atoi(optarg);
        else if (c == 'm') max_occ = atoll(optarg);
        else if (c == 'r') rank_fn = optarg;
    }
    if (optind + 2 > argc || max_occ < 1) {
        fprintf(stderr, "\nUsage:   fermi-amd locate [-g GPU] [-m INT] [-r reads.rank] <reads.fmd> <query.fa>\n\n");
        fprintf(stderr, "Options: -m INT    list the occurrences of a query that has at most INT of them [1000]\n");
        fprintf(stderr, "         -r FILE   the rank -> read map `seqsort` wrote for the index [computed]\n\n");
        fprintf(stderr, "Output:  SQ name length count located(1/0), then OC read +|- offset per occurrence, then //\n\n");
        return 1;
    }
    if (max_occ > 0xffffffffll) max_occ = 0xffffffffll;
    {
        const char *fn[3] = { argv[optind], strcmp(argv[optind + 1], "-") == 0 ? 0 : argv[optind + 1], rank_fn };
        for (int j = 0; j < 3; ++j) {
            FILE *fp = fn[j] ? fopen(fn[j], "rb") : 0;
            if (fn[j] && !fp) { fprintf(stderr, "[E::main_locate] fail to open file '%s'\n", fn[j]); return 1; }
            if (fp) fclose(fp);
        }
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_locate] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    if (rank_fn) {
        FILE *fp = fopen(rank_fn, "rb");
        long long bytes = -1;
        if (fp && fseek(fp, 0, SEEK_END) == 0) bytes = ftell(fp);
        if (fp && bytes >= 0 && bytes % 8 == 0 && (sorted = (uint64_t *)malloc(bytes ? (size_t)bytes : 8)) != 0) {
            rewind(fp);
            n_sorted = (uint64_t)bytes / 8;
            if (fread(sorted, 8, n_sorted, fp) != n_sorted) { free(sorted); sorted = 0; }
        }
        if (fp) fclose(fp);
        if (!sorted) { fprintf(stderr, "[E::main_locate] cannot read the rank file '%s'\n", rank_fn); return 1; }
    } else if (fmdh_seqsort(argv[optind], device, &sorted, &n_sorted)) return 1;
    rc = fmd_dev_open_file(device, argv[optind], &d);
    if (rc) { fprintf(stderr, "[E::main_locate] cannot load `%s': %s\n", argv[optind], fmd_strerror(rc)); free(sorted); return 1; }
    fmd_dev_info(d, &info);
    if (n_sorted != info.mcnt[1]) {
        fprintf(stderr, "[E::main_locate] the rank file has %llu entries, the index %llu sequences\n", (unsigned long long)n_sorted, (unsigned long long)info.mcnt[1]);
        rc = 1;
    }
    fmdh_seqio_t *io = rc ? 0 : fmdh_seq_open(argv[optind + 1]);
    if (!rc && !io) { fprintf(stderr, "[E::main_locate] fail to open file '%s'\n", argv[optind + 1]); rc = 1; }
    if (rc == 0) {
        char **names = (char **)calloc(LOCATE_BATCH, sizeof(char *));
        uint64_t *off = (uint64_t *)malloc((LOCATE_BATCH + 1) * 8), *res = (uint64_t *)malloc((size_t)LOCATE_BATCH * 3 * 8);
        size_t n = 0, cap = 1 << 20, tot = 0;
        uint8_t *bases = (uint8_t *)malloc(cap);
        if (!names || !off || !res || !bases) { fprintf(stderr, "[E::main_locate] out of memory\n"); rc = 1; }
        else off[0] = 0;
        while (rc == 0) {
            l = fmdh_seq_read(io);
            if (l < 0 || n == LOCATE_BATCH) {
                if (n) rc = flush_batch(d, sorted, n_sorted, (uint32_t)max_occ, n, names, bases, off, res, stdout);
                for (size_t i = 0; i < n; ++i) free(names[i]);
                n = 0; tot = 0;
                if (rc || l < 0) break;
            }
            if (tot + (size_t)l + 8 > cap) {
                while (tot + (size_t)l + 8 > cap) cap <<= 1;
                if ((bases = (uint8_t *)realloc(bases, cap)) == 0) { fprintf(stderr, "[E::main_locate] out of memory\n"); rc = 1; break; }
            }
            const char *s = fmdh_seq_bases(io);
            for (int i = 0; i < l; ++i) bases[tot + i] = fmdh_nt6[(unsigned char)s[i]];
            names[n] = strdup(fmdh_seq_name(io));
            tot += (size_t)l; off[++n] = tot;
        }
        free(names); free(off); free(res); free(bases);
    }
    if (io) fmdh_seq_close(io);
    fmd_dev_close(d);
    free(sorted);
    return rc ? 1 : 0;
}
