#define _GNU_SOURCE
/* msearch_cmd.c -- `fermi-amd msearch [-g dev] <query.fa> <a.fmd> [<b.fmd> ...]`: backward search of every query over SEVERAL FMD-indexes at once
 * (fmd_multi_bsearch_batch, fm_multi_backward_search exact.c:25-57): the count and SA interval the query has in the merged index of a, b, ..,
 * from the per-lane files the driver script's splitfa + ropebwt leave, without merging them.  The reference has only a commented-out `test`
 * command for this (main.c:36-62).  Index files are RLD\2 or RLE\6.  One line per query, in input order:
 *     name <tab> length <tab> count <tab> beg <tab> end          (a miss: 0 0 0)
 * Usage and unreadable-file errors return 1 before the device is looked for. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "fmd_host.h"

#define MSEARCH_BATCH 262144

static int flush_batch(int n_idx, fmd_dev_t **idx, size_t n, char **names, const uint8_t *bases, const uint64_t *off, uint64_t *res, FILE *out)
{
    uint64_t *cnt = res, *beg = res + n, *end = res + 2 * n;
    int rc = fmd_multi_bsearch_batch(n_idx, idx, n, bases, off, cnt, beg, end);
    if (rc) { fprintf(stderr, "[E::main_msearch] %s\n", fmd_strerror(rc)); return 1; }
    for (size_t i = 0; i < n; ++i)
        fprintf(out, "%s\t%llu\t%llu\t%llu\t%llu\n", names[i], (unsigned long long)(off[i + 1] - off[i]), (unsigned long long)cnt[i],
                (unsigned long long)beg[i], (unsigned long long)end[i]);
    return 0;
}

int fmdh_main_msearch(int argc, char *argv[])
{
    int c, device = 0, n_idx, j, rc = 0, l;
    fmd_dev_t *idx[FMD_MULTI_MAX];
    while ((c = getopt(argc, argv, "g:")) >= 0) if (c == 'g') device = atoi(optarg);
    if (optind + 2 > argc) {
        fprintf(stderr, "\nUsage:   fermi-amd msearch [-g GPU] <query.fa> <a.fmd> [<b.fmd> ...]\n\n");
        fprintf(stderr, "         count and SA interval of every query in the merged index of the files (at most %d), from the files as they are\n", FMD_MULTI_MAX);
        fprintf(stderr, "Output:  name, length, count, beg, end per query, tab-separated; a miss is 0 0 0\n\n");
        return 1;
    }
    n_idx = argc - optind - 1;
    if (n_idx > FMD_MULTI_MAX) { fprintf(stderr, "[E::main_msearch] %d index files: at most %d\n", n_idx, FMD_MULTI_MAX); return 1; }
    for (j = strcmp(argv[optind], "-") == 0 ? 1 : 0; j <= n_idx; ++j) {
        FILE *fp = fopen(argv[optind + j], "rb");
        if (!fp) { fprintf(stderr, "[E::main_msearch] fail to open file '%s'\n", argv[optind + j]); return 1; }
        fclose(fp);
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_msearch] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    memset(idx, 0, sizeof(idx));
    for (j = 0; j < n_idx && rc == 0; ++j) {
        rc = fmd_dev_open_file_ex(device, argv[optind + 1 + j], FMD_OPEN_EMPTY_OK, &idx[j]);   /* a lane that got no reads is a part like any other */
        if (rc) fprintf(stderr, "[E::main_msearch] cannot load `%s': %s\n", argv[optind + 1 + j], fmd_strerror(rc));
    }
    fmdh_seqio_t *io = rc ? 0 : fmdh_seq_open(argv[optind]);
    if (!rc && !io) { fprintf(stderr, "[E::main_msearch] fail to open file '%s'\n", argv[optind]); rc = 1; }
    if (rc == 0) {
        char **names = (char **)calloc(MSEARCH_BATCH, sizeof(char *));
        uint64_t *off = (uint64_t *)malloc((MSEARCH_BATCH + 1) * 8), *res = (uint64_t *)malloc((size_t)MSEARCH_BATCH * 3 * 8);
        size_t n = 0, cap = 1 << 20, tot = 0;
        uint8_t *bases = (uint8_t *)malloc(cap);
        if (!names || !off || !res || !bases) { fprintf(stderr, "[E::main_msearch] out of memory\n"); rc = 1; }
        else off[0] = 0;
        while (rc == 0) {
            l = fmdh_seq_read(io);
            if (l < 0 || n == MSEARCH_BATCH) {
                if (n) rc = flush_batch(n_idx, idx, n, names, bases, off, res, stdout);
                for (size_t i = 0; i < n; ++i) free(names[i]);
                n = 0; tot = 0;
                if (rc || l < 0) break;
            }
            if (tot + (size_t)l + 8 > cap) {
                while (tot + (size_t)l + 8 > cap) cap <<= 1;
                if ((bases = (uint8_t *)realloc(bases, cap)) == 0) { fprintf(stderr, "[E::main_msearch] out of memory\n"); rc = 1; break; }
            }
            const char *s = fmdh_seq_bases(io);
            for (int i = 0; i < l; ++i) bases[tot + i] = fmdh_nt6[(unsigned char)s[i]];
            names[n] = strdup(fmdh_seq_name(io));
            tot += (size_t)l; off[++n] = tot;
        }
        free(names); free(off); free(res); free(bases);
    }
    if (io) fmdh_seq_close(io);
    for (j = 0; j < n_idx; ++j) if (idx[j]) fmd_dev_close(idx[j]);
    return rc ? 1 : 0;
}
