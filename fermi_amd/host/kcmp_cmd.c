#define _GNU_SOURCE
/* kcmp_cmd.c -- `fermi-amd kcmp [-k 21] [-a 0] [-A inf] [-b 0] [-B inf] [-n 256] [-d] [-g GPU] <a.fmd> <b.fmd>`: the joint k-mer counts of two indexes of both
 * strands (fmd_kcmp: the tries of both walked together on the resident indexes).  The reference has no such command.
 *     without -d    c0 <tab> c1 <tab> n_kmers     per non-empty cell of the n x n histogram, row-major; a label of n - 1 means "that many or more"
 *     with -d       KMER <tab> c0 <tab> c1        per canonical k-mer with -a <= c0 <= -A and -b <= c1 <= -B, ascending; streamed from the sink, never held whole
 * and on stderr [M::main_kcmp] k=.. distinct=.. only0=.. only1=.. shared=.. total0=.. total1=.. parts=...  Usage and unreadable-file errors return 1 before the
 * device is looked for.  A file of no symbols (what `sub` writes when nothing is kept) is a side on which every count is 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "fmd_host.h"

void fmdh_kcmp_print_hist(FILE *out, const uint64_t *hist, uint32_t n_bins)
{
    for (uint32_t i = 0; i < n_bins; ++i)
        for (uint32_t j = 0; j < n_bins; ++j)
            if (hist[(size_t)i * n_bins + j]) fprintf(out, "%u\t%u\t%llu\n", i, j, (unsigned long long)hist[(size_t)i * n_bins + j]);
}

typedef struct { FILE *out; int k; } dump_t;

static int dump_sink(void *ctx, uint64_t n, const uint64_t *kmer, const uint32_t *c0, const uint32_t *c1)
{
    dump_t *d = (dump_t *)ctx;
    char buf[33];
    for (uint64_t i = 0; i < n; ++i)
        if (fprintf(d->out, "%s\t%u\t%u\n", fmdh_kmer_text(kmer[i], d->k, buf), c0[i], c1[i]) < 0) return 1;
    return 0;
}

/* an upper bound: a number, or `inf` for none; -1 for anything else */
static long long max_arg(const char *s)
{
    char *end;
    if (strcmp(s, "inf") == 0) return FMD_KCMP_NO_MAX;
    const long long v = strtoll(s, &end, 10);
    if (*s == 0 || *end != 0 || v < 0) return -1;
    return v >= FMD_KCMP_NO_MAX ? FMD_KCMP_NO_MAX : v;
}

int fmdh_main_kcmp(int argc, char *argv[])
{
    int c, device = 0, dump = 0, rc;
    long long k = 21, min0 = 0, max0 = FMD_KCMP_NO_MAX, min1 = 0, max1 = FMD_KCMP_NO_MAX, n_bins = 256;
    fmd_dev_t *d[2] = { 0, 0 };
    while ((c = getopt(argc, argv, "k:a:A:b:B:n:dg:")) >= 0) {
        if (c == 'k') k = atoll(optarg);
        else if (c == 'a') min0 = atoll(optarg);
        else if (c == 'A') max0 = max_arg(optarg);
        else if (c == 'b') min1 = atoll(optarg);
        else if (c == 'B') max1 = max_arg(optarg);
        else if (c == 'n') n_bins = atoll(optarg);
        else if (c == 'd') dump = 1;
        else if (c == 'g') device = atoi(optarg);
    }
    if (optind + 2 > argc || k < 1 || k > 32 || min0 < 0 || min1 < 0 || max0 < 0 || max1 < 0 || min0 > max0 || min1 > max1 || n_bins < 2 || n_bins > 1024) {
        fprintf(stderr, "\nUsage:   fermi-amd kcmp [-k 21] [-a 0] [-A inf] [-b 0] [-B inf] [-n 256] [-d] [-g GPU] <a.fmd> <b.fmd>\n\n");
        fprintf(stderr, "Options: -k INT    k-mer length, 1..32 [21]\n");
        fprintf(stderr, "         -a INT    least count in the first index [0]\n");
        fprintf(stderr, "         -A INT    largest count in the first index, at least -a; inf = no bound [inf]\n");
        fprintf(stderr, "         -b INT    least count in the second index [0]\n");
        fprintf(stderr, "         -B INT    largest count in the second index, at least -b; inf = no bound [inf]\n");
        fprintf(stderr, "         -n INT    bins per axis of the histogram, 2..1024; the last holds the counts of INT-1 and more [256]\n");
        fprintf(stderr, "         -d        print the selected k-mers with both counts instead of the histogram\n\n");
        fprintf(stderr, "Output:  c0 c1 n_kmers per non-empty cell; with -d KMER c0 c1 per canonical k-mer, ascending\n\n");
        return 1;
    }
    for (int i = 0; i < 2; ++i) {
        FILE *fp = fopen(argv[optind + i], "rb");
        if (!fp) { fprintf(stderr, "[E::main_kcmp] fail to open file '%s'\n", argv[optind + i]); return 1; }
        fclose(fp);
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_kcmp] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    if (dump) n_bins = 2;
    uint64_t *hist = (uint64_t *)calloc((size_t)(n_bins * n_bins), 8);
    if (!hist) { fprintf(stderr, "[E::main_kcmp] out of memory\n"); return 1; }
    for (int i = 0; i < 2; ++i) {
        rc = fmd_dev_open_file_ex(device, argv[optind + i], FMD_OPEN_EMPTY_OK, &d[i]);
        if (rc) { fprintf(stderr, "[E::main_kcmp] cannot load `%s': %s\n", argv[optind + i], fmd_strerror(rc)); fmd_dev_close(d[0]); free(hist); return 1; }
    }
    fmd_kcmp_stat_t st;
    const fmd_kcmp_sel_t sel = { (uint32_t)(min0 > FMD_KCMP_NO_MAX ? FMD_KCMP_NO_MAX : min0), (uint32_t)max0, (uint32_t)(min1 > FMD_KCMP_NO_MAX ? FMD_KCMP_NO_MAX : min1), (uint32_t)max1 };
    dump_t ctx = { stdout, (int)k };
    rc = fmd_kcmp(d[0], d[1], (int)k, &sel, (uint32_t)n_bins, hist, 0, dump ? dump_sink : 0, &ctx, &st);
    if (rc == FMD_E_ARG) fprintf(stderr, "[E::main_kcmp] `%s' or `%s' is not an index of both strands: its base counts are not symmetric\n", argv[optind], argv[optind + 1]);
    else if (rc) fprintf(stderr, "[E::main_kcmp] %s\n", fmd_strerror(rc));
    else {
        if (!dump) fmdh_kcmp_print_hist(stdout, hist, (uint32_t)n_bins);
        fprintf(stderr, "[M::main_kcmp] k=%d distinct=%llu only0=%llu only1=%llu shared=%llu total0=%llu total1=%llu parts=%llu\n", (int)k, (unsigned long long)st.n_kmers,
                (unsigned long long)st.n_only0, (unsigned long long)st.n_only1, (unsigned long long)st.n_shared, (unsigned long long)st.n_total0,
                (unsigned long long)st.n_total1, (unsigned long long)st.n_parts);
    }
    fmd_dev_close(d[0]); fmd_dev_close(d[1]);
    free(hist);
    return rc ? 1 : 0;
}
