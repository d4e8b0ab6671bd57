#define _GNU_SOURCE
/* kcount_cmd.c -- `fermi-amd kcount [-k 21] [-o 1] [-b 10001] [-d] [-g GPU] <reads.fmd>`: the k-mer spectrum of the indexed reads, or their counted k-mers
 * (fmd_kcount: one backward extension on the resident index counts a k-mer exactly).  The reference has no such command.
 *     without -d    count <tab> n_kmers      per non-empty bin, ascending; the last bin's count is b - 1 and means "that many or more"
 *     with -d       KMER <tab> count         per canonical k-mer with at least -o occurrences, ascending; streamed from the sink, never held whole
 * and on stderr [M::main_kcount] k=.. distinct=.. total=.. parts=...  Usage and unreadable-file errors return 1 before the device is looked for. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "fmd_host.h"

char *fmdh_kmer_text(uint64_t kmer, int k, char *buf)
{
    if (k < 1 || k > 32 || !buf) return 0;
    for (int i = 0; i < k; ++i) buf[i] = "ACGT"[kmer >> (2 * (k - 1 - i)) & 3];
    buf[k] = 0;
    return buf;
}

void fmdh_kcount_print_hist(FILE *out, const uint64_t *hist, uint32_t n_bins)
{
    for (uint32_t i = 0; i < n_bins; ++i)
        if (hist[i]) fprintf(out, "%u\t%llu\n", i, (unsigned long long)hist[i]);
}

typedef struct { FILE *out; int k; } dump_t;

static int dump_sink(void *ctx, uint64_t n, const uint64_t *kmer, const uint32_t *count)
{
    dump_t *d = (dump_t *)ctx;
    char buf[33];
    for (uint64_t i = 0; i < n; ++i)
        if (fprintf(d->out, "%s\t%u\n", fmdh_kmer_text(kmer[i], d->k, buf), count[i]) < 0) return 1;
    return 0;
}

int fmdh_main_kcount(int argc, char *argv[])
{
    int c, device = 0, dump = 0, rc;
    long long k = 21, min_occ = 1, n_bins = 10001;
    fmd_dev_t *d = 0;
    while ((c = getopt(argc, argv, "k:o:b:dg:")) >= 0) {
        if (c == 'k') k = atoll(optarg);
        else if (c == 'o') min_occ = atoll(optarg);
        else if (c == 'b') n_bins = atoll(optarg);
        else if (c == 'd') dump = 1;
        else if (c == 'g') device = atoi(optarg);
    }
    if (optind + 1 > argc || k < 1 || k > 32 || min_occ < 1 || min_occ > 0x7fffffffll || n_bins < 2 || n_bins > 0xffffffffll) {
        fprintf(stderr, "\nUsage:   fermi-amd kcount [-k 21] [-o 1] [-b 10001] [-d] [-g GPU] <reads.fmd>\n\n");
        fprintf(stderr, "Options: -k INT    k-mer length, 1..32 [21]\n");
        fprintf(stderr, "         -o INT    leave out k-mers with fewer than INT occurrences, at least 1 [1]\n");
        fprintf(stderr, "         -b INT    bins of the histogram, at least 2; the last holds the counts of INT-1 and more [10001]\n");
        fprintf(stderr, "         -d        print the k-mers and their counts instead of the histogram\n\n");
        fprintf(stderr, "Output:  count n_kmers per non-empty bin; with -d KMER count per canonical k-mer, ascending\n\n");
        return 1;
    }
    {
        FILE *fp = fopen(argv[optind], "rb");
        if (!fp) { fprintf(stderr, "[E::main_kcount] fail to open file '%s'\n", argv[optind]); return 1; }
        fclose(fp);
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_kcount] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    uint64_t *hist = (uint64_t *)calloc(dump ? 2 : (size_t)n_bins, 8);
    if (!hist) { fprintf(stderr, "[E::main_kcount] out of memory\n"); return 1; }
    rc = fmd_dev_open_file(device, argv[optind], &d);
    if (rc) { fprintf(stderr, "[E::main_kcount] cannot load `%s': %s\n", argv[optind], fmd_strerror(rc)); free(hist); return 1; }
    fmd_kcount_stat_t st;
    dump_t ctx = { stdout, (int)k };
    rc = fmd_kcount(d, (int)k, (int)min_occ, dump ? 2 : (uint32_t)n_bins, hist, 0, dump ? dump_sink : 0, &ctx, &st);
    if (rc == FMD_E_ARG) fprintf(stderr, "[E::main_kcount] `%s' is not an index of both strands: its base counts are not symmetric\n", argv[optind]);
    else if (rc) fprintf(stderr, "[E::main_kcount] %s\n", fmd_strerror(rc));
    else {
        if (!dump) fmdh_kcount_print_hist(stdout, hist, (uint32_t)n_bins);
        fprintf(stderr, "[M::main_kcount] k=%d distinct=%llu total=%llu parts=%llu\n", (int)k, (unsigned long long)st.n_kmers, (unsigned long long)st.n_total,
                (unsigned long long)st.n_parts);
    }
    fmd_dev_close(d);
    free(hist);
    return rc ? 1 : 0;
}
