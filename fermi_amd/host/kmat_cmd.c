#define _GNU_SOURCE
/* kmat_cmd.c -- `fermi-amd kmat [-k 21] [-p 1] [-s min:max,min:max,...] [-d] [-g GPU] <a.fmd> <b.fmd> [<c.fmd> ...]`: the k-mer matrix of up to eight
 * indexes of both strands -- rows are canonical k-mers, columns are the indexes -- from the tries of all of them walked together on the resident indexes
 * (fmd_kmat).  The reference has no such command.
 *     without -d    PT <tab> bits <tab> n_kmers          per non-empty presence pattern, ascending by pattern value; bits = one character per index, index 0
 *                                                        first, 1 where the k-mer occurs at least -p times
 *                   SM <tab> i <tab> n_present <tab> n_total   per index
 *     with -d       KMER <tab> c0 <tab> c1 ...           per selected canonical k-mer, ascending; streamed from the sink, never held whole
 * and on stderr [M::main_kmat] k=.. n=.. distinct=.. parts=...  Usage and unreadable-file errors return 1 before the device is looked for.  A file of no
 * symbols (what `sub` writes when nothing is kept) is a column of zeros. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "fmd_host.h"

/* one end of a bound: digits only -> the value, clamped to 2^32 - 1; -1 for anything else (the empty string included) */
static long long bound_arg(const char *s, size_t len)
{
    unsigned long long v = 0;
    if (len == 0) return -1;
    for (size_t i = 0; i < len; ++i) {
        if (s[i] < '0' || s[i] > '9') return -1;
        v = v * 10 + (unsigned long long)(s[i] - '0');
        if (v > FMD_KMAT_NO_MAX) v = FMD_KMAT_NO_MAX;
    }
    return (long long)v;
}

int fmdh_kmat_parse_sel(const char *s, int n_idx, fmd_kmat_sel_t *sel)
{
    memset(sel, 0, sizeof(*sel));
    for (int i = 0; i < FMD_KMAT_MAX_IDX; ++i) sel->max[i] = FMD_KMAT_NO_MAX;
    sel->present = 1;
    if (n_idx < 1 || n_idx > FMD_KMAT_MAX_IDX) return 1;
    if (!s) return 0;
    for (int i = 0; ; ++i) {
        const char *end = strchr(s, ','), *colon;
        const size_t len = end ? (size_t)(end - s) : strlen(s);
        if (i >= n_idx) return 1;                     /* more entries than indexes */
        colon = (const char *)memchr(s, ':', len);
        if (!colon) return 1;
        if (colon > s) { const long long v = bound_arg(s, (size_t)(colon - s)); if (v < 0) return 1; sel->min[i] = (uint32_t)v; }
        if (colon + 1 < s + len) { const long long v = bound_arg(colon + 1, (size_t)(s + len - colon - 1)); if (v < 0) return 1; sel->max[i] = (uint32_t)v; }
        if (sel->min[i] > sel->max[i]) return 1;
        if (!end) return 0;
        s = end + 1;
    }
}

void fmdh_kmat_print_pt(FILE *out, const uint64_t *hist, int n_idx)
{
    char bits[FMD_KMAT_MAX_IDX + 1];
    if (n_idx < 1 || n_idx > FMD_KMAT_MAX_IDX) return;
    for (uint32_t p = 0; p < 1u << n_idx; ++p) {
        if (!hist[p]) continue;
        for (int i = 0; i < n_idx; ++i) bits[i] = (p >> i & 1) ? '1' : '0';
        bits[n_idx] = 0;
        fprintf(out, "PT\t%s\t%llu\n", bits, (unsigned long long)hist[p]);
    }
}

void fmdh_kmat_print_sm(FILE *out, int n_idx, const fmd_kmat_stat_t *st)
{
    for (int i = 0; i < n_idx && i < FMD_KMAT_MAX_IDX; ++i)
        fprintf(out, "SM\t%d\t%llu\t%llu\n", i, (unsigned long long)st->n_present[i], (unsigned long long)st->n_total[i]);
}

typedef struct { FILE *out; int k, n_idx; } dump_t;

static int dump_sink(void *ctx, uint64_t n, const uint64_t *kmer, const uint32_t *const *count)
{
    dump_t *d = (dump_t *)ctx;
    char buf[33];
    for (uint64_t j = 0; j < n; ++j) {
        if (fputs(fmdh_kmer_text(kmer[j], d->k, buf), d->out) < 0) return 1;
        for (int i = 0; i < d->n_idx; ++i)
            if (fprintf(d->out, "\t%u", count[i][j]) < 0) return 1;
        if (fputc('\n', d->out) < 0) return 1;
    }
    return 0;
}

int fmdh_main_kmat(int argc, char *argv[])
{
    int c, device = 0, dump = 0, rc = 0, n_idx, bad_sel = 0;
    long long k = 21, present = 1;
    const char *sel_text = 0;
    fmd_kmat_sel_t sel;
    fmd_dev_t *d[FMD_KMAT_MAX_IDX] = { 0 };
    while ((c = getopt(argc, argv, "k:p:s:dg:")) >= 0) {
        if (c == 'k') k = atoll(optarg);
        else if (c == 'p') present = atoll(optarg);
        else if (c == 's') sel_text = optarg;
        else if (c == 'd') dump = 1;
        else if (c == 'g') device = atoi(optarg);
    }
    n_idx = argc - optind;
    if (n_idx >= 1 && n_idx <= FMD_KMAT_MAX_IDX) bad_sel = fmdh_kmat_parse_sel(sel_text, n_idx, &sel);
    if (n_idx < 1 || n_idx > FMD_KMAT_MAX_IDX || k < 1 || k > 32 || present < 1 || present > FMD_KMAT_NO_MAX || bad_sel) {
        fprintf(stderr, "\nUsage:   fermi-amd kmat [-k 21] [-p 1] [-s min:max,min:max,...] [-d] [-g GPU] <a.fmd> <b.fmd> [<c.fmd> ...]\n\n");
        fprintf(stderr, "Options: -k INT    k-mer length, 1..32 [21]\n");
        fprintf(stderr, "         -p INT    a k-mer is present in an index where it occurs at least INT times, INT >= 1 [1]\n");
        fprintf(stderr, "         -s LIST   one min:max per index, in order: only the k-mers with min <= count <= max in every index; either end may be\n");
        fprintf(stderr, "                   empty (no bound), missing trailing entries are `0:'.  `-s 3:,0:0,0:0': at least 3 in the first, none in the others\n");
        fprintf(stderr, "         -d        print the selected k-mers with their counts in every index instead of the pattern spectrum\n\n");
        fprintf(stderr, "Input:   1 to %d indexes of both strands\n", FMD_KMAT_MAX_IDX);
        fprintf(stderr, "Output:  PT bits n_kmers per non-empty presence pattern (index 0 first), then SM i n_present n_total per index;\n");
        fprintf(stderr, "         with -d KMER c0 c1 ... per canonical k-mer, ascending\n\n");
        return 1;
    }
    sel.present = (uint32_t)present;
    for (int i = 0; i < n_idx; ++i) {
        FILE *fp = fopen(argv[optind + i], "rb");
        if (!fp) { fprintf(stderr, "[E::main_kmat] fail to open file '%s'\n", argv[optind + i]); return 1; }
        fclose(fp);
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_kmat] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    uint64_t *hist = (uint64_t *)calloc((size_t)1 << n_idx, 8);
    if (!hist) { fprintf(stderr, "[E::main_kmat] out of memory\n"); return 1; }
    for (int i = 0; i < n_idx && !rc; ++i) {
        rc = fmd_dev_open_file_ex(device, argv[optind + i], FMD_OPEN_EMPTY_OK, &d[i]);
        if (rc) fprintf(stderr, "[E::main_kmat] cannot load `%s': %s\n", argv[optind + i], fmd_strerror(rc));
    }
    if (!rc) {
        fmd_kmat_stat_t st;
        dump_t ctx = { stdout, (int)k, n_idx };
        rc = fmd_kmat(n_idx, d, (int)k, &sel, hist, 0, dump ? dump_sink : 0, &ctx, &st);
        if (rc == FMD_E_ARG) fprintf(stderr, "[E::main_kmat] one of the files is not an index of both strands: its base counts are not symmetric\n");
        else if (rc) fprintf(stderr, "[E::main_kmat] %s\n", fmd_strerror(rc));
        else {
            if (!dump) { fmdh_kmat_print_pt(stdout, hist, n_idx); fmdh_kmat_print_sm(stdout, n_idx, &st); }
            fprintf(stderr, "[M::main_kmat] k=%d n=%d distinct=%llu parts=%llu\n", (int)k, n_idx, (unsigned long long)st.n_kmers, (unsigned long long)st.n_parts);
        }
    }
    for (int i = 0; i < n_idx; ++i) fmd_dev_close(d[i]);
    free(hist);
    return rc ? 1 : 0;
}
