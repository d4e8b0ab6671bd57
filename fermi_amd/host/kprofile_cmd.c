#define _GNU_SOURCE
/* kprofile_cmd.c -- `fermi-amd kprofile [-k 21] [-s] [-q] [-g GPU] <queries.fa> <a.fmd> [<b.fmd> ...]`: how often every k-mer of every query sequence occurs in
 * the indexed reads (fmd_kprofile_batch: kcount's COUNT of every window).  The reference has no such command.  All indexes are opened
 * once; the queries are read in batches of about KPROFILE_BATCH bases -- a longer sequence is a batch of its own -- and every batch is profiled against every
 * index.  Per sequence, in input order:
 *     SQ <tab> name <tab> length <tab> n_windows
 *     KP <tab> i <tab> c_0,c_1,..        per index i (0-based, command-line order); * when the sequence has no window
 *     //
 * with -s, instead of the KP line:  KS <tab> i <tab> n_valid <tab> n_zero <tab> min <tab> median <tab> max <tab> mean   over the N-free windows
 * with -q (one index only) a FASTQ record for `cnt2qual`: the sequence as read, and per base the quality 33 + min(93, the largest count among the windows
 * that cover it).  Usage and unreadable-file errors return 1 before the device is looked for. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "fmd_host.h"

#define KPROFILE_BATCH ((size_t)64 << 20)

void fmdh_kprofile_print_kp(FILE *out, int idx, const uint32_t *count, uint64_t n_windows)
{
    fprintf(out, "KP\t%d\t", idx);
    if (n_windows == 0) fputc('*', out);
    for (uint64_t j = 0; j < n_windows; ++j) fprintf(out, j ? ",%u" : "%u", count[j]);
    fputc('\n', out);
}

static int cmp_u32(const void *a, const void *b)
{
    const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return x < y ? -1 : x > y;
}

int fmdh_kprofile_print_ks(FILE *out, int idx, const uint8_t *nt6, uint64_t len, int k, const uint32_t *count)
{
    const uint64_t nw = k >= 1 && len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0;
    uint32_t *v = (uint32_t *)malloc((nw ? nw : 1) * sizeof(uint32_t));
    uint64_t n_valid = 0, n_zero = 0, bad = 0;      /* bad: the bases outside A/C/G/T in the window that ends at p */
    double sum = 0;
    if (!v) return 1;
    for (uint64_t p = 0; p < len && nw; ++p) {
        bad += nt6[p] < 1 || nt6[p] > 4;
        if (p >= (uint64_t)k) bad -= nt6[p - k] < 1 || nt6[p - k] > 4;
        if (p + 1 >= (uint64_t)k && bad == 0) {
            const uint32_t c = count[p + 1 - k];
            v[n_valid++] = c; n_zero += c == 0; sum += c;
        }
    }
    qsort(v, n_valid, sizeof(uint32_t), cmp_u32);
    fprintf(out, "KS\t%d\t%llu\t%llu\t", idx, (unsigned long long)n_valid, (unsigned long long)n_zero);
    if (n_valid == 0) fprintf(out, "*\t*\t*\t*\n");
    else fprintf(out, "%u\t%u\t%u\t%.3f\n", v[0], v[(n_valid - 1) / 2], v[n_valid - 1], sum / (double)n_valid);
    free(v);
    return 0;
}

/* the largest count over the windows [max(0, p - k + 1), min(p, nw - 1)] for every p: a sliding maximum (the window starts that are still candidates, their
 * counts descending, in a ring of k + 1 places) */
int fmdh_kprofile_qual(const uint32_t *count, uint64_t len, int k, char *qual)
{
    const uint64_t nw = k >= 1 && len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0, cap = (uint64_t)(k > 0 ? k : 0) + 1;
    uint64_t *ring = (uint64_t *)malloc(cap * sizeof(uint64_t)), head = 0, tail = 0;   /* ring[head % cap .. tail % cap) */
    if (!ring) return 1;
    for (uint64_t p = 0; p < len; ++p) {
        if (p < nw) {
            while (tail > head && count[ring[(tail - 1) % cap]] <= count[p]) --tail;
            ring[tail++ % cap] = p;
        }
        while (tail > head && ring[head % cap] + (uint64_t)k <= p) ++head;      /* a window that ended before p */
        const uint32_t m = tail > head ? count[ring[head % cap]] : 0;
        qual[p] = (char)(33 + (m > 93 ? 93 : m));
    }
    qual[len] = 0;
    free(ring);
    return 0;
}

typedef struct {
    size_t n, m_n, tot, m_tot, txt, m_txt;
    char **names;
    uint64_t *off, *woff;
    uint8_t *bases;      /* nt6, back to back (+ 8 bytes of room) */
    char *text;          /* the sequences as read, back to back (-q) */
} batch_t;

static int batch_add(batch_t *b, const char *name, const char *s, int l, int keep_text)
{
    if (b->n + 2 > b->m_n) {
        b->m_n = b->m_n ? b->m_n * 2 : 1024;
        b->names = (char **)realloc(b->names, b->m_n * sizeof(char *));
        b->off = (uint64_t *)realloc(b->off, (b->m_n + 1) * 8); b->woff = (uint64_t *)realloc(b->woff, (b->m_n + 1) * 8);
        if (!b->names || !b->off || !b->woff) return 1;
    }
    if (b->tot + (size_t)l + 8 > b->m_tot) {
        b->m_tot = b->m_tot ? b->m_tot : 1 << 20;
        while (b->tot + (size_t)l + 8 > b->m_tot) b->m_tot <<= 1;
        if ((b->bases = (uint8_t *)realloc(b->bases, b->m_tot)) == 0) return 1;
        if (keep_text && (b->text = (char *)realloc(b->text, b->m_tot)) == 0) return 1;
    }
    for (int i = 0; i < l; ++i) b->bases[b->tot + i] = fmdh_nt6[(unsigned char)s[i]];
    if (keep_text) memcpy(b->text + b->tot, s, (size_t)l);
    if ((b->names[b->n] = strdup(name)) == 0) return 1;
    b->off[0] = 0;
    b->tot += (size_t)l; b->off[++b->n] = b->tot;
    return 0;
}

static int batch_flush(batch_t *b, FILE *out, int n_idx, fmd_dev_t *const *idx, int k, int mode, uint32_t **cnt)
{
    int rc = 0;
    char *qual = 0;
    for (int j = 0; j < n_idx; ++j) cnt[j] = 0;
    for (int j = 0; j < n_idx && !rc; ++j) {
        fmd_kprofile_stat_t st;
        const int e = fmd_kprofile_batch(idx[j], b->n, b->bases, b->off, k, 0, b->woff, &cnt[j], &st);
        if (e == FMD_E_ARG) fprintf(stderr, "[E::main_kprofile] index %d is not an index of both strands: its base counts are not symmetric\n", j);
        else if (e) fprintf(stderr, "[E::main_kprofile] %s\n", fmd_strerror(e));
        rc = e != 0;
    }
    for (size_t i = 0; i < b->n && !rc; ++i) {
        const uint64_t len = b->off[i + 1] - b->off[i], nw = b->woff[i + 1] - b->woff[i];
        if (mode == 'q') {
            char *q2 = (char *)realloc(qual, len + 1);
            if (!q2 || fmdh_kprofile_qual(cnt[0] ? cnt[0] + b->woff[i] : 0, len, k, qual = q2)) { fprintf(stderr, "[E::main_kprofile] out of memory\n"); rc = 1; break; }
            fprintf(out, "@%s\n", b->names[i]);
            fwrite(b->text + b->off[i], 1, len, out);
            fprintf(out, "\n+\n%s\n", qual);
            continue;
        }
        fprintf(out, "SQ\t%s\t%llu\t%llu\n", b->names[i], (unsigned long long)len, (unsigned long long)nw);
        for (int j = 0; j < n_idx && !rc; ++j) {
            const uint32_t *c = cnt[j] ? cnt[j] + b->woff[i] : 0;
            if (mode == 's') { if ((rc = fmdh_kprofile_print_ks(out, j, b->bases + b->off[i], len, k, c)) != 0) fprintf(stderr, "[E::main_kprofile] out of memory\n"); }
            else fmdh_kprofile_print_kp(out, j, c, nw);
        }
        fprintf(out, "//\n");
    }
    free(qual);
    for (int j = 0; j < n_idx; ++j) { fmd_host_free(cnt[j]); cnt[j] = 0; }
    for (size_t i = 0; i < b->n; ++i) free(b->names[i]);
    b->n = 0; b->tot = 0;
    return rc;
}

int fmdh_kprofile_run(FILE *out, const char *query_fn, int n_idx, fmd_dev_t *const *idx, int k, int mode, size_t batch_bases)
{
    int rc = 0, l;
    batch_t b;
    uint32_t **cnt = (uint32_t **)calloc((size_t)(n_idx > 0 ? n_idx : 1), sizeof(uint32_t *));
    fmdh_seqio_t *io = fmdh_seq_open(query_fn);
    memset(&b, 0, sizeof(b));
    if (!io) fprintf(stderr, "[E::main_kprofile] fail to open file '%s'\n", query_fn);
    if (!io || !cnt || n_idx < 1 || (mode == 'q' && n_idx != 1)) { if (io) fmdh_seq_close(io); free(cnt); return 1; }
    if (batch_bases == 0) batch_bases = KPROFILE_BATCH;
    while (rc == 0) {
        l = fmdh_seq_read(io);
        if (l < 0 || (b.n && b.tot + (size_t)l > batch_bases)) {      /* the end, or this sequence would take the batch past its size */
            if (b.n) rc = batch_flush(&b, out, n_idx, idx, k, mode, cnt);
            if (rc || l < 0) break;
        }
        if (batch_add(&b, fmdh_seq_name(io), fmdh_seq_bases(io), l, mode == 'q')) { fprintf(stderr, "[E::main_kprofile] out of memory\n"); rc = 1; }
    }
    for (size_t i = 0; i < b.n; ++i) free(b.names[i]);
    free(b.names); free(b.off); free(b.woff); free(b.bases); free(b.text); free(cnt);
    fmdh_seq_close(io);
    return rc;
}

int fmdh_main_kprofile(int argc, char *argv[])
{
    int c, device = 0, mode = 0, two_modes = 0, n_idx, j, rc = 0;
    long long k = 21;
    while ((c = getopt(argc, argv, "k:sqg:")) >= 0) {
        if (c == 'k') k = atoll(optarg);
        else if (c == 's' || c == 'q') { two_modes |= mode && mode != c; mode = c; }
        else if (c == 'g') device = atoi(optarg);
    }
    n_idx = argc - optind - 1;
    if (n_idx < 1 || k < 1 || k > FMD_KPROFILE_MAX_K || two_modes || (mode == 'q' && n_idx != 1)) {
        fprintf(stderr, "\nUsage:   fermi-amd kprofile [-k 21] [-s] [-q] [-g GPU] <queries.fa> <a.fmd> [<b.fmd> ...]\n\n");
        fprintf(stderr, "Options: -k INT    k-mer length, 1..%d [21]\n", FMD_KPROFILE_MAX_K);
        fprintf(stderr, "         -s        per sequence and index a summary of the counts of the N-free windows instead of the counts\n");
        fprintf(stderr, "         -q        FASTQ for `cnt2qual`: per base the largest count among the windows that cover it, capped at 93; one index only\n\n");
        fprintf(stderr, "Output:  SQ name length n_windows, then per index i (0-based): KP i c_0,c_1,.. -- the count of the k-mer at every position of the\n");
        fprintf(stderr, "         sequence in the reads of index i, 0 for a window with an N --, then //; -s: KS i n_valid n_zero min median max mean\n\n");
        return 1;
    }
    for (j = strcmp(argv[optind], "-") == 0 ? 1 : 0; j <= n_idx; ++j) {
        FILE *fp = fopen(argv[optind + j], "rb");
        if (!fp) { fprintf(stderr, "[E::main_kprofile] fail to open file '%s'\n", argv[optind + j]); return 1; }
        fclose(fp);
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_kprofile] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    fmd_dev_t **idx = (fmd_dev_t **)calloc((size_t)n_idx, sizeof(fmd_dev_t *));
    if (!idx) { fprintf(stderr, "[E::main_kprofile] out of memory\n"); return 1; }
    for (j = 0; j < n_idx && rc == 0; ++j) {
        rc = fmd_dev_open_file_ex(device, argv[optind + 1 + j], FMD_OPEN_EMPTY_OK, &idx[j]);   /* (an index of no reads: every count 0) */
        if (rc) fprintf(stderr, "[E::main_kprofile] cannot load `%s': %s\n", argv[optind + 1 + j], fmd_strerror(rc));
    }
    if (rc == 0) rc = fmdh_kprofile_run(stdout, argv[optind], n_idx, idx, (int)k, mode, 0);
    for (j = 0; j < n_idx; ++j) if (idx[j]) fmd_dev_close(idx[j]);
    free(idx);
    return rc ? 1 : 0;
}
