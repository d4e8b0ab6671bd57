#define _GNU_SOURCE
/* ropebwt_cmd.c -- `fermi ropebwt [-a bpr|bcr] [-FRObNt] [-o FILE] [-f FILE] [-r INT] [-n INT] [-v INT] <in.fq.gz>` (ropebwt.c:47-158): the index
 * builder of the reference's driver script (`ropebwt -a bcr -v3 -btNf PRE.tmp -`), one strand or both, the BWT on the GPU.
 *
 * What goes in, in the reference's order (ropebwt.c:102-123):
 *   - every record of the input (`-` = stdin, gzip transparent) is converted to nt6, a byte >= 128 to 5 (ropebwt.c:105-106);
 *   - with -N it is cut at every 5 and each non-empty piece is a sequence of its own (ropebwt.c:107-116);
 *   - without -N under `-a bcr` every 5 becomes (lrand48() & 3) + 1, in read order and position order, and nothing else in the command draws
 *     from that stream, which nobody seeds: the same call gives the bases the reference gives (ropebwt.c:118-120);
 *   - without -N under `-a bpr` the 5s stay, and are sorted as the sixth symbol;
 *   - every piece of even length that is its own reverse complement loses its last base unless -O (ropebwt.c:25-29);
 *   - -F and -R clear a strand (ropebwt.c:30-44): fmd_build_bwt_strands builds  read $  /  revcomp $  /  read $ revcomp $ ; with both
 *     cleared the BWT is empty, and the output is that of an empty BWT: a newline, or the four magic bytes.
 * A record without bases, when -N does not drop it: the reference's trim turns its length 0 into -1 (ropebwt.c:25-28); bpr_insert_string then
 * inserts a '$' alone for every strand (bprope6.c:218-224) -- an empty sequence, which is what is built here -- and bcr_append stops the
 * program at its assertion (bcr.c:361): here `-a bcr` refuses such an input with a message, returns 1 and writes nothing.
 *
 * -a selects the rule for 5s and nothing else: both algorithms of the reference compute one BWT, and here it is the GPU's suffix sort.
 * -t, -r, -n and -v below 3 change nothing; -v3 prints phase lines of our own; -f FILE is accepted and no file is written (the reference
 * unlinks its own, bcr.c:518); -T (print the rope) is not supported.
 *
 * What comes out, to -o FILE or stdout:
 *   - without -b the BWT as `$ACGTN` characters and one newline: the reference's bytes (ropebwt.c:137-141).  It is copied from the device
 *     and written in slices; the host never holds the whole BWT;
 *   - with -b `RLE\6` and run bytes `len << 3 | sym` (ropebwt.c:132-135).  The BWT stays on the device and leaves it as runs
 *     (fmd_bwt_to_rle6, the FMD_BUILD_RUNS route of build_cmd.c): maximal runs split at 31.  The reference cuts its runs where its
 *     internal buckets and leaves end, and every reader of this stream merges neighbouring runs of one symbol (rld.c:177-184), so these
 *     bytes are NOT the reference's: the decoded symbols are, and `recode` of either file is the same RLD\2 file byte for byte. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include "fmd_host.h"

static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

enum { ALGO_BPR, ALGO_BCR };
typedef struct { uint8_t *bases; uint64_t *off; size_t n, m_n, tot, m_tot; int no_trim; } seqs_t;

/* insert1 (ropebwt.c:22-45) up to the strands, which the builder lays out: the piece, trimmed, is the next sequence */
static int add_piece(seqs_t *q, const uint8_t *s, uint32_t l)
{
    if (!q->no_trim) l = fmdh_trim_palindrome(s, l);
    if (q->tot + l + 8 > q->m_tot) {
        while (q->tot + l + 8 > q->m_tot) q->m_tot = q->m_tot ? q->m_tot << 1 : 1 << 20;
        if ((q->bases = (uint8_t *)realloc(q->bases, q->m_tot)) == 0) return -1;
    }
    if (q->n + 2 > q->m_n) {
        q->m_n = q->m_n ? q->m_n << 1 : 1 << 16;
        if ((q->off = (uint64_t *)realloc(q->off, q->m_n * 8)) == 0) return -1;
        q->off[0] = 0;
    }
    memcpy(q->bases + q->tot, s, l);
    q->tot += l; q->off[++q->n] = q->tot;
    return 0;
}

/* the BWT on the device as `$ACGTN` characters, slice by slice */
#define TEXT_SLICE ((uint64_t)4 << 20)
static int write_text(const uint8_t *d_bwt, uint64_t n_sym, FILE *out)
{
    uint8_t *buf = (uint8_t *)malloc(n_sym < TEXT_SLICE ? n_sym + 1 : TEXT_SLICE);
    uint64_t o, i;
    int rc = 0;
    if (!buf) return FMD_E_NOMEM;
    for (o = 0; o < n_sym && !rc; o += TEXT_SLICE) {
        const uint64_t m = n_sym - o < TEXT_SLICE ? n_sym - o : TEXT_SLICE;
        if ((rc = fmd_memcpy_d2h(buf, d_bwt + o, m, 0)) != 0) break;
        for (i = 0; i < m; ++i) buf[i] = (uint8_t)"$ACGTN??"[buf[i] & 7];
        if (fwrite(buf, 1, m, out) != m) rc = FMD_E_IO;
    }
    free(buf);
    return rc;
}

int fmdh_main_ropebwt(int argc, char *argv[])
{
    int c, algo = ALGO_BPR, max_runs = 512, max_nodes = 64, verbose = 2, device = 0, rc = 0, l;
    int is_bin = 0, cut_n = 0, tree = 0;
    unsigned strands = FMD_STRAND_BOTH;
    const char *out_fn = 0;
    FILE *out = stdout;
    seqs_t q;
    fmdh_seqio_t *io;
    uint8_t *d_bwt = 0;
    uint64_t n_sym = 0;
    double t0 = now_s(), t1, t2;
    memset(&q, 0, sizeof(q));
    while ((c = getopt(argc, argv, "TFRObNo:r:n:ta:f:v:g:")) >= 0) {   /* ropebwt.c:59, and -g */
        switch (c) {
        case 'a':
            if (strcmp(optarg, "bpr") == 0) algo = ALGO_BPR;
            else if (strcmp(optarg, "bcr") == 0) algo = ALGO_BCR;
            else fprintf(stderr, "[W::main_ropebwt] available algorithms: bpr or bcr; default to bpr\n");
            break;
        case 'o': out_fn = optarg; break;
        case 'F': strands &= ~FMD_STRAND_FWD; break;
        case 'R': strands &= ~FMD_STRAND_REV; break;
        case 'O': q.no_trim = 1; break;
        case 'T': tree = 1; break;
        case 'b': is_bin = 1; break;
        case 'N': cut_n = 1; break;
        case 't': break;                           /* threads of bcr: the GPU sorts */
        case 'r': max_runs = atoi(optarg); break;  /* the shape of the rope: there is none */
        case 'n': max_nodes = atoi(optarg); break;
        case 'f': break;                           /* bcr's temporary file: nothing to spill, nothing left behind */
        case 'v': verbose = atoi(optarg); break;
        case 'g': device = atoi(optarg); break;
        }
    }
    if (optind == argc) {
        fprintf(stderr, "\n");
        fprintf(stderr, "Usage:   ropebwt [options] <in.fq.gz>\n\n");
        fprintf(stderr, "Options: -a STR     algorithm: bpr or bcr [bpr]\n");
        fprintf(stderr, "         -r INT     max number of runs in leaves (bpr only) [%d]\n", max_runs);
        fprintf(stderr, "         -n INT     max number children per internal node (bpr only) [%d]\n", max_nodes);
        fprintf(stderr, "         -o FILE    output file [stdout]\n");
        fprintf(stderr, "         -f FILE    temporary sequence file name (bcr only) [null]\n");
        fprintf(stderr, "         -v INT     verbose level (bcr only) [%d]\n", verbose);
        fprintf(stderr, "         -b         binary output (5+3 runs starting after 4 bytes)\n");
        fprintf(stderr, "         -t         enable threading (bcr only)\n");
        fprintf(stderr, "         -F         skip forward strand\n");
        fprintf(stderr, "         -R         skip reverse strand\n");
        fprintf(stderr, "         -N         cut at ambiguous bases\n");
        fprintf(stderr, "         -O         suppress end trimming when forward==reverse\n");
        fprintf(stderr, "         -T         print the tree stdout (bpr only)\n\n");
        return 1;
    }
    if (tree) { fprintf(stderr, "[E::main_ropebwt] -T is not supported: the BWT is sorted on the GPU, there is no rope to print\n"); return 1; }
    if (algo == ALGO_BCR && !cut_n) fprintf(stderr, "Warning: With bcr, an ambiguous base will be converted to a random base\n");
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_ropebwt] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    io = fmdh_seq_open(argv[optind]);
    if (!io) { fprintf(stderr, "[E::main_ropebwt] fail to open file '%s'\n", argv[optind]); return 1; }
    while (rc == 0 && (l = fmdh_seq_read(io)) >= 0) {
        uint8_t *t = (uint8_t *)fmdh_seq_bases(io);
        int j;
        for (j = 0; j < l; ++j) t[j] = fmdh_nt6[t[j]];   /* (the table holds 5 from 128 on) */
        if (cut_n) {   /* cut at ambiguous bases */
            int beg = 0;
            for (j = 0; j <= l && rc == 0; ++j)
                if (j == l || t[j] == 5) {
                    if (j > beg) rc = add_piece(&q, t + beg, (uint32_t)(j - beg));
                    beg = j + 1;
                }
        } else {
            if (algo == ALGO_BCR) {
                if (l == 0) {
                    fprintf(stderr, "[E::main_ropebwt] record `%s' has no bases: -a bcr takes such a record only with -N (the reference stops at an assertion, bcr.c:361)\n",
                            fmdh_seq_name(io));
                    rc = 1;
                    break;
                }
                for (j = 0; j < l; ++j)   /* a random base for an ambiguous one; the only draws of the command */
                    if (t[j] == 5) t[j] = (uint8_t)((lrand48() & 3) + 1);
            }
            rc = add_piece(&q, t, (uint32_t)l);
        }
    }
    fmdh_seq_close(io);
    if (rc) { if (rc < 0) fprintf(stderr, "[E::main_ropebwt] out of memory\n"); free(q.bases); free(q.off); return 1; }
    t1 = now_s();
    if (verbose >= 3) fprintf(stderr, "[M::main_ropebwt] read %zu sequences, %zu bases into memory (%.3fs)\n", q.n, q.tot, t1 - t0);
    if (q.n && strands) {
        void *d_reads = 0, *d_off = 0;
        uint32_t mx = 0; int uniform = 1;
        size_t i;
        for (i = 0; i < q.n; ++i) { const uint64_t ll = q.off[i + 1] - q.off[i]; if (ll > mx) mx = (uint32_t)ll; if (ll != q.off[1] - q.off[0]) uniform = 0; }
        rc = fmd_dev_malloc(device, q.tot + 64, &d_reads);
        if (!rc) rc = fmd_dev_malloc(device, (q.n + 1) * 8, &d_off);
        if (!rc) rc = fmd_memcpy_h2d(d_reads, q.bases, q.tot, 0);
        if (!rc) rc = fmd_memcpy_h2d(d_off, q.off, (q.n + 1) * 8, 0);
        if (!rc) rc = fmd_build_bwt_strands_dev(device, 0, q.n, (const uint8_t *)d_reads, (const uint64_t *)d_off, q.tot, mx, uniform, strands, &d_bwt, &n_sym);
        fmd_dev_free(d_reads); fmd_dev_free(d_off);
        if (rc) { fprintf(stderr, "[E::main_ropebwt] BWT construction failed: %s\n", fmd_strerror(rc)); free(q.bases); free(q.off); return 1; }
    }
    free(q.bases); free(q.off);
    t2 = now_s();
    if (verbose >= 3) fprintf(stderr, "[M::main_ropebwt] BWT of %llu symbols on the GPU (%.3fs)\n", (unsigned long long)n_sym, t2 - t1);
    if (out_fn && (out = fopen(out_fn, "wb")) == 0) { fprintf(stderr, "[E::main_ropebwt] fail to write file '%s'\n", out_fn); fmd_dev_free(d_bwt); return 1; }
    if (is_bin) {
        uint8_t *rle6 = 0;
        uint64_t n_rle6 = 0;
        if (n_sym) rc = fmd_bwt_to_rle6(device, d_bwt, n_sym, &rle6, &n_rle6);
        if (!rc && (fwrite("RLE\6", 1, 4, out) != 4 || fwrite(rle6, 1, n_rle6, out) != n_rle6)) rc = FMD_E_IO;
        fmd_host_free(rle6);
    } else {
        if (n_sym) rc = write_text(d_bwt, n_sym, out);
        if (!rc && fputc('\n', out) == EOF) rc = FMD_E_IO;
    }
    fmd_dev_free(d_bwt);
    if (fflush(out) != 0 && !rc) rc = FMD_E_IO;
    if (out != stdout) fclose(out);
    if (rc) { fprintf(stderr, "[E::main_ropebwt] cannot write the BWT: %s\n", fmd_strerror(rc)); return 1; }
    if (verbose >= 3) fprintf(stderr, "[M::main_ropebwt] output written (%.3fs)\n", now_s() - t2);
    return 0;
}
