/* readprep_cmd.c -- the read-preparation commands of fermi's driver script: `fermi fltuniq` (seq.c:122-210), `trimseq` (seq.c:289-373),
 * `pe2cofq` (seq.c:257-287), `cg2cofq` (seq.c:212-255), `splitfa` (seq.c:79-120) and `cnt2qual` (cmd.c:13-45), same argv, messages and output bytes.
 * fltuniq: the k-mer table lives on the GPU (fmd_fltuniq_*: include/fmd_hip.h); the file is read twice in batches of at most
 * fmd_fltuniq_batch_limits() bases and reads -- pass 1 counts, pass 2 tests -- and a batch is parsed while the one before it is copied and worked on.  What the host keeps
 * is two batches of bases and, in pass 2, the text of their records until their verdicts are back; the pairing machine of
 * seq.c:185-204 then runs over (name, verdict) in file order exactly as the reference runs it over the records.
 * Bytes >= 128 in a sequence: the reference indexes seq_nt6_table out of range with them (undefined); here they are non-bases.
 * The other five touch no GPU. */
#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>
#include "fmd_host.h"

static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

typedef struct { size_t l, m; char *s; } str_t;
static void str_putsn(str_t *s, const char *p, size_t n)
{
    if (s->l + n + 1 > s->m) { s->m = s->l + n + 1; s->m += s->m >> 1; s->s = (char *)realloc(s->s, s->m); }
    memcpy(s->s + s->l, p, n); s->l += n; s->s[s->l] = 0;
}
static void str_putc(str_t *s, int c) { const char x = (char)c; str_putsn(s, &x, 1); }

/* write_seq (seq.c:62-77) */
static void write_seq(str_t *out, const char *name, size_t name_l, const char *comment, const char *seq, size_t seq_l, const char *qual)
{
    str_putc(out, qual ? '@' : '>');
    str_putsn(out, name, name_l);
    if (comment && comment[0]) { str_putc(out, ' '); str_putsn(out, comment, strlen(comment)); }
    str_putc(out, '\n');
    str_putsn(out, seq, seq_l);
    if (qual) { str_putsn(out, "\n+\n", 3); str_putsn(out, qual, seq_l); }
    str_putc(out, '\n');
}
static void write_rec(str_t *out, fmdh_seqio_t *io, int len)
{
    const char *name = fmdh_seq_name(io);
    write_seq(out, name, strlen(name), fmdh_seq_comment(io), fmdh_seq_bases(io), (size_t)len, fmdh_seq_qual(io));
}

/* ---- fltuniq ---- */
int fmdh_fltuniq_auto_k(long long file_bytes) /* seq.c:147-150 */
{
    int k = file_bytes > 0 ? (int)(log((double)file_bytes) / log(4) + 1.499) : 15;
    if (k > 18) k = 18;
    if (k < 15) k = 15;
    return k;
}

/* the records of one batch of pass 2 as they would be printed, and where each starts: name '\0' text '\0' */
typedef struct { str_t txt; size_t *at, m_at; uint8_t *pass; uint64_t n; } fu_text_t;
/* the pairing machine (seq.c:185-204) between two records */
typedef struct { str_t out, prev_name; FILE *fp; uint64_t n_held, n_out; } fu_emit_t;   /* n_held: records in `out` */

static void fu_emit(fu_emit_t *e, const fu_text_t *b)
{
    uint64_t i;
    for (i = 0; i < b->n; ++i) {
        const char *name = b->txt.s + b->at[i], *text = name + strlen(name) + 1;
        const int is_paired = e->prev_name.l && strcmp(e->prev_name.s, name) == 0;
        if (is_paired) {
            if (e->out.l == 0) continue;
        } else {
            if (e->out.l) { fputs(e->out.s, e->fp); e->n_out += e->n_held; }
            e->out.l = 0; e->n_held = 0;
        }
        if (b->pass[i]) { str_putsn(&e->out, text, strlen(text)); ++e->n_held; }
        else if (is_paired) { e->out.l = 0; e->n_held = 0; }
        e->prev_name.l = 0;
        str_putsn(&e->prev_name, name, strlen(name));
    }
}

static int fu_pass(const char *fn, fmd_fltuniq_t *f, uint64_t max_bytes, uint64_t max_reads, int testing, fu_emit_t *e, uint64_t *n_rec, uint64_t *n_bases,
                   uint64_t *n_batches)
{
    fmdh_seqio_t *io = fmdh_seq_open(fn);
    fu_text_t text[2];
    uint8_t *hs = 0;
    uint64_t *ho = 0, n = 0, fill = 0;
    int len, rc = 0, cur = 1;
    memset(text, 0, sizeof(text));
    if (!io) return 1;
    if (testing) { text[0].pass = (uint8_t *)malloc(max_reads); text[1].pass = (uint8_t *)malloc(max_reads); }
    for (;;) {
        len = fmdh_seq_read(io);
        if (len < 0 || hs == 0 || n == max_reads || fill + (uint64_t)len > max_bytes) {   /* the batch is complete (or there is none yet) */
            if (hs && n) {
                ho[n] = fill;
                rc = testing ? fmd_fltuniq_test(f, n, text[cur].pass) : fmd_fltuniq_count(f, n);
                if (rc) break;
                text[cur].n = n; ++*n_batches;
            }
            if (len < 0) break;
            if ((uint64_t)len > max_bytes) { fprintf(stderr, "[E::main_fltuniq] a sequence of %d bases: longer than a batch\n", len); rc = 1; break; }
            cur ^= 1;
            if ((rc = fmd_fltuniq_slot(f, &hs, &ho)) != 0) break;      /* the slot's earlier batch is done: its verdicts are in text[cur].pass */
            if (testing) { fu_emit(e, &text[cur]); text[cur].n = 0; text[cur].txt.l = 0; }
            n = 0; fill = 0; ho[0] = 0;
        }
        {
            const unsigned char *s = (const unsigned char *)fmdh_seq_bases(io);
            int i;
            for (i = 0; i < len; ++i) hs[fill + (uint64_t)i] = fmdh_nt6[s[i]];
        }
        if (testing) {
            fu_text_t *b = &text[cur];
            const char *name = fmdh_seq_name(io);
            if (n == b->m_at) { b->m_at = b->m_at ? b->m_at << 1 : 1 << 16; b->at = (size_t *)realloc(b->at, b->m_at * sizeof(size_t)); }
            b->at[n] = b->txt.l;
            str_putsn(&b->txt, name, strlen(name) + 1);
            write_rec(&b->txt, io, len);
            str_putc(&b->txt, 0);
        }
        ho[n++] = fill; fill += (uint64_t)len;
        ++*n_rec; *n_bases += (uint64_t)len;
    }
    if (rc == 0) rc = fmd_fltuniq_sync(f, 0);
    if (rc == 0 && testing) {          /* the two batches still held, the older one first */
        fu_emit(e, &text[cur ^ 1]); fu_emit(e, &text[cur]);
        if (e->out.l) { fputs(e->out.s, e->fp); e->n_out += e->n_held; }
        e->out.l = 0; e->n_held = 0;
    }
    if (rc > 1 || rc < 0) fprintf(stderr, "[E::main_fltuniq] %s\n", fmd_strerror(rc));
    fmdh_seq_close(io);
    free(text[0].txt.s); free(text[1].txt.s); free(text[0].at); free(text[1].at); free(text[0].pass); free(text[1].pass);
    return rc != 0;
}

int fmdh_main_fltuniq(int argc, char *argv[])
{
    int c, k = 0, device = 0, rc;
    const int timing = getenv("FMD_TIMING") != 0;
    fmd_fltuniq_t *f = 0;
    fu_emit_t e;
    uint64_t n_rec[2] = {0, 0}, n_bases[2] = {0, 0}, n_batches[2] = {0, 0}, max_bytes, max_reads;
    double t0 = now_s(), t1, t2, ms[2] = {0, 0};
    while ((c = getopt(argc, argv, "k:g:")) >= 0) {
        switch (c) {
        case 'k': k = atoi(optarg); break;
        case 'g': device = atoi(optarg); break;
        }
    }
    if (optind == argc) {
        fprintf(stderr, "Usage: fermi-amd fltuniq [-k INT] [-g GPU] <in.fa>\n");
        return 1;
    }
    if (k == 0) { /* the k-mer length from the size of the input file as it lies on disk */
        FILE *fp;
        long size;
        if ((fp = fopen(argv[optind], "rb")) == 0) {
            fprintf(stderr, "[E::main_fltuniq] fail to open the input file\n");
            return 1;
        }
        fseek(fp, 0, SEEK_END);
        size = ftell(fp);
        fclose(fp);
        k = fmdh_fltuniq_auto_k(size);
        fprintf(stderr, "[M::main_fltuniq] set the k-mer size as %d\n", k);
    }
    {
        gzFile fp = gzopen(argv[optind], "r");
        if (fp == 0) {
            fprintf(stderr, "[E::main_fltuniq] fail to open file '%s'\n", argv[optind]);
            return 1;
        }
        gzclose(fp);
    }
    if (fmd_fltuniq_table_bytes(k) == 0) {
        fprintf(stderr, "[E::main_fltuniq] -k %d: the k-mer size must be between 3 and 20\n", k);
        return 1;
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_fltuniq] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    fmd_fltuniq_batch_limits(&max_bytes, &max_reads);
    rc = fmd_fltuniq_open(device, k, max_bytes, max_reads, &f);
    if (rc) {
        fprintf(stderr, "[E::main_fltuniq] a table of %.1f GB for k = %d: %s\n", (double)fmd_fltuniq_table_bytes(k) / 1e9, k, fmd_strerror(rc));
        return 1;
    }
    memset(&e, 0, sizeof(e));
    e.fp = stdout;
    fprintf(stderr, "[M::main_fltuniq] building the hash table...\n");
    rc = fu_pass(argv[optind], f, max_bytes, max_reads, 0, &e, &n_rec[0], &n_bases[0], &n_batches[0]);
    t1 = now_s();
    if (rc == 0) {
        fprintf(stderr, "[M::main_fltuniq] filtering the reads...\n");
        rc = fu_pass(argv[optind], f, max_bytes, max_reads, 1, &e, &n_rec[1], &n_bases[1], &n_batches[1]);
    }
    t2 = now_s();
    if (rc == 0) fmd_fltuniq_sync(f, ms);
    fmd_fltuniq_close(f);
    free(e.out.s); free(e.prev_name.s);
    if (timing && rc == 0) {
        fprintf(stderr, "[M::main_fltuniq] k = %d, table %.3f GB; %llu records, %llu bases; kept %llu records\n", k, (double)fmd_fltuniq_table_bytes(k) / 1e9,
                (unsigned long long)n_rec[0], (unsigned long long)n_bases[0], (unsigned long long)e.n_out);
        fprintf(stderr, "[M::main_fltuniq] pass 1: %.3f s (count kernels %.3f s); pass 2: %.3f s (test kernels %.3f s)\n", t1 - t0, ms[0] * 1e-3, t2 - t1, ms[1] * 1e-3);
        fprintf(stderr, "[M::main_fltuniq] batches: %llu in pass 1, %llu in pass 2\n", (unsigned long long)n_batches[0], (unsigned long long)n_batches[1]);
    }
    return rc;
}

/* ---- trimseq ---- */
int fmdh_main_trimseq(int argc, char *argv[])
{
    int c, min_l = 20, min_q = 3, drop_ambi = 1, len;
    fmdh_seqio_t *io;
    str_t prev_name = {0, 0, 0}, str = {0, 0, 0};
    while ((c = getopt(argc, argv, "q:Nl:")) >= 0) {
        switch (c) {
        case 'q': min_q = atoi(optarg); break;
        case 'l': min_l = atoi(optarg); break;
        case 'N': drop_ambi = 0; break;
        }
    }
    if (argc == optind) {
        fprintf(stderr, "Usage: fermi-amd trimseq [-N] [-q qual=%d] [-l minLen=%d] <in.fq>\n", min_q, min_l);
        return 1;
    }
    io = fmdh_seq_open(argv[optind]);
    if (!io) { fprintf(stderr, "[E::main_trimseq] fail to open file '%s'\n", argv[optind]); return 1; }
    while ((len = fmdh_seq_read(io)) >= 0) {
        const char *name = fmdh_seq_name(io), *seq = fmdh_seq_bases(io), *qual = fmdh_seq_qual(io);
        const size_t name_l = strlen(name);
        int i, is_paired = 0, left, right, drop = 0;
        if (name_l == prev_name.l && prev_name.l) { /* test pairing */
            if (strncmp(name, prev_name.s, name_l - 1) == 0) {
                const int c2 = name[prev_name.l - 1], c1 = prev_name.s[prev_name.l - 1];
                if (c1 == c2) is_paired = 1;
                else if (prev_name.l >= 2 && prev_name.s[prev_name.l - 2] == '/') {
                    if (isdigit(c1) && isdigit(c2)) is_paired = 1;
                }
            }
        }
        if (is_paired) {
            if (str.l == 0) continue; /* the mate was dropped: so is this one */
        } else { /* output the previous sequence(s) */
            if (str.l) fputs(str.s, stdout);
            str.l = 0;
        }
        left = 0; right = len;
        if (min_q > 0 && qual) { /* trim */
            int s, max, max_i;
            for (i = right - 1, max = s = 0, max_i = right; i >= left; --i) { /* from the 3'-end */
                s += min_q - (qual[i] - 33);
                if (s < 0) break;
                if (max < s) max = s, max_i = i;
            }
            right = max_i;
            for (i = 0, max = s = 0, max_i = -1; i < right; ++i) { /* from the 5'-end */
                s += min_q - (qual[i] - 33);
                if (s < 0) break;
                if (max < s) max = s, max_i = i;
            }
            left = max_i + 1;
            if (right - left < min_l) drop = 1;
        }
        if (!drop && drop_ambi) {
            for (i = left; i < right; ++i)
                if (fmdh_nt6[(unsigned char)seq[i]] >= 5) break;
            if (i != right) drop = 1;
        }
        if (!drop) write_seq(&str, name, name_l, fmdh_seq_comment(io), seq + left, (size_t)(right - left), qual ? qual + left : 0);
        else if (is_paired) str.l = 0;
        prev_name.l = 0;
        str_putsn(&prev_name, name, name_l);
    }
    if (str.l) fputs(str.s, stdout);
    fmdh_seq_close(io);
    free(str.s); free(prev_name.s);
    return 0;
}

/* ---- pe2cofq ---- */
int fmdh_main_pe2cofq(int argc, char *argv[])
{
    fmdh_seqio_t *io[2];
    str_t str = {0, 0, 0};
    int len[2];
    if (argc < 3) {
        fprintf(stderr, "Usage: fermi-amd pe2cofq <in1.fq> <in2.fq>\n");
        return 1;
    }
    io[0] = fmdh_seq_open(argv[1]);
    io[1] = fmdh_seq_open(argv[2]);
    if (!io[0] || !io[1]) { fprintf(stderr, "[E::main_pe2cofq] fail to open file '%s'\n", argv[io[0] ? 2 : 1]); fmdh_seq_close(io[0]); fmdh_seq_close(io[1]); return 1; }
    while ((len[0] = fmdh_seq_read(io[0])) >= 0) {
        const char *name = fmdh_seq_name(io[0]);
        size_t name_l = strlen(name);
        if ((len[1] = fmdh_seq_read(io[1])) < 0) break; /* one file ends */
        str.l = 0;
        if (name_l > 2 && name[name_l - 2] == '/' && isdigit((unsigned char)name[name_l - 1])) name_l -= 2; /* trim tailing "/[0-9]$" */
        write_seq(&str, name, name_l, fmdh_seq_comment(io[0]), fmdh_seq_bases(io[0]), (size_t)len[0], fmdh_seq_qual(io[0]));
        write_seq(&str, name, name_l, fmdh_seq_comment(io[1]), fmdh_seq_bases(io[1]), (size_t)len[1], fmdh_seq_qual(io[1])); /* both ends under one name */
        fputs(str.s, stdout);
    }
    fmdh_seq_close(io[0]); fmdh_seq_close(io[1]);
    free(str.s);
    return 0;
}

/* ---- cg2cofq ---- */
/* A record whose sequence is two runs of letters with something else between them -- the two arms of a pair in one line -- becomes two records
 * under the one name (no comment): the letters up to the first other character, then everything from the next letter on, each with its part of
 * the quality.  A record without a second run of letters gives the first record alone: the reference's scan for the second run has no
 * end (seq.c:238 tests the length, not the index) and reads past the sequence there. */
int fmdh_main_cg2cofq(int argc, char *argv[])
{
    fmdh_seqio_t *io;
    str_t str = {0, 0, 0};
    int len;
    if (argc == 1) {
        fprintf(stderr, "Usage: fermi-amd cg2cofq <in.cgfq>\n");
        return 1;
    }
    io = fmdh_seq_open(argv[1]);
    if (!io) { fprintf(stderr, "[E::main_cg2cofq] fail to open file '%s'\n", argv[1]); return 1; }
    while ((len = fmdh_seq_read(io)) >= 0) {
        const char *name = fmdh_seq_name(io), *seq = fmdh_seq_bases(io), *qual = fmdh_seq_qual(io);
        int i, j;
        str.l = 0;
        for (i = 0; i < len; ++i)
            if (!isalpha((unsigned char)seq[i])) break;
        write_seq(&str, name, strlen(name), 0, seq, (size_t)i, qual);
        for (j = i; j < len; ++j)
            if (isalpha((unsigned char)seq[j])) break;
        if (j < len) write_seq(&str, name, strlen(name), 0, seq + j, (size_t)(len - j), qual ? qual + j : 0);
        fputs(str.s, stdout);
    }
    fmdh_seq_close(io);
    free(str.s);
    return 0;
}

/* ---- splitfa ---- */
int fmdh_main_splitfa(int argc, char *argv[])
{
    int64_t n_seqs = 0;
    int i, n_files = 8, len;
    gzFile *out;
    fmdh_seqio_t *io;
    char *fn;
    str_t *ss;
    if (argc < 3) {
        fprintf(stderr, "Usage: fermi-amd splitfa <in.fq> <out.prefix> [%d]\n", n_files);
        return 1;
    }
    if (argc >= 4) n_files = atoi(argv[3]);
    if (n_files < 1) { fprintf(stderr, "[E::main_splitfa] the number of files must be positive\n"); return 1; }
    io = fmdh_seq_open(argv[1]);
    if (!io) { fprintf(stderr, "[E::main_splitfa] fail to open file '%s'\n", argv[1]); return 1; }
    out = (gzFile *)calloc((size_t)n_files, sizeof(gzFile));
    fn = (char *)calloc(strlen(argv[2]) + 20, 1);
    ss = (str_t *)calloc((size_t)n_files, sizeof(str_t));
    for (i = 0; i < n_files; ++i) {
        sprintf(fn, "%s.%.4d.fq.gz", argv[2], i);
        out[i] = gzopen(fn, "wb1");
        if (!out[i]) { fprintf(stderr, "[E::main_splitfa] fail to write file '%s'\n", fn); return 1; }
    }
    while ((len = fmdh_seq_read(io)) >= 0) {
        i = (int)((n_seqs >> 1) % n_files); /* a pair stays in one file */
        write_rec(&ss[i], io, len);
        if (ss[i].l > 64000) {
            gzwrite(out[i], ss[i].s, (unsigned)ss[i].l);
            ss[i].l = 0;
        }
        ++n_seqs;
    }
    for (i = 0; i < n_files; ++i) {
        if (ss[i].l) gzwrite(out[i], ss[i].s, (unsigned)ss[i].l);
        gzclose(out[i]);
        free(ss[i].s);
    }
    free(out); free(ss); free(fn);
    fmdh_seq_close(io);
    return 0;
}

/* ---- cnt2qual ---- */
int fmdh_main_cnt2qual(int argc, char *argv[])
{
    int q = 17, i, len;
    fmdh_seqio_t *io;
    if (argc < 2) {
        fprintf(stderr, "Usage: fermi-amd cnt2qual <in.fq> [%d]\n", q);
        return 1;
    }
    if (argc >= 3) q = atoi(argv[2]);
    io = fmdh_seq_open(argv[1]);
    if (!io) { fprintf(stderr, "[E::main_cnt2qual] fail to open file '%s'\n", argv[1]); return 1; }
    while ((len = fmdh_seq_read(io)) >= 0) {
        char *qual = fmdh_seq_qual(io);
        const char *comment = fmdh_seq_comment(io);
        if (qual) {
            for (i = 0; i < len; ++i) {
                const int x = q * (qual[i] - 33) + 33;
                qual[i] = (char)(x > 126 ? 126 : x);
            }
        }
        putchar('@'); fputs(fmdh_seq_name(io), stdout);
        if (comment) {
            putchar('\t'); puts(comment);   /* a TAB here, where write_seq puts a space */
        } else putchar('\n');
        puts(fmdh_seq_bases(io));
        if (qual) {
            putchar('+'); putchar('\n');
            puts(qual);
        }
    }
    fmdh_seq_close(io);
    return 0;
}
