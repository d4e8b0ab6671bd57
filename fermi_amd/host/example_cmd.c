/* example_cmd.c -- `fermi example [-ceU] [-k ecKmer] [-l utgKmer] <in.fq>` (example.c): the reference's own caller of its in-memory API.
 * The reads go into one buffer (fm6_api_readseq, seq.c:385-408), are corrected there with -e (fmdh_api_correct), and are then either
 * written back (-U: fm6_api_writeseq, seq.c:410-428) or assembled into unitigs (fmdh_api_unitig); with -c the unitig graph is
 * cleaned with AGGRESSIVE | CLEAN and the other defaults before it is printed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "fmd_host.h"
#include "mag.h"

#define EXAMPLE_DEFAULT_QUAL (20 + 33)   /* seq.c:383 */
/* The step of the correction's jump heuristic.  fm6_api_correct never sets it (fmecopt_t opt on the stack, correct.c:470-479); compiled as the
 * reference's Makefile compiles it, `fermi example -e` prints what a step no shorter than the reads gives (any value from the read length up:
 * a jump then runs to the start of the read) and not what the 5 of `fermi correct` gives.  Positions in a read are 16 bits wide.
 * This is one build's answer to an undefined value, and it is tied to the two goldens that binary wrote: tests/golden/tiny.api_ec_k17.fq.gz
 * (`example -eU -k 17`) and tests/golden/clean3.example_ce_k17_l40.mag.gz (`example -ce -k 17 -l 40`).  If they are ever made again with
 * another build of the reference, this constant is what to look at. */
#define EXAMPLE_EC_STEP 0x10000

typedef struct { char *s; size_t l, m; } buf_t;
static int buf_put(buf_t *b, const char *p, size_t n)
{
    if (b->l + n > b->m) {
        size_t m = b->m ? b->m : 1 << 16;
        char *s;
        while (m < b->l + n) m <<= 1;
        if (!(s = (char *)realloc(b->s, m))) return -1;
        b->s = s; b->m = m;
    }
    memcpy(b->s + b->l, p, n); b->l += n;
    return 0;
}

int fmdh_main_example(int argc, char *argv[])
{
    int c, do_ec = 0, skip_unitig = 0, ec_k = -1, unitig_k = -1, do_clean = 0, device = 0, len, rc = 1;
    buf_t seq = {0, 0, 0}, qual = {0, 0, 0};
    fmdh_seqio_t *io;
    while ((c = getopt(argc, argv, "ceUk:l:g:")) >= 0) {
        switch (c) {
        case 'e': do_ec = 1; break;
        case 'U': skip_unitig = 1; break;
        case 'k': ec_k = atoi(optarg); break;
        case 'l': unitig_k = atoi(optarg); break;
        case 'c': do_clean = 1; break;
        case 'g': device = atoi(optarg); break;
        }
    }
    if (optind == argc) {
        fprintf(stderr, "Usage: fermi-amd example [-ceU] [-k ecKmer] [-l utgKmer] [-g GPU] <in.fq>\n");
        return 1;
    }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::%s] GPU %d: this node has %d\n", __func__, device, fmd_device_count()); return 1; }
    if (!(io = fmdh_seq_open(argv[optind]))) { fprintf(stderr, "[E::%s] cannot open `%s'\n", __func__, argv[optind]); return 1; }
    while ((len = fmdh_seq_read(io)) >= 0) {   /* every read and its qualities, a NUL after each */
        const char *q = fmdh_seq_qual(io);
        size_t at = qual.l;
        if (buf_put(&seq, fmdh_seq_bases(io), (size_t)len + 1)) goto done;
        if (q) { if (buf_put(&qual, q, (size_t)len + 1)) goto done; }
        else {
            if (buf_put(&qual, fmdh_seq_bases(io), (size_t)len + 1)) goto done;
            memset(qual.s + at, EXAMPLE_DEFAULT_QUAL, (size_t)len);
        }
    }
    fmdh_seq_close(io); io = 0;
    if (seq.l == 0) { fprintf(stderr, "[E::%s] no reads in `%s'\n", __func__, argv[optind]); goto done; }
    if (do_ec && fmdh_api_correct(device, ec_k, EXAMPLE_EC_STEP, (int64_t)seq.l, seq.s, qual.s)) goto done;
    if (skip_unitig) {
        size_t i, beg = 0;
        for (i = 0; i < seq.l; ++i) {
            if (seq.s[i]) continue;
            printf("@%ld\n", (long)i);
            fwrite(seq.s + beg, 1, i - beg, stdout); fputs("\n+\n", stdout);
            fwrite(qual.s + beg, 1, i - beg, stdout); fputc('\n', stdout);
            beg = i + 1;
        }
        rc = 0;
    } else if (!do_clean) rc = fmdh_api_unitig(device, unitig_k, (int64_t)seq.l, seq.s, stdout);
    else {
        /* the unitigs as records in memory, then the graph as fm6_api_unitig hands it over: the dictionary and nothing else */
        char *text = 0;
        size_t n_text = 0;
        FILE *mem = open_memstream(&text, &n_text);
        fmdh_magopt_t opt;
        fmdh_mag_t *g = 0;
        if (!mem) goto done;
        rc = fmdh_api_unitig(device, unitig_k, (int64_t)seq.l, seq.s, mem);
        fclose(mem);
        if (rc == 0) {
            fmdh_mag_init_opt(&opt);
            opt.flag = FMDH_MAG_F_READ_ORI | FMDH_MAG_F_NO_AMEND;
            g = fmdh_mag_read_mem(text, n_text, &opt);
            rc = 1;
        }
        if (g) {
            fmdh_mag_init_opt(&opt);
            opt.flag |= FMDH_MAG_F_AGGRESSIVE | FMDH_MAG_F_CLEAN;
            fmdh_mag_clean(g, &opt);
            if (g->err) fprintf(stderr, "[E::%s] the unitig graph is inconsistent; nothing is written\n", __func__);
            else { fmdh_mag_print(g, stdout); rc = 0; }
            fmdh_mag_destroy(g);
        }
        free(text);
    }
done:
    if (io) fmdh_seq_close(io);
    free(seq.s); free(qual.s);
    return rc;
}
