/* contrast_cmd.c -- contrast assembly: `fermi contrast` (cmd.c:589-638, cmp.c), `fermi sub` (cmd.c:640-672, sub.c) and `fermi bitand`
 * (cmd.c:717-743).  contrast: both indexes resident together, without prefix / tail tables (the walk only ranks); the GPU returns one
 * bit per sequence in sorted order (fmd_contrast), fm6_sub_conv (cmp.c:128-144) moves bit i to bit rank[i] >> 2 on the host.  sub: the
 * mark walk on the GPU (fmd_sub_mark_dev), the kept rows leave the device in slices (fmd_sub_select_dev) for the host encoder
 * (rld_writer.c).  bitand touches no GPU.  Nothing is written before the result is complete: a failure leaves no output. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "fmd_host.h"

#define SUB_SLICE (1ull << 30)   /* kept symbols per device -> host slice */

static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

static fmd_dev_t *open_input(const char *fn, int device, const char *func)
{
    fmd_dev_t *h = 0;
    const int rc = fmd_dev_open_file_ex(device, fn, FMD_OPEN_NO_TABLES, &h);
    if (rc) { fprintf(stderr, "[E::%s] Fail to open the index file `%s': %s.\n", func, fn, fmd_strerror(rc)); return 0; }
    return h;
}

static uint64_t count_bits(uint64_t n_words, const uint64_t *x)
{
    uint64_t k, c = 0;
    for (k = 0; k < n_words; ++k) c += (uint64_t)__builtin_popcountll(x[k]);
    return c;
}

/* a bit array file: its length in bits (8 bytes), then (len + 63) / 64 words.  NULL when it cannot be read in full */
static uint64_t *read_bits(const char *fn, uint64_t *len)
{
    FILE *fp = fopen(fn, "rb");
    uint64_t *a = 0, n_words;
    *len = 0;
    if (!fp) return 0;
    if (fread(len, 8, 1, fp) == 1 && *len < (1ull << 48)) {
        n_words = (*len + 63) / 64;
        a = (uint64_t *)calloc(n_words + 1, 8);
        if (a && fread(a, 8, n_words, fp) != n_words) { free(a); a = 0; }
    }
    fclose(fp);
    return a;
}

/* fm6_sub_conv (cmp.c:128-144): bit i (the i-th sequence in sorted order) -> bit rank[i] >> 2 (the sequence's number in the input); returns the number of
 * selected sequences, -1 where the reference's closing assert would fire (one strand of a read selected without the other) or the rank
 * file does not belong to the index */
static int64_t sub_conv(uint64_t n_seqs, uint64_t *sub, const uint64_t *rank)
{
    const uint64_t n_words = (n_seqs + 63) / 64;
    uint64_t i, n_sel = 0, *tmp = (uint64_t *)calloc(n_words + 1, 8);
    if (!tmp) return -1;
    for (i = 0; i < n_seqs; ++i)
        if (sub[i >> 6] >> (i & 0x3f) & 1) {
            const uint64_t k = rank[i] >> 2;
            if (k >= n_seqs) { free(tmp); return -1; }
            tmp[k >> 6] |= 1ull << (k & 0x3f);
            ++n_sel;
        }
    memcpy(sub, tmp, n_words * 8);
    free(tmp);
    for (i = 0; i + 1 < n_seqs; i += 2)
        if (((sub[i >> 6] >> (i & 0x3f)) ^ (sub[i >> 6] >> ((i ^ 1) & 0x3f))) & 1) return -1;
    return (int64_t)n_sel;
}

static int write_bits(const char *fn, uint64_t n_bits, const uint64_t *a)
{
    FILE *fp = fopen(fn, "wb");
    int ok;
    if (!fp) return -1;
    ok = fwrite(&n_bits, 8, 1, fp) == 1 && fwrite(a, 8, (n_bits + 63) / 64, fp) == (n_bits + 63) / 64;
    return (fclose(fp) == 0 && ok) ? 0 : -1;
}

/* the messages are main_contrast's (cmd.c:629), under its name.  fmd / rank / out: the two sides in argv order */
int fmdh_contrast(const char *const fmd[2], const char *const rank_fn[2], const char *const out[2], int k, int min_occ, int device)
{
    static const char *F = "main_contrast";
    const int timing = getenv("FMD_TIMING") != 0;
    fmd_dev_t *h[2] = {0, 0};
    fmd_info_t info[2];
    uint64_t *sub[2] = {0, 0}, *rank = 0;
    int i, rc, ret = 1;
    double t0 = now_s(), t1;
    if (k <= 4) { fprintf(stderr, "[E::%s] the k-mer length must be larger than 4\n", F); return 1; }   /* cmp.c:101 */
    if (min_occ < 1) { fprintf(stderr, "[E::%s] the minimum occurrence must be positive\n", F); return 1; }
    for (i = 0; i < 2; ++i) {
        if (!(h[i] = open_input(fmd[i], device, F))) goto end;
        fmd_dev_info(h[i], &info[i]);
    }
    t1 = now_s();
    rc = fmd_contrast(h[0], h[1], k, min_occ, &sub[0], &sub[1]);
    if (rc) { fprintf(stderr, "[E::%s] the walk failed on the GPU: %s\n", F, fmd_strerror(rc)); goto end; }
    if (timing) fprintf(stderr, "[M::%s] load %.3f s, walk %.3f s\n", F, t1 - t0, now_s() - t1);
    fmd_dev_close(h[0]); fmd_dev_close(h[1]); h[0] = h[1] = 0;
    for (i = 0; i < 2; ++i) {
        const uint64_t n = info[i].mcnt[1];
        FILE *fp = fopen(rank_fn[i], "rb");
        int64_t n_sel;
        rank = (uint64_t *)malloc((n + 1) * 8);
        if (!fp || !rank || fread(rank, 8, n, fp) != n) {
            fprintf(stderr, "[E::%s] cannot read %llu ranks from `%s'\n", F, (unsigned long long)n, rank_fn[i]);
            if (fp) fclose(fp);
            goto end;
        }
        fclose(fp);
        n_sel = sub_conv(n, sub[i], rank);
        free(rank); rank = 0;
        if (n_sel < 0) {
            fprintf(stderr, "[E::%s] one strand of a read of `%s' is selected without the other (or `%s' is not its rank file)\n", F, fmd[i], rank_fn[i]);
            goto end;
        }
        fprintf(stderr, "[M::%s] %ld reads selected from %s\n", F, (long)n_sel, fmd[i]);
    }
    for (i = 0; i < 2; ++i)
        if (write_bits(out[i], info[i].mcnt[1], sub[i])) { fprintf(stderr, "[E::%s] cannot write `%s'\n", F, out[i]); goto end; }
    ret = 0;
end:
    if (h[0]) fmd_dev_close(h[0]);
    if (h[1]) fmd_dev_close(h[1]);
    free(rank);
    fmd_host_free(sub[0]); fmd_host_free(sub[1]);
    return ret;
}

/* main_sub (cmd.c:640-672) */
int fmdh_sub(const char *fmd_path, const char *bits_path, int is_comp, int device, const char *out_path)
{
    static const char *F = "main_sub";
    const int timing = getenv("FMD_TIMING") != 0;
    fmd_dev_t *h = 0;
    fmd_info_t info;
    uint64_t n_seqs = 0, *sub, n_set = 0, n_out, n_words, at;
    void *d_sub = 0, *d_bits = 0, *d_work = 0, *d_slice = 0;
    uint8_t *bwt = 0;
    size_t wb;
    int rc;
    double t0 = now_s(), t_mark, t;
    if (!(sub = read_bits(bits_path, &n_seqs))) { fprintf(stderr, "[E::%s] cannot read the bit array `%s'\n", F, bits_path); return 1; }
    if (!(h = open_input(fmd_path, device, F))) { free(sub); return 1; }
    fmd_dev_info(h, &info);
    if (n_seqs != info.mcnt[1]) {
        fprintf(stderr, "[E::%s] unmatched index and the bit array\n", F);
        fmd_dev_close(h); free(sub);
        return 1;
    }
    n_words = (info.mcnt[0] + 63) / 64;
    wb = fmd_sub_work_bytes(info.mcnt[0]);
    rc = fmd_dev_malloc(info.device, (n_seqs + 63) / 64 * 8 + 8, &d_sub);
    if (!rc) rc = fmd_dev_malloc(info.device, n_words * 8 + 8, &d_bits);
    if (!rc) rc = fmd_dev_malloc(info.device, wb, &d_work);
    if (!rc) rc = fmd_memcpy_h2d(d_sub, sub, (n_seqs + 63) / 64 * 8, 0);
    if (!rc) rc = fmd_memset_dev(d_bits, 0, n_words * 8 + 8, 0);
    if (!rc) rc = fmd_sub_mark_dev(h, 0, (const uint64_t *)d_sub, (uint64_t *)d_bits, d_work, wb, (uint64_t *)d_bits + n_words);
    if (!rc) rc = fmd_memcpy_d2h(&n_set, (uint64_t *)d_bits + n_words, 8, 0);
    t_mark = now_s() - t0;
    n_out = is_comp ? info.mcnt[0] - n_set : n_set;
    if (!rc) {
        const uint64_t slice = n_out < SUB_SLICE ? n_out : SUB_SLICE;
        bwt = (uint8_t *)malloc(n_out + 1);
        if (!bwt) rc = FMD_E_NOMEM;
        if (!rc && slice) rc = fmd_dev_malloc(info.device, slice, &d_slice);
        for (at = 0; at < n_out && !rc; at += slice) {
            const uint64_t m = n_out - at < slice ? n_out - at : slice;
            rc = fmd_sub_select_dev(h, 0, (const uint64_t *)d_bits, d_work, is_comp, at, m, (uint8_t *)d_slice);
            if (!rc) rc = fmd_memcpy_d2h(bwt + at, d_slice, m, 0);
        }
    }
    fmd_dev_free(d_slice); fmd_dev_free(d_work); fmd_dev_free(d_bits); fmd_dev_free(d_sub);
    fmd_dev_close(h);
    free(sub);
    if (rc) { fprintf(stderr, "[E::%s] the selection failed on the GPU: %s\n", F, fmd_strerror(rc)); free(bwt); return 1; }
    t = now_s();
    rc = fmdh_write_rld_from_bwt(bwt, n_out, out_path);
    free(bwt);
    if (rc) { fprintf(stderr, "[E::%s] cannot write `%s'\n", F, out_path); return 1; }
    if (timing) fprintf(stderr, "[M::%s] %llu of %llu symbols kept: load + mark %.3f s, select + export %.3f s, encode %.3f s\n", F, (unsigned long long)n_out,
                        (unsigned long long)info.mcnt[0], t_mark, t - t0 - t_mark, now_s() - t);
    return 0;
}

/* main_bitand (cmd.c:717-743); a file that cannot be read is an error here, whatever the others are */
int fmdh_bitand(int n_in, char *const *in, FILE *out)
{
    uint64_t len0 = 0, *sub0 = 0, n_words = 0, k;
    int i;
    for (i = 0; i < n_in; ++i) {
        uint64_t len1, *sub1 = read_bits(in[i], &len1);
        if (!sub1) { fprintf(stderr, "[E::main_bitand] cannot read the bit array `%s'\n", in[i]); free(sub0); return 1; }
        fprintf(stderr, "[M::read_sub] loaded file `%s' containing %ld bits\n", in[i], (long)count_bits((len1 + 63) / 64, sub1));
        if (i == 0) { sub0 = sub1; len0 = len1; n_words = (len0 + 63) / 64; continue; }
        if (len1 != len0) { fprintf(stderr, "[E::main_bitand] unequal array length\n"); free(sub0); free(sub1); return 1; }
        for (k = 0; k < n_words; ++k) sub0[k] &= sub1[k];
        free(sub1);
    }
    fprintf(stderr, "[M::main_bitand] the output contains %ld bits\n", (long)count_bits(n_words, sub0));
    fwrite(&len0, 8, 1, out);
    fwrite(sub0, 8, n_words, out);
    free(sub0);
    return ferror(out) ? 1 : 0;
}
