/* merge_cmd.c -- index algebra on the GPU: `fermi merge [-f] [-o out] [-t N] in0.fmd in1.fmd [...]` (cmd.c:335-376, fm_merge
 * merge.c:100-134), `fermi recode in.fmd` (cmd.c:674-685) and the append behind `fermi build -i FILE` (cmd.c:390-397).
 * The inputs are opened without their prefix and tail tables (fmd_dev_open_file_ex): a merge only ranks and decodes them.
 * Every merge but the last keeps its result resident, without tables (fmd_dev_merge_ex); the last one walks (fmd_merge_walk_dev) and its merged
 * BWT leaves the device in slices (fmd_merge_interleave_dev) for the host encoder (rld_writer.c), so that the device never
 * holds both inputs and a merged index at once.  Nothing is written before the merged BWT is complete on the host: a
 * failure before the write leaves no output file.  The encoder writes asize 6 / sbits 3, the only header
 * fmd_dev_open_file accepts, so the first input's header -- which fm_merge keeps -- is always reproduced. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "fmd_host.h"

#define MERGE_SLICE (1ull << 30)   /* merged symbols per device -> host slice */

static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

int fmdh_merge_pair_to_file(fmd_dev_t *h0, fmd_dev_t *h1, const char *out_path)
{
    const int timing = getenv("FMD_TIMING") != 0;
    fmd_info_t i0, i1;
    void *d_bits = 0, *d_work = 0, *d_slice = 0;
    uint8_t *bwt = 0;
    int rc, walked = 1;
    double t0 = now_s(), t_walk = 0, t_il = 0, t_ex = 0, t_enc = 0, t;
    fmd_dev_info(h0, &i0); fmd_dev_info(h1, &i1);
    const uint64_t n_tot = i0.mcnt[0] + i1.mcnt[0], n_words = (n_tot + 63) / 64;
    const uint64_t slice = n_tot < MERGE_SLICE ? n_tot : MERGE_SLICE;
    const size_t wb = fmd_merge_work_bytes(n_tot);
    bwt = (uint8_t *)malloc(n_tot + 1);
    rc = bwt ? FMD_OK : FMD_E_NOMEM;
    if (!rc) rc = fmd_dev_malloc(i0.device, n_words * 8, &d_bits);
    if (!rc) rc = fmd_dev_malloc(i0.device, wb, &d_work);
    if (!rc) rc = fmd_dev_malloc(i0.device, slice, &d_slice);
    if (!rc) rc = fmd_memset_dev(d_bits, 0, n_words * 8, 0);
    if (!rc) rc = fmd_merge_walk_dev(h0, h1, 0, (uint64_t *)d_bits, d_work, wb, &walked);
    if (!rc) rc = fmd_dev_sync(h0, 0);
    t = now_s(); t_walk = t - t0;
    for (uint64_t at = 0; at < n_tot && !rc; at += slice) {
        const uint64_t m = n_tot - at < slice ? n_tot - at : slice;
        double t1;
        rc = fmd_merge_interleave_dev(h0, h1, 0, (const uint64_t *)d_bits, d_work, at, m, (uint8_t *)d_slice);
        if (!rc) rc = fmd_dev_sync(h0, 0);
        t1 = now_s(); t_il += t1 - t; t = t1;
        if (!rc) rc = fmd_memcpy_d2h(bwt + at, d_slice, m, 0);
        t1 = now_s(); t_ex += t1 - t; t = t1;
    }
    fmd_dev_free(d_slice); fmd_dev_free(d_work); fmd_dev_free(d_bits);
    fmd_dev_close(h0); fmd_dev_close(h1);
    if (rc) {
        fprintf(stderr, "[E::%s] the merge failed on the GPU: %s\n", __func__, fmd_strerror(rc));
        free(bwt);
        return 1;
    }
    t = now_s();
    rc = fmdh_write_rld_from_bwt(bwt, n_tot, out_path);
    t_enc = now_s() - t;
    free(bwt);
    if (rc) { fprintf(stderr, "[E::%s] cannot write `%s'\n", __func__, out_path); return 1; }
    if (timing)
        fprintf(stderr, "[M::%s] %llu + %llu symbols (walked index %d): walk %.3f s, interleave %.3f s, export %.3f s, encode %.3f s\n", __func__,
                (unsigned long long)i0.mcnt[0], (unsigned long long)i1.mcnt[0], walked, t_walk, t_il, t_ex, t_enc);
    return 0;
}

/* `-`: the index from stdin (rld_restore_header, rld.c:273), as the driver's `ropebwt ... | recode -` would hand it over: all of it read
 * into memory, then the container's payload (header as rld.c:242-263) or the run bytes behind a 4-byte magic (rld.c:295-308) */
static int open_stdin(int device, fmd_dev_t **h)
{
    size_t n = 0, m = 1 << 20, k;
    uint8_t *buf = (uint8_t *)malloc(m);
    int rc;
    while (buf && (k = fread(buf + n, 1, m - n, stdin)) > 0)
        if ((n += k) == m) buf = (uint8_t *)realloc(buf, m <<= 1);
    if (!buf) return FMD_E_NOMEM;
    if (n <= 4) rc = FMD_E_FORMAT;
    else if (memcmp(buf, "RLD\2", 4) == 0) {
        uint32_t a = 0; uint64_t hdr[3] = {0, 0, 0}, mcnt[7];
        if (n >= 80) { memcpy(&a, buf + 4, 4); memcpy(hdr, buf + 8, 24); memcpy(mcnt + 1, buf + 32, 48); }
        if (n < 80 || (a >> 16) != 6 || (a & 0xffff) != 3 || (hdr[1] & 7) || hdr[1] > n - 80) rc = FMD_E_FORMAT;
        else {
            int j;
            for (mcnt[0] = 0, j = 1; j < 7; ++j) mcnt[0] += mcnt[j];
            rc = fmd_dev_open_rld(device, (const uint64_t *)(buf + 80), hdr[1] / 8, mcnt, h);   /* (a malloc'ed block + 80: aligned) */
        }
    } else rc = fmd_dev_open_rle6(device, buf + 4, n - 4, h);
    free(buf);
    return rc;
}

static fmd_dev_t *open_input(const char *fn, int device, const char *func)
{
    fmd_dev_t *h = 0;
    const int rc = strcmp(fn, "-") ? fmd_dev_open_file_ex(device, fn, FMD_OPEN_NO_TABLES, &h) : open_stdin(device, &h);
    if (rc) { fprintf(stderr, "[E::%s] Fail to open the index file `%s': %s.\n", func, fn, fmd_strerror(rc)); return 0; }
    return h;
}

/* the messages are main_merge's (cmd.c:360-371), under its name */
int fmdh_merge(int n_in, char *const *in, const char *out_path, int device)
{
    static const char *F = "main_merge";
    const int timing = getenv("FMD_TIMING") != 0;
    double t = now_s();
    fmd_dev_t *cur, *nxt, *m;
    int j, rc;
    if (n_in < 2) return 1;
    if (!(cur = open_input(in[0], device, F))) return 1;
    fprintf(stderr, "[M::%s] Loaded file `%s'.\n", F, in[0]);
    for (j = 1; j < n_in; ++j) {
        if (!(nxt = open_input(in[j], device, F))) { fmd_dev_close(cur); return 1; }
        fprintf(stderr, "[M::%s] Loaded file `%s'.\n", F, in[j]);
        if (timing) fprintf(stderr, "[M::%s] load %.3f s\n", F, now_s() - t);
        if (j + 1 == n_in) {
            if (fmdh_merge_pair_to_file(cur, nxt, out_path)) return 1;
            fprintf(stderr, "[M::%s] Merged file `%s' to the existing index.\n", F, in[j]);
            return 0;
        }
        t = now_s();
        rc = fmd_dev_merge_ex(cur, nxt, FMD_OPEN_NO_TABLES, &m);   /* only merged again: no prefix / tail table */
        fmd_dev_close(cur); fmd_dev_close(nxt);
        if (rc) { fprintf(stderr, "[E::%s] the merge failed on the GPU: %s\n", F, fmd_strerror(rc)); return 1; }
        fprintf(stderr, "[M::%s] Merged file `%s' to the existing index.\n", F, in[j]);
        if (timing) fprintf(stderr, "[M::%s] resident merge %.3f s\n", F, now_s() - t);
        cur = m;
        t = now_s();
    }
    return 1;
}

int fmdh_recode(const char *in, int device, const char *out_path)
{
    fmd_dev_t *h = open_input(in, device, __func__);
    fmd_info_t info;
    uint8_t *bwt;
    int rc = FMD_OK;
    if (!h) return 1;
    fmd_dev_info(h, &info);
    bwt = (uint8_t *)malloc(info.mcnt[0] + 1);
    if (!bwt) rc = FMD_E_NOMEM;
    for (uint64_t at = 0; at < info.mcnt[0] && !rc; at += MERGE_SLICE) {
        const uint64_t m = info.mcnt[0] - at < MERGE_SLICE ? info.mcnt[0] - at : MERGE_SLICE;
        rc = fmd_dev_export_bwt(h, at, m, bwt + at);
    }
    fmd_dev_close(h);
    if (rc) { fprintf(stderr, "[E::%s] %s\n", __func__, fmd_strerror(rc)); free(bwt); return 1; }
    rc = fmdh_write_rld_from_bwt(bwt, info.mcnt[0], out_path);
    free(bwt);
    if (rc) { fprintf(stderr, "[E::%s] cannot write `%s'\n", __func__, out_path); return 1; }
    return 0;
}
