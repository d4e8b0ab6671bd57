#define _GNU_SOURCE
/* esearch_cmd.c -- `fermi-amd esearch [-g GPU] [-e 1] [-b] [-m 1000] [-l] [-M 1000] [-r reads.rank] <reads.fmd> <query.fa>`: the patterns within -e
 * edits (substitutions, insertions and deletions) of every query that occur in the indexed reads (fmd_esearch_batch), and with -l the reads that hold
 * each of them (fmd_locate_batch + fmdh_locate_hits, as `locate` does for an exact match).  The reference has no such command.  Per query, in input
 * order:
 *     SQ <tab> name <tab> length <tab> n_hits <tab> n_occ <tab> listed(1/0) <tab> h0,h1,..,he     h_j = hits at distance j; listed = 0: more than -m hits, none listed
 *     EH <tab> n_edit <tab> pattern <tab> count <tab> cigar                                     by (n_edit, SA interval, length); cigar: fmdh_esearch_cigar
 *     OC <tab> read <tab> +|- <tab> offset                                                      with -l, after each EH, as `locate` prints them (none above -M occurrences)
 *     //
 * A hit carries the SA interval and the length of its pattern, not the pattern: fmdh_esearch_patterns reads it back from the index, for the listed
 * hits only.  Usage and unreadable-file errors return 1 before the device is looked for. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "fmd_host.h"

#define ESEARCH_BATCH 65536
#define ESEARCH_PAT_BATCH 65536

/* ---- one optimal alignment of a pattern to its query ---------------------------------------------------------------------------------------------
 * Unit costs; a base equals another only if both are the same of A/C/G/T.  The table T[r][c] = ed(pat[0 .. r), query[0 .. c)) is kept in a band of
 * |c - r| <= k, k doubled until the distance fits it (Ukkonen), so time and memory are O(plen * distance).  The alignment is traced back from the END
 * of both strings, and among the moves that keep the cost optimal the FIRST of: '=' / 'X' (diagonal), 'I' (the query base is absent from the pattern),
 * 'D' (the pattern base is absent from the query) -- so a gap in a run of equal bases comes out at the run's left end.  The operations are written
 * from the start of the strings, run-length encoded: 12=1X7=1I5=. */
char *fmdh_esearch_cigar(const uint8_t *query, uint32_t qlen, const uint8_t *pat, uint32_t plen, uint32_t *n_edit)
{
    const uint32_t longer = qlen > plen ? qlen : plen, INF = 0xffffffffu;
    uint32_t k = qlen > plen ? qlen - plen : plen - qlen, *T = 0, dist = 0;
    size_t w = 0;
    if (k < 4) k = 4;
    for (;;) {
        if (k > longer) k = longer;
        w = 2 * (size_t)k + 1;
        free(T);
        if (!(T = (uint32_t *)malloc(((size_t)plen + 1) * w * sizeof(uint32_t)))) return 0;
#define CELL(r, c) (((int64_t)(c) - (int64_t)(r) + (int64_t)k) < 0 || ((int64_t)(c) - (int64_t)(r) + (int64_t)k) >= (int64_t)w ? INF : T[(size_t)(r) * w + (size_t)((int64_t)(c) - (int64_t)(r) + (int64_t)k)])
        for (uint32_t r = 0; r <= plen; ++r) {
            const uint32_t c0 = r > k ? r - k : 0, c1 = r + k < qlen ? r + k : qlen;
            for (uint32_t j = 0; j < w; ++j) T[(size_t)r * w + j] = INF;
            for (uint32_t c = c0; c <= c1; ++c) {
                uint32_t v = INF, x;
                if (r == 0) v = c;
                else if (c == 0) v = r;
                else {
                    const int eq = pat[r - 1] == query[c - 1] && pat[r - 1] >= 1 && pat[r - 1] <= 4;
                    if ((x = CELL(r - 1, c - 1)) != INF) v = x + !eq;
                    if ((x = CELL(r, c - 1)) != INF && x + 1 < v) v = x + 1;
                    if ((x = CELL(r - 1, c)) != INF && x + 1 < v) v = x + 1;
                }
                T[(size_t)r * w + (c - r + k)] = v;
            }
        }
        dist = CELL(plen, qlen);
        if (dist <= k || k >= longer) break;
        k *= 2;
    }
    /* trace back: the operations in reverse */
    char *ops = (char *)malloc((size_t)qlen + plen + 1), *out = 0;
    size_t n_ops = 0;
    if (ops) {
        uint32_t r = plen, c = qlen;
        while (r || c) {
            const uint32_t v = CELL(r, c);
            if (r && c) {
                const int eq = pat[r - 1] == query[c - 1] && pat[r - 1] >= 1 && pat[r - 1] <= 4;
                const uint32_t x = CELL(r - 1, c - 1);
                if (x != INF && x + !eq == v) { ops[n_ops++] = eq ? '=' : 'X'; --r; --c; continue; }
            }
            if (c) {
                const uint32_t x = CELL(r, c - 1);
                if (x != INF && x + 1 == v) { ops[n_ops++] = 'I'; --c; continue; }
            }
            ops[n_ops++] = 'D'; --r;
        }
        if ((out = (char *)malloc(n_ops * 2 + 16)) != 0) {       /* a run takes at most as many characters as two of its operations, 1= included */
            size_t o = 0;
            for (size_t i = n_ops; i > 0;) {
                size_t j = i;
                while (j > 0 && ops[j - 1] == ops[i - 1]) --j;
                o += (size_t)sprintf(out + o, "%zu%c", i - j, ops[i - 1]);
                i = j;
            }
            out[o] = 0;
        }
    }
#undef CELL
    free(ops); free(T);
    if (out && n_edit) *n_edit = dist;
    return out;
}

/* ---- the patterns of hits, read back from the index ------------------------------------------------------------------------------------------------
 * The pattern of a hit is the first len symbols of the suffix of row beg.  The LF-walk from row beg (fmd_retrieve_batch) ends on the sentinel rank of
 * the sequence that holds that suffix after as many steps as bases stand before it; the walk from row i < n_seq gives sequence i whole, as `unpack`
 * reads it, and ITS sentinel rank: fmdh_esearch_rankmap inverts that (row_of[rank] = i; one walk over every sequence, 4 bytes kept of each). */
int fmdh_esearch_rankmap(fmd_dev_t *d, uint64_t **row_of_out, uint64_t *n_seq_out)
{
    fmd_info_t info;
    fmd_dev_info(d, &info);
    const uint64_t n_seq = info.mcnt[1], batch = 1u << 20;
    const size_t m = (size_t)(n_seq < batch ? n_seq : batch) + 1;
    uint64_t *row_of = (uint64_t *)malloc((size_t)(n_seq ? n_seq : 1) * 8), *x = (uint64_t *)malloc(m * 8), *rank = (uint64_t *)malloc(m * 8);
    uint32_t *len = (uint32_t *)malloc(m * 4);
    uint8_t *seq = (uint8_t *)malloc(m * 4);
    int rc = !row_of || !x || !rank || !len || !seq;
    for (uint64_t i = 0; i < n_seq && !rc; ++i) row_of[i] = ~0ull;
    for (uint64_t o = 0; o < n_seq && !rc; o += batch) {
        const uint64_t n = n_seq - o < batch ? n_seq - o : batch;
        for (uint64_t i = 0; i < n; ++i) x[i] = o + i;
        if (fmd_retrieve_batch(d, n, x, seq, 4, len, rank)) { rc = 1; break; }
        for (uint64_t i = 0; i < n; ++i) { if (rank[i] >= n_seq || row_of[rank[i]] != ~0ull) { rc = 1; break; } row_of[rank[i]] = o + i; }
    }
    free(x); free(rank); free(len); free(seq);
    if (rc) { free(row_of); return 1; }
    *row_of_out = row_of; *n_seq_out = n_seq;
    return 0;
}

/* pats[pat_off[j] .. pat_off[j] + hits[j].len) = the pattern of hit j in nt6; pat_off[j + 1] >= pat_off[j] + hits[j].len.  1: a row that is not in the
 * index, a sequence that ends before len bases, a symbol that is no base, a device error or no memory. */
int fmdh_esearch_patterns(fmd_dev_t *d, const uint64_t *row_of, uint64_t n_seq, size_t n, const fmd_esearch_hit_t *hits, const uint64_t *pat_off, uint8_t *pats)
{
    const size_t m = (n < ESEARCH_PAT_BATCH ? n : ESEARCH_PAT_BATCH) + 1;
    uint64_t *x = (uint64_t *)malloc(m * 8), *rank = (uint64_t *)malloc(m * 8);
    uint32_t *at = (uint32_t *)malloc(m * 4), *len = (uint32_t *)malloc(m * 4), stride = 256;
    uint8_t *seq = 0, *tmp = (uint8_t *)malloc(m * 4);
    int rc = !x || !rank || !at || !len || !tmp || !d || (n && (!row_of || !hits || !pat_off || !pats));
    for (size_t o = 0; o < n && !rc; o += ESEARCH_PAT_BATCH) {
        const size_t b = n - o < ESEARCH_PAT_BATCH ? n - o : ESEARCH_PAT_BATCH;
        for (size_t j = 0; j < b; ++j) x[j] = hits[o + j].beg;
        if (fmd_retrieve_batch(d, b, x, tmp, 4, at, rank)) { rc = 1; break; }      /* at = the bases before the pattern */
        for (size_t j = 0; j < b && !rc; ++j) { if (rank[j] >= n_seq || row_of[rank[j]] >= n_seq) rc = 1; else x[j] = row_of[rank[j]]; }
        while (!rc) {                                                              /* a sequence longer than the stride: run the batch again with room for it */
            uint32_t mx = 0;
            free(seq);
            if (!(seq = (uint8_t *)malloc(b * (size_t)stride)) || fmd_retrieve_batch(d, b, x, seq, stride, len, rank)) { rc = 1; break; }
            for (size_t j = 0; j < b; ++j) if (len[j] > mx) mx = len[j];
            if (mx <= stride) break;
            while (stride < mx) stride *= 2;
        }
        for (size_t j = 0; j < b && !rc; ++j) {                                     /* the walk gives the sequence reversed */
            const uint8_t *s = seq + j * (size_t)stride;
            const uint32_t pl = hits[o + j].len;
            if ((uint64_t)at[j] + pl > len[j]) { rc = 1; break; }
            for (uint32_t i = 0; i < pl; ++i) {
                const uint8_t c = s[len[j] - 1 - (at[j] + i)];
                if (c < 1 || c > 4) rc = 1;
                pats[pat_off[o + j] + i] = c;
            }
        }
    }
    free(x); free(rank); free(at); free(len); free(seq); free(tmp);
    return rc;
}

typedef struct {
    int max_edit, locate;
    uint32_t max_hits, max_occ;
    unsigned flags;
    const uint64_t *sorted;
    uint64_t n_seq, *row_of;        /* row_of: made when the first hit is listed */
} esearch_opt_t;

static int flush_batch(fmd_dev_t *d, esearch_opt_t *o, size_t n, char **names, const uint8_t *bases, const uint64_t *off, FILE *out)
{
    const size_t cols = (size_t)o->max_edit + 1;
    uint64_t *strata = (uint64_t *)calloc(n * cols * 2, 8), n_hits = 0, n_runs = 0, n_oc = 0, k = 0, oc = 0, *pat_off = 0;
    fmd_esearch_hit_t *hits = 0;
    fmd_esearch_stat_t st;
    fmd_locate_run_t *runs = 0;
    fmd_locate_stat_t lst;
    fmdh_locate_hit_t *ocs = 0;
    uint8_t *pats = 0;
    int rc = 1;
    if (!strata) { fprintf(stderr, "[E::main_esearch] out of memory\n"); return 1; }
    const int e = fmd_esearch_batch(d, n, bases, off, o->max_edit, o->max_hits, o->flags, 0, &hits, &n_hits, strata, &st);
    if (e) { fprintf(stderr, "[E::main_esearch] %s\n", fmd_strerror(e)); goto done; }
    if (n_hits) {
        uint64_t n_seq = 0;
        if (!o->row_of && fmdh_esearch_rankmap(d, &o->row_of, &n_seq)) { fprintf(stderr, "[E::main_esearch] cannot walk the sequences of the index\n"); goto done; }
        if (!(pat_off = (uint64_t *)malloc((n_hits + 1) * 8))) { fprintf(stderr, "[E::main_esearch] out of memory\n"); goto done; }
        pat_off[0] = 0;
        for (uint64_t j = 0; j < n_hits; ++j) pat_off[j + 1] = pat_off[j] + hits[j].len;
        if (!(pats = (uint8_t *)malloc(pat_off[n_hits] + 1))) { fprintf(stderr, "[E::main_esearch] out of memory\n"); goto done; }
        if (fmdh_esearch_patterns(d, o->row_of, o->n_seq, n_hits, hits, pat_off, pats)) { fprintf(stderr, "[E::main_esearch] cannot read the patterns back from the index\n"); goto done; }
    }
    if (o->locate && n_hits) {
        uint64_t *beg = (uint64_t *)malloc(n_hits * 16), *cnt = beg ? beg + n_hits : 0;
        if (!beg) { fprintf(stderr, "[E::main_esearch] out of memory\n"); goto done; }
        for (uint64_t j = 0; j < n_hits; ++j) { beg[j] = hits[j].beg; cnt[j] = hits[j].cnt; }
        const int e2 = fmd_locate_batch(d, n_hits, beg, cnt, o->max_occ, 0, &runs, &n_runs, &lst);
        free(beg);
        if (e2) { fprintf(stderr, "[E::main_esearch] %s\n", fmd_strerror(e2)); goto done; }
        if (fmdh_locate_hits(runs, n_runs, o->sorted, o->n_seq, &ocs, &n_oc)) {
            fprintf(stderr, "[E::main_esearch] a sentinel rank beyond the index's %llu sequences, or out of memory\n", (unsigned long long)o->n_seq);
            goto done;
        }
    }
    for (size_t i = 0; i < n; ++i) {
        const uint64_t *w = strata + i * cols * 2;
        const uint32_t len = (uint32_t)(off[i + 1] - off[i]);
        uint64_t nh = 0, no = 0;
        for (size_t c = 0; c < cols; ++c) { nh += w[2 * c]; no += w[2 * c + 1]; }
        fprintf(out, "SQ\t%s\t%u\t%llu\t%llu\t%d\t", names[i], len, (unsigned long long)nh, (unsigned long long)no, nh <= o->max_hits);
        for (size_t c = 0; c < cols; ++c) fprintf(out, "%s%llu", c ? "," : "", (unsigned long long)w[2 * c]);
        fputc('\n', out);
        for (; k < n_hits && hits[k].query == i; ++k) {
            const fmd_esearch_hit_t *h = &hits[k];
            const uint8_t *pat = pats + pat_off[k];
            uint32_t ne = 0;
            char *cigar = fmdh_esearch_cigar(bases + off[i], len, pat, h->len, &ne);
            if (!cigar || ne != h->n_edit) {
                fprintf(stderr, "[E::main_esearch] a hit of query %s at distance %u whose pattern is at distance %u\n", names[i], h->n_edit, ne);
                free(cigar);
                goto done;
            }
            fprintf(out, "EH\t%u\t", h->n_edit);
            for (uint32_t j = 0; j < h->len; ++j) fputc("$ACGTN"[pat[j] < 6 ? pat[j] : 5], out);
            fprintf(out, "\t%llu\t%s\n", (unsigned long long)h->cnt, cigar);
            free(cigar);
            for (; oc < n_oc && ocs[oc].query == k; ++oc)
                fprintf(out, "OC\t%llu\t%c\t%u\n", (unsigned long long)(ocs[oc].id >> 1), "+-"[ocs[oc].id & 1], ocs[oc].off);
        }
        fputs("//\n", out);
    }
    rc = 0;
done:
    free(pats); free(pat_off); free(ocs); free(strata);
    fmd_host_free(runs); fmd_host_free(hits);
    return rc;
}

int fmdh_main_esearch(int argc, char *argv[])
{
    int c, device = 0, rc = 0, l, best = 0;
    long long max_hits = 1000, max_occ = 1000, max_edit = 1;
    const char *rank_fn = 0;
    fmd_dev_t *d = 0;
    uint64_t *sorted = 0, n_sorted = 0;
    fmd_info_t info;
    esearch_opt_t o;
    memset(&o, 0, sizeof(o));
    while ((c = getopt(argc, argv, "g:e:bm:lM:r:")) >= 0) {
        if (c == 'g') device = atoi(optarg);
        else if (c == 'e') max_edit = atoll(optarg);
        else if (c == 'b') best = 1;
        else if (c == 'm') max_hits = atoll(optarg);
        else if (c == 'l') o.locate = 1;
        else if (c == 'M') max_occ = atoll(optarg);
        else if (c == 'r') rank_fn = optarg;
        else max_edit = -1;                                  /* an unknown option: the usage */
    }
    if (optind + 2 > argc || max_edit < 0 || max_edit > FMD_ESEARCH_MAX_EDIT || max_hits < 1 || max_occ < 1) {
        fprintf(stderr, "\nUsage:   fermi-amd esearch [-g GPU] [-e INT] [-b] [-m INT] [-l] [-M INT] [-r reads.rank] <reads.fmd> <query.fa>\n\n");
        fprintf(stderr, "Options: -e INT    edits allowed -- substitutions, insertions, deletions --, 0 to %d [1]\n", FMD_ESEARCH_MAX_EDIT);
        fprintf(stderr, "         -b        only the hits at the smallest distance of each query\n");
        fprintf(stderr, "         -m INT    list the hits of a query that has at most INT of them [1000]\n");
        fprintf(stderr, "         -l        locate every hit: the reads that hold it, strand and offset\n");
        fprintf(stderr, "         -M INT    with -l, list the occurrences of a hit that has at most INT of them [1000]\n");
        fprintf(stderr, "         -r FILE   with -l, the rank -> read map `seqsort` wrote for the index [computed]\n\n");
        fprintf(stderr, "Output:  SQ name length n_hits n_occ listed(1/0) h0,..,he; EH n_edit pattern count cigar per hit (=, X, I: query base not in the pattern,\n");
        fprintf(stderr, "         D: pattern base not in the query); OC read +|- offset per occurrence (-l); //\n\n");
        return 1;
    }
    if (max_hits > 0xffffffffll) max_hits = 0xffffffffll;
    if (max_occ > 0xffffffffll) max_occ = 0xffffffffll;
    {
        const char *fn[3] = { argv[optind], strcmp(argv[optind + 1], "-") == 0 ? 0 : argv[optind + 1], o.locate ? rank_fn : 0 };
        for (int j = 0; j < 3; ++j) {
            FILE *fp = fn[j] ? fopen(fn[j], "rb") : 0;
            if (fn[j] && !fp) { fprintf(stderr, "[E::main_esearch] fail to open file '%s'\n", fn[j]); return 1; }
            if (fp) fclose(fp);
        }
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_esearch] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    if (o.locate && rank_fn) {
        FILE *fp = fopen(rank_fn, "rb");
        long long bytes = -1;
        if (fp && fseek(fp, 0, SEEK_END) == 0) bytes = ftell(fp);
        if (fp && bytes >= 0 && bytes % 8 == 0 && (sorted = (uint64_t *)malloc(bytes ? (size_t)bytes : 8)) != 0) {
            rewind(fp);
            n_sorted = (uint64_t)bytes / 8;
            if (fread(sorted, 8, n_sorted, fp) != n_sorted) { free(sorted); sorted = 0; }
        }
        if (fp) fclose(fp);
        if (!sorted) { fprintf(stderr, "[E::main_esearch] cannot read the rank file '%s'\n", rank_fn); return 1; }
    } else if (o.locate && fmdh_seqsort(argv[optind], device, &sorted, &n_sorted)) return 1;
    rc = fmd_dev_open_file(device, argv[optind], &d);
    if (rc) { fprintf(stderr, "[E::main_esearch] cannot load `%s': %s\n", argv[optind], fmd_strerror(rc)); free(sorted); return 1; }
    fmd_dev_info(d, &info);
    if (o.locate && n_sorted != info.mcnt[1]) {
        fprintf(stderr, "[E::main_esearch] the rank file has %llu entries, the index %llu sequences\n", (unsigned long long)n_sorted, (unsigned long long)info.mcnt[1]);
        rc = 1;
    }
    o.max_edit = (int)max_edit; o.max_hits = (uint32_t)max_hits; o.max_occ = (uint32_t)max_occ; o.flags = best ? FMD_ESEARCH_BEST : 0;
    o.sorted = sorted; o.n_seq = info.mcnt[1];
    fmdh_seqio_t *io = rc ? 0 : fmdh_seq_open(argv[optind + 1]);
    if (!rc && !io) { fprintf(stderr, "[E::main_esearch] fail to open file '%s'\n", argv[optind + 1]); rc = 1; }
    if (rc == 0) {
        char **names = (char **)calloc(ESEARCH_BATCH, sizeof(char *));
        uint64_t *off = (uint64_t *)malloc((ESEARCH_BATCH + 1) * 8);
        size_t n = 0, cap = 1 << 20, tot = 0;
        uint8_t *bases = (uint8_t *)malloc(cap);
        if (!names || !off || !bases) { fprintf(stderr, "[E::main_esearch] out of memory\n"); rc = 1; }
        else off[0] = 0;
        while (rc == 0) {
            l = fmdh_seq_read(io);
            if (l < 0 || n == ESEARCH_BATCH) {
                if (n) rc = flush_batch(d, &o, n, names, bases, off, stdout);
                for (size_t i = 0; i < n; ++i) free(names[i]);
                n = 0; tot = 0;
                if (rc || l < 0) break;
            }
            if (tot + (size_t)l + 8 > cap) {
                while (tot + (size_t)l + 8 > cap) cap <<= 1;
                if ((bases = (uint8_t *)realloc(bases, cap)) == 0) { fprintf(stderr, "[E::main_esearch] out of memory\n"); rc = 1; break; }
            }
            const char *s = fmdh_seq_bases(io);
            for (int i = 0; i < l; ++i) bases[tot + i] = fmdh_nt6[(unsigned char)s[i]];
            names[n] = strdup(fmdh_seq_name(io));
            tot += (size_t)l; off[++n] = tot;
        }
        free(names); free(off); free(bases);
    }
    if (io) fmdh_seq_close(io);
    fmd_dev_close(d);
    free(sorted); free(o.row_of);
    return rc ? 1 : 0;
}
