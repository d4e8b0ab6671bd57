#define _GNU_SOURCE
/* kgraph_cmd.c -- `fermi-amd kgraph [-k 21] [-o 2] [-f] [-a] [-g GPU] <reads.fmd>`: the de Bruijn graph of the k-mers of the indexed reads with at least -o
 * occurrences, compacted to unitigs (fmd_kunitig; DESIGN.md section 27, the definitions are in include/fmd_hip.h).  The reference has no such command.
 *     default   GFA1: H; S <id> <seq> KC:i:<sum of the nodes' counts> LN:i:<len> per unitig, ascending; L <a> <+|-> <b> <+|-> <k-1>M per arc between
 *               unitig ends, an arc and its reverse-complement twin once, from the smaller (id, orientation) pair, + before -; self-links included
 *     -f        FASTA of the unitigs: >id KC:i:<sum> LN:i:<len>
 *     -a        no compaction: KMER <tab> count <tab> right <tab> left per node, ascending, streamed (fmd_karcs); right / left = ACGT, a . for no arc
 * and on stderr [M::main_kgraph] k=.. nodes=.. arcs=.. unitigs=.. cycles=...  Usage and unreadable-file errors return 1 before the device is looked for.
 * The strings are put together here from (unitig, offset, orient); fmdh_kgraph_compact_host is the same labelling walked by one thread from (kmer, arcs). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "fmd_host.h"

#define KG_NONE 0xffffffffu

static uint64_t kg_rc(uint64_t x, int k)
{
    uint64_t r = 0;
    for (int i = 0; i < k; ++i) { r = r << 2 | (3 - (x & 3)); x >>= 2; }
    return r;
}
static uint32_t kg_rev4(uint32_t v) { return (v & 1u) << 3 | (v & 2u) << 1 | (v & 4u) >> 1 | (v & 8u) >> 3; }
static int kg_pop4(uint32_t v) { return (int)((v & 1u) + (v >> 1 & 1u) + (v >> 2 & 1u) + (v >> 3 & 1u)); }

/* the node of a canonical k-mer, or n */
static uint64_t kg_find(const uint64_t *kmer, uint64_t n, uint64_t y)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (kmer[mid] < y) lo = mid + 1; else hi = mid; }
    return lo < n && kmer[lo] == y ? lo : n;
}

/* the right arcs of node i read in orientation o (1 = reversed), and the oriented string */
static uint32_t kg_right(const uint8_t *arcs, uint64_t i, int o) { return o ? kg_rev4((uint32_t)arcs[i] >> 4) : arcs[i] & 15u; }

/* the oriented node that follows (i, o) through base c -> its node (n when it is not listed), *vo = its orientation */
static uint64_t kg_step(int k, uint64_t n, const uint64_t *kmer, uint64_t i, int o, int c, int *vo)
{
    const uint64_t mask = ~0ull >> (64 - 2 * k), u = o ? kg_rc(kmer[i], k) : kmer[i];
    const uint64_t v = (u << 2 | (uint64_t)c) & mask, rv = kg_rc(v, k);
    *vo = rv < v;
    return kg_find(kmer, n, v < rv ? v : rv);
}

/* the port (2 j + side) a compactable link out of port p = 2 i + side arrives at, or KG_NONE: side 0 = the right end of the canonical string */
static uint32_t kg_mate(int k, uint64_t n, const uint64_t *kmer, const uint8_t *arcs, const uint8_t *pat, uint64_t p)
{
    const uint64_t i = p >> 1;
    const int o = (int)(p & 1);
    const uint32_t r = kg_right(arcs, i, o);
    int c = 0, vo;
    if (kg_pop4(r) != 1) return KG_NONE;
    while (!(r >> c & 1u)) ++c;
    const uint64_t j = kg_step(k, n, kmer, i, o, c, &vo);
    if (j == n || j == i || (pat && pat[j] != pat[i])) return KG_NONE;   /* (pat: kcgraph's split rule) */
    if (kg_pop4(vo ? arcs[j] & 15u : (uint32_t)arcs[j] >> 4) != 1) return KG_NONE;   /* the left arcs of the successor as oriented */
    return (uint32_t)(2 * j) + (vo ? 0u : 1u);
}

int fmdh_kgraph_compact_host(int k, uint64_t n, const uint64_t *kmer, const uint8_t *arcs, fmd_kunitig_t *out) { return fmdh_kgraph_compact_pat(k, n, kmer, arcs, 0, out); }

int fmdh_kgraph_compact_pat(int k, uint64_t n, const uint64_t *kmer, const uint8_t *arcs, const uint8_t *pat, fmd_kunitig_t *out)
{
    if (!out) return 2;
    memset(out, 0, sizeof(*out));
    if (k < 3 || k > 31 || !(k & 1) || n > FMD_KGRAPH_MAX_NODES || (n && (!kmer || !arcs))) return 2;
    out->n_nodes = out->stat.n_nodes = n;
    if (n == 0) return 0;
    uint32_t *mate = (uint32_t *)malloc(2 * n * 4);
    out->unitig = (uint32_t *)malloc(n * 4); out->offset = (uint32_t *)malloc(n * 4); out->orient = (uint8_t *)malloc(n);
    out->u_nodes = (uint32_t *)malloc(n * 4); out->u_first = (uint32_t *)malloc(n * 4); out->u_flags = (uint8_t *)malloc(n);
    if (!mate || !out->unitig || !out->offset || !out->orient || !out->u_nodes || !out->u_first || !out->u_flags) {
        free(mate); free(out->unitig); free(out->offset); free(out->orient); free(out->u_nodes); free(out->u_first); free(out->u_flags);
        memset(out, 0, sizeof(*out));
        return 1;
    }
    const uint64_t mask1 = ~0ull >> (64 - 2 * (k + 1));
    uint64_t bits = 0, pal = 0, mates = 0, nu = 0;
    for (uint64_t p = 0; p < 2 * n; ++p) mates += (mate[p] = kg_mate(k, n, kmer, arcs, pat, p)) != KG_NONE;
    for (uint64_t i = 0; i < n; ++i) {
        out->unitig[i] = KG_NONE;
        for (int c = 0; c < 4; ++c) {
            const uint64_t R = (kmer[i] << 2 | (uint64_t)c) & mask1, L = (uint64_t)c << (2 * k) | kmer[i];
            if (arcs[i] >> c & 1) { ++bits; pal += kg_rc(R, k + 1) == R; }
            if (arcs[i] >> (4 + c) & 1) { ++bits; pal += kg_rc(L, k + 1) == L; }
        }
    }
    for (uint64_t i = 0; i < n; ++i) {
        if (out->unitig[i] != KG_NONE) continue;      /* else i is the smallest node of a chain nobody has walked yet */
        uint32_t e[2] = { 0, 0 };                     /* the free port reached through i's right end, and through its left end */
        int cyc = 0;
        for (int s = 0; s < 2 && !cyc; ++s) {
            uint32_t p = (uint32_t)(2 * i) + (uint32_t)s;
            while (mate[p] != KG_NONE) {
                p = mate[p] ^ 1u;
                if (p >> 1 == i) { cyc = 1; break; }
            }
            e[s] = p;
        }
        uint32_t start;                               /* the free port the printed string starts at: its node reads forward when that is its left port */
        if (cyc) {
            const uint32_t q = mate[2 * i + 1];
            mate[2 * i + 1] = KG_NONE; mate[q] = KG_NONE;   /* opened at the left port of its smallest node */
            start = (uint32_t)(2 * i + 1);
            ++out->stat.n_cycles;
        } else {
            const uint64_t a = e[1] & 1u ? kmer[e[1] >> 1] : kg_rc(kmer[e[1] >> 1], k), b = e[0] & 1u ? kmer[e[0] >> 1] : kg_rc(kmer[e[0] >> 1], k);
            start = a < b ? e[1] : e[0];
        }
        uint32_t p = start, len = 0;
        out->u_first[nu] = start >> 1; out->u_flags[nu] = cyc ? FMD_KGRAPH_CYCLE : 0;
        for (;;) {                                    /* p = the port the walk came in through */
            const uint32_t j = p >> 1;
            out->unitig[j] = (uint32_t)nu; out->offset[j] = len++; out->orient[j] = p & 1u ? 0 : 1;
            if (mate[p ^ 1u] == KG_NONE) break;
            p = mate[p ^ 1u];
        }
        out->u_nodes[nu++] = len;
    }
    free(mate);
    out->n_unitigs = nu;
    out->stat.n_arcs = (bits + pal) / 2; out->stat.n_links = mates / 2; out->stat.n_unitigs = nu;
    return 0;
}

void fmdh_kgraph_print_arcs(FILE *out, int k, uint64_t n, const uint64_t *kmer, const uint32_t *count, const uint8_t *arcs)
{
    char buf[33], r[5], l[5];
    r[4] = l[4] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        for (int c = 0; c < 4; ++c) { r[c] = arcs[i] >> c & 1 ? "ACGT"[c] : '.'; l[c] = arcs[i] >> (4 + c) & 1 ? "ACGT"[c] : '.'; }
        fprintf(out, "%s\t%u\t%s\t%s\n", fmdh_kmer_text(kmer[i], k, buf), count[i], r, l);
    }
}

/* order[first[u] + t] = the node at offset t of unitig u; first has n_unitigs + 1 entries.  1 without memory, 2 when the arrays are not a partition */
static int kg_order(const fmd_kunitig_t *g, uint64_t **first_, uint32_t **order_)
{
    uint64_t *first = (uint64_t *)calloc(g->n_unitigs + 1, 8);
    uint32_t *order = (uint32_t *)malloc((g->n_nodes ? g->n_nodes : 1) * 4);
    if (!first || !order) { free(first); free(order); return 1; }
    for (uint64_t u = 0; u < g->n_unitigs; ++u) first[u + 1] = first[u] + g->u_nodes[u];
    int bad = first[g->n_unitigs] != g->n_nodes;
    for (uint64_t i = 0; i < g->n_nodes && !bad; ++i) {
        if (g->unitig[i] >= g->n_unitigs || g->offset[i] >= g->u_nodes[g->unitig[i]]) bad = 1;
        else order[first[g->unitig[i]] + g->offset[i]] = (uint32_t)i;
    }
    if (bad) { free(first); free(order); return 2; }
    *first_ = first; *order_ = order;
    return 0;
}

/* the string of unitig u into seq (u_nodes + k - 1 characters and a NUL), *kc = the sum of its nodes' counts */
static void kg_seq(int k, const fmd_kunitig_t *g, const uint64_t *first, const uint32_t *order, uint64_t u, char *seq, uint64_t *kc)   /* (no counts: *kc = 0) */
{
    uint64_t len = 0, sum = 0;
    for (uint64_t t = first[u]; t < first[u + 1]; ++t) {
        const uint32_t i = order[t];
        const uint64_t x = g->orient[i] ? kg_rc(g->kmer[i], k) : g->kmer[i];
        if (t == first[u]) { fmdh_kmer_text(x, k, seq); len = (uint64_t)k; }
        else seq[len++] = "ACGT"[x & 3];
        if (g->count) sum += g->count[i];
    }
    seq[len] = 0;
    *kc = sum;
}

/* the bits of a pattern, index 0 first */
static const char *kg_bits(uint32_t p, int n_idx, char *buf) { for (int i = 0; i < n_idx; ++i) buf[i] = p >> i & 1 ? '1' : '0'; buf[n_idx] = 0; return buf; }

/* the tags of unitig u that only a coloured graph has */
static void kg_colour_tags(FILE *out, const fmdh_kgraph_colours_t *x, uint64_t u, int sep)
{
    fprintf(out, "%ckc:B:I", sep);
    for (int i = 0; i < x->n_idx; ++i) fprintf(out, ",%llu", (unsigned long long)x->u_count[u * x->n_idx + i]);
    fprintf(out, "%ckn:B:I", sep);
    for (int i = 0; i < x->n_idx; ++i) fprintf(out, ",%u", x->u_present[u * x->n_idx + i]);
}

static int kg_print_unitigs(FILE *out, int k, const fmd_kunitig_t *g, int gfa) { return fmdh_kgraph_print_coloured(out, k, g, gfa, 0); }

int fmdh_kgraph_print_coloured(FILE *out, int k, const fmd_kunitig_t *g, int gfa, const fmdh_kgraph_colours_t *x)
{
    char bits[9];
    uint64_t *first = 0, longest = 0, kc;
    uint32_t *order = 0;
    const int rc = kg_order(g, &first, &order);
    if (rc) return rc;
    for (uint64_t u = 0; u < g->n_unitigs; ++u) if (g->u_nodes[u] > longest) longest = g->u_nodes[u];
    char *seq = (char *)malloc(longest + (uint64_t)k + 1);
    if (!seq) { free(first); free(order); return 1; }
    if (gfa) fprintf(out, "H\tVN:Z:1.0\n");
    for (uint64_t u = 0; u < g->n_unitigs; ++u) {
        if (x && x->filter && x->u_pattern[u] != x->want) continue;
        kg_seq(k, g, first, order, u, seq, &kc);
        for (int i = 0; x && i < x->n_idx; ++i) kc += x->u_count[u * x->n_idx + i];   /* KC of a coloured unitig: the sum over the colours */
        const unsigned long long ln = (unsigned long long)g->u_nodes[u] + (unsigned long long)k - 1;
        if (gfa) {
            fprintf(out, "S\t%llu\t%s\tKC:i:%llu\tLN:i:%llu", (unsigned long long)u, seq, (unsigned long long)kc, ln);
            if (x) kg_colour_tags(out, x, u, '\t');
            fputc('\n', out);
        } else {
            fprintf(out, ">%llu KC:i:%llu LN:i:%llu", (unsigned long long)u, (unsigned long long)kc, ln);
            if (x) { fprintf(out, " PT:Z:%s", kg_bits(x->u_pattern[u], x->n_idx, bits)); kg_colour_tags(out, x, u, ' '); }
            fprintf(out, "\n%s\n", seq);
        }
    }
    for (uint64_t a = 0; gfa && a < g->n_unitigs; ++a)
        for (int oa = 0; oa < 2; ++oa) {
            if (x && x->filter && x->u_pattern[a] != x->want) continue;              /* leaving a read as printed (+) through its last node, or reversed (-) through its first */
            const uint32_t e = oa ? order[first[a]] : order[first[a + 1] - 1];
            const int eo = oa ? !g->orient[e] : g->orient[e];
            const uint32_t r = kg_right(g->arcs, e, eo);
            for (int c = 0; c < 4; ++c) {
                int vo;
                if (!(r >> c & 1u)) continue;
                const uint64_t j = kg_step(k, g->n_nodes, g->kmer, e, eo, c, &vo);
                if (j == g->n_nodes) continue;        /* (arcs that name no node: not from this library) */
                const uint32_t b = g->unitig[j];
                int ob;
                if (x && x->filter && x->u_pattern[b] != x->want) continue;   /* links between printed unitigs only */
                if (g->offset[j] == 0 && vo == g->orient[j]) ob = 0;
                else if (g->offset[j] == g->u_nodes[b] - 1 && vo != g->orient[j]) ob = 1;
                else continue;
                if (2 * a + (uint64_t)oa <= 2 * (uint64_t)b + (uint64_t)!ob)   /* its twin leaves (b, !ob) */
                    fprintf(out, "L\t%llu\t%c\t%u\t%c\t%dM\n", (unsigned long long)a, "+-"[oa], b, "+-"[ob], k - 1);
            }
        }
    free(seq); free(first); free(order);
    return 0;
}
int fmdh_kgraph_print_gfa(FILE *out, int k, const fmd_kunitig_t *g) { return kg_print_unitigs(out, k, g, 1); }
int fmdh_kgraph_print_fasta(FILE *out, int k, const fmd_kunitig_t *g) { return kg_print_unitigs(out, k, g, 0); }

void fmdh_kgraph_free(fmd_kunitig_t *g)
{
    fmd_host_free(g->kmer); fmd_host_free(g->count); fmd_host_free(g->arcs); fmd_host_free(g->unitig); fmd_host_free(g->offset); fmd_host_free(g->orient);
    fmd_host_free(g->u_nodes); fmd_host_free(g->u_first); fmd_host_free(g->u_flags);
    memset(g, 0, sizeof(*g));
}

typedef struct { FILE *out; int k; } dump_t;
static int dump_sink(void *ctx, uint64_t n, const uint64_t *kmer, const uint32_t *count, const uint8_t *arcs)
{
    dump_t *d = (dump_t *)ctx;
    fmdh_kgraph_print_arcs(d->out, d->k, n, kmer, count, arcs);
    return ferror(d->out) != 0;
}

int fmdh_main_kgraph(int argc, char *argv[])
{
    int c, device = 0, fasta = 0, plain = 0, rc;
    long long k = 21, min_occ = 2;
    fmd_dev_t *d = 0;
    while ((c = getopt(argc, argv, "k:o:fag:")) >= 0) {
        if (c == 'k') k = atoll(optarg);
        else if (c == 'o') min_occ = atoll(optarg);
        else if (c == 'f') fasta = 1;
        else if (c == 'a') plain = 1;
        else if (c == 'g') device = atoi(optarg);
    }
    if (optind + 1 > argc || k < 3 || k > 31 || !(k & 1) || min_occ < 1 || min_occ > 0x7fffffffll || (fasta && plain)) {
        fprintf(stderr, "\nUsage:   fermi-amd kgraph [-k 21] [-o 2] [-f] [-a] [-g GPU] <reads.fmd>\n\n");
        fprintf(stderr, "Options: -k INT    k-mer length, odd, 3..31 [21]\n");
        fprintf(stderr, "         -o INT    leave out k-mers and arcs with fewer than INT occurrences, at least 1 [2]\n");
        fprintf(stderr, "         -f        print the unitigs as FASTA instead of GFA\n");
        fprintf(stderr, "         -a        no compaction: KMER count right left per k-mer, the arcs as ACGT with . for none\n\n");
        return 1;
    }
    {
        FILE *fp = fopen(argv[optind], "rb");
        if (!fp) { fprintf(stderr, "[E::main_kgraph] fail to open file '%s'\n", argv[optind]); return 1; }
        fclose(fp);
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_kgraph] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    rc = fmd_dev_open_file(device, argv[optind], &d);
    if (rc) { fprintf(stderr, "[E::main_kgraph] cannot load `%s': %s\n", argv[optind], fmd_strerror(rc)); return 1; }
    fmd_kunitig_t g;
    fmd_kgraph_stat_t st;
    memset(&g, 0, sizeof(g));
    if (plain) {
        dump_t ctx = { stdout, (int)k };
        rc = fmd_karcs(d, (int)k, (int)min_occ, 0, dump_sink, &ctx, &st);
    } else {
        rc = fmd_kunitig(d, (int)k, (int)min_occ, 0, &g);
        st = g.stat;
    }
    if (rc == FMD_E_ARG) fprintf(stderr, "[E::main_kgraph] `%s' is not an index of both strands: its base counts are not symmetric\n", argv[optind]);
    else if (rc) fprintf(stderr, "[E::main_kgraph] %s\n", fmd_strerror(rc));
    else {
        if (!plain && (fasta ? fmdh_kgraph_print_fasta(stdout, (int)k, &g) : fmdh_kgraph_print_gfa(stdout, (int)k, &g))) { fprintf(stderr, "[E::main_kgraph] out of memory\n"); rc = 1; }
        fprintf(stderr, "[M::main_kgraph] k=%d nodes=%llu arcs=%llu unitigs=%llu cycles=%llu\n", (int)k, (unsigned long long)st.n_nodes, (unsigned long long)st.n_arcs,
                (unsigned long long)st.n_unitigs, (unsigned long long)st.n_cycles);
    }
    fmdh_kgraph_free(&g);
    fmd_dev_close(d);
    return rc ? 1 : 0;
}
