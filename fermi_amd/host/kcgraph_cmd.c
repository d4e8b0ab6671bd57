#define _GNU_SOURCE
/* kcgraph_cmd.c -- `fermi-amd kcgraph [-k 21] [-o 2] [-c] [-f] [-a] [-p bits] [-g GPU] <a.fmd> [<b.fmd> ...]`: the coloured de Bruijn graph of 1 to 8 indexes of
 * both strands, compacted to unitigs (fmd_kcunitig; DESIGN.md section 28, the definitions are in include/fmd_hip.h).  The reference has no such command.
 *     default   GFA1 as `kgraph` prints it; KC:i = the sum over the colours, and on every S line kc:B:I,s_0,.. (the per-colour count sums) and kn:B:I,n_0,..
 *               (the nodes present per colour)
 *     -c        FMD_KCGRAPH_SPLIT: a unitig never runs across a change of pattern, so every unitig has one pattern
 *     -f        FASTA of the unitigs: >id KC:i:<sum> LN:i:<len> PT:Z:<pattern, index 0 first> kc:B:I,.. kn:B:I,..
 *     -p bits   only the unitigs whose pattern equals bits (one 0 / 1 per index, index 0 first), links between printed unitigs only; `-c -f -p 10`: the
 *               sequence private to the first of two samples
 *     -a        no compaction: KMER <tab> c_0,..,c_{N-1} <tab> pattern <tab> right <tab> left of the union, then <tab> right/left per colour; streamed (fmd_kcarcs)
 * and on stderr [M::main_kcgraph] k=.. n=.. nodes=.. arcs=.. unitigs=.. cycles=...  Usage and unreadable-file errors return 1 before the device is looked for.
 * The labelling and the strings are kgraph_cmd.c's (fmdh_kgraph_compact_pat, fmdh_kgraph_print_coloured) on the union bytes. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "fmd_host.h"

/* the plain graph a coloured one is over its union bytes (no counts: KC comes from u_count) */
static void kc_view(const fmd_kcunitig_t *g, fmd_kunitig_t *v)
{
    memset(v, 0, sizeof(*v));
    v->n_nodes = g->n_nodes; v->n_unitigs = g->n_unitigs;
    v->kmer = g->kmer; v->arcs = g->uarcs;
    v->unitig = g->unitig; v->offset = g->offset; v->orient = g->orient;
    v->u_nodes = g->u_nodes; v->u_first = g->u_first; v->u_flags = g->u_flags;
}

int fmdh_kcgraph_compact_host(int k, int n_idx, uint64_t n, const uint64_t *kmer, const uint32_t *count, const uint8_t *uarcs, const uint8_t *pattern, unsigned flags,
                              fmd_kcunitig_t *out)
{
    if (!out) return 2;
    memset(out, 0, sizeof(*out));
    if (n_idx < 1 || n_idx > FMD_KMAT_MAX_IDX || (flags & ~FMD_KCGRAPH_SPLIT) || (n && !pattern)) return 2;
    fmd_kunitig_t v;
    const int rc = fmdh_kgraph_compact_pat(k, n, kmer, uarcs, (flags & FMD_KCGRAPH_SPLIT) ? pattern : 0, &v);
    if (rc) return rc;
    out->n_idx = n_idx; out->n_nodes = v.n_nodes; out->n_unitigs = v.n_unitigs;
    out->unitig = v.unitig; out->offset = v.offset; out->orient = v.orient; out->u_nodes = v.u_nodes; out->u_first = v.u_first; out->u_flags = v.u_flags;
    out->stat.g = v.stat;
    if (n == 0) return 0;
    const uint64_t nu = v.n_unitigs;
    out->u_count = (uint64_t *)calloc(nu * n_idx, 8); out->u_present = (uint32_t *)calloc(nu * n_idx, 4); out->u_pattern = (uint8_t *)calloc(nu, 1);
    if (!out->u_count || !out->u_present || !out->u_pattern) { fmdh_kcgraph_free(out); return 1; }
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t u = out->unitig[j];
        for (int i = 0; i < n_idx; ++i) {
            if (count) out->u_count[u * n_idx + i] += count[(uint64_t)i * n + j];
            out->u_present[u * n_idx + i] += pattern[j] >> i & 1;
            out->stat.n_nodes_in[i] += pattern[j] >> i & 1;
        }
        out->u_pattern[u] |= pattern[j];
    }
    return 0;
}

static int kc_print(FILE *out, int k, const fmd_kcunitig_t *g, int gfa, int filter, unsigned want)
{
    fmd_kunitig_t v;
    fmdh_kgraph_colours_t x = { g->n_idx, g->u_count, g->u_present, g->u_pattern, filter, (uint8_t)want };
    kc_view(g, &v);
    return fmdh_kgraph_print_coloured(out, k, &v, gfa, &x);
}
int fmdh_kcgraph_print_gfa(FILE *out, int k, const fmd_kcunitig_t *g, int filter, unsigned want) { return kc_print(out, k, g, 1, filter, want); }
int fmdh_kcgraph_print_fasta(FILE *out, int k, const fmd_kcunitig_t *g, int filter, unsigned want) { return kc_print(out, k, g, 0, filter, want); }

static void kc_arc_text(uint32_t a, char *r, char *l)
{
    for (int c = 0; c < 4; ++c) { r[c] = a >> c & 1 ? "ACGT"[c] : '.'; l[c] = a >> (4 + c) & 1 ? "ACGT"[c] : '.'; }
    r[4] = l[4] = 0;
}

static void kc_print_arcs(FILE *out, int k, int n_idx, uint32_t min_occ, uint64_t n, const uint64_t *kmer, const uint32_t *const *count, const uint8_t *const *arcs,
                          const uint8_t *uarcs)
{
    char buf[33], r[5], l[5];
    for (uint64_t j = 0; j < n; ++j) {
        fputs(fmdh_kmer_text(kmer[j], k, buf), out);
        for (int i = 0; i < n_idx; ++i) fprintf(out, "%c%u", i ? ',' : '\t', count[i][j]);
        fputc('\t', out);
        for (int i = 0; i < n_idx; ++i) fputc(count[i][j] >= min_occ ? '1' : '0', out);
        kc_arc_text(uarcs[j], r, l);
        fprintf(out, "\t%s\t%s", r, l);
        for (int i = 0; i < n_idx; ++i) { kc_arc_text(arcs[i][j], r, l); fprintf(out, "\t%s/%s", r, l); }
        fputc('\n', out);
    }
}

void fmdh_kcgraph_print_arcs(FILE *out, int k, int n_idx, uint32_t min_occ, uint64_t n, uint64_t stride, const uint64_t *kmer, const uint32_t *count, const uint8_t *arcs,
                             const uint8_t *uarcs)
{
    const uint32_t *cc[FMD_KMAT_MAX_IDX];
    const uint8_t *ac[FMD_KMAT_MAX_IDX];
    if (n_idx < 1 || n_idx > FMD_KMAT_MAX_IDX) return;
    for (int i = 0; i < n_idx; ++i) { cc[i] = count + (uint64_t)i * stride; ac[i] = arcs + (uint64_t)i * stride; }
    kc_print_arcs(out, k, n_idx, min_occ, n, kmer, cc, ac, uarcs);
}

void fmdh_kcgraph_free(fmd_kcunitig_t *g)
{
    fmd_host_free(g->kmer); fmd_host_free(g->count); fmd_host_free(g->arcs); fmd_host_free(g->uarcs); fmd_host_free(g->pattern);
    fmd_host_free(g->unitig); fmd_host_free(g->offset); fmd_host_free(g->orient); fmd_host_free(g->u_nodes); fmd_host_free(g->u_first); fmd_host_free(g->u_flags);
    fmd_host_free(g->u_count); fmd_host_free(g->u_present); fmd_host_free(g->u_pattern);
    memset(g, 0, sizeof(*g));
}

typedef struct { FILE *out; int k, n_idx; uint32_t min_occ; } dump_t;
static int dump_sink(void *ctx, uint64_t n, const uint64_t *kmer, const uint32_t *const *count, const uint8_t *const *arcs, const uint8_t *uarcs)
{
    dump_t *d = (dump_t *)ctx;
    kc_print_arcs(d->out, d->k, d->n_idx, d->min_occ, n, kmer, count, arcs, uarcs);
    return ferror(d->out) != 0;
}

int fmdh_main_kcgraph(int argc, char *argv[])
{
    int c, device = 0, fasta = 0, plain = 0, split = 0, rc = 0, n_idx, bad_bits = 0;
    long long k = 21, min_occ = 2;
    const char *bits = 0;
    unsigned want = 0;
    fmd_dev_t *d[FMD_KMAT_MAX_IDX] = { 0 };
    while ((c = getopt(argc, argv, "k:o:cfap:g:")) >= 0) {
        if (c == 'k') k = atoll(optarg);
        else if (c == 'o') min_occ = atoll(optarg);
        else if (c == 'c') split = 1;
        else if (c == 'f') fasta = 1;
        else if (c == 'a') plain = 1;
        else if (c == 'p') bits = optarg;
        else if (c == 'g') device = atoi(optarg);
    }
    n_idx = argc - optind;
    if (bits) {
        bad_bits = (int)strlen(bits) != n_idx;
        for (int i = 0; !bad_bits && i < n_idx; ++i) {
            if (bits[i] == '1') want |= 1u << i;
            else if (bits[i] != '0') bad_bits = 1;
        }
    }
    if (n_idx < 1 || n_idx > FMD_KMAT_MAX_IDX || k < 3 || k > 31 || !(k & 1) || min_occ < 1 || min_occ > 0x7fffffffll || (plain && (fasta || bits || split)) || bad_bits) {
        fprintf(stderr, "\nUsage:   fermi-amd kcgraph [-k 21] [-o 2] [-c] [-f] [-a] [-p bits] [-g GPU] <a.fmd> [<b.fmd> ...]\n\n");
        fprintf(stderr, "Options: -k INT    k-mer length, odd, 3..31 [21]\n");
        fprintf(stderr, "         -o INT    a k-mer or an arc is in an index where it occurs at least INT times, INT >= 1; a node is in some index [2]\n");
        fprintf(stderr, "         -c        end a unitig where the set of indexes that hold its k-mers changes: every unitig has one pattern\n");
        fprintf(stderr, "         -f        print the unitigs as FASTA instead of GFA, the pattern in the header\n");
        fprintf(stderr, "         -p BITS   only the unitigs whose pattern is BITS, one 0 or 1 per index, the first index first\n");
        fprintf(stderr, "         -a        no compaction: KMER counts pattern right left, then right/left per index; the arcs as ACGT with . for none\n\n");
        fprintf(stderr, "Input:   1 to %d indexes of both strands\n\n", FMD_KMAT_MAX_IDX);
        return 1;
    }
    for (int i = 0; i < n_idx; ++i) {
        FILE *fp = fopen(argv[optind + i], "rb");
        if (!fp) { fprintf(stderr, "[E::main_kcgraph] fail to open file '%s'\n", argv[optind + i]); return 1; }
        fclose(fp);
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_kcgraph] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    for (int i = 0; i < n_idx && !rc; ++i) {
        rc = fmd_dev_open_file_ex(device, argv[optind + i], FMD_OPEN_EMPTY_OK, &d[i]);
        if (rc) fprintf(stderr, "[E::main_kcgraph] cannot load `%s': %s\n", argv[optind + i], fmd_strerror(rc));
    }
    fmd_kcunitig_t g;
    memset(&g, 0, sizeof(g));
    if (!rc) {
        fmd_kcgraph_stat_t st;
        if (plain) {
            dump_t ctx = { stdout, (int)k, n_idx, (uint32_t)min_occ };
            rc = fmd_kcarcs(n_idx, d, (int)k, (int)min_occ, 0, dump_sink, &ctx, &st);
        } else {
            rc = fmd_kcunitig(n_idx, d, (int)k, (int)min_occ, split ? FMD_KCGRAPH_SPLIT : 0, 0, &g);
            st = g.stat;
        }
        if (rc == FMD_E_ARG) fprintf(stderr, "[E::main_kcgraph] one of the files is not an index of both strands: its base counts are not symmetric\n");
        else if (rc) fprintf(stderr, "[E::main_kcgraph] %s\n", fmd_strerror(rc));
        else {
            g.n_idx = n_idx;
            if (!plain && (fasta ? fmdh_kcgraph_print_fasta(stdout, (int)k, &g, bits != 0, want) : fmdh_kcgraph_print_gfa(stdout, (int)k, &g, bits != 0, want))) {
                fprintf(stderr, "[E::main_kcgraph] out of memory\n"); rc = 1;
            }
            fprintf(stderr, "[M::main_kcgraph] k=%d n=%d nodes=%llu arcs=%llu unitigs=%llu cycles=%llu\n", (int)k, n_idx, (unsigned long long)st.g.n_nodes,
                    (unsigned long long)st.g.n_arcs, (unsigned long long)st.g.n_unitigs, (unsigned long long)st.g.n_cycles);
        }
    }
    fmdh_kcgraph_free(&g);
    for (int i = 0; i < n_idx; ++i) fmd_dev_close(d[i]);
    return rc ? 1 : 0;
}
