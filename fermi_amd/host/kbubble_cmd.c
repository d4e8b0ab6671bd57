#define _GNU_SOURCE
/* kbubble_cmd.c -- `fermi-amd kbubble [-k 21] [-o 2] [-L 0] [-d] [-g GPU] <a.fmd> [<b.fmd> ...]`: the simple variant bubbles of the coloured de Bruijn graph of 1 to
 * 8 indexes of both strands (fmd_kcbubble; DESIGN.md section 29, the definitions are in include/fmd_hip.h).  The reference has no such command.
 *     SM <n_nodes> <n_unitigs> <n_forks> <n_bubbles>
 *     BB <index> <type> <left flank> <allele 0> <allele 1> <right flank> <len 0> <len 1> <unitig 0> <unitig 1> kc:B:I,.. kn:B:I,.. GT:Z:..    per bubble, by src
 *     -L INT    only bubbles whose branches have at most INT nodes (0: any)
 *     -d        only the bubbles that not every index holds alike (SM still counts all of them; the index column stays the record's)
 * kc / kn: the 2 N count sums / present nodes of the two branches, branch 0's N colours first; GT: per colour `10` = it holds every node of branch 0 and not
 * every node of branch 1, `01`, `11`, `00`.  Usage and unreadable-file errors return 1 before the device is looked for.
 * fmdh_kcbubble_host is the definition walked node by node by one thread, with a binary search per step and none of the unitig labels: the test oracle of
 * the device's stage and its timing yardstick. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "fmd_host.h"

#define KB_NONE 0xffffffffu

static uint64_t kb_rc(uint64_t x, int k)
{
    uint64_t r = 0;
    for (int i = 0; i < k; ++i) { r = r << 2 | (3 - (x & 3)); x >>= 2; }
    return r;
}
static uint32_t kb_rev4(uint32_t v) { return (v & 1u) << 3 | (v & 2u) << 1 | (v & 4u) >> 1 | (v & 8u) >> 3; }
static int kb_pop4(uint32_t v) { return (int)((v & 1u) + (v >> 1 & 1u) + (v >> 2 & 1u) + (v >> 3 & 1u)); }

typedef struct { int k; uint64_t n; const uint64_t *kmer; const uint8_t *arcs; } kb_graph_t;

/* the right arcs of the oriented node u = 2 id + o, and its k bases as a packed word */
static uint32_t kb_right(const kb_graph_t *g, uint32_t u) { const uint32_t a = g->arcs[u >> 1]; return u & 1u ? kb_rev4(a >> 4) : a & 15u; }
static uint64_t kb_word(const kb_graph_t *g, uint32_t u) { return u & 1u ? kb_rc(g->kmer[u >> 1], g->k) : g->kmer[u >> 1]; }

/* follow(u, c), or KB_NONE when it is no node */
static uint32_t kb_follow(const kb_graph_t *g, uint32_t u, int c)
{
    const uint64_t mask = ~0ull >> (64 - 2 * g->k), v = (kb_word(g, u) << 2 | (uint64_t)c) & mask, rv = kb_rc(v, g->k), y = v < rv ? v : rv;
    uint64_t lo = 0, hi = g->n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (g->kmer[mid] < y) lo = mid + 1; else hi = mid; }
    if (lo >= g->n || g->kmer[lo] != y) return KB_NONE;
    return (uint32_t)(2 * lo) + (v == y ? 0u : 1u);
}

static int kb_only(uint32_t r) { int c = 0; while (!(r >> c & 1u)) ++c; return c; }

/* the branch from the oriented node a, node by node: 1 and its target and length, 0 when a starts none */
static int kb_branch(const kb_graph_t *g, uint32_t a, uint32_t *t, uint32_t *len)
{
    uint32_t v = a;
    if (a == KB_NONE || kb_pop4(kb_right(g, a ^ 1u)) != 1) return 0;
    for (uint64_t m = 1; m <= 2 * g->n; ++m) {        /* a chain passes an oriented node once: no input spins this */
        const uint32_t r = kb_right(g, v);
        if (kb_pop4(r) != 1) return 0;
        const uint32_t w = kb_follow(g, v, kb_only(r));
        if (w == KB_NONE) return 0;
        if (kb_pop4(kb_right(g, w ^ 1u)) != 1) { *t = w; *len = (uint32_t)m; return 1; }
        v = w;
    }
    return 0;
}

int fmdh_kcbubble_host(int k, const fmd_kcunitig_t *g, uint32_t max_len, uint64_t *n_forks, uint64_t *n, fmd_kbubble_t **bubble)
{
    if (!g || !n_forks || !n || !bubble || k < 3 || k > 31 || !(k & 1) || g->n_nodes > FMD_KGRAPH_MAX_NODES || (g->n_nodes && (!g->kmer || !g->uarcs))) return 2;
    const kb_graph_t G = { k, g->n_nodes, g->kmer, g->uarcs };
    uint64_t cap = 0;
    *n_forks = 0; *n = 0; *bubble = 0;
    for (uint64_t p = 0; p < 2 * G.n; ++p) {
        const uint32_t r = kb_right(&G, (uint32_t)p);
        if (kb_pop4(r) != 2) continue;
        ++*n_forks;
        int c0 = 0, c1 = 3;
        while (!(r >> c0 & 1u)) ++c0;
        while (!(r >> c1 & 1u)) --c1;
        fmd_kbubble_t b;
        uint32_t t0, t1;
        b.src = (uint32_t)p;
        b.first[0] = kb_follow(&G, b.src, c0); b.first[1] = kb_follow(&G, b.src, c1);
        if (!kb_branch(&G, b.first[0], &t0, &b.len[0]) || !kb_branch(&G, b.first[1], &t1, &b.len[1])) continue;
        if (t0 != t1 || kb_pop4(kb_right(&G, t0 ^ 1u)) != 2 || (t0 >> 1) == (b.src >> 1)) continue;
        if (max_len && (b.len[0] > max_len || b.len[1] > max_len)) continue;
        if ((b.src >> 1) > (t0 >> 1)) continue;       /* met again from t ^ 1: reported from the smaller node */
        b.dst = t0;
        if (*n == cap) {
            cap = cap ? 2 * cap : 64;
            fmd_kbubble_t *q = (fmd_kbubble_t *)realloc(*bubble, cap * sizeof(fmd_kbubble_t));
            if (!q) { free(*bubble); *bubble = 0; *n = 0; return 1; }
            *bubble = q;
        }
        (*bubble)[(*n)++] = b;
    }
    return 0;
}

/* P_b = text(s) + the last base of every branch node + the last base of text(t), NUL-terminated; 0 when the record is not a walk of the graph */
static int kb_path(const kb_graph_t *g, const fmd_kbubble_t *b, int br, char *out)
{
    const int k = g->k;
    uint64_t w = kb_word(g, b->src);
    uint32_t v = b->first[br];
    size_t at = 0;
    for (int i = 0; i < k; ++i) out[at++] = "ACGT"[w >> (2 * (k - 1 - i)) & 3];
    for (uint32_t j = 0; j < b->len[br]; ++j) {
        if (v == KB_NONE || (uint64_t)(v >> 1) >= g->n) return 0;
        out[at++] = "ACGT"[kb_word(g, v) & 3];
        const uint32_t r = kb_right(g, v);
        if (kb_pop4(r) != 1) return 0;
        v = kb_follow(g, v, kb_only(r));
    }
    if (v != b->dst) return 0;
    out[at++] = "ACGT"[kb_word(g, v) & 3];
    out[at] = 0;
    return 1;
}

int fmdh_kbubble_print(FILE *out, int k, const fmd_kcunitig_t *g, uint64_t n, const fmd_kbubble_t *b, int differing_only)
{
    if (!out || !g || (n && !b) || k < 3 || k > 31 || !(k & 1) || g->n_idx < 1 || g->n_idx > FMD_KMAT_MAX_IDX) return 2;
    const kb_graph_t G = { k, g->n_nodes, g->kmer, g->uarcs };
    const int n_idx = g->n_idx;
    for (uint64_t x = 0; x < n; ++x) {
        const fmd_kbubble_t *r = &b[x];
        if ((uint64_t)(r->src >> 1) >= G.n || (uint64_t)(r->dst >> 1) >= G.n) return 2;
        uint32_t held[2] = { 0, 0 };
        uint64_t u[2];
        for (int br = 0; br < 2; ++br) {
            if ((uint64_t)(r->first[br] >> 1) >= G.n) return 2;
            u[br] = g->unitig[r->first[br] >> 1];
            for (int i = 0; i < n_idx; ++i)
                if (g->u_present[u[br] * n_idx + i] == g->u_nodes[u[br]]) held[br] |= 1u << i;
        }
        if (differing_only) {
            int same = 1;
            for (int i = 1; i < n_idx; ++i) same = same && (held[0] >> i & 1u) == (held[0] & 1u) && (held[1] >> i & 1u) == (held[1] & 1u);
            if (same) continue;
        }
        char *P[2];
        size_t L[2];
        P[0] = (char *)malloc((size_t)k + r->len[0] + 2); P[1] = (char *)malloc((size_t)k + r->len[1] + 2);
        if (!P[0] || !P[1]) { free(P[0]); free(P[1]); return 1; }
        if (!kb_path(&G, r, 0, P[0]) || !kb_path(&G, r, 1, P[1])) { free(P[0]); free(P[1]); return 2; }
        L[0] = strlen(P[0]); L[1] = strlen(P[1]);
        size_t pre = 0, suf = 0;
        while (pre < L[0] && pre < L[1] && P[0][pre] == P[1][pre]) ++pre;               /* >= k: text(s) */
        while (suf < L[0] - pre && suf < L[1] - pre && P[0][L[0] - 1 - suf] == P[1][L[1] - 1 - suf]) ++suf;
        const size_t a0 = L[0] - pre - suf, a1 = L[1] - pre - suf, rf = suf < (size_t)k ? suf : (size_t)k;
        const char *type = a0 == 1 && a1 == 1 ? "SNP" : a0 == a1 && a0 > 1 ? "MNP" : (a0 == 0) != (a1 == 0) ? "INDEL" : "COMPLEX";
        fprintf(out, "BB\t%llu\t%s\t%.*s\t", (unsigned long long)x, type, k, P[0] + pre - k);
        if (a0) fprintf(out, "%.*s\t", (int)a0, P[0] + pre); else fputs("-\t", out);
        if (a1) fprintf(out, "%.*s\t", (int)a1, P[1] + pre); else fputs("-\t", out);
        fprintf(out, "%.*s\t%u\t%u\t%llu\t%llu\tkc:B:I", (int)rf, P[0] + L[0] - suf, r->len[0], r->len[1], (unsigned long long)u[0], (unsigned long long)u[1]);
        for (int br = 0; br < 2; ++br)
            for (int i = 0; i < n_idx; ++i) fprintf(out, ",%llu", (unsigned long long)g->u_count[u[br] * n_idx + i]);
        fputs("\tkn:B:I", out);
        for (int br = 0; br < 2; ++br)
            for (int i = 0; i < n_idx; ++i) fprintf(out, ",%u", g->u_present[u[br] * n_idx + i]);
        fputs("\tGT:Z:", out);
        for (int i = 0; i < n_idx; ++i) fprintf(out, "%s%c%c", i ? "," : "", held[0] >> i & 1u ? '1' : '0', held[1] >> i & 1u ? '1' : '0');
        fputc('\n', out);
        free(P[0]); free(P[1]);
    }
    return 0;
}

int fmdh_main_kbubble(int argc, char *argv[])
{
    int c, device = 0, differing = 0, rc = 0, n_idx;
    long long k = 21, min_occ = 2, max_len = 0;
    fmd_dev_t *d[FMD_KMAT_MAX_IDX] = { 0 };
    while ((c = getopt(argc, argv, "k:o:L:dg:")) >= 0) {
        if (c == 'k') k = atoll(optarg);
        else if (c == 'o') min_occ = atoll(optarg);
        else if (c == 'L') max_len = atoll(optarg);
        else if (c == 'd') differing = 1;
        else if (c == 'g') device = atoi(optarg);
    }
    n_idx = argc - optind;
    if (n_idx < 1 || n_idx > FMD_KMAT_MAX_IDX || k < 3 || k > 31 || !(k & 1) || min_occ < 1 || min_occ > 0x7fffffffll || max_len < 0 || max_len > 0xffffffffll) {
        fprintf(stderr, "\nUsage:   fermi-amd kbubble [-k 21] [-o 2] [-L 0] [-d] [-g GPU] <a.fmd> [<b.fmd> ...]\n\n");
        fprintf(stderr, "Options: -k INT    k-mer length, odd, 3..31 [21]\n");
        fprintf(stderr, "         -o INT    a k-mer or an arc is in an index where it occurs at least INT times, INT >= 1; a node is in some index [2]\n");
        fprintf(stderr, "         -L INT    only bubbles whose two branches have at most INT nodes each, 0 = any [0]\n");
        fprintf(stderr, "         -d        only the bubbles that the indexes do not all hold alike\n\n");
        fprintf(stderr, "Input:   1 to %d indexes of both strands\n", FMD_KMAT_MAX_IDX);
        fprintf(stderr, "Output:  SM nodes unitigs forks bubbles, then per bubble\n");
        fprintf(stderr, "         BB index type left allele_0 allele_1 right len_0 len_1 unitig_0 unitig_1 kc:B:I,.. kn:B:I,.. GT:Z:..\n\n");
        return 1;
    }
    for (int i = 0; i < n_idx; ++i) {
        FILE *fp = fopen(argv[optind + i], "rb");
        if (!fp) { fprintf(stderr, "[E::main_kbubble] fail to open file '%s'\n", argv[optind + i]); return 1; }
        fclose(fp);
    }
    if (fmd_device_count() <= 0) { fprintf(stderr, "[E::main] %s\n", fmd_strerror(FMD_E_NODEV)); return 1; }
    if (device < 0 || device >= fmd_device_count()) { fprintf(stderr, "[E::main_kbubble] GPU %d: this node has %d\n", device, fmd_device_count()); return 1; }
    for (int i = 0; i < n_idx && !rc; ++i) {
        rc = fmd_dev_open_file_ex(device, argv[optind + i], FMD_OPEN_EMPTY_OK, &d[i]);
        if (rc) fprintf(stderr, "[E::main_kbubble] cannot load `%s': %s\n", argv[optind + i], fmd_strerror(rc));
    }
    fmd_kcbubble_t o;
    memset(&o, 0, sizeof(o));
    if (!rc) {
        rc = fmd_kcbubble(n_idx, d, (int)k, (int)min_occ, (uint32_t)max_len, 0, &o);
        if (rc == FMD_E_ARG) fprintf(stderr, "[E::main_kbubble] one of the files is not an index of both strands: its base counts are not symmetric\n");
        else if (rc) fprintf(stderr, "[E::main_kbubble] %s\n", fmd_strerror(rc));
        else {
            o.g.n_idx = n_idx;
            printf("SM\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)o.g.n_nodes, (unsigned long long)o.g.n_unitigs, (unsigned long long)o.n_forks,
                   (unsigned long long)o.n_bubbles);
            if (fmdh_kbubble_print(stdout, (int)k, &o.g, o.n_bubbles, o.bubble, differing)) { fprintf(stderr, "[E::main_kbubble] out of memory\n"); rc = 1; }
            fprintf(stderr, "[M::main_kbubble] k=%d n=%d nodes=%llu unitigs=%llu forks=%llu bubbles=%llu\n", (int)k, n_idx, (unsigned long long)o.g.n_nodes,
                    (unsigned long long)o.g.n_unitigs, (unsigned long long)o.n_forks, (unsigned long long)o.n_bubbles);
        }
    }
    fmd_host_free(o.bubble);
    fmdh_kcgraph_free(&o.g);
    for (int i = 0; i < n_idx; ++i) fmd_dev_close(d[i]);
    return rc ? 1 : 0;
}
