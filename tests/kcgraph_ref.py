"""The definitions of kcgraph (include/fmd_hip.h) restated in plain Python on top of tests/kgraph_ref.py, for tests/test_kcgraph_host.py and
tests/test_gpu_kcgraph.py: the joint graph of N lists of strings by count dicts (a node is a canonical k-mer with COUNT >= min_occ in SOME colour, arcs per
colour and their union), the compaction on the union byte with and without the split rule, the per-unitig sums, and the three outputs of `fermi-amd
kcgraph`.  Nothing here calls the library."""
import kgraph_ref as R


def joint_graph_from_counts(cnt_k, cnt_k1, k, min_occ):
    """cnt_k[i], cnt_k1[i]: COUNT of the canonical k-mers and (k+1)-mers of colour i -> nodes (ascending canonical strings), counts[n][N], arcs[n][N],
    uarcs[n], pattern[n]"""
    n_idx = len(cnt_k)
    nodes = sorted(set(w for d in cnt_k for w, c in d.items() if c >= min_occ))
    counts, arcs, uarcs, pattern = [], [], [], []
    for x in nodes:
        row = []
        for i in range(n_idx):
            cnt = lambda w: cnt_k1[i].get(min(w, R.rc(w)), 0)
            a = 0
            for c in range(4):
                if cnt(x + "ACGT"[c]) >= min_occ:
                    a |= 1 << c
                if cnt("ACGT"[c] + x) >= min_occ:
                    a |= 16 << c
            row.append(a)
        counts.append([d.get(x, 0) for d in cnt_k])
        arcs.append(row)
        u = 0
        for a in row:
            u |= a
        uarcs.append(u)
        pattern.append(sum(1 << i for i in range(n_idx) if counts[-1][i] >= min_occ))
        assert pattern[-1] != 0
    return nodes, counts, arcs, uarcs, pattern


def joint_graph(string_lists, k, min_occ):
    return joint_graph_from_counts([R.count_dict(s, k) for s in string_lists], [R.count_dict(s, k + 1) for s in string_lists], k, min_occ)


def compact(nodes, uarcs, pattern, k, counts, split=False):
    """kgraph_ref.compact on the union bytes, a link compactable under `split` only between nodes of one pattern; plus u_count / u_present / u_pattern
    (lists of N per unitig) and kc = the sum of u_count over the colours"""
    n = len(nodes)
    n_idx = len(counts[0]) if n else 0
    if not split:
        g = R.compact(nodes, uarcs, k)
    else:
        g = _compact_split(nodes, uarcs, pattern, k)
    g.n_idx = n_idx
    g.u_count = [[sum(counts[v[0]][i] for v in path) for i in range(n_idx)] for path in g.paths]
    g.u_present = [[sum(pattern[v[0]] >> i & 1 for v in path) for i in range(n_idx)] for path in g.paths]
    g.u_pattern = []
    for path in g.paths:
        p = 0
        for v in path:
            p |= pattern[v[0]]
        g.u_pattern.append(p)
    g.kc = [sum(row) for row in g.u_count]
    if split:
        assert all(pattern[v[0]] == g.u_pattern[u] for u, path in enumerate(g.paths) for v in path)
    return g


def _compact_split(nodes, arcs, pattern, k):
    """kgraph_ref.compact, its link rule with one more condition: both nodes have the same pattern"""
    n = len(nodes)
    ident = {x: i for i, x in enumerate(nodes)}

    def text(u):
        return nodes[u[0]] if u[1] == 0 else R.rc(nodes[u[0]])

    def right(u):
        i, o = u
        return [c for c in range(4) if (arcs[i] >> c & 1 if o == 0 else arcs[i] >> (4 + 3 - c) & 1)]

    def left_n(u):
        return len(right((u[0], 1 - u[1])))

    def follow(u, c):
        v = text(u)[1:] + "ACGT"[c]
        r = R.rc(v)
        return (ident[min(v, r)], 0 if v < r else 1)

    nxt = {}
    for i in range(n):
        for o in (0, 1):
            r = right((i, o))
            if len(r) == 1:
                v = follow((i, o), r[0])
                if left_n(v) == 1 and v[0] != i and pattern[v[0]] == pattern[i]:
                    nxt[(i, o)] = v
    for u, v in nxt.items():
        assert nxt[(v[0], 1 - v[1])] == (u[0], 1 - u[1])
    g = R.Compacted()
    g.unitig, g.offset, g.orient = [None] * n, [None] * n, [None] * n
    g.u_nodes, g.u_first, g.u_flags, g.strings, g.paths = [], [], [], [], []
    g.n_links, g.n_cycles = len(nxt) // 2, 0
    g.n_arcs = R.compact(nodes, arcs, k).n_arcs
    for i in range(n):
        if g.unitig[i] is not None:
            continue
        u, cyc = (i, 0), False
        while (u[0], 1 - u[1]) in nxt:
            p = nxt[(u[0], 1 - u[1])]
            u = (p[0], 1 - p[1])
            if u[0] == i:
                cyc = True
                break
        path = [(i, 0)] if cyc else [u]
        while path[-1] in nxt and nxt[path[-1]] != path[0]:
            path.append(nxt[path[-1]])
        s = text(path[0]) + "".join(text(v)[-1] for v in path[1:])
        if cyc:
            g.n_cycles += 1
        elif R.rc(s) < s:
            s, path = R.rc(s), [(v[0], 1 - v[1]) for v in reversed(path)]
        uid = len(g.u_nodes)
        for t, v in enumerate(path):
            assert g.unitig[v[0]] is None
            g.unitig[v[0]], g.offset[v[0]], g.orient[v[0]] = uid, t, v[1]
        assert min(v[0] for v in path) == i
        g.u_nodes.append(len(path)); g.u_first.append(path[0][0]); g.u_flags.append(1 if cyc else 0)
        g.strings.append(s); g.paths.append(path)
    g.n_unitigs = len(g.u_nodes)
    assert sum(g.u_nodes) == n and g.n_unitigs == n - g.n_links + g.n_cycles
    g.right, g.follow = right, follow
    return g


def bits(p, n_idx):
    return "".join("1" if p >> i & 1 else "0" for i in range(n_idx))


def _tags(g, u, sep):
    return sep + "kc:B:I" + "".join(",%d" % v for v in g.u_count[u]) + sep + "kn:B:I" + "".join(",%d" % v for v in g.u_present[u])


def _shown(g, pattern):
    return [pattern is None or bits(p, g.n_idx) == pattern for p in g.u_pattern]


def gfa_text(g, k, pattern=None):
    """kgraph_ref.gfa_text with the two tags, and with `pattern` (the bits of -p) only the unitigs of that pattern and the links between them"""
    show = _shown(g, pattern)
    out = ["H\tVN:Z:1.0\n"]
    for u, s in enumerate(g.strings):
        if show[u]:
            out.append("S\t%d\t%s\tKC:i:%d\tLN:i:%d%s\n" % (u, s, g.kc[u], len(s), _tags(g, u, "\t")))
    for ln in R.gfa_text(g, k).splitlines(True):
        if ln.startswith("L\t"):
            f = ln.split("\t")
            if show[int(f[1])] and show[int(f[3])]:
                out.append(ln)
    return "".join(out)


def fasta_text(g, pattern=None):
    show = _shown(g, pattern)
    return "".join(">%d KC:i:%d LN:i:%d PT:Z:%s%s\n%s\n" % (u, g.kc[u], len(s), bits(g.u_pattern[u], g.n_idx), _tags(g, u, " "), s)
                   for u, s in enumerate(g.strings) if show[u])


def _arc_text(a):
    return "".join("ACGT"[c] if a >> c & 1 else "." for c in range(4)), "".join("ACGT"[c] if a >> (4 + c) & 1 else "." for c in range(4))


def arcs_text(nodes, counts, arcs, uarcs, min_occ):
    out = []
    for j, x in enumerate(nodes):
        n_idx = len(counts[j])
        out.append("%s\t%s\t%s\t%s\t%s%s\n" % (x, ",".join("%d" % c for c in counts[j]), "".join("1" if c >= min_occ else "0" for c in counts[j]),
                                             _arc_text(uarcs[j])[0], _arc_text(uarcs[j])[1], "".join("\t%s/%s" % _arc_text(arcs[j][i]) for i in range(n_idx))))
    return "".join(out)
