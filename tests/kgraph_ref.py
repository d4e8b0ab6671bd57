"""The definitions of kgraph (include/fmd_hip.h) restated in plain Python, for tests/test_kgraph_host.py and tests/test_gpu_kgraph.py: COUNT from a dict
over the strings and their reverse complements, the arc bytes, the compactable links, the chains with their cycle and orientation rules, and the three
outputs of `fermi-amd kgraph`.  Nothing here calls the library."""
import numpy as np

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def pack(s):
    v = 0
    for c in s:
        v = v << 2 | CODE[c]
    return v


def unpack(v, k):
    return "".join("ACGT"[v >> (2 * (k - 1 - i)) & 3] for i in range(k))


def count_dict(strings, m):
    """COUNT of every m-mer: occurrences over the strings and their reverse complements, halved for an m-mer that is its own reverse complement;
    keyed by the canonical form"""
    occ = {}
    for s in strings:
        for t in (s, rc(s)):
            for j in range(len(t) - m + 1):
                w = t[j:j + m]
                if "N" not in w:
                    occ[w] = occ.get(w, 0) + 1
    out = {}
    for w, c in occ.items():
        r = rc(w)
        assert occ[r] == c
        if w <= r:
            out[w] = c // 2 if w == r else c
    return out


def graph_from_counts(cnt_k, cnt_k1, k, min_occ):
    """nodes (ascending canonical strings), their counts, their arc bytes"""
    nodes = sorted(w for w, c in cnt_k.items() if c >= min_occ)
    count = lambda w: cnt_k1.get(min(w, rc(w)), 0)
    arcs = []
    for x in nodes:
        a = 0
        for c in range(4):
            if count(x + "ACGT"[c]) >= min_occ:
                a |= 1 << c
            if count("ACGT"[c] + x) >= min_occ:
                a |= 16 << c
        arcs.append(a)
    return nodes, [cnt_k[x] for x in nodes], arcs


def graph_from_strings(strings, k, min_occ):
    return graph_from_counts(count_dict(strings, k), count_dict(strings, k + 1), k, min_occ)


class Compacted:
    pass


def compact(nodes, arcs, k, counts=None):
    """unitigs of the graph (nodes: ascending canonical strings; arcs: their bytes) by the definitions -> a Compacted with unitig / offset / orient per
    node, u_nodes / u_first / u_flags / strings / kc per unitig, paths (the oriented nodes of every unitig as printed) and n_arcs, n_links, n_cycles"""
    n = len(nodes)
    ident = {x: i for i, x in enumerate(nodes)}
    counts = [0] * n if counts is None else counts

    def text(u):
        return nodes[u[0]] if u[1] == 0 else rc(nodes[u[0]])

    def right(u):                                      # the bases c with an arc text(u) . c
        i, o = u
        return [c for c in range(4) if (arcs[i] >> c & 1 if o == 0 else arcs[i] >> (4 + 3 - c) & 1)]

    def left_n(u):
        return len(right((u[0], 1 - u[1])))

    def follow(u, c):
        v = text(u)[1:] + "ACGT"[c]
        r = rc(v)
        return (ident[min(v, r)], 0 if v < r else 1)

    nxt = {}
    for i in range(n):
        for o in (0, 1):
            r = right((i, o))
            if len(r) == 1:
                v = follow((i, o), r[0])
                if left_n(v) == 1 and v[0] != i:
                    nxt[(i, o)] = v
    for u, v in nxt.items():
        assert nxt[(v[0], 1 - v[1])] == (u[0], 1 - u[1])   # a link and its twin
    g = Compacted()
    g.unitig, g.offset, g.orient = [None] * n, [None] * n, [None] * n
    g.u_nodes, g.u_first, g.u_flags, g.strings, g.kc, g.paths = [], [], [], [], [], []
    g.n_links, g.n_cycles = len(nxt) // 2, 0
    pal = sum(1 for i in range(n) for c in right((i, 0)) if nodes[i] + "ACGT"[c] == rc(nodes[i] + "ACGT"[c])) + \
        sum(1 for i in range(n) for c in right((i, 1)) if rc(nodes[i]) + "ACGT"[c] == rc(rc(nodes[i]) + "ACGT"[c]))
    g.n_arcs = (sum(bin(a).count("1") for a in arcs) + pal) // 2
    for i in range(n):                                 # ascending: i is the smallest node of a chain not seen yet
        if g.unitig[i] is not None:
            continue
        u, cyc = (i, 0), False
        while (u[0], 1 - u[1]) in nxt:                 # back to where the chain starts
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
            assert nxt[path[-1]] == path[0]
            g.n_cycles += 1
        elif rc(s) < s:
            s, path = rc(s), [(v[0], 1 - v[1]) for v in reversed(path)]
        uid = len(g.u_nodes)
        for t, v in enumerate(path):
            assert g.unitig[v[0]] is None
            g.unitig[v[0]], g.offset[v[0]], g.orient[v[0]] = uid, t, v[1]
        assert min(v[0] for v in path) == i
        g.u_nodes.append(len(path)); g.u_first.append(path[0][0]); g.u_flags.append(1 if cyc else 0)
        g.strings.append(s); g.kc.append(sum(counts[v[0]] for v in path)); g.paths.append(path)
    g.n_unitigs = len(g.u_nodes)
    assert sum(g.u_nodes) == n and g.n_unitigs == n - g.n_links + g.n_cycles
    g.right, g.follow = right, follow
    return g


def gfa_text(g, k):
    out = ["H\tVN:Z:1.0\n"]
    for u, s in enumerate(g.strings):
        out.append("S\t%d\t%s\tKC:i:%d\tLN:i:%d\n" % (u, s, g.kc[u], len(s)))
    enter = {}
    for u, path in enumerate(g.paths):
        enter[(path[-1][0], 1 - path[-1][1])] = (u, 1)
    for u, path in enumerate(g.paths):
        enter[path[0]] = (u, 0)                        # (a unitig of one node read forward is entered as +)
    for a, path in enumerate(g.paths):
        for oa in (0, 1):
            end = path[-1] if oa == 0 else (path[0][0], 1 - path[0][1])
            for c in g.right(end):
                b, ob = enter[g.follow(end, c)]
                if (a, oa) <= (b, 1 - ob):
                    out.append("L\t%d\t%s\t%d\t%s\t%dM\n" % (a, "+-"[oa], b, "+-"[ob], k - 1))
    return "".join(out)


def fasta_text(g):
    return "".join(">%d KC:i:%d LN:i:%d\n%s\n" % (u, g.kc[u], len(s), s) for u, s in enumerate(g.strings))


def arcs_text(nodes, counts, arcs):
    return "".join("%s\t%d\t%s\t%s\n" % (x, counts[i], "".join("ACGT"[c] if arcs[i] >> c & 1 else "." for c in range(4)),
                                          "".join("ACGT"[c] if arcs[i] >> (4 + c) & 1 else "." for c in range(4))) for i, x in enumerate(nodes))


def np_revcomp(w, m):
    """the reverse complement of packed m-mers (numpy uint64)"""
    w = np.asarray(w, dtype=np.uint64)
    out = np.zeros_like(w)
    for i in range(m):
        out |= (np.uint64(3) - (w >> np.uint64(2 * i) & np.uint64(3))) << np.uint64(2 * (m - 1 - i))
    return out


def arcs_from_k1_list(km, k1, k):
    """the arc bytes of the ascending packed canonical k-mers km that the packed canonical (k+1)-mers k1 imply (numpy)"""
    km = np.asarray(km, dtype=np.uint64); k1 = np.asarray(k1, dtype=np.uint64)
    arcs = np.zeros(len(km), dtype=np.uint8)
    if not len(k1):
        return arcs
    revcomp = np_revcomp
    for q in (k1, revcomp(k1, k + 1)):                 # each (k+1)-mer in both orientations: its first k bases have it as a right arc
        x, c = q >> np.uint64(2), (q & np.uint64(3)).astype(np.int64)
        r = revcomp(x, k)
        fw = x < r
        node = np.searchsorted(km, np.where(fw, x, r))
        assert (node < len(km)).all() and np.array_equal(km[node], np.where(fw, x, r)), "a (k+1)-mer whose k-mer is not listed"
        np.bitwise_or.at(arcs, node, np.where(fw, 1 << c, 16 << (3 - c)).astype(np.uint8))
    return arcs


# The hand-made graphs: name -> (k, min_occ, reads).  What each is for is asserted where it is used (check_shape).
SHAPES = {
    "path": (5, 1, ["TTTCCTCATGCAATTC"]),
    "bubble": (5, 1, ["AGTAAACACATTTTA", "AGTAAACCCATTTTA"]),
    "tip": (5, 1, ["CCTGAGGTAAACCAGG", "AGGTATC"]),
    "cycle": (5, 1, ["AATGTAGGCGAAAT" + "AATGT"]),            # a circle of 14 bases, read once round and k bases on
    "homopolymer": (5, 1, ["GTCAAAAAAAACTG"]),
    "hairpin": (5, 1, ["GGATACGCGTCAA"]),                      # ACGCGT is its own reverse complement
    "hairpin_halved": (5, 2, ["GGATACGCGTCAA", "GGATACG", "GGATACG", "CGCGTCAA", "CGCGTCAA"]),   # occ(ACGCGT) = 2, COUNT = 1 < min_occ
    "opposite": (5, 1, ["AAAGTT"]),                            # AAAGT forward, then AAGTT = rc(AACTT): two nodes, the second reversed
    "empty": (5, 1, []),
    "single": (5, 1, ["ACCGT"]),
}


def check_shape(name, nodes, counts, arcs, g):
    """the property each hand-made graph is there for, on the restated result"""
    k = SHAPES[name][0]
    idx = {x: i for i, x in enumerate(nodes)}
    if name == "path":
        assert g.n_unitigs == 1 and g.n_links == len(nodes) - 1 == 11 and g.n_cycles == 0 and 0 < sum(g.orient) < 12
    elif name == "bubble":
        assert g.n_unitigs == 4 and sorted(g.u_nodes) == [3, 3, 5, 5] and g.n_cycles == 0
    elif name == "tip":
        assert g.n_unitigs == 3 and 2 in g.u_nodes
    elif name == "cycle":
        assert g.n_unitigs == 1 and g.n_cycles == 1 and g.u_flags == [1] and g.n_links == len(nodes) == 14
        first = SHAPES[name][2][0][:k]
        assert nodes[g.u_first[0]] != min(first, rc(first)) and g.u_first[0] == 0 and g.orient[0] == 0 and len(g.strings[0]) == 14 + k - 1
    elif name == "homopolymer":
        i = idx["AAAAA"]
        assert arcs[i] & 0x11 == 0x11 and g.u_nodes[g.unitig[i]] == 1     # A^k -> A^k on both sides, and it is an end
    elif name == "hairpin":
        i = idx["ACGCG"]
        assert arcs[i] >> 3 & 1 and g.offset[i] == g.u_nodes[g.unitig[i]] - 1 and g.n_arcs == len(count_dict(SHAPES[name][2], k + 1))
    elif name == "hairpin_halved":
        i = idx["ACGCG"]
        assert counts[i] >= 2 and not arcs[i] >> 3 & 1
    elif name == "opposite":
        assert nodes == ["AAAGT", "AACTT"] and g.n_unitigs == 1 and g.orient == [0, 1] and g.strings == ["AAAGTT"]
    elif name == "empty":
        assert nodes == [] and g.n_unitigs == 0
    elif name == "single":
        assert nodes == ["ACCGT"] and g.strings == ["ACCGT"] and arcs == [0]
