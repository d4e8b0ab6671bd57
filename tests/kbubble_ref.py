"""The definitions of kbubble (include/fmd_hip.h) restated in plain Python on top of tests/kcgraph_ref.py and tests/kgraph_ref.py, for
tests/test_kbubble_host.py and tests/test_gpu_kbubble.py: oriented nodes 2 * id + o, the branch rule walked node by node, every bubble found from both of
its sides with the two findings asserted to mirror each other, the alleles, and the lines of `fermi-amd kbubble`.  Nothing here calls the library."""
import kgraph_ref as R
import kcgraph_ref as KR


class Graph:
    """the node graph: ascending canonical strings and their (union) arc bytes"""

    def __init__(self, nodes, arcs, k):
        self.nodes, self.arcs, self.k, self.n = nodes, arcs, k, len(nodes)
        self.ident = {x: i for i, x in enumerate(nodes)}

    def text(self, u):
        return R.rc(self.nodes[u >> 1]) if u & 1 else self.nodes[u >> 1]

    def right(self, u):
        a = self.arcs[u >> 1]
        return [c for c in range(4) if (a >> (4 + 3 - c) & 1 if u & 1 else a >> c & 1)]

    def left_n(self, u):
        return len(self.right(u ^ 1))

    def follow(self, u, c):
        v = self.text(u)[1:] + "ACGT"[c]
        r = R.rc(v)
        return 2 * self.ident[min(v, r)] + (0 if v < r else 1)

    def branch(self, a):
        """the branch that starts at a -> (target, its nodes), or None"""
        if self.left_n(a) != 1:
            return None
        path = [a]
        while True:
            assert len(path) <= 2 * self.n, "a chain that does not end"
            r = self.right(path[-1])
            if len(r) != 1:
                return None
            w = self.follow(path[-1], r[0])
            if self.left_n(w) != 1:
                return w, path
            path.append(w)


def find(G, max_len=0):
    """-> (n_forks, records): every bubble from both sides, mirrored; records = (src, dst, first_0, first_1, len_0, len_1) ascending by src, one per bubble"""
    met, n_forks = {}, 0
    for s in range(2 * G.n):
        r = G.right(s)
        if len(r) != 2:
            continue
        n_forks += 1
        A, B = G.branch(G.follow(s, r[0])), G.branch(G.follow(s, r[1]))
        if A is None or B is None or A[0] != B[0]:
            continue
        t = A[0]
        if G.left_n(t) != 2 or t >> 1 == s >> 1:
            continue
        if max_len and (len(A[1]) > max_len or len(B[1]) > max_len):
            continue
        met[s] = (t, A[1], B[1])
    rev = lambda path: tuple(v ^ 1 for v in reversed(path))
    for s, (t, A, B) in met.items():
        m = met.get(t ^ 1)
        assert m is not None and m[0] == s ^ 1 and {tuple(m[1]), tuple(m[2])} == {rev(A), rev(B)}, (s, t)
        ids = [v >> 1 for v in A + B]
        assert len(set(ids)) == len(ids) and s >> 1 not in ids and t >> 1 not in ids            # the consequences the header names
    recs = [(s, t, A[0], B[0], len(A), len(B)) for s, (t, A, B) in sorted(met.items()) if s >> 1 < t >> 1]
    assert 2 * len(recs) == len(met)
    return n_forks, recs


def paths(G, rec):
    """P_0, P_1 of a record"""
    out = []
    for b in (0, 1):
        s, v = G.text(rec[0]), rec[2 + b]
        for _ in range(rec[4 + b]):
            s += G.text(v)[-1]
            v = G.follow(v, G.right(v)[0])
        assert v == rec[1]
        out.append(s + G.text(v)[-1])
    return out


def alleles(G, rec):
    """(type, left flank, allele_0, allele_1, right flank)"""
    P, k = paths(G, rec), G.k
    pre = 0
    while pre < min(len(P[0]), len(P[1])) and P[0][pre] == P[1][pre]:
        pre += 1
    assert pre >= k
    rest = [p[pre:] for p in P]
    suf = 0
    while suf < min(len(rest[0]), len(rest[1])) and rest[0][-1 - suf] == rest[1][-1 - suf]:
        suf += 1
    a = [r[:len(r) - suf] for r in rest]
    common = rest[0][len(rest[0]) - suf:]
    if len(a[0]) == 1 and len(a[1]) == 1:
        kind = "SNP"
    elif len(a[0]) == len(a[1]) and len(a[0]) > 1:
        kind = "MNP"
    elif (a[0] == "") != (a[1] == ""):
        kind = "INDEL"
    else:
        kind = "COMPLEX"
    return kind, P[0][pre - k:pre], a[0] or "-", a[1] or "-", common[:k]


def codes(g, rec):
    """per colour the two characters of GT: does it hold branch 0, branch 1"""
    u = [g.unitig[rec[2] >> 1], g.unitig[rec[3] >> 1]]
    return ["".join("1" if g.u_present[x][i] == g.u_nodes[x] else "0" for x in u) for i in range(g.n_idx)]


def text(G, g, recs, differing_only=False):
    """the BB lines; g = kcgraph_ref.compact(.., split=False) of the same graph"""
    out = []
    for x, rec in enumerate(recs):
        u = [g.unitig[rec[2] >> 1], g.unitig[rec[3] >> 1]]
        assert g.u_nodes[u[0]] == rec[4] and g.u_nodes[u[1]] == rec[5] and u[0] != u[1]           # a branch is one whole unitig
        gt = codes(g, rec)
        if differing_only and len(set(gt)) == 1:
            continue
        kind, left, a0, a1, right = alleles(G, rec)
        out.append("BB\t%d\t%s\t%s\t%s\t%s\t%s\t%d\t%d\t%d\t%d\tkc:B:I,%s\tkn:B:I,%s\tGT:Z:%s\n" % (
            x, kind, left, a0, a1, right, rec[4], rec[5], u[0], u[1], ",".join("%d" % v for b in u for v in g.u_count[b]),
            ",".join("%d" % v for b in u for v in g.u_present[b]), ",".join(gt)))
    return "".join(out)


def sm_text(g, n_forks, n_bubbles):
    return "SM\t%d\t%d\t%d\t%d\n" % (len(g.unitig), g.n_unitigs, n_forks, n_bubbles)


class Called:
    pass


def call(colours, k, min_occ, max_len=0):
    """everything for N lists of strings: the joint graph, its unsplit compaction, the bubbles and the printed text"""
    c = Called()
    c.k, c.n_idx = k, len(colours)
    c.nodes, c.counts, c.arcs, c.uarcs, c.pattern = KR.joint_graph(colours, k, min_occ)
    return finish(c, max_len)


def finish(c, max_len=0):
    c.g = KR.compact(c.nodes, c.uarcs, c.pattern, c.k, c.counts, False)
    c.g.n_idx = c.n_idx
    c.G = Graph(c.nodes, c.uarcs, c.k)
    c.n_forks, c.recs = find(c.G, max_len)
    c.text, c.text_d = text(c.G, c.g, c.recs), text(c.G, c.g, c.recs, True)
    c.sm = sm_text(c.g, c.n_forks, len(c.recs))
    return c


def from_arrays(km, counts, uarcs, pattern, k, max_len=0):
    """the same from a graph given as numpy arrays (packed k-mers, counts[n, N], union bytes, patterns)"""
    c = Called()
    c.k, c.n_idx = k, counts.shape[1]
    c.nodes, c.counts, c.uarcs, c.pattern = [R.unpack(int(x), k) for x in km], counts.tolist(), uarcs.tolist(), pattern.tolist()
    return finish(c, max_len)


def as_tuples(bubbles):
    """an api.KBUBBLE_DT array as the records of find()"""
    return [(int(b["src"]), int(b["dst"]), int(b["first"][0]), int(b["first"][1]), int(b["len"][0]), int(b["len"][1])) for b in bubbles]
