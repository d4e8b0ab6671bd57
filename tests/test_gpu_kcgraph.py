"""GPU: kcgraph (fmd_kcarcs / fmd_kcunitig, api.kmer_joint_arcs / kmer_joint_unitigs, `fermi-amd kcgraph`) against brute force over the forward sequences as
indexed (the oracle of tests/test_gpu_kgraph.py, one per colour, joined here in numpy), against kgraph and kcount of every handle alone, against the one-thread
host walk (fmdh_kcgraph_compact_host) and -- on the small sets -- against the definitions restated in Python (tests/kcgraph_ref.py).  Every comparison is exact."""
import os
import random
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib
import kgraph_ref as R
import kcgraph_ref as KR
from test_gpu_kgraph import Want, forward_as_indexed, windows_packed, nt6, circle_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
EMPTY = "sub.empty"
EIGHT = ("ctA", "ctB", "cnA", "cnB", "tiny", "repeat", "palin", "special")
LABELS = ("unitig", "offset", "orient", "u_nodes", "u_first", "u_flags")
SUMS = ("u_count", "u_present", "u_pattern")


def gold(name):
    return os.path.join(GOLD, name + ".fmd")


class Joint:
    """brute force for named read sets: per set a Want, per (names, k, min_occ) the joint graph, computed once and never changed"""

    def __init__(self):
        self.sets, self.graphs = {EMPTY: Want([])}, {}

    def want(self, name):
        if name not in self.sets:
            self.sets[name] = Want(forward_as_indexed(name))
        return self.sets[name]

    def graph(self, names, k, min_occ, wants=None):
        """(kmers, counts[n, N], arcs[n, N], uarcs, pattern, n_arcs of the union, n_arcs per colour)"""
        key = (tuple(names) if names is not None else None, k, min_occ)
        if wants is not None or key not in self.graphs:
            ws = wants if wants is not None else [self.want(n) for n in names]
            per = [w.graph(k, min_occ) for w in ws]
            km = np.unique(np.concatenate([p[0] for p in per] + [np.zeros(0, np.uint64)]))
            counts, arcs = np.zeros((len(km), len(ws)), np.uint32), np.zeros((len(km), len(ws)), np.uint8)
            k1s = []
            for i, w in enumerate(ws):
                tk, tc = w.table(k)                       # the exact count, also below min_occ
                if len(tk) and len(km):
                    pos = np.minimum(np.searchsorted(tk, km), len(tk) - 1)
                    hit = tk[pos] == km
                    counts[hit, i] = np.minimum(tc[pos[hit]], 2 ** 32 - 1)
                arcs[np.searchsorted(km, per[i][0]), i] = per[i][2]
                t1, c1 = w.table(k + 1)
                k1s.append(t1[c1 >= min_occ])
            pattern = np.zeros(len(km), np.uint8)
            for i in range(len(ws)):
                pattern |= ((counts[:, i] >= min_occ).astype(np.uint8) << i).astype(np.uint8)
            out = (km, counts, arcs, np.bitwise_or.reduce(arcs, axis=1) if len(ws) else np.zeros(len(km), np.uint8), pattern,
                   len(np.unique(np.concatenate(k1s + [np.zeros(0, np.uint64)]))), [len(x) for x in k1s])
            if wants is not None:
                return out
            self.graphs[key] = out
        return self.graphs[key]


@pytest.fixture(scope="module")
def joint():
    return Joint()


class Open:
    """golden indexes open for a test, one handle per distinct name"""

    def __init__(self, gpu, names, opener=None):
        opener = opener or (lambda n: gpu.DevIndex.open(gold(n), empty_ok=(n == EMPTY)))
        self.by_name = {n: opener(n) for n in dict.fromkeys(names)}
        self.idx = [self.by_name[n] for n in names]

    def __enter__(self):
        return self.idx

    def __exit__(self, *exc):
        for d in self.by_name.values():
            d.close()


def same(got, ref, fields):
    for f in fields:
        a = getattr(got, f)
        b = np.asarray(getattr(ref, f), dtype=a.dtype).reshape(a.shape)
        assert np.array_equal(a, b), (f, np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[:8])


def restated(km, counts, uarcs, pattern, k, split):
    return KR.compact([R.unpack(int(x), k) for x in km], uarcs.tolist(), pattern.tolist(), k, counts.tolist(), split)


def check(idx, want, k, min_occ, restate=False, cap=0, alone=True):
    """one joint graph of the open indexes against want = Joint.graph(..) -> {split: KCUnitigs}"""
    km, ct, ar, ua, pt, n_arcs, n_arcs_in = want
    n_idx = len(idx)
    # (i) nodes, counts, arcs per colour, union: brute force
    slices = []
    gk, gc, ga, gu, st = api.kmer_joint_arcs(idx, k, min_occ, cap=cap, with_stat=True, slices=slices)
    assert gk.dtype == np.uint64 and gc.dtype == np.uint32 and ga.dtype == np.uint8 and gu.dtype == np.uint8 and gc.shape == ga.shape == (len(gk), n_idx)
    assert np.array_equal(gk, km), (k, min_occ, len(gk), len(km))
    assert np.array_equal(gc, ct), np.argwhere(gc != ct)[:8]
    assert np.array_equal(ga, ar), np.argwhere(ga != ar)[:8]
    assert np.array_equal(gu, ua) and sum(slices) == len(km)
    assert st["n_nodes"] == len(km) and st["n_arcs"] == n_arcs and st["n_links"] == 0 and st["n_unitigs"] == 0
    assert st["n_nodes_in"] == [int((pt >> i & 1).sum()) for i in range(n_idx)] and st["n_arcs_in"] == n_arcs_in
    assert (pt != 0).all() and not (ga[(pt[:, None] >> np.arange(n_idx) & 1) == 0]).any()      # an arc bit in colour i implies pattern bit i
    # (ii) the slice of colour i is what kgraph and kcount say of handle i alone
    for i, d in enumerate(idx if alone else []):
        if idx.index(d) != i:
            continue
        ak, ac, aa, ast = d.kmer_arcs(k, min_occ, with_stat=True)
        sel = (pt >> i & 1).astype(bool)
        assert np.array_equal(gk[sel], ak) and np.array_equal(gc[sel, i], ac) and np.array_equal(ga[sel, i], aa) and not ga[~sel, i].any()
        assert st["n_nodes_in"][i] == ast["n_nodes"] and st["n_arcs_in"][i] == ast["n_arcs"] == len(d.kmer_counts(k + 1, min_occ)[0])
    # the union byte is symmetric: every arc bit as an oriented (k+1)-mer is seen from both its nodes, once when they are one
    bits = []
    for c in range(4):
        bits.append(km[(ua >> c & 1).astype(bool)] << np.uint64(2) | np.uint64(c))
        bits.append(np.uint64(c) << np.uint64(2 * k) | km[(ua >> (4 + c) & 1).astype(bool)])
    bits = np.concatenate(bits)
    u, cnt = np.unique(np.minimum(bits, R.np_revcomp(bits, k + 1)), return_counts=True)
    assert len(u) == n_arcs and np.array_equal(cnt, np.where(u == R.np_revcomp(u, k + 1), 1, 2))
    # (iii) the labelling and the sums: the one-thread walk, and the restatement
    out = {}
    for split in (False, True):
        g = api.kmer_joint_unitigs(idx, k, min_occ, split=split, cap=cap, with_stat=True)
        assert np.array_equal(g.kmers, km) and np.array_equal(g.counts, ct) and np.array_equal(g.arcs, ar) and np.array_equal(g.uarcs, ua) and np.array_equal(g.pattern, pt)
        host = hostlib.kcgraph_compact_host(k, km, ct, ua, pt, split=split)
        same(g, host, LABELS + SUMS)
        s = g.stat
        for f in ("n_nodes", "n_arcs", "n_links", "n_unitigs", "n_cycles", "n_nodes_in"):
            assert s[f] == host.stat[f], (f, s[f], host.stat[f])
        assert s["n_arcs"] == n_arcs and s["n_arcs_in"] == n_arcs_in and s["n_unitigs"] == len(g.u_nodes) == s["n_nodes"] - s["n_links"] + s["n_cycles"]
        assert s["n_ext"] >= len(km) and (len(km) == 0 or s["n_rounds"] >= 1)
        uc = np.zeros(g.u_count.shape, np.uint64)
        np.add.at(uc, g.unitig.astype(np.int64), ct.astype(np.uint64))
        assert np.array_equal(g.u_count, uc) and int(g.u_nodes.sum()) == len(km)
        if split:
            assert np.array_equal(g.u_pattern[g.unitig], pt)                             # every unitig has one pattern
        if restate:
            ref = restated(km, ct, ua, pt, k, split)
            same(g, ref, LABELS + SUMS)
            assert g.strings() == ref.strings and (s["n_arcs"], s["n_links"], s["n_cycles"]) == (ref.n_arcs, ref.n_links, ref.n_cycles)
            assert hostlib.kcgraph_gfa_text(g) == KR.gfa_text(ref, k) and hostlib.kcgraph_fasta_text(g) == KR.fasta_text(ref)
        out[split] = g
    return out


# ---- 1. across N ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("tiny", 21), ("repeat", 21), ("palin", 5), ("special", 11), ("special", 3), ("tiny", 31)])
def test_one_index_is_kgraph(gpu, joint, name, k):
    with Open(gpu, (name,)) as idx:
        for min_occ in (1, 2):
            g = check(idx, joint.graph((name,), k, min_occ), k, min_occ)
            p = idx[0].kmer_unitigs(k, min_occ, with_stat=True)
            for split in (False, True):
                same(g[split], p, LABELS)
                assert np.array_equal(g[split].counts[:, 0], p.counts) and np.array_equal(g[split].arcs[:, 0], p.arcs) and np.array_equal(g[split].uarcs, p.arcs)
                for f in ("n_nodes", "n_arcs", "n_links", "n_unitigs", "n_cycles"):
                    assert g[split].stat[f] == p.stat[f], f
                assert g[split].stat["n_nodes_in"] == [p.stat["n_nodes"]] and g[split].stat["n_arcs_in"] == [p.stat["n_arcs"]]
                strip = lambda text: "".join(ln.split("\tkc:B:I")[0] + "\n" if ln.startswith("S\t") else ln for ln in text.splitlines(True))
                assert strip(hostlib.kcgraph_gfa_text(g[split])) == hostlib.kgraph_gfa_text(p)


@pytest.mark.parametrize("k", (3, 5, 11, 21, 31))
def test_two_indexes(gpu, joint, k):
    with Open(gpu, ("ctA", "ctB")) as idx:
        for min_occ in (1, 2, 3):
            check(idx, joint.graph(("ctA", "ctB"), k, min_occ), k, min_occ, alone=(min_occ == 2))


@pytest.mark.parametrize("names,k,min_occ", [(("ctA", "ctB", "cnA"), 21, 2), (("palin", "special", "tiny"), 5, 1), (("palin", "special", "tiny"), 11, 3),
                                             (("ctA", "ctB", "cnA", "tiny", "palin"), 21, 2), (("ctA", "ctB", "cnA", "tiny", "palin"), 31, 1), (EIGHT, 21, 2)])
def test_three_five_and_eight_indexes(gpu, joint, names, k, min_occ):
    with Open(gpu, names) as idx:
        check(idx, joint.graph(names, k, min_occ), k, min_occ)


# ---- 2. handles and colours ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (2, 8))
def test_the_same_handle_n_times(gpu, joint, n):
    with Open(gpu, ("repeat",) * n) as idx:
        assert len(idx) == n and all(d is idx[0] for d in idx)
        g = check(idx, joint.graph(("repeat",) * n, 21, 2), 21, 2)[True]
        p = idx[0].kmer_unitigs(21, 2)
        same(g, p, LABELS)
        for i in range(n):
            assert np.array_equal(g.counts[:, i], p.counts) and np.array_equal(g.arcs[:, i], p.arcs)
        assert np.array_equal(g.uarcs, p.arcs) and (g.pattern == (1 << n) - 1).all()


def test_a_permutation_permutes_the_columns(gpu, joint):
    names, perm = ("ctA", "palin", "special", "ctB"), (2, 0, 3, 1)
    with Open(gpu, names) as idx:
        a = api.kmer_joint_unitigs(idx, 11, 2, split=True)
        b = api.kmer_joint_unitigs([idx[j] for j in perm], 11, 2, split=True)
        check([idx[j] for j in perm], joint.graph(tuple(names[j] for j in perm), 11, 2), 11, 2, alone=False)
    same(b, a, LABELS + ("kmers", "uarcs"))
    for f in ("counts", "arcs", "u_count", "u_present"):
        assert np.array_equal(getattr(b, f), getattr(a, f)[:, list(perm)]), f
    for f in ("pattern", "u_pattern"):
        assert np.array_equal(getattr(b, f), sum(((getattr(a, f) >> j & 1) << i) for i, j in enumerate(perm)).astype(np.uint8)), f


@pytest.mark.parametrize("place", (0, 1, 2))
def test_an_empty_index_is_an_empty_colour(gpu, joint, place):
    names = ["palin", "special"]
    names.insert(place, EMPTY)
    with Open(gpu, names) as idx:
        g = check(idx, joint.graph(tuple(names), 11, 1), 11, 1, restate=True)[False]
        assert not g.counts[:, place].any() and not g.arcs[:, place].any() and not (g.pattern >> place & 1).any() and len(g.kmers) > 100
    with Open(gpu, (EMPTY, EMPTY)) as idx:
        g = check(idx, joint.graph((EMPTY, EMPTY), 21, 1), 21, 1, restate=True)[True]
        assert len(g.kmers) == 0 and len(g.u_nodes) == 0 and g.strings() == [] and hostlib.kcgraph_gfa_text(g) == "H\tVN:Z:1.0\n"


def test_palindromic_arcs_are_halved_per_colour(gpu, joint):
    names, k = ("palin", "tiny"), 5
    with Open(gpu, names) as idx:
        got = {mo: check(idx, joint.graph(names, k, mo), k, mo, restate=(mo == 2))[False] for mo in (1, 2, 3)}
    flips = 0
    for mo in (2, 3):                                      # an arc through a (k+1)-mer that is its own reverse complement, there at mo - 1 and gone at mo, in some colour,
        a, b = got[mo - 1], got[mo]                        # while its node stays in that colour with an occ of the (k+1)-mer of at least mo: only the halving drops it
        pos = np.searchsorted(a.kmers, b.kmers)
        for i, name in enumerate(names):
            t1, c1 = joint.want(name).table(k + 1)
            for c in range(4):
                w = b.kmers << np.uint64(2) | np.uint64(c)
                pal = w == R.np_revcomp(w, k + 1)
                gone = pal & (a.arcs[pos, i] >> c & 1).astype(bool) & ~(b.arcs[:, i] >> c & 1).astype(bool)
                for x in w[gone]:
                    j = int(np.searchsorted(t1, x))
                    assert t1[j] == x and c1[j] == mo - 1  # COUNT = occ / 2
                    flips += 2 * int(c1[j]) >= mo
    assert flips >= 1


# ---- 3. the any-rule, and compaction on hand-made graphs, as reads -----------------------------------------------------------------------------------------------
def open_reads(gpu, reads):
    return gpu.DevIndex.from_bwt(gpu.build_bwt([nt6(r) for r in reads])) if reads else gpu.DevIndex.open(gold(EMPTY), empty_ok=True)


def check_reads(gpu, joint, colours, k, min_occ):
    idx = [open_reads(gpu, reads) for reads in colours]
    try:
        want = joint.graph(None, k, min_occ, wants=[Want([nt6(r) for r in reads]) for reads in colours])
        got = check(idx, want, k, min_occ, restate=True)
        nodes, counts, arcs, uarcs, pattern = KR.joint_graph(colours, k, min_occ)   # the dicts over both strands give what the window counts give
        g = got[False]
        assert [R.pack(x) for x in nodes] == g.kmers.tolist() and counts == g.counts.tolist() and arcs == g.arcs.tolist() and uarcs == g.uarcs.tolist()
        return nodes, got
    finally:
        for d in idx:
            d.close()


def test_the_any_rule(gpu, joint):
    k, _, reads = R.SHAPES["path"]
    s = reads[0]
    one = [s[:9]] * 2 + [s[6:]] * 2 + [s]                  # the k-mer at 5 is in s alone: min_occ - 1 = 1 in each colour, 2 in their sum
    m = min(s[5:10], R.rc(s[5:10]))
    nodes, got = check_reads(gpu, joint, [one, one], k, 2)
    assert m not in nodes and len(nodes) == 11 and len(got[False].u_nodes) == 2
    nodes, got = check_reads(gpu, joint, [one, one], k, 1)
    assert m in nodes and len(nodes) == 12 and len(got[False].u_nodes) == 1
    nodes, got = check_reads(gpu, joint, [one, [s] * 2, one], k, 2)   # a colour that does reach it makes the node, for every colour
    assert m in nodes and got[False].counts[nodes.index(m)].tolist() == [1, 2, 1] and int(got[False].pattern[nodes.index(m)]) == 2


@pytest.mark.parametrize("name", sorted(n for n in R.SHAPES if n != "empty"))
def test_shapes_in_two_colours(gpu, joint, name):
    k, min_occ, reads = R.SHAPES[name]
    nodes, got = check_reads(gpu, joint, [reads, []], k, min_occ)
    ref = R.compact(*R.graph_from_strings(reads, k, min_occ)[::2], k)
    same(got[False], ref, LABELS)
    same(got[True], ref, LABELS)
    if reads:
        nodes, got = check_reads(gpu, joint, [[], reads, [reads[0][:len(reads[0]) // 2 + k]]], k, min_occ)   # the first half of the first read again, as a third colour
        assert set(got[True].u_pattern.tolist()) <= {2, 6}


def test_partly_shared_path_and_bubble(gpu, joint):
    k, _, reads = R.SHAPES["path"]
    s = reads[0]
    nodes, got = check_reads(gpu, joint, [[s], [s[4:13]]], k, 1)
    assert len(got[False].u_nodes) == 1 and got[False].u_count.tolist() == [[12, 5]] and got[False].u_present.tolist() == [[12, 5]] and got[False].u_pattern.tolist() == [3]
    assert len(got[True].u_nodes) == 3 and sorted(got[True].u_pattern.tolist()) == [1, 1, 3]
    k, _, reads = R.SHAPES["bubble"]
    nodes, got = check_reads(gpu, joint, [[reads[0]], [reads[1]]], k, 1)
    assert sorted(got[True].u_pattern.tolist()) == [1, 2, 3, 3] and sorted(got[False].u_nodes.tolist()) == [3, 3, 5, 5]


def test_partly_covered_cycle_in_an_index(gpu, joint):
    """a circular sequence cut into overlapping reads on both strands, and a second colour that covers a stretch of it"""
    rng = random.Random(3)
    circ = "".join(rng.choice("ACGT") for _ in range(777))
    reads = circle_reads(circ, 60, 20)
    reads = [R.rc(r) if i % 3 == 0 else r for i, r in enumerate(reads)]
    for k in (11, 21):
        nodes, got = check_reads(gpu, joint, [reads, [circ[100:300]]], k, 1)
        g = got[False]
        assert g.stat["n_cycles"] == 1 and g.u_flags.tolist() == [api.KGRAPH_CYCLE] and g.u_first[0] == 0 and g.orient[0] == 0 and len(g.strings()[0]) == 777 + k - 1
        assert g.u_present.tolist() == [[777, 200 - k + 1]] and g.u_pattern.tolist() == [3]
        g = got[True]
        assert g.stat["n_cycles"] == 0 and not g.u_flags.any() and sorted(g.u_nodes.tolist()) == sorted([200 - k + 1, 777 - (200 - k + 1)]) and sorted(g.u_pattern.tolist()) == [1, 3]
    nodes, got = check_reads(gpu, joint, [reads, reads], 11, 1)          # all its nodes agree: a cycle under the split rule too
    assert got[True].stat["n_cycles"] == 1 and got[True].u_flags.tolist() == [api.KGRAPH_CYCLE]


def test_a_few_thousand_nodes(gpu, joint):
    names = ("repeat", "tiny")
    with Open(gpu, names) as idx:
        g = check(idx, joint.graph(names, 21, 2), 21, 2, restate=True)
        assert len(g[False].kmers) > 2000 and len(g[True].u_nodes) >= len(g[False].u_nodes) > 1


def test_dup32_large_counts_sum_as_uint64(gpu, joint):
    d = gpu.DevIndex.open(gold("dup32"))
    try:
        n_seq = int(d.mcnt[1])
        seqs, ln, _ = d.retrieve(np.arange(n_seq, dtype=np.uint64), stride=256)
        joint.sets["dup32"] = Want([seqs[x, :ln[x]] for x in range(0, n_seq, 2)])   # no FASTQ: sequence 2 i + 1 is the reverse complement of sequence 2 i
    finally:
        d.close()
    names = ("dup32", "tiny")
    with Open(gpu, names) as idx:
        g = check(idx, joint.graph(names, 21, 1), 21, 1)[False]
    assert int(g.counts[:, 0].max()) >= 40000 and g.u_count.dtype == np.uint64
    u = int(g.u_count[:, 0].argmax())
    assert int(g.u_count[u, 0]) == int(g.counts[g.unitig == u, 0].astype(np.uint64).sum()) > 40000


# ---- 4. tables, capacity, arguments --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [2, 4, "bare"])
def test_with_and_without_tables(gpu, joint, monkeypatch, cfg):
    names = ("tiny", "palin", "special")
    if cfg == "bare":
        opener = lambda n: gpu.DevIndex.open_bare(gold(n))
    else:
        monkeypatch.setenv("FMD_PTAB_DEPTH", str(cfg))
        opener = None
    with Open(gpu, names, opener) as idx:
        check(idx, joint.graph(names, 21, 2), 21, 2)
        check(idx, joint.graph(names, 3, 1), 3, 1)


def test_capacity(gpu, joint):
    names = ("repeat", "special")
    want = joint.graph(names, 21, 2)
    n = len(want[0])
    with Open(gpu, names) as idx:
        for f in (api.kmer_joint_arcs, api.kmer_joint_unitigs):
            with pytest.raises(api.FmdError, match=r"\(-5\)"):
                f(idx, 21, 2, cap=n - 1)
            with pytest.raises(api.FmdError, match=r"\(-5\)"):
                f(idx, 21, 2, cap=1)
        check(idx, want, 21, 2, cap=n)                     # a good call after the refused ones, at exactly the size
        check(idx, want, 21, 2)
        for f in (api.kmer_joint_arcs, api.kmer_joint_unitigs):
            with pytest.raises(api.FmdError, match=r"\(-2\)"):
                f(idx, 21, 2, cap=api.KGRAPH_MAX_NODES + 1)


def test_arguments(gpu, joint):
    L = gpu.lib()
    with Open(gpu, ("tiny", "palin")) as idx:
        for kw in (dict(k=20), dict(k=2), dict(k=1), dict(k=32), dict(k=33), dict(k=0), dict(k=-3), dict(min_occ=0), dict(min_occ=-1)):
            for f in (api.kmer_joint_arcs, api.kmer_joint_unitigs):
                with pytest.raises(api.FmdError, match=r"\(-2\)"):
                    f(idx, **dict(dict(k=21, min_occ=1), **kw))
        for f in (api.kmer_joint_arcs, api.kmer_joint_unitigs):
            for bad in ([], [idx[0]] * 9, [idx[0], None]):
                with pytest.raises(api.FmdError, match=r"\(-2\)"):
                    f(bad, 21, 1)
        hs = api._handles(idx)
        out, st = api.KCUnitigC(), api.KCGraphStatC()
        assert L.fmd_kcunitig(2, hs, 21, 1, 2, 0, api.C.byref(out)) == api.FMD_E_ARG and L.fmd_kcunitig(2, hs, 21, 1, 0x80000001, 0, api.C.byref(out)) == api.FMD_E_ARG
        assert L.fmd_kcunitig(2, hs, 21, 1, 0, 0, None) == api.FMD_E_ARG and L.fmd_kcunitig(2, None, 21, 1, 0, 0, api.C.byref(out)) == api.FMD_E_ARG
        assert L.fmd_kcarcs(2, hs, 21, 1, 0, None, None, None) == api.FMD_E_ARG and L.fmd_kcarcs(2, None, 21, 1, 0, None, None, api.C.byref(st)) == api.FMD_E_ARG
        assert L.fmd_kcarcs(2, hs, 21, 2, 0, None, None, api.C.byref(st)) == 0              # without a sink: the counters only
        assert st.g.n_nodes == len(joint.graph(("tiny", "palin"), 21, 2)[0])
        reads = [np.array([1, 1, 1, 2, 1, 3, 1, 1, 2, 1], dtype=np.uint8), np.array([2, 2, 1, 2, 2, 3, 2, 1], dtype=np.uint8)]   # many A and C, no T
        one = gpu.DevIndex.from_bwt(gpu.build_bwt_strands(reads, strands=api.STRAND_FWD))
        try:
            for f in (api.kmer_joint_arcs, api.kmer_joint_unitigs):
                for bad in ([idx[0], one], [one], [idx[0], idx[1], one]):                  # a one-strand handle, in the second place too
                    with pytest.raises(api.FmdError, match=r"\(-2\)"):
                        f(bad, 5, 1)
        finally:
            one.close()
        check(idx, joint.graph(("tiny", "palin"), 5, 1), 5, 1)                              # the handles are as good as before
    if gpu.device_count() > 1:
        a, b = gpu.DevIndex.open(gold("tiny")), gpu.DevIndex.open(gold("palin"), device=1)
        try:
            with pytest.raises(api.FmdError, match=r"\(-2\)"):
                api.kmer_joint_arcs([a, b], 21, 1)
        finally:
            a.close(); b.close()


# ---- 5. the command --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names,k,min_occ", [(("ctA", "ctB"), 21, 2), (("palin", "tiny"), 5, 1)])
def test_cli(gpu, joint, names, k, min_occ):
    files = [gold(n) for n in names]
    km, ct, ar, ua, pt, _, _ = joint.graph(names, k, min_occ)
    with Open(gpu, names) as idx:
        g = {split: api.kmer_joint_unitigs(idx, k, min_occ, split=split) for split in (False, True)}
    ref = {split: restated(km, ct, ua, pt, k, split) for split in (False, True)}
    args = [AMD, "kcgraph", "-k", str(k), "-o", str(min_occ)]
    run = lambda extra: subprocess.run(args + extra + files, capture_output=True, timeout=120)
    a = run([])
    assert a.returncode == 0, a.stderr
    assert a.stdout.decode() == hostlib.kcgraph_gfa_text(g[False]) == KR.gfa_text(ref[False], k)
    assert ("[M::main_kcgraph] k=%d n=2 nodes=%d " % (k, len(km))).encode() in a.stderr
    c = run(["-c"])
    assert c.returncode == 0 and c.stdout.decode() == hostlib.kcgraph_gfa_text(g[True]) == KR.gfa_text(ref[True], k)
    f = run(["-f"])
    assert f.returncode == 0 and f.stdout.decode() == hostlib.kcgraph_fasta_text(g[False]) == KR.fasta_text(ref[False])
    p = run(["-a"])
    assert p.returncode == 0 and p.stdout.decode() == hostlib.kcgraph_arcs_text(k, min_occ, km, ct, ar, ua) == \
        KR.arcs_text([R.unpack(int(x), k) for x in km], ct.tolist(), ar.tolist(), ua.tolist(), min_occ)
    for bits in ("10", "01", "11"):
        q = run(["-c", "-f", "-p", bits])
        assert q.returncode == 0 and q.stdout.decode() == hostlib.kcgraph_fasta_text(g[True], bits) == KR.fasta_text(ref[True], bits)
        q = run(["-c", "-p", bits])
        assert q.returncode == 0 and q.stdout.decode() == hostlib.kcgraph_gfa_text(g[True], bits) == KR.gfa_text(ref[True], k, bits)
    if names[0] == "ctA":                                  # sequence private to the first sample
        assert 1 in ref[True].u_pattern and run(["-c", "-f", "-p", "10"]).stdout.count(b">") == ref[True].u_pattern.count(1)


def test_default_command_line_and_one_index(gpu):
    files = [gold("ctA"), gold("ctB")]
    a = subprocess.run([AMD, "kcgraph"] + files, capture_output=True, timeout=120)
    b = subprocess.run([AMD, "kcgraph", "-k", "21", "-o", "2"] + files, capture_output=True, timeout=120)
    assert a.returncode == 0 and a.stdout == b.stdout and a.stdout.startswith(b"H\tVN:Z:1.0\nS\t0\t")
    x = subprocess.run([AMD, "kcgraph", gold("repeat")], capture_output=True, timeout=120)
    y = subprocess.run([AMD, "kgraph", gold("repeat")], capture_output=True, timeout=120)
    assert x.returncode == 0 and y.returncode == 0
    strip = lambda text: "".join(ln.split("\tkc:B:I")[0] + "\n" if ln.startswith("S\t") else ln for ln in text.splitlines(True))
    assert strip(x.stdout.decode()) == y.stdout.decode() and x.stdout.count(b"\tkn:B:I,") == y.stdout.count(b"\nS\t")
