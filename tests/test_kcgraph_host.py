"""CPU: the host side of kcgraph -- fmdh_kcgraph_compact_host (the one-thread labelling of the union graph with the split rule, plus the per-unitig sums) and
the printers of `fermi-amd kcgraph` -- against the definitions restated in Python (tests/kcgraph_ref.py) on hand-made graphs of two and three colours."""
import os
import random
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib
import kgraph_ref as R
import kcgraph_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")


def arrays(nodes, counts, arcs, uarcs, pattern, n_idx):
    n = len(nodes)
    return (np.array([R.pack(x) for x in nodes], dtype=np.uint64), np.array(counts, dtype=np.uint32).reshape(n, n_idx), np.array(arcs, dtype=np.uint8).reshape(n, n_idx),
            np.array(uarcs, dtype=np.uint8), np.array(pattern, dtype=np.uint8))


def same(got, want):
    """an api.KCUnitigs against the restated graph, every array"""
    for f in ("unitig", "offset", "orient", "u_nodes", "u_first", "u_flags", "u_pattern"):
        assert getattr(got, f).tolist() == getattr(want, f), f
    assert got.u_count.tolist() == want.u_count and got.u_present.tolist() == want.u_present
    assert got.u_count.dtype == np.uint64 and got.u_present.dtype == np.uint32 and got.u_pattern.dtype == np.uint8
    assert got.strings() == want.strings


def run(colours, k, min_occ, split):
    n_idx = len(colours)
    nodes, counts, arcs, uarcs, pattern = KR.joint_graph(colours, k, min_occ)
    want = KR.compact(nodes, uarcs, pattern, k, counts, split)
    km, ct, ar, ua, pt = arrays(nodes, counts, arcs, uarcs, pattern, n_idx)
    got = hostlib.kcgraph_compact_host(k, km, ct, ua, pt, split=split, arcs=ar)
    same(got, want)
    assert got.stat == dict(n_nodes=len(nodes), n_arcs=want.n_arcs, n_links=want.n_links, n_unitigs=want.n_unitigs, n_cycles=want.n_cycles,
                            n_nodes_in=[sum(p >> i & 1 for p in pattern) for i in range(n_idx)])
    pats = [None] + sorted(set(KR.bits(p, n_idx) for p in want.u_pattern)) + ["0" * n_idx]
    for p in pats:
        assert hostlib.kcgraph_gfa_text(got, p) == KR.gfa_text(want, k, p), p
        assert hostlib.kcgraph_fasta_text(got, p) == KR.fasta_text(want, p), p
    assert hostlib.kcgraph_arcs_text(k, min_occ, km, ct, ar, ua) == KR.arcs_text(nodes, counts, arcs, uarcs, min_occ)
    for j in range(len(nodes)):                            # an arc bit in colour i implies pattern bit i; the union is the OR
        for i in range(n_idx):
            assert not arcs[j][i] or pattern[j] >> i & 1
    return nodes, counts, arcs, uarcs, pattern, want, got


# (a) every hand-made shape of kgraph as colour 0 beside an empty colour 1: the plain graph
@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_shapes_beside_an_empty_colour(name):
    k, min_occ, reads = R.SHAPES[name]
    nodes, counts, arcs, uarcs, pattern, want, got = run([reads, []], k, min_occ, False)
    pn, pc, pa = R.graph_from_strings(reads, k, min_occ)
    assert nodes == pn and [c[0] for c in counts] == pc and [a[0] for a in arcs] == pa == uarcs and all(c[1] == 0 and a[1] == 0 for c, a in zip(counts, arcs))
    plain = hostlib.kgraph_compact_host(k, np.array([R.pack(x) for x in pn], dtype=np.uint64), np.array(pa, dtype=np.uint8), np.array(pc, dtype=np.uint32))
    for f in ("unitig", "offset", "orient", "u_nodes", "u_first", "u_flags"):
        assert np.array_equal(getattr(got, f), getattr(plain, f)), f
    assert got.strings() == plain.strings()
    R.check_shape(name, nodes, pc, pa, want)
    sp = run([reads, []], k, min_occ, True)[6]           # one pattern everywhere: the split rule changes nothing
    for f in ("unitig", "offset", "orient", "u_flags"):
        assert np.array_equal(getattr(sp, f), getattr(got, f)), f
    strip = lambda text: "".join(ln.split("\tkc:B:I")[0] + "\n" if ln.startswith("S\t") else ln for ln in text.splitlines(True))
    assert strip(hostlib.kcgraph_gfa_text(got)) == hostlib.kgraph_gfa_text(plain)   # kgraph's S and L lines apart from the two extra tags


# (b) a path whose middle third is also in colour 1
def test_partly_shared_path():
    k, _, reads = R.SHAPES["path"]
    s = reads[0]
    colours = [[s], [s[4:13]]]
    nodes, counts, arcs, uarcs, pattern, want, got = run(colours, k, 1, False)
    assert want.n_unitigs == 1 and want.u_count == [[12, 5]] and want.u_present == [[12, 5]] and want.u_pattern == [3] and want.kc == [17]
    nodes, counts, arcs, uarcs, pattern, want, got = run(colours, k, 1, True)
    assert want.n_unitigs == 3 and sorted(want.u_pattern) == [1, 1, 3] and sorted(want.u_nodes) == sorted([5] + [n for n, p in zip(want.u_nodes, want.u_pattern) if p == 1])
    assert sum(want.u_nodes) == 12 and want.u_nodes[want.u_pattern.index(3)] == 5 and want.u_count[want.u_pattern.index(3)] == [5, 5]
    assert got.u_count.sum(axis=0).tolist() == [12, 5] and got.u_present.sum(axis=0).tolist() == [12, 5]


# (c) an SNP bubble: the flanks in both colours, one branch each
def test_snp_bubble():
    k, _, reads = R.SHAPES["bubble"]
    for split in (False, True):
        nodes, counts, arcs, uarcs, pattern, want, got = run([[reads[0]], [reads[1]]], k, 1, split)
        assert want.n_unitigs == 4 and sorted(want.u_pattern) == [1, 2, 3, 3] and sorted(want.u_nodes) == [3, 3, 5, 5]
        assert hostlib.kcgraph_fasta_text(got, "10").count(">") == 1 and hostlib.kcgraph_fasta_text(got, "01").count(">") == 1


# (d) an isolated cycle in colour 0, colour 1 covering an arc of it
def test_partly_covered_cycle():
    k, _, reads = R.SHAPES["cycle"]
    colours = [reads, [reads[0][3:11]]]
    nodes, counts, arcs, uarcs, pattern, want, got = run(colours, k, 1, False)
    assert want.n_unitigs == 1 and want.n_cycles == 1 and want.u_flags == [1] and want.u_first == [0] and want.u_pattern == [3] and want.u_present == [[14, 4]]
    nodes, counts, arcs, uarcs, pattern, want, got = run(colours, k, 1, True)
    assert want.n_unitigs == 2 and want.n_cycles == 0 and want.u_flags == [0, 0] and sorted(want.u_nodes) == [4, 10] and sorted(want.u_pattern) == [1, 3]
    all_in = run([reads, reads], k, 1, True)[5]             # all its nodes agree: still a cycle
    assert all_in.n_cycles == 1 and all_in.u_flags == [1] and all_in.u_pattern == [3]


# (e) min_occ - 1 in each of two colours is no node
def test_the_any_rule():
    k, _, reads = R.SHAPES["path"]
    s = reads[0]
    one = [s[:9]] * 2 + [s[6:]] * 2 + [s]                  # the k-mer at 5 is in s alone
    m = min(s[5:10], R.rc(s[5:10]))
    for colours in ([one, one], [one, one, []]):
        nodes, counts, arcs, uarcs, pattern, want, got = run(colours, k, 2, False)
        assert R.count_dict(one, k)[m] == 1 and m not in nodes and len(nodes) == 11 and want.n_unitigs == 2
        assert all(c[0] == c[1] == 3 for c in counts)
    nodes = run([one, one], k, 1, False)[0]
    assert m in nodes and len(nodes) == 12


# (f) the hairpin, and the halved palindromic (k+1)-mer, in colour 1 only
@pytest.mark.parametrize("name", ["hairpin", "hairpin_halved"])
def test_hairpins_in_the_second_colour(name):
    k, min_occ, reads = R.SHAPES[name]
    for split in (False, True):
        nodes, counts, arcs, uarcs, pattern, want, got = run([[], reads], k, min_occ, split)
        pn, pc, pa = R.graph_from_strings(reads, k, min_occ)
        assert nodes == pn and [c[1] for c in counts] == pc and [a[1] for a in arcs] == pa and set(pattern) == {2}
        R.check_shape(name, nodes, pc, pa, want)


# (g) no node; one node
def test_no_node_and_one_node():
    for split in (False, True):
        nodes, _, _, _, _, want, got = run([[], []], 5, 1, split)
        assert nodes == [] and want.n_unitigs == 0 and hostlib.kcgraph_gfa_text(got) == "H\tVN:Z:1.0\n" and hostlib.kcgraph_fasta_text(got) == ""
        nodes, _, _, _, _, want, got = run([["ACCGT"], []], 5, 1, split)
        assert nodes == ["ACCGT"] and want.strings == ["ACCGT"] and want.u_count == [[1, 0]] and want.u_pattern == [1]
        assert hostlib.kcgraph_gfa_text(got) == "H\tVN:Z:1.0\nS\t0\tACCGT\tKC:i:1\tLN:i:5\tkc:B:I,1,0\tkn:B:I,1,0\n"
        assert hostlib.kcgraph_fasta_text(got) == ">0 KC:i:1 LN:i:5 PT:Z:10 kc:B:I,1,0 kn:B:I,1,0\nACCGT\n"


# (h) the -p filter and the L lines that survive it
def test_pattern_filter():
    k, _, reads = R.SHAPES["bubble"]
    nodes, counts, arcs, uarcs, pattern, want, got = run([reads, [reads[0]]], k, 1, True)
    assert sorted(want.u_pattern) == [1, 3, 3, 3]
    full, both, first = hostlib.kcgraph_gfa_text(got), hostlib.kcgraph_gfa_text(got, "11"), hostlib.kcgraph_gfa_text(got, "10")
    assert full.count("\nL\t") == 4 and both.count("\nL\t") == 2 and first.count("\nL\t") == 0
    assert full.count("\nS\t") == 4 and both.count("\nS\t") == 3 and first.count("\nS\t") == 1
    assert set(both.splitlines()) <= set(full.splitlines()) and hostlib.kcgraph_gfa_text(got, "01") == "H\tVN:Z:1.0\n"
    with pytest.raises(ValueError):
        hostlib.kcgraph_gfa_text(got, "1")
    with pytest.raises(ValueError):
        hostlib.kcgraph_fasta_text(got, "12")


@pytest.mark.parametrize("k,min_occ", [(3, 1), (5, 1), (5, 2), (7, 2), (11, 1)])
def test_random_reads_in_three_colours(k, min_occ):
    """reads off a short random genome with a repeat, both strands, some with a substitution, dealt to three overlapping colours"""
    rng = random.Random(k * 10 + min_occ)
    genome = "".join(rng.choice("ACGT") for _ in range(150))
    genome += genome[20:60] + "".join(rng.choice("ACGT") for _ in range(60))
    colours = [[], [], []]
    for _ in range(150):
        a = rng.randrange(len(genome) - 30)
        r = genome[a:a + 30]
        if rng.random() < 0.15:
            p = rng.randrange(30)
            r = r[:p] + rng.choice("ACGT") + r[p + 1:]
        r = R.rc(r) if rng.random() < 0.5 else r
        for i in range(3):
            if rng.random() < (0.7, 0.4, 0.2)[i]:
                colours[i].append(r)
    colours[2].append("ACGTNNACGTACGGTNACGTTGCA")
    plain = run(colours, k, min_occ, False)[5]
    split = run(colours, k, min_occ, True)[5]
    assert split.n_unitigs >= plain.n_unitigs > 3 and (k == 3 or len(set(split.u_pattern)) > 2)    # (at k = 3 nearly every 3-mer is in every colour)
    for i in range(3):                                     # the nodes with pattern bit i, with count[i] and arcs[i]: the plain graph of colour i
        nodes, counts, arcs, uarcs, pattern = KR.joint_graph(colours, k, min_occ)
        pn, pc, pa = R.graph_from_strings(colours[i], k, min_occ)
        sel = [j for j in range(len(nodes)) if pattern[j] >> i & 1]
        assert [nodes[j] for j in sel] == pn and [counts[j][i] for j in sel] == pc and [arcs[j][i] for j in sel] == pa


def test_refused_arguments():
    km = np.array([R.pack("ACCGT")], dtype=np.uint64)
    one = (np.ones((1, 2), np.uint32), np.zeros(1, np.uint8), np.ones(1, np.uint8))
    for k in (4, 1, 2, 32, 33, 0, -1):
        with pytest.raises(ValueError):
            hostlib.kcgraph_compact_host(k, km, *one)
    with pytest.raises(ValueError):
        hostlib.kcgraph_compact_host(5, km, np.ones((1, 9), np.uint32), one[1], one[2])
    with pytest.raises(ValueError):
        hostlib.kcgraph_compact_host(5, km, one[0], np.zeros(2, np.uint8), one[2])
    fmd = os.path.join(ROOT, "tests", "golden", "tiny.fmd")
    for args in (["-k", "20"], ["-k", "33"], ["-k", "1"], ["-o", "0"], ["-f", "-a"], ["-a", "-c"], ["-p", "10"], ["-p", "2"], []):   # refused before a device is looked for
        a = subprocess.run([AMD, "kcgraph"] + args + ([fmd] if args else []), capture_output=True, timeout=60)
        assert a.returncode == 1 and b"Usage:   fermi-amd kcgraph" in a.stderr and a.stdout == b"", args
    a = subprocess.run([AMD, "kcgraph"] + [fmd] * 9, capture_output=True, timeout=60)
    assert a.returncode == 1 and b"Usage:   fermi-amd kcgraph" in a.stderr
    a = subprocess.run([AMD, "kcgraph", fmd, "/nonexistent.fmd"], capture_output=True, timeout=60)
    assert a.returncode == 1 and b"fail to open file" in a.stderr
    a = subprocess.run([AMD], capture_output=True, timeout=60)
    assert b"kcgraph" in a.stderr


def test_symbols_are_declared():
    assert "fmd_kcarcs" in api.ABI_SYMBOLS and "fmd_kcunitig" in api.ABI_SYMBOLS
    assert api.KCGRAPH_STAT_DT.itemsize == 80 + 128 == __import__("ctypes").sizeof(api.KCGraphStatC)
