"""CPU: the host side of kbubble -- fmdh_kcbubble_host (the definition walked node by node by one thread) and fmdh_kbubble_print (the BB lines of `fermi-amd
kbubble`) -- against the definitions restated in Python (tests/kbubble_ref.py).  The graphs are made as tests/test_kcgraph_host.py makes them: brute-force counts
(kcgraph_ref.joint_graph), then fmdh_kcgraph_compact_host.  Everything is exact."""
import os
import random
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib
import kgraph_ref as R
import kbubble_ref as BR
import kbubble_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")


def host_graph(c):
    """the api.KCUnitigs of a restated case, labelled by the one-thread host walk"""
    n, n_idx = len(c.nodes), c.n_idx
    km = np.array([R.pack(x) for x in c.nodes], dtype=np.uint64)
    ct = np.array(c.counts, dtype=np.uint32).reshape(n, n_idx)
    return hostlib.kcgraph_compact_host(c.k, km, ct, np.array(c.uarcs, dtype=np.uint8), np.array(c.pattern, dtype=np.uint8), arcs=np.array(c.arcs, dtype=np.uint8).reshape(n, n_idx))


def run(colours, k, min_occ, max_len=0):
    """one case through the restatement and through the library's host code: records, n_forks, both texts, the alleles -> the restated case"""
    c = BR.call(colours, k, min_occ, max_len)
    g = host_graph(c)
    n_forks, b = hostlib.kcbubble_host(g, max_len)
    assert b.dtype == api.KBUBBLE_DT and BR.as_tuples(b) == c.recs and n_forks == c.n_forks
    assert hostlib.kbubble_text(g, b) == c.text and hostlib.kbubble_text(g, b, True) == c.text_d
    assert hostlib.kbubble_sm_text(g, n_forks, len(b)) == c.sm
    assert api.bubble_alleles(g, b) == [BR.alleles(c.G, rec) for rec in c.recs]
    assert [int(x) for x in b["src"]] == sorted(set(int(x) for x in b["src"]))      # ascending, a port once
    return c


def fields(c, x=0):
    return c.text.splitlines()[x].split("\t")


# ---- every hand-made shape of kgraph, in one and in two colours ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_shapes(name):
    k, min_occ, reads = R.SHAPES[name]
    one = run([reads], k, min_occ)
    two = run([[r] for r in reads] if name == "bubble" else [reads, reads[:1]], k, min_occ)
    if name == "bubble":
        for c, gt in ((one, "GT:Z:11"), (two, "GT:Z:01,10"), (run([[reads[1]], [reads[0]]], k, min_occ), "GT:Z:10,01")):
            f = fields(c)
            assert len(c.recs) == 1 and c.n_forks == 2 and f[2] == "SNP" and f[7:9] == ["5", "5"] and f[-1] == gt, f
        # branch 0 leaves s = AAATG by G, the smaller base: it is the read with CCC as printed, whichever colour that read is
        assert fields(two)[3:7] == ["AAATG", "G", "T", "GTTTA"] and one.text_d == "" and two.text_d == two.text
    else:
        assert one.recs == [] and two.recs == [] and one.text == "" and two.text == ""


# ---- the negative controls: no bubble, and for the reason the case is there ------------------------------------------------------------------------------------------
def forks(G):
    """(s, branch A, branch B) of every port with two right arcs"""
    for s in range(2 * G.n):
        r = G.right(s)
        if len(r) == 2:
            yield s, G.branch(G.follow(s, r[0])), G.branch(G.follow(s, r[1]))


@pytest.mark.parametrize("name", sorted(K.controls()))
def test_negative_controls(name):
    colours, k, min_occ = K.controls()[name]
    c = run(colours, k, min_occ)
    G = c.G
    assert c.recs == [] and c.text == "" and c.n_forks >= 1
    both = [(s, A, B) for s, A, B in forks(G) if A and B]
    if name == "fork_of_three":
        three = [s for s in range(2 * G.n) if len(G.right(s)) == 3]
        assert len(three) == 1 and any(A[0] == B[0] == three[0] ^ 1 for s, A, B in both)       # seen from t ^ 1: two branches into a node with three left arcs
    elif name == "join_of_three":
        assert any(A[0] == B[0] and G.left_n(A[0]) == 3 for s, A, B in both)
    elif name == "tip_on_an_allele":
        cut = [(s, A, B) for s, A, B in forks(G) if (A is None) != (B is None)]
        assert any(G.text(s) == K.L5[-5:] for s, A, B in cut) and not any(A[0] == B[0] for s, A, B in both)   # the fork of the variant has lost a branch
    elif name == "opposite_target":
        assert any(A[0] == B[0] ^ 1 and G.left_n(A[0]) == 2 and G.left_n(B[0]) == 2 for s, A, B in both)
    elif name == "s_and_t_on_one_node":
        assert any(A[0] == B[0] == s ^ 1 for s, A, B in both)


def test_the_flanks_are_clean():
    for a, b in ((K.L5 + "A" + K.R5, K.L5 + "C" + K.R5),):
        c = run([[a, b]], 5, 1)
        assert len(c.recs) == 1 and fields(c)[2] == "SNP"                      # the controls' flanks alone make one plain bubble


# ---- indel, max_len, once only -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", [(5, 1), (5, 3), (11, 1), (11, 3)])
def test_indel_and_max_len(k, d):
    colours, left, ins, right = K.indel(k, d)
    c = run(colours, k, 1)
    assert len(c.recs) == 1 and sorted(c.recs[0][4:6]) == [k - 1, k - 1 + d]
    kind, lf, a0, a1, rf = BR.alleles(c.G, c.recs[0])
    assert kind == "INDEL" and "-" in (a0, a1)
    assert (a0 if a1 == "-" else a1, lf + rf) in ((ins, left[-k:] + right[:k]), (R.rc(ins), R.rc(left[-k:] + right[:k])))   # (no repeat at the site: one placement)
    longer = k - 1 + d
    assert len(run(colours, k, 1, longer).recs) == 1 and run(colours, k, 1, longer - 1).recs == [] and len(run(colours, k, 1, 0).recs) == 1
    assert len(run(colours, k, 1, 0xffffffff).recs) == 1 and run(colours, k, 1, 1).recs == []


def test_once_only_whatever_the_strand_and_the_order():
    rng = random.Random(7)
    P = K.Planted(K.PLANTED_SEED)
    for colours, k in ((K.indel(5, 3)[0], 5), (P.colours(2), 21), (K.fuzz(6), 5)):
        c = run(colours, k, 1)
        turned = run([[R.rc(r) for r in reads] for reads in colours], k, 1)
        mixed = run([rng.sample(reads, len(reads)) for reads in colours], k, 1)
        assert c.sm + c.text == turned.sm + turned.text == mixed.sm + mixed.text and c.text_d == turned.text_d == mixed.text_d


# ---- planted variants ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,min_occ,n", [(11, 1, 2), (21, 2, 2), (31, 1, 2), (21, 1, 3), (11, 2, 8)])
def test_planted_variants(k, min_occ, n):
    P = K.Planted(K.PLANTED_SEED)
    c = run(P.colours(n), k, min_occ)
    P.check(c.G, c.recs)
    kinds = [ln.split("\t")[2] for ln in c.text.splitlines()]
    assert kinds.count("SNP") == 30 and kinds.count("INDEL") == 10
    if n == 2:
        assert c.text_d == c.text and all(ln.split("\t")[-1] in ("GT:Z:10,01", "GT:Z:01,10") for ln in c.text.splitlines())
    else:
        assert all(ln.split("\t")[-1].split(",")[n - 2] == "00" for ln in c.text.splitlines())   # the empty colour holds nothing


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", K.FUZZ_SEEDS)
def test_fuzz(seed):
    total = 0
    for k in (3, 5):
        c = run(K.fuzz(seed), k, 1)
        total += c.n_forks
        assert 2 * len(c.recs) <= c.n_forks
    assert total >= 10                                  # tangles: many forks, few of them bubbles


# ---- arguments, the command, the bindings -------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments():
    c = BR.call([R.SHAPES["bubble"][2]], 5, 1)
    g = host_graph(c)
    for k in (4, 1, 33, 0):
        g.k = k
        with pytest.raises(ValueError):
            hostlib.kcbubble_host(g)
        with pytest.raises(ValueError):
            hostlib.kbubble_text(g, np.zeros(0, api.KBUBBLE_DT))
    g.k = 5
    bad = np.zeros(1, api.KBUBBLE_DT)
    bad["src"], bad["dst"] = 0, 2 * len(g.kmers)          # a record that names no node
    with pytest.raises(ValueError):
        hostlib.kbubble_text(g, bad)
    good = hostlib.kcbubble_host(g)[1]
    good["len"][0, 0] += 1                                 # a record that is no walk of the graph
    with pytest.raises(ValueError):
        hostlib.kbubble_text(g, good)
    fmd = os.path.join(ROOT, "tests", "golden", "tiny.fmd")
    for args in (["-k", "20"], ["-k", "33"], ["-k", "1"], ["-o", "0"], ["-L", "-1"], []):   # refused before a device is looked for
        a = subprocess.run([AMD, "kbubble"] + args + ([fmd] if args else []), capture_output=True, timeout=60)
        assert a.returncode == 1 and b"Usage:   fermi-amd kbubble" in a.stderr and a.stdout == b"", args
    a = subprocess.run([AMD, "kbubble"] + [fmd] * 9, capture_output=True, timeout=60)
    assert a.returncode == 1 and b"Usage:   fermi-amd kbubble" in a.stderr
    a = subprocess.run([AMD, "kbubble", fmd, "/nonexistent.fmd"], capture_output=True, timeout=60)
    assert a.returncode == 1 and b"fail to open file" in a.stderr
    a = subprocess.run([AMD], capture_output=True, timeout=60)
    assert b"kbubble" in a.stderr


def test_symbols_are_declared():
    import ctypes as C
    assert "fmd_kcbubble" in api.ABI_SYMBOLS and "fmd_kcbubble_dev" in api.ABI_SYMBOLS
    assert api.KBUBBLE_DT.itemsize == 24 and C.sizeof(api.KCBubbleC) == C.sizeof(api.KCUnitigC) + 32
