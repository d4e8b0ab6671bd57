"""GPU: kbubble (fmd_kcbubble / fmd_kcbubble_dev, api.kmer_joint_bubbles, `fermi-amd kbubble`) against the definitions restated in Python (tests/kbubble_ref.py),
against the one-thread host walk (fmdh_kcbubble_host), and its graph field by field against fmd_kcunitig without flags.  The indexes are built from reads as
tests/test_gpu_kcgraph.py builds them; the read sets are those of tests/test_kbubble_host.py (tests/kbubble_cases.py).  Every comparison is exact."""
import random
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib
import kgraph_ref as R
import kbubble_ref as BR
import kbubble_cases as K
from test_gpu_kcgraph import Open, open_reads, gold, EMPTY, AMD

pytestmark = pytest.mark.gpu

FIELDS = [name for name, _, _ in api.KCUnitigs.NODE + api.KCUnitigs.UNITIG]
STAT = ("n_nodes", "n_arcs", "n_links", "n_unitigs", "n_cycles", "n_rounds", "n_nodes_in", "n_arcs_in")


def check(idx, k, min_occ, max_len=0, colours=None, case=None):
    """fmd_kcbubble of the open indexes: g against fmd_kcunitig, the records against the host walk and the restatement -> (g, records, restated case)"""
    g, b = api.kmer_joint_bubbles(idx, k, min_occ, max_len=max_len, with_stat=True)
    u = api.kmer_joint_unitigs(idx, k, min_occ, split=False, with_stat=True)
    for f in FIELDS:
        x, y = getattr(g, f), getattr(u, f)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f
    for f in STAT:
        assert g.stat[f] == u.stat[f], f
    assert b.dtype == api.KBUBBLE_DT and g.stat["n_forks"] == g.n_forks and g.stat["n_bubbles"] == len(b) and g.stat["ms_bubble"] >= 0
    n_forks, hb = hostlib.kcbubble_host(g, max_len)
    assert n_forks == g.n_forks and np.array_equal(hb, b), (n_forks, g.n_forks, len(hb), len(b))
    if colours is not None:                                # the graph from brute-force counts of the reads, nothing of the library's
        c = case or BR.call(colours, k, min_occ, max_len)
        assert [R.pack(x) for x in c.nodes] == g.kmers.tolist() and c.uarcs == g.uarcs.tolist()
    else:
        c = BR.from_arrays(g.kmers, g.counts, g.uarcs, g.pattern, k, max_len)
    assert BR.as_tuples(b) == c.recs and g.n_forks == c.n_forks
    assert hostlib.kbubble_text(g, b) == c.text and hostlib.kbubble_text(g, b, True) == c.text_d
    assert hostlib.kbubble_sm_text(g, g.n_forks, len(b)) == c.sm
    assert api.bubble_alleles(g, b) == [BR.alleles(c.G, rec) for rec in c.recs]
    return g, b, c


def check_reads(gpu, colours, k, min_occ, max_len=0):
    idx = [open_reads(gpu, reads) for reads in colours]
    try:
        return check(idx, k, min_occ, max_len, colours)
    finally:
        for d in idx:
            d.close()


def fields(c, x=0):
    return c.text.splitlines()[x].split("\t")


# ---- every shape -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_shapes(gpu, name):
    k, min_occ, reads = R.SHAPES[name]
    one = check_reads(gpu, [reads], k, min_occ)[2]
    two = check_reads(gpu, [[r] for r in reads] if name == "bubble" else [reads, reads[:1]], k, min_occ)[2]
    if name == "bubble":
        # branch 0 leaves s = AAATG by G, the smaller base: the read with CCC as printed, whichever colour it is
        for c, gt in ((one, "GT:Z:11"), (two, "GT:Z:01,10"), (check_reads(gpu, [[reads[1]], [reads[0]]], k, min_occ)[2], "GT:Z:10,01")):
            f = fields(c)
            assert len(c.recs) == 1 and c.n_forks == 2 and f[2] == "SNP" and f[7:9] == ["5", "5"] and f[-1] == gt, f
    else:
        assert one.recs == [] and two.recs == []


@pytest.mark.parametrize("name", sorted(K.controls()))
def test_negative_controls(gpu, name):
    colours, k, min_occ = K.controls()[name]
    g, b, c = check_reads(gpu, colours, k, min_occ)
    assert len(b) == 0 and g.n_forks >= 1


@pytest.mark.parametrize("k,d", [(5, 1), (5, 3), (11, 3)])
def test_indel_and_max_len(gpu, k, d):
    colours, left, ins, right = K.indel(k, d)
    idx = [open_reads(gpu, reads) for reads in colours]
    try:
        g, b, c = check(idx, k, 1, 0, colours)
        assert len(b) == 1 and sorted(b["len"][0].tolist()) == [k - 1, k - 1 + d]
        kind, lf, a0, a1, rf = api.bubble_alleles(g, b)[0]
        assert kind == "INDEL" and "-" in (a0, a1)
        assert (a0 if a1 == "-" else a1, lf + rf) in ((ins, left[-k:] + right[:k]), (R.rc(ins), R.rc(left[-k:] + right[:k])))
        longer = k - 1 + d
        assert len(check(idx, k, 1, longer, colours)[1]) == 1 and len(check(idx, k, 1, longer - 1, colours)[1]) == 0
        assert len(check(idx, k, 1, 0xffffffff, colours)[1]) == 1 and len(check(idx, k, 1, 1, colours)[1]) == 0
    finally:
        for x in idx:
            x.close()


def test_once_only_whatever_the_strand_and_the_order(gpu):
    rng = random.Random(7)
    P = K.Planted(K.PLANTED_SEED)
    for colours, k in ((K.indel(5, 3)[0], 5), (P.colours(2), 21), (K.fuzz(6), 5)):
        c = check_reads(gpu, colours, k, 1)[2]
        turned = check_reads(gpu, [[R.rc(r) for r in reads] for reads in colours], k, 1)[2]
        mixed = check_reads(gpu, [rng.sample(reads, len(reads)) for reads in colours], k, 1)[2]
        assert c.sm + c.text == turned.sm + turned.text == mixed.sm + mixed.text and c.text_d == turned.text_d == mixed.text_d


# ---- planted variants ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    return K.Planted(K.PLANTED_SEED)


@pytest.mark.parametrize("n,k", [(2, 11), (2, 21), (2, 31), (3, 21), (8, 11)])
def test_planted_variants(gpu, planted, n, k):
    colours = planted.colours(n)
    cases = {}
    for min_occ in (1, 2):                                 # first, on the CPU: the restatement recovers exactly the planted sites
        c = cases[min_occ] = BR.call(colours, k, min_occ)
        planted.check(c.G, c.recs)
        assert len(c.recs) == 40
    idx = [open_reads(gpu, reads) for reads in colours]
    try:
        for min_occ in (1, 2):
            g, b, c = check(idx, k, min_occ, 0, colours, cases[min_occ])
            kinds = [x[0] for x in api.bubble_alleles(g, b)]
            assert len(b) == 40 and kinds.count("SNP") == 30 and kinds.count("INDEL") == 10
            if n > 2:
                assert all(ln.split("\t")[-1].split(",")[n - 2] == "00" for ln in c.text.splitlines())   # the empty colour holds nothing
    finally:
        for d in idx:
            d.close()


# ---- fuzz ------------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", K.FUZZ_SEEDS)
def test_fuzz(gpu, seed):
    colours = K.fuzz(seed)
    idx = [open_reads(gpu, reads) for reads in colours]
    try:
        for k in (3, 5):
            check(idx, k, 1, 0, colours)
    finally:
        for d in idx:
            d.close()


# ---- golden indexes: a few thousand nodes, the grid seam, the command ------------------------------------------------------------------------------------------------------------
GOLDEN = [(("repeat", "tiny"), 21, 2), (("ctA", "ctB"), 21, 2), (("palin", "tiny", EMPTY), 5, 1)]


@pytest.mark.parametrize("names,k,min_occ", GOLDEN)
def test_golden_indexes(gpu, names, k, min_occ):
    with Open(gpu, names) as idx:
        g, b, c = check(idx, k, min_occ)
        assert g.n_forks > 0 or k == 5                     # (at k = 5 these reads fill the graph: every port has four arcs)


def test_grid_seam(gpu):
    """the stage on one block, on a few and on more blocks than there are ports to share out: the records are placed by the scan, not by arrival"""
    with Open(gpu, ("repeat", "tiny")) as idx:
        g, b, c = check(idx, 21, 2)
        assert len(g.kmers) > 2000 and len(b) >= 1
        for grid in (1, 3, 17, 4096):
            n_forks, got = api.kmer_bubbles_dev(idx[0], 21, g.kmers, g.uarcs, grid=grid)
            assert n_forks == g.n_forks and np.array_equal(got, b), grid
        for max_len in (1, 20, 21):
            n_forks, got = api.kmer_bubbles_dev(idx[0], 21, g.kmers, g.uarcs, max_len=max_len, grid=2)
            assert n_forks == g.n_forks and BR.as_tuples(got) == BR.find(c.G, max_len)[1], max_len
        assert api.kmer_bubbles_dev(idx[0], 21, g.kmers[:0], g.uarcs[:0])[1].shape == (0,)
        with pytest.raises(api.FmdError, match=r"\(-2\)"):
            api.kmer_bubbles_dev(idx[0], 21, g.kmers, g.uarcs, grid=-1)
        with pytest.raises(api.FmdError, match=r"\(-2\)"):
            api.kmer_bubbles_dev(idx[0], 20, g.kmers, g.uarcs)


def test_arguments_and_capacity(gpu):
    with Open(gpu, ("repeat", "tiny")) as idx:
        n = len(api.kmer_joint_unitigs(idx, 21, 2).kmers)
        for kw in (dict(k=20), dict(k=2), dict(k=1), dict(k=32), dict(k=33), dict(k=0), dict(k=-3), dict(min_occ=0), dict(min_occ=-1)):
            with pytest.raises(api.FmdError, match=r"\(-2\)"):
                api.kmer_joint_bubbles(idx, **dict(dict(k=21, min_occ=1), **kw))
        for bad in ([], [idx[0]] * 9, [idx[0], None]):
            with pytest.raises(api.FmdError, match=r"\(-2\)"):
                api.kmer_joint_bubbles(bad, 21, 1)
        with pytest.raises(api.FmdError, match=r"\(-2\)"):
            api.kmer_joint_bubbles(idx, 21, 2, cap=api.KGRAPH_MAX_NODES + 1)
        assert gpu.lib().fmd_kcbubble(2, api._handles(idx), 21, 2, 0, 0, None) == api.FMD_E_ARG
        for cap in (n - 1, 1):
            o = api.KCBubbleC()
            assert gpu.lib().fmd_kcbubble(2, api._handles(idx), 21, 2, 0, cap, api.C.byref(o)) == api.FMD_E_NOMEM
            assert o.bubble is None and o.n_bubbles == 0 and o.n_forks == 0 and o.g.kmer is None and o.g.n_nodes == 0
            with pytest.raises(api.FmdError, match=r"\(-5\)"):
                api.kmer_joint_bubbles(idx, 21, 2, cap=cap)
        g, b, c = check(idx, 21, 2)                        # the handles are as good as before
        g2, b2 = api.kmer_joint_bubbles(idx, 21, 2, cap=n)
        assert np.array_equal(b2, b) and len(g2.kmers) == n


@pytest.mark.parametrize("names,k,min_occ", GOLDEN[:2])
def test_cli(gpu, names, k, min_occ):
    files = [gold(n) for n in names]
    with Open(gpu, names) as idx:
        g, b, c = check(idx, k, min_occ)
    args = [AMD, "kbubble", "-k", str(k), "-o", str(min_occ)]
    a = subprocess.run(args + files, capture_output=True, timeout=120)
    assert a.returncode == 0, a.stderr
    assert a.stdout.decode() == c.sm + c.text and len(c.recs) >= 1
    assert ("[M::main_kbubble] k=%d n=2 nodes=%d " % (k, len(g.kmers))).encode() in a.stderr
    d = subprocess.run(args + ["-d"] + files, capture_output=True, timeout=120)
    assert d.returncode == 0 and d.stdout.decode() == c.sm + c.text_d
    longest = max(max(r[4:6]) for r in c.recs)
    short = BR.from_arrays(g.kmers, g.counts, g.uarcs, g.pattern, k, longest - 1)
    s = subprocess.run(args + ["-L", str(longest - 1)] + files, capture_output=True, timeout=120)
    assert s.returncode == 0 and s.stdout.decode() == short.sm + short.text and len(short.recs) < len(c.recs)
    if names[0] == "repeat":
        one = subprocess.run([AMD, "kbubble", files[0]], capture_output=True, timeout=120)   # the defaults, and one index: the heterozygous sites of a sample
        assert one.returncode == 0 and one.stdout.startswith(b"SM\t") and b"\tGT:Z:01" not in one.stdout and b"\tGT:Z:10" not in one.stdout
