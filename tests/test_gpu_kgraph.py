"""GPU: kgraph (fmd_karcs / fmd_kunitig, DevIndex.kmer_arcs / kmer_unitigs, `fermi-amd kgraph`) against brute force over the forward sequences as indexed,
independent of any index code, and against the definitions restated in Python (tests/kgraph_ref.py).  Everything is compared exactly: the node list and
its counts (also with kmer_counts), the arc bytes (brute force, and what kmer_counts(k + 1) implies), the labelling, the strings and the counters (the
restatement, and the one-thread walk fmdh_kgraph_compact_host), the invariants, and the command's three outputs byte for byte."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib
import kgraph_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
KS = (3, 5, 11, 21, 31)
MIN_OCCS = (1, 2, 3)


# ---- the forward sequences as indexed (as tests/test_gpu_kprofile.py obtains them), and brute force over them -------------------------------------------
def fastq_reads(name):
    tab = np.full(256, 5, dtype=np.uint8)
    for ch, v in zip(b"ACGTacgt", [1, 2, 3, 4, 1, 2, 3, 4]):
        tab[ch] = v
    with gzip.open(os.path.join(GOLD, name + ".fq.gz"), "rb") as f:
        lines = f.read().split(b"\n")
    return [tab[np.frombuffer(lines[i], dtype=np.uint8)] for i in range(1, len(lines) - 1, 4)]


def forward_as_indexed(name):
    """the reads of the golden FASTQ; an even-length read that is its own reverse complement loses its last base, as `build` trims it"""
    out = []
    for r in fastq_reads(name):
        r = np.ascontiguousarray(r, dtype=np.uint8)
        out.append(r[:hostlib.trim_palindrome(r)])
    return out


def revcomp(s):
    out = s[::-1].copy()
    m = (out >= 1) & (out <= 4)
    out[m] = 5 - out[m]
    return out


def windows_packed(r, k):
    """(canonical packed k-mer, N-free?) of every k-window of r, k <= 32"""
    sh = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    base = (r.astype(np.uint64) - np.uint64(1)) & np.uint64(3)
    w = np.lib.stride_tricks.sliding_window_view(base, k)
    good = np.lib.stride_tricks.sliding_window_view((r >= 1) & (r <= 4), k).all(axis=1)
    fw = np.bitwise_or.reduce(w << sh, axis=1)
    rc = np.bitwise_or.reduce((np.uint64(3) - w[:, ::-1]) << sh, axis=1)
    return np.minimum(fw, rc), good


def nt6(s):
    return np.array(["?ACGTN".index(c) for c in s], dtype=np.uint8)


class Want:
    """brute force for one read set (nt6 arrays, forward strand), per (k, min_occ) computed once and never changed"""

    def __init__(self, seqs):
        self.seqs, self.tables, self.graphs, self.compacted = seqs, {}, {}, {}

    def table(self, m):
        """COUNT of every canonical m-mer: the N-free m-windows of the forward sequences whose canonical form it is (identical sequences weighed)"""
        if m not in self.tables:
            uniq, mult = np.unique(np.array([s.tobytes() for s in self.seqs] + [b""], dtype=object), return_counts=True)
            parts, wts = [np.zeros(0, dtype=np.uint64)], [np.zeros(0, dtype=np.float64)]
            for b, n in zip(uniq, mult):
                if len(b) >= m:
                    c, good = windows_packed(np.frombuffer(b, dtype=np.uint8), m)
                    parts.append(c[good]); wts.append(np.full(int(good.sum()), float(n)))
            km, inv = np.unique(np.concatenate(parts), return_inverse=True)
            self.tables[m] = (km, np.bincount(inv.reshape(-1), weights=np.concatenate(wts), minlength=len(km)).astype(np.int64))
        return self.tables[m]

    def graph(self, k, min_occ):
        """(kmers, counts, arcs) by brute force"""
        if (k, min_occ) not in self.graphs:
            km, ct = self.table(k)
            k1, c1 = self.table(k + 1)
            keep = ct >= min_occ
            self.graphs[(k, min_occ)] = (km[keep], np.minimum(ct[keep], 2 ** 32 - 1).astype(np.uint32), R.arcs_from_k1_list(km[keep], k1[c1 >= min_occ], k))
        return self.graphs[(k, min_occ)]

    def compact(self, k, min_occ):
        if (k, min_occ) not in self.compacted:
            km, ct, ar = self.graph(k, min_occ)
            self.compacted[(k, min_occ)] = R.compact([R.unpack(int(x), k) for x in km], ar.tolist(), k, ct.tolist())
        return self.compacted[(k, min_occ)]


@pytest.fixture(scope="module")
def want(gpu):
    """per golden read set the brute force, filled in as the tests ask; dup32 has no FASTQ: its sequences are read back from the index"""
    sets = {name: Want(forward_as_indexed(name)) for name in ("tiny", "special", "palin", "repeat")}
    d = gpu.DevIndex.open(os.path.join(GOLD, "dup32.fmd"))
    try:
        n_seq = int(d.mcnt[1])
        seqs, ln, _ = d.retrieve(np.arange(n_seq, dtype=np.uint64), stride=256)
        assert int(ln.max()) <= 256
        both = [seqs[x, :ln[x]] for x in range(n_seq)]
        for x in range(0, n_seq, 997):                                             # sequence 2 i + 1 is the reverse complement of sequence 2 i
            assert np.array_equal(both[x ^ 1], revcomp(both[x]))
        sets["dup32"] = Want(both[0::2])
    finally:
        d.close()
    return sets


def same_labelling(got, ref):
    for f in ("unitig", "offset", "orient", "u_nodes", "u_first", "u_flags"):
        a, b = getattr(got, f), getattr(ref, f)
        assert np.array_equal(a, np.asarray(b, dtype=a.dtype)), (f, np.flatnonzero(a != np.asarray(b, dtype=a.dtype))[:8])


def check(d, w, k, min_occ, restated=True, cap=0):
    """one graph of the open index d against brute force w and the restatements -> (KUnitigs, stat)"""
    km, ct, ar = w.graph(k, min_occ)
    # (i) the nodes and their counts: brute force, and kcount's list
    gk, gc, ga, ast = d.kmer_arcs(k, min_occ, cap=cap, with_stat=True)
    assert gk.dtype == np.uint64 and gc.dtype == np.uint32 and ga.dtype == np.uint8
    assert np.array_equal(gk, km) and np.array_equal(gc, ct), (k, min_occ, len(gk), len(km))
    ck, cc, _ = d.kmer_counts(k, min_occ)
    assert np.array_equal(gk, ck) and np.array_equal(gc, cc)
    # (ii) the arcs: brute force, and what kcount's list for k + 1 implies
    assert np.array_equal(ga, ar), (k, min_occ, np.flatnonzero(ga != ar)[:8])
    k1, _, _ = d.kmer_counts(k + 1, min_occ)
    assert np.array_equal(ga, R.arcs_from_k1_list(gk, k1, k))
    assert ast["n_nodes"] == len(km) and ast["n_arcs"] == len(k1) and ast["n_links"] == 0 and ast["n_unitigs"] == 0
    # (iii) the labelling: the one-thread walk, and the restatement
    g = d.kmer_unitigs(k, min_occ, cap=cap, with_stat=True)
    assert np.array_equal(g.kmers, km) and np.array_equal(g.counts, ct) and np.array_equal(g.arcs, ar)
    host = hostlib.kgraph_compact_host(k, km, ar, ct)
    same_labelling(g, host)
    st = g.stat
    for f in ("n_nodes", "n_arcs", "n_links", "n_unitigs", "n_cycles"):
        assert st[f] == host.stat[f], (f, st[f], host.stat[f])
    assert st["n_arcs"] == len(k1) and st["n_unitigs"] == len(g.u_nodes) == st["n_nodes"] - st["n_links"] + st["n_cycles"]
    assert st["n_ext"] >= 2 * len(km) and (len(km) == 0 or st["n_rounds"] >= 1)
    strings = g.strings()
    if restated:
        ref = w.compact(k, min_occ)
        same_labelling(g, ref)
        assert strings == ref.strings
        assert (st["n_arcs"], st["n_links"], st["n_cycles"]) == (ref.n_arcs, ref.n_links, ref.n_cycles)
    # (iv) the invariants: a partition of the nodes, the node-count sum, every string cut back into the nodes, symmetric arcs
    n = len(km)
    first = np.zeros(len(g.u_nodes) + 1, dtype=np.int64)
    np.cumsum(g.u_nodes, out=first[1:])
    slot = first[g.unitig.astype(np.int64)] + g.offset.astype(np.int64)
    assert (g.offset < g.u_nodes[g.unitig]).all() and np.array_equal(np.sort(slot), np.arange(n)) and int(g.u_nodes.sum()) == n
    assert sum(len(s) - k + 1 for s in strings) == n
    cut = np.concatenate([windows_packed(nt6(s), k)[0] for s in strings] + [np.zeros(0, np.uint64)])
    assert np.array_equal(np.sort(cut), km)
    bits = []
    for c in range(4):
        x = km[(ar >> c & 1).astype(bool)]
        bits.append(x << np.uint64(2) | np.uint64(c))
        x = km[(ar >> (4 + c) & 1).astype(bool)]
        bits.append(np.uint64(c) << np.uint64(2 * k) | x)
    bits = np.concatenate(bits)                                                  # every arc bit as an oriented (k+1)-mer
    rcb = R.np_revcomp(bits, k + 1)
    u, cnt = np.unique(np.minimum(bits, rcb), return_counts=True)
    assert np.array_equal(u, k1) and np.array_equal(cnt, np.where(u == R.np_revcomp(u, k + 1), 1, 2))   # an arc is seen from both its nodes: once when they are one
    return g, st


# ---- 1. the golden sets ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["tiny", "special", "palin", "repeat", "dup32"])
def test_golden_sets(gpu, want, name, k):
    w = want[name]
    d = gpu.DevIndex.open(os.path.join(GOLD, name + ".fmd"))
    try:
        for min_occ in MIN_OCCS:
            g, st = check(d, w, k, min_occ)
            if name == "palin" and min_occ == 1:
                k1 = [R.unpack(int(x), k + 1) for x in w.table(k + 1)[0]]
                assert any(x == R.rc(x) for x in k1)   # (k+1)-mers that are their own reverse complement: halved counts decide arcs
    finally:
        d.close()


# ---- 2. hand-made graphs, as reads -------------------------------------------------------------------------------------------------------------------------
def open_reads(gpu, reads):
    return gpu.DevIndex.from_bwt(gpu.build_bwt([nt6(r) for r in reads]))


@pytest.mark.parametrize("name", sorted(n for n in R.SHAPES if n != "empty"))
def test_shapes(gpu, name):
    k, min_occ, reads = R.SHAPES[name]
    w = Want([nt6(r) for r in reads])
    d = open_reads(gpu, reads)
    try:
        g, st = check(d, w, k, min_occ)
        ref = w.compact(k, min_occ)
        nodes, counts, arcs = R.graph_from_strings(reads, k, min_occ)                # the dict over both strands gives what the window count gives
        assert [R.pack(x) for x in nodes] == g.kmers.tolist() and counts == g.counts.tolist() and arcs == g.arcs.tolist()
        R.check_shape(name, nodes, counts, arcs, ref)
        assert hostlib.kgraph_gfa_text(g) == R.gfa_text(ref, k) and hostlib.kgraph_fasta_text(g) == R.fasta_text(ref)
        for mo in MIN_OCCS:
            check(d, w, k, mo)
            check(d, w, 3, mo)
    finally:
        d.close()


def circle_reads(circ, read_len, step):
    """the circle cut into overlapping reads, every junction covered"""
    text = circ + circ[:read_len]
    return [text[a:a + read_len] for a in range(0, len(circ), step)]


def test_cycle_in_an_index(gpu):
    """a circular sequence cut into overlapping reads on both strands: an isolated cycle really occurs, at min_occ 1 and 2"""
    rng = random.Random(3)
    circ = "".join(rng.choice("ACGT") for _ in range(777))
    reads = circle_reads(circ, 60, 20)
    reads = [R.rc(r) if i % 3 == 0 else r for i, r in enumerate(reads)]
    w = Want([nt6(r) for r in reads])
    d = open_reads(gpu, reads)
    try:
        for k, min_occ in ((11, 1), (11, 2), (21, 1), (31, 1)):    # (reads of 60 every 20 bases: every 12-mer is in two reads, not every 22-mer)
            if True:
                g, st = check(d, w, k, min_occ)
                assert st["n_cycles"] == 1 and st["n_unitigs"] == 1 and st["n_nodes"] == st["n_links"] == 777 and g.u_flags.tolist() == [api.KGRAPH_CYCLE]
                s = g.strings()[0]
                assert len(s) == 777 + k - 1 and g.u_first[0] == 0 and g.orient[0] == 0 and R.pack(s[:k]) == int(g.kmers[0]) and s[:k - 1] == s[777:]
                assert s[:777] in (circ + circ) or R.rc(s)[k - 1:] in (circ + circ)
                assert hostlib.kgraph_gfa_text(g).endswith("LN:i:%d\nL\t0\t+\t0\t+\t%dM\n" % (777 + k - 1, k - 1))
    finally:
        d.close()


# ---- 3. more than 2^16 nodes in one chain: more than 16 doubling rounds -----------------------------------------------------------------------------------
LONG = 70050


@pytest.fixture(scope="module")
def long_text():
    rng = random.Random(2026)
    return "".join(rng.choice("ACGT") for _ in range(LONG))


def test_long_chain(gpu, long_text):
    k = 21
    reads = [long_text[a:a + 250] for a in range(0, LONG - 250 + 1, 100)]
    assert reads[-1] == long_text[-250:]
    w = Want([nt6(r) for r in reads])
    d = open_reads(gpu, reads)
    try:
        g, st = check(d, w, k, 1, restated=False)
        n = LONG - k + 1
        assert st["n_nodes"] == n > 2 ** 16 and st["n_unitigs"] == 1 and st["n_links"] == n - 1 and st["n_cycles"] == 0 and st["n_rounds"] > 16
        assert g.strings() == [min(long_text, R.rc(long_text))]
        fw = g.strings()[0] == long_text                                           # offsets run along the printed string, orientations follow it
        for j in range(0, n, 997):
            x = long_text[j:j + k]
            i = int(np.searchsorted(g.kmers, R.pack(min(x, R.rc(x)))))
            assert int(g.offset[i]) == (j if fw else n - 1 - j) and int(g.orient[i]) == int((x > R.rc(x)) == fw)
        g2, st2 = check(d, w, k, 2, restated=False)                                # every k-mer but those at the two ends is in two reads and more
        assert st2["n_unitigs"] == 1 and n - 400 < st2["n_nodes"] < n and st2["n_rounds"] > 16
    finally:
        d.close()


def test_long_cycle(gpu, long_text):
    k = 21
    reads = circle_reads(long_text, 250, 125)
    w = Want([nt6(r) for r in reads])
    d = open_reads(gpu, reads)
    try:
        g, st = check(d, w, k, 1, restated=False)
        assert st["n_nodes"] == st["n_links"] == LONG and st["n_unitigs"] == 1 and st["n_cycles"] == 1 and st["n_rounds"] > 2 * 16
        s = g.strings()[0]
        assert len(s) == LONG + k - 1 and g.u_first[0] == 0 and g.orient[0] == 0 and g.offset[0] == 0 and R.pack(s[:k]) == int(g.kmers[0])
        two = long_text + long_text
        assert s[:LONG] in two or R.rc(s)[k - 1:] in two
        assert np.array_equal(np.sort(g.offset), np.arange(LONG))
    finally:
        d.close()


# ---- 4. tables, capacity, arguments, an empty index -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [2, 4, "bare"])
def test_with_and_without_tables(gpu, want, monkeypatch, cfg):
    fn = os.path.join(GOLD, "tiny.fmd")
    if cfg == "bare":
        d = gpu.DevIndex.open_bare(fn)
    else:
        monkeypatch.setenv("FMD_PTAB_DEPTH", str(cfg))
        d = gpu.DevIndex.open(fn)
    try:
        check(d, want["tiny"], 21, 2)
        check(d, want["tiny"], 3, 1)
    finally:
        d.close()


def test_capacity(gpu, want):
    w = want["repeat"]
    n = len(w.graph(21, 2)[0])
    d = gpu.DevIndex.open(os.path.join(GOLD, "repeat.fmd"))
    try:
        for f in (d.kmer_arcs, d.kmer_unitigs):
            with pytest.raises(api.FmdError, match=r"\(-5\)"):
                f(21, 2, cap=n - 1)
            with pytest.raises(api.FmdError, match=r"\(-5\)"):
                f(21, 2, cap=1)
        check(d, w, 21, 2, cap=n)                                                  # a good call after the refused ones, at exactly the size
        check(d, w, 21, 2)
        with pytest.raises(api.FmdError, match=r"\(-2\)"):
            d.kmer_arcs(21, 2, cap=api.KGRAPH_MAX_NODES + 1)
    finally:
        d.close()


def test_arguments_one_strand_and_empty(gpu, want):
    d = gpu.DevIndex.open(os.path.join(GOLD, "tiny.fmd"))
    try:
        for kw in (dict(k=20), dict(k=2), dict(k=1), dict(k=32), dict(k=33), dict(k=0), dict(k=-3), dict(min_occ=0), dict(min_occ=-1)):
            for f in (d.kmer_arcs, d.kmer_unitigs):
                with pytest.raises(api.FmdError, match=r"\(-2\)"):
                    f(**dict(dict(k=21, min_occ=1), **kw))
        assert gpu.lib().fmd_kunitig(d.h, 21, 1, 0, None) == api.FMD_E_ARG and gpu.lib().fmd_karcs(d.h, 21, 1, 0, None, None, None) == api.FMD_E_ARG
        assert gpu.lib().fmd_kunitig(None, 21, 1, 0, None) == api.FMD_E_ARG
        stat = np.zeros(1, dtype=api.KGRAPH_STAT_DT)
        assert gpu.lib().fmd_karcs(d.h, 21, 2, 0, None, None, stat.ctypes.data) == 0   # without a sink: the counters only
        assert int(stat[0]["n_nodes"]) == len(want["tiny"].graph(21, 2)[0])
    finally:
        d.close()
    reads = [np.array([1, 1, 1, 2, 1, 3, 1, 1, 2, 1], dtype=np.uint8), np.array([2, 2, 1, 2, 2, 3, 2, 1], dtype=np.uint8)]   # many A and C, no T
    d = gpu.DevIndex.from_bwt(gpu.build_bwt_strands(reads, strands=api.STRAND_FWD))
    try:
        for f in (d.kmer_arcs, d.kmer_unitigs):
            with pytest.raises(api.FmdError, match=r"\(-2\)"):
                f(5, 1)
    finally:
        d.close()
    d = gpu.DevIndex.open(os.path.join(GOLD, "sub.empty.fmd"), empty_ok=True)
    try:
        g, st = check(d, Want([]), 21, 1)
        assert st["n_nodes"] == 0 and len(g.kmers) == 0 and len(g.u_nodes) == 0 and g.strings() == []
        assert hostlib.kgraph_gfa_text(g) == "H\tVN:Z:1.0\n"
    finally:
        d.close()


# ---- 5. the command --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,min_occ", [("repeat", 21, 2), ("tiny", 21, 2), ("palin", 5, 1), ("special", 11, 1)])
def test_cli(gpu, want, name, k, min_occ):
    fmd = os.path.join(GOLD, name + ".fmd")
    d = gpu.DevIndex.open(fmd)
    try:
        g = d.kmer_unitigs(k, min_occ)
    finally:
        d.close()
    args = [AMD, "kgraph", "-k", str(k), "-o", str(min_occ)]
    a = subprocess.run(args + [fmd], capture_output=True, timeout=120)
    assert a.returncode == 0, a.stderr
    assert a.stdout.decode() == hostlib.kgraph_gfa_text(g)
    assert ("[M::main_kgraph] k=%d nodes=%d " % (k, len(g.kmers))).encode() in a.stderr
    f = subprocess.run(args + ["-f", fmd], capture_output=True, timeout=120)
    assert f.returncode == 0 and f.stdout.decode() == hostlib.kgraph_fasta_text(g)
    p = subprocess.run(args + ["-a", fmd], capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stdout.decode() == hostlib.kgraph_arcs_text(k, g.kmers, g.counts, g.arcs)
    if name == "repeat":                                                           # the S strings, cut back into 21-mers, are the node list of kcount -k21 -o2 -d
        kc = subprocess.run([AMD, "kcount", "-k", "21", "-o", "2", "-d", fmd], capture_output=True, timeout=120)
        assert kc.returncode == 0
        listed = [ln.split("\t")[0] for ln in kc.stdout.decode().splitlines()]
        cut = []
        for ln in a.stdout.decode().splitlines():
            if ln.startswith("S\t"):
                s = ln.split("\t")[2]
                cut += [min(s[j:j + 21], R.rc(s[j:j + 21])) for j in range(len(s) - 20)]
        assert sorted(cut) == listed and len(listed) > 1000
        ref = want[name].compact(k, min_occ)
        assert a.stdout.decode() == R.gfa_text(ref, k) and f.stdout.decode() == R.fasta_text(ref)


def test_default_command_line(gpu):
    fmd = os.path.join(GOLD, "repeat.fmd")
    a = subprocess.run([AMD, "kgraph", fmd], capture_output=True, timeout=120)
    b = subprocess.run([AMD, "kgraph", "-k", "21", "-o", "2", fmd], capture_output=True, timeout=120)
    assert a.returncode == 0 and a.stdout == b.stdout and a.stdout.startswith(b"H\tVN:Z:1.0\nS\t0\t")
