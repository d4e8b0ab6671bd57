"""GPU: kcmp (fmd_kcmp / fmd_kcmp_part_dev, DevIndex.kmer_compare_spectrum / kmer_compare, `fermi-amd kcmp`) against brute force over the sequences as
indexed: per read set the canonical form of every N-free k-window of the forward sequences, counted with numpy, the two sets joined on the union.  The
kernel computes the other form of the same numbers -- occ(W) on two indexes of both strands, each halved for a k-mer that is its own reverse complement
-- so the two meet only if both are right."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
GUARD = 0x5A5A5A5A5A5A5A5A
INF = api.KCMP_NO_MAX
UNION, A_SPEC, B_SPEC, SHARED, BAND = (0, INF, 0, INF), (3, INF, 0, 0), (0, 0, 3, INF), (1, INF, 1, INF), (2, INF, 0, 1)
STAT_SUMS = ("n_kmers", "n_total0", "n_total1", "n_only0", "n_only1", "n_shared")


def gold(name):
    return os.path.join(GOLD, name + ".fmd")


# ---- the forward sequences as indexed, and brute force over them --------------------------------------------------------------------------------
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


def windows(seqs, k):
    """(forward, reverse complement) packed k-mers of every N-free k-window of seqs, in no order"""
    sh = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    r = np.concatenate([np.append(s, np.uint8(5)) for s in seqs] + [np.zeros(0, dtype=np.uint8)])   # one text, an N between the sequences: no window spans two
    if len(r) < k:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    base = (r.astype(np.uint64) - np.uint64(1)) & np.uint64(3)
    bad = np.concatenate([[0], np.cumsum((r < 1) | (r > 4))])
    good = bad[k:] == bad[:-k]
    w = np.lib.stride_tricks.sliding_window_view(base, k)[good]
    return np.bitwise_or.reduce(w << sh, axis=1), np.bitwise_or.reduce((np.uint64(3) - w[:, ::-1]) << sh, axis=1)


def packed_revcomp(km, k):
    sh = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    bases = (km[:, None] >> sh) & np.uint64(3)
    return np.bitwise_or.reduce((np.uint64(3) - bases[:, ::-1]) << sh, axis=1) if len(km) else km


class Want:
    """brute force for one read set, per k computed once"""

    def __init__(self, seqs):
        self.seqs, self.by_k, self.nodes = seqs, {}, {}

    def counts(self, k):
        if k not in self.by_k:
            fw, rc = windows(self.seqs, k)
            self.by_k[k] = np.unique(np.minimum(fw, rc), return_counts=True)
        return self.by_k[k]

    def n_windows(self, k):
        return len(windows(self.seqs, k)[0])

    def n_strings(self, d):
        """the distinct strings of d bases on either strand: the nodes at depth d of this set's trie"""
        if d not in self.nodes:
            fw, rc = windows(self.seqs, d)
            self.nodes[d] = len(np.unique(np.concatenate([fw, rc])))
        return self.nodes[d]


class Joint:
    """two sets joined on the union of their canonical k-mers"""

    def __init__(self, wa, wb, k):
        (ka, ca), (kb, cb) = wa.counts(k), wb.counts(k)
        self.k, self.km = k, np.union1d(ka, kb)
        self.c0, self.c1 = np.zeros(len(self.km), dtype=np.uint64), np.zeros(len(self.km), dtype=np.uint64)
        self.c0[np.searchsorted(self.km, ka)] = ca
        self.c1[np.searchsorted(self.km, kb)] = cb
        self.pal = packed_revcomp(self.km, k) == self.km

    def answer(self, sel, n_bins):
        """(kmers, c0, c1, hist2d, the sums of the stat) as fmd_kcmp defines them"""
        lo0, hi0, lo1, hi1 = (np.uint64(v) for v in sel)
        keep = (self.c0 >= lo0) & (self.c1 >= lo1)
        if sel[1] != INF:
            keep &= self.c0 <= hi0
        if sel[3] != INF:
            keep &= self.c1 <= hi1
        km, c0, c1 = self.km[keep], self.c0[keep], self.c1[keep]
        cell = np.minimum(c0, np.uint64(n_bins - 1)).astype(np.int64) * n_bins + np.minimum(c1, np.uint64(n_bins - 1)).astype(np.int64)
        hist = np.bincount(cell, minlength=n_bins * n_bins).astype(np.uint64).reshape(n_bins, n_bins)
        sums = dict(n_kmers=len(km), n_total0=int(c0.sum()), n_total1=int(c1.sum()), n_only0=int((c1 == 0).sum()), n_only1=int((c0 == 0).sum()),
                    n_shared=int(((c0 > 0) & (c1 > 0)).sum()))
        return km, c0, c1, hist, sums


class Wants:
    def __init__(self, gpu):
        self.gpu, self.sets, self.joints = gpu, {}, {}

    def set(self, name):
        if name not in self.sets:
            if name == "empty":
                self.sets[name] = Want([])
            elif name == "dup32":                                                  # no FASTQ: its sequences are read back from the index
                d = self.gpu.DevIndex.open(gold("dup32"))
                try:
                    n_seq = int(d.mcnt[1])
                    seqs, ln, _ = d.retrieve(np.arange(n_seq, dtype=np.uint64), stride=256)
                    assert int(ln.max()) <= 256
                    both = [seqs[x, :ln[x]] for x in range(n_seq)]
                    for x in range(0, n_seq, 997):                                 # sequence 2 i + 1 is the reverse complement of sequence 2 i
                        assert np.array_equal(both[x ^ 1], revcomp(both[x]))
                    self.sets[name] = Want(both[0::2])
                finally:
                    d.close()
            else:
                self.sets[name] = Want(forward_as_indexed(name))
        return self.sets[name]

    def joint(self, a, b, k):
        if (a, b, k) not in self.joints:
            self.joints[(a, b, k)] = Joint(self.set(a), self.set(b), k)
        return self.joints[(a, b, k)]


@pytest.fixture(scope="module")
def want(gpu):
    """per pair of golden read sets the brute force, filled in as the tests ask and shared among them"""
    return Wants(gpu)


class Pair:
    """two golden indexes open for a test"""

    def __init__(self, gpu, a, b, opener=None):
        opener = opener or (lambda n: gpu.DevIndex.open(gold(n), empty_ok=(n == "sub.empty")))
        self.a = opener(a)
        self.b = self.a if b is None else opener(b)

    def __enter__(self):
        return self.a, self.b

    def __exit__(self, *exc):
        if self.b is not self.a:
            self.b.close()
        self.a.close()


def check_all(a, b, j, sel, n_bins=64, cap=0):
    """spectrum and list of one selection against brute force, exactly -> (stat of the spectrum, stat of the list)"""
    km, c0, c1, hist, sums = j.answer(sel, n_bins)
    got_hist, st = a.kmer_compare_spectrum(b, j.k, sel=sel, n_bins=n_bins, cap=cap)
    assert got_hist.shape == (n_bins, n_bins) and np.array_equal(got_hist, hist), (j.k, sel, n_bins)
    assert {f: st[f] for f in STAT_SUMS} == sums and st["overflow"] == 0 and got_hist[0, 0] == 0, (j.k, sel, st, sums)
    assert (st["n_parts"] >= 1 and st["n_retries"] < st["n_parts"] and st["n_ext"] > 0) or (j.k == 1 and st["n_parts"] == 0) or len(j.km) == 0   # (k = 1: no part is run)
    got_km, g0, g1, st2 = a.kmer_compare(b, j.k, sel=sel, cap=cap)
    assert got_km.dtype == np.uint64 and g0.dtype == np.uint32 and g1.dtype == np.uint32
    assert np.array_equal(got_km, km) and np.array_equal(g0.astype(np.uint64), c0) and np.array_equal(g1.astype(np.uint64), c1), (j.k, sel)
    assert {f: st2[f] for f in STAT_SUMS} == sums and st2["overflow"] == 0
    return st, st2


# ---- 1. the numbers of the brute force itself -----------------------------------------------------------------------------------------------------
def test_fixture_numbers(want):
    """the cases hit what they aim at.  (From the sequences as indexed: `build` trims 2 reads of special and 4 of palin by a base, none of the other
    sets; the numbers are those of the untrimmed FASTQs all the same.)"""
    j = want.joint("ctA", "ctB", 21)
    assert len(j.km) == 23758 and int(((j.c0 > 0) & (j.c1 > 0)).sum()) == 5998 and int((j.c1 == 0).sum()) == 8882 and int((j.c0 == 0).sum()) == 8878
    assert int(((j.c0 >= 3) & (j.c1 == 0)).sum()) == 206
    j = want.joint("ctA", "ctB", 6)
    assert len(j.km) == 2069 and int(j.pal.sum()) == 62 and int((j.pal & ((j.c0 == 0) | (j.c1 == 0))).sum()) == 9
    j = want.joint("cnA", "cnB", 25)
    assert len(j.km) == 5974 and int((j.c1 == 0).sum()) == 211 and int((j.c0 == 0).sum()) == 175
    j = want.joint("tiny", "special", 21)
    assert len(j.km) == 28424 and int(((j.c0 > 0) & (j.c1 > 0)).sum()) == 0
    j = want.joint("palin", "special", 32)
    assert int(j.pal.sum()) == 2 and int((j.pal & (j.c1 == 0)).sum()) == 2


# ---- 2. ctA / ctB ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 6, 21, 32])
def test_ct(gpu, want, k):
    j = want.joint("ctA", "ctB", k)
    with Pair(gpu, "ctA", "ctB") as (a, b):
        for sel in (UNION, A_SPEC, B_SPEC, SHARED, BAND):
            st, _ = check_all(a, b, j, sel)
            if sel == UNION:                                                       # every N-free k-window of each set, once
                assert st["n_total0"] == want.set("ctA").n_windows(k) and st["n_total1"] == want.set("ctB").n_windows(k)
                if k > 1 and st["n_retries"] == 0:                                 # one extension per (node, non-empty side): the strings of 1 .. k - 1 bases of each set
                    assert st["n_ext"] == sum(want.set("ctA").n_strings(d) + want.set("ctB").n_strings(d) for d in range(1, k))


# ---- 3. cnA / cnB ---------------------------------------------------------------------------------------------------------------------------------
def test_cn(gpu, want):
    j = want.joint("cnA", "cnB", 25)
    with Pair(gpu, "cnA", "cnB") as (a, b):
        st, _ = check_all(a, b, j, (2, INF, 0, 0))
        assert st["n_kmers"] == st["n_only0"] > 0
        check_all(a, b, j, UNION)


# ---- 4. palindromes: each side is halved on its own -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,k", [(("ctA", "ctB"), 6), (("palin", "special"), 32)])
def test_palindromes(gpu, want, pair, k):
    """a k-mer that is its own reverse complement occurs occ = 2 count times in an index: with c0 = m it must be gone at min0 = m + 1 <= occ0, although
    every inner level -- which sees occ -- lets it through; and the halving of one side does not wait for the other"""
    j = want.joint(pair[0], pair[1], k)
    assert j.pal.any() and (j.pal & (j.c0 > 0) & (j.c1 == 0)).any()
    with Pair(gpu, *pair) as (a, b):
        check_all(a, b, j, UNION)
        seen = 0
        for m in sorted(set(int(c) for c in j.c0[j.pal & (j.c0 > 0)]))[:3]:
            km, c0, c1, st = a.kmer_compare(b, k, sel=(m + 1, INF, 0, INF))
            gone = j.km[j.pal & (j.c0 == m)]
            assert len(gone) > 0 and not np.isin(gone, km).any() and np.isin(j.km[j.pal & (j.c0 > m)], km).all()
            km, c0, c1, st = a.kmer_compare(b, k, sel=(m, m, 0, INF))
            assert np.isin(gone, km).all() and (c0 == m).all()
            seen += 1
        assert seen > 0
        if pair[0] == "ctA":                                                       # the same from the other side
            m = int(j.c1[j.pal & (j.c1 > 0)].min())
            km, c0, c1, st = a.kmer_compare(b, k, sel=(0, INF, m + 1, INF))
            assert not np.isin(j.km[j.pal & (j.c1 == m)], km).any()
            check_all(a, b, j, (0, INF, m + 1, INF))


# ---- 5. one index twice ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", [None, "tiny.rle"])
def test_one_index_twice(gpu, want, other):
    with Pair(gpu, "tiny", other) as (a, b):
        for k in (6, 21):
            km0, ct0, _ = a.kmer_counts(k)
            km, c0, c1, st = a.kmer_compare(b, k)
            assert np.array_equal(km, km0) and np.array_equal(c0, ct0) and np.array_equal(c1, ct0)
            assert st["n_shared"] == st["n_kmers"] == len(km0) and st["n_only0"] == 0 and st["n_only1"] == 0
            hist, st = a.kmer_compare_spectrum(b, k, n_bins=32)
            assert np.array_equal(hist, np.diag(np.diag(hist))) and int(hist.sum()) == len(km0)
            assert np.array_equal(np.diag(hist), a.kmer_spectrum(k, n_bins=32)[0])


def test_swapped(gpu, want):
    with Pair(gpu, "ctA", "ctB") as (a, b):
        for k, sel in ((21, UNION), (21, BAND), (6, A_SPEC)):
            km, c0, c1, st = a.kmer_compare(b, k, sel=sel)
            swapped = (sel[2], sel[3], sel[0], sel[1])
            km2, d0, d1, st2 = b.kmer_compare(a, k, sel=swapped)
            assert np.array_equal(km, km2) and np.array_equal(c0, d1) and np.array_equal(c1, d0)
            assert st2["n_only0"] == st["n_only1"] and st2["n_only1"] == st["n_only0"] and st2["n_total0"] == st["n_total1"] and st2["n_total1"] == st["n_total0"]
            h, _ = a.kmer_compare_spectrum(b, k, sel=sel, n_bins=32)
            h2, _ = b.kmer_compare_spectrum(a, k, sel=swapped, n_bins=32)
            assert np.array_equal(h2, h.T)


# ---- 6. projection; 7. disjoint sets; 8. an empty side --------------------------------------------------------------------------------------------
def test_projection(gpu, want):
    with Pair(gpu, "ctA", "ctB") as (a, b):
        for k in (6, 21):
            km, c0, c1, st = a.kmer_compare(b, k, sel=(1, INF, 0, INF))
            km0, ct0, _ = a.kmer_counts(k)
            assert np.array_equal(km, km0) and np.array_equal(c0, ct0)
            km, c0, c1, st = a.kmer_compare(b, k, sel=(0, INF, 1, INF))
            km1, ct1, _ = b.kmer_counts(k)
            assert np.array_equal(km, km1) and np.array_equal(c1, ct1)


def test_disjoint_sets(gpu, want):
    j = want.joint("tiny", "special", 21)
    with Pair(gpu, "tiny", "special") as (a, b):
        km, c0, c1, st = a.kmer_compare(b, 21, sel=SHARED)
        assert len(km) == 0 and len(c0) == 0 and st["n_kmers"] == 0 and st["overflow"] == 0
        hist, st = a.kmer_compare_spectrum(b, 21, sel=SHARED, n_bins=16)
        assert not hist.any() and st["n_kmers"] == 0
        km, c0, c1, st = a.kmer_compare(b, 21)
        ka, ca, _ = a.kmer_counts(21)
        kb, cb, _ = b.kmer_counts(21)
        order = np.argsort(np.concatenate([ka, kb]), kind="stable")
        assert np.array_equal(km, np.concatenate([ka, kb])[order])
        assert np.array_equal(c0, np.concatenate([ca, np.zeros_like(cb)])[order]) and np.array_equal(c1, np.concatenate([np.zeros_like(ca), cb])[order])
        check_all(a, b, j, UNION)


@pytest.mark.parametrize("k", [1, 2, 21])
def test_empty_side(gpu, want, k):
    with Pair(gpu, "tiny", "sub.empty") as (a, e):
        assert int(e.mcnt[0]) == 0
        km0, ct0, _ = a.kmer_counts(k)
        km, c0, c1, st = a.kmer_compare(e, k)
        assert np.array_equal(km, km0) and np.array_equal(c0, ct0) and not c1.any() and st["n_only0"] == st["n_kmers"] == len(km0) and st["n_total1"] == 0
        km, c0, c1, st = e.kmer_compare(a, k)
        assert np.array_equal(km, km0) and np.array_equal(c1, ct0) and not c0.any() and st["n_only1"] == st["n_kmers"]
        km, c0, c1, st = e.kmer_compare(e, k)
        assert len(km) == 0 and st["n_kmers"] == 0
        check_all(a, e, want.joint("tiny", "empty", k), UNION, n_bins=8)


# ---- 9. large counts, short histograms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [2, 8, 256])
def test_dup32_large_counts(gpu, want, n_bins):
    j = want.joint("dup32", "tiny", 21)
    assert int(j.c0.max()) >= 40000
    with Pair(gpu, "dup32", "tiny") as (a, b):
        st, _ = check_all(a, b, j, UNION, n_bins=n_bins)
        hist, st = a.kmer_compare_spectrum(b, 21, n_bins=n_bins)
        assert hist[n_bins - 1].any() and int(hist.sum()) == st["n_kmers"]
        check_all(a, b, j, (1000, INF, 0, INF), n_bins=n_bins)
        check_all(b, a, want.joint("tiny", "dup32", 21), UNION, n_bins=n_bins)


# ---- 10. the split ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 32])
def test_split_gives_the_same(gpu, want, k):
    """a capacity far below the frontier: parts overflow, are discarded and cut; histogram, list and sums do not change, and the sink sees ascending
    slices with no k-mer twice"""
    L = gpu.lib()
    j = want.joint("ctA", "ctB", k)
    with Pair(gpu, "ctA", "ctB") as (a, b):
        hist0, st0 = a.kmer_compare_spectrum(b, k, n_bins=64)
        km0, c00, c10, _ = a.kmer_compare(b, k)
        assert np.array_equal(km0, j.km)
        for cap in (api.KCMP_MIN_CAP, 16384):
            hist, st = a.kmer_compare_spectrum(b, k, n_bins=64, cap=cap)
            assert np.array_equal(hist, hist0) and {f: st[f] for f in STAT_SUMS} == {f: st0[f] for f in STAT_SUMS}
            assert st["n_parts"] > 1
            if cap == api.KCMP_MIN_CAP:
                assert st["n_retries"] > 0
            slices = []
            km, c0, c1, st = a.kmer_compare(b, k, cap=cap, slices=slices)
            assert st["n_parts"] > 1 and len(slices) > 1 and sum(slices) == len(km0)
            assert np.array_equal(km, km0) and np.array_equal(c0, c00) and np.array_equal(c1, c10)   # ascending over the whole run as they came: nothing was sorted here
            assert (km[1:] > km[:-1]).all()
            check_all(a, b, j, A_SPEC, cap=cap)
        for bad in (1, api.KCMP_MIN_CAP - 1, api.KCMP_MAX_CAP + 1):
            with pytest.raises(api.FmdError, match=r"\(-2\)"):
                a.kmer_compare_spectrum(b, k, cap=bad)
        assert L.fmd_kcmp_work_bytes(api.KCMP_MIN_CAP - 1) == 0 and L.fmd_kcmp_work_bytes(api.KCMP_MIN_CAP) > 0 and L.fmd_kcmp_work_bytes(api.KCMP_MAX_CAP + 1) == 0


# ---- 11. the part entry -----------------------------------------------------------------------------------------------------------------------------
class DevMem:
    def __init__(self, gpu):
        self.gpu, self.L, self.ptrs = gpu, gpu.lib(), []

    def put(self, a):
        p = C.c_void_p()
        self.gpu.check(self.L.fmd_dev_malloc(0, max(int(a.nbytes), 16), C.byref(p)))
        self.ptrs.append(p)
        if a.nbytes:
            self.gpu.check(self.L.fmd_memcpy_h2d(p, a.ctypes.data, a.nbytes, None))
        return p

    def get(self, p, a):
        self.gpu.check(self.L.fmd_memcpy_d2h(a.ctypes.data, p, a.nbytes, None))
        return a

    def free(self):
        for p in self.ptrs:
            self.L.fmd_dev_free(p)


def pair_roots(a, b):
    roots = np.zeros(4, dtype=api.KCMP_NODE_DT)
    for i, c in enumerate((4, 3, 2, 1)):
        roots[i]["x0"] = (a.cnt[c], b.cnt[c]); roots[i]["size"] = (a.cnt[c + 1] - a.cnt[c], b.cnt[c + 1] - b.cnt[c]); roots[i]["kmer"] = c - 1
    return roots


def sel_array(sel):
    s = np.zeros(1, dtype=api.KCMP_SEL_DT)
    s[0] = tuple(sel)
    return s


def part_dev(gpu, a, b, mem, k, sel, cap, n_bins, out_cap, listed=True):
    """one fmd_kcmp_part_dev call from the four single-base pair roots, on buffers of exactly the stated sizes with guard words behind each"""
    L = gpu.lib()
    wb = L.fmd_kcmp_work_bytes(cap)
    assert wb % 16 == 0
    n_cells = n_bins * n_bins
    work = np.full(wb // 8 + 8, GUARD, dtype=np.uint64)
    hist = np.zeros(n_cells + 4, dtype=np.uint64); hist[n_cells:] = GUARD
    kmer = np.full(out_cap + 4, GUARD, dtype=np.uint64)
    c01 = np.full(out_cap + 4, GUARD, dtype=np.uint64)
    s = sel_array(sel)
    d_work, d_hist, d_kmer, d_c01, d_stat = mem.put(work), mem.put(hist), mem.put(kmer), mem.put(c01), mem.put(np.zeros(11, dtype=np.uint64))
    gpu.check(L.fmd_kcmp_part_dev(a.h, b.h, None, k, s.ctypes.data, 1, 4, mem.put(pair_roots(a, b)), cap, n_bins, d_hist, d_kmer if listed else None,
                                  d_c01 if listed else None, out_cap, d_stat, d_work, wb))
    a.sync()
    assert (mem.get(d_work, work)[wb // 8:] == GUARD).all()
    mem.get(d_hist, hist); mem.get(d_kmer, kmer); mem.get(d_c01, c01)
    assert (hist[n_cells:] == GUARD).all() and (kmer[out_cap:] == GUARD).all() and (c01[out_cap:] == GUARD).all()
    stat = mem.get(d_stat, np.zeros(1, dtype=api.KCMP_STAT_DT))[0]
    return hist[:n_cells].reshape(n_bins, n_bins), kmer[:out_cap], c01[:out_cap], {f: int(stat[f]) for f in api.KCMP_STAT_DT.names}


def test_part_entry(gpu, want):
    L = gpu.lib()
    k, n_bins = 21, 32
    j = want.joint("ctA", "ctB", k)
    km, c0, c1, hist, sums = j.answer(UNION, n_bins)
    n = len(km)
    packed = c0 | c1 << np.uint64(32)
    fwd = gpu.DevIndex.from_bwt(gpu.build_bwt_strands([np.array([1, 1, 1, 2, 1, 3, 1, 1, 2, 1], dtype=np.uint8)], strands=api.STRAND_FWD))
    mem = DevMem(gpu)
    try:
        with Pair(gpu, "ctA", "ctB") as (a, b):
            cap = 1 << 18
            h, gk, gc, st = part_dev(gpu, a, b, mem, k, UNION, cap, n_bins, n)     # a list of exactly the answer
            assert st["overflow"] == 0 and {f: st[f] for f in STAT_SUMS} == sums and st["n_parts"] == 1 and st["n_ext"] > n
            order = np.argsort(gk)
            assert np.array_equal(gk[order], km) and np.array_equal(gc[order], packed) and np.array_equal(h, hist)
            h, gk, gc, st = part_dev(gpu, a, b, mem, k, UNION, cap, n_bins, n - 1)   # one short: the flag, and nothing past the end (part_dev looks at the guards)
            assert st["overflow"] == 1 and np.isin(gk, km).all() and np.array_equal(gc, packed[np.searchsorted(km, gk)])
            h, gk, gc, st = part_dev(gpu, a, b, mem, k, UNION, cap, n_bins, 8, listed=False)   # no list: out_cap means nothing
            assert st["overflow"] == 0 and st["n_kmers"] == n and np.array_equal(h, hist) and (gk == GUARD).all() and (gc == GUARD).all()
            wa = want.joint("ctA", "ctB", k).answer(A_SPEC, n_bins)
            h, gk, gc, st = part_dev(gpu, a, b, mem, k, A_SPEC, cap, n_bins, len(wa[0]))
            assert st["overflow"] == 0 and np.array_equal(np.sort(gk), wa[0]) and np.array_equal(h, wa[3]) and {f: st[f] for f in STAT_SUMS} == wa[4]
            h, gk, gc, st = part_dev(gpu, a, b, mem, k, UNION, api.KCMP_MIN_CAP, n_bins, n)   # a frontier that does not fit: the flag, the work area's guards intact
            assert st["overflow"] == 1
            # arguments
            wb = L.fmd_kcmp_work_bytes(cap)
            buf = mem.put(np.zeros(wb // 8, dtype=np.uint64))
            small = mem.put(np.zeros(64 * 64, dtype=np.uint64))
            good_sel, bad0, bad1 = sel_array(UNION), sel_array((3, 2, 0, INF)), sel_array((0, INF, 1, 0))
            ok = dict(k=21, sel=good_sel, root_len=1, n_roots=4, cap=cap, n_bins=n_bins, wb=wb, h0=a.h, h1=b.h, hist=small, stat=small, work=buf)

            def call(**kw):
                v = dict(ok, **kw)
                return L.fmd_kcmp_part_dev(v["h0"], v["h1"], None, v["k"], v["sel"].ctypes.data if v["sel"] is not None else None, v["root_len"], v["n_roots"], small,
                                           v["cap"], v["n_bins"], v["hist"], None, None, 0, v["stat"], v["work"], v["wb"])
            for kw in (dict(k=1), dict(k=33), dict(n_bins=1), dict(n_bins=1025), dict(root_len=0), dict(root_len=21), dict(cap=api.KCMP_MIN_CAP - 1),
                       dict(cap=api.KCMP_MAX_CAP + 1), dict(wb=wb - 1), dict(n_roots=cap + 1), dict(h0=None), dict(h1=None), dict(hist=None), dict(stat=None),
                       dict(work=None), dict(sel=None), dict(sel=bad0), dict(sel=bad1), dict(h0=fwd.h), dict(h1=fwd.h)):
                assert call(**kw) == api.FMD_E_ARG, kw
    finally:
        mem.free()
        fwd.close()


# ---- 12. handles ------------------------------------------------------------------------------------------------------------------------------------
def test_handles_without_tables(gpu, want):
    j = want.joint("ctA", "ctB", 21)
    with Pair(gpu, "ctA", "ctB", opener=lambda n: gpu.DevIndex.open_bare(gold(n))) as (a, b):
        check_all(a, b, j, UNION)
        st, _ = check_all(a, b, j, BAND, cap=api.KCMP_MIN_CAP)                     # the split asks fmd_extend_batch for a root's children
        assert st["n_retries"] > 0


def test_refused(gpu):
    reads = [np.array([1, 1, 1, 2, 1, 3, 1, 1, 2, 1], dtype=np.uint8), np.array([2, 2, 1, 2, 2, 3, 2, 1], dtype=np.uint8)]   # many A and C, no T
    fwd = gpu.DevIndex.from_bwt(gpu.build_bwt_strands(reads, strands=api.STRAND_FWD))
    d = gpu.DevIndex.open(gold("tiny"))
    try:
        for a, b in ((fwd, d), (d, fwd), (fwd, fwd)):
            with pytest.raises(api.FmdError, match=r"\(-2\)"):
                a.kmer_compare_spectrum(b, 5)
            with pytest.raises(api.FmdError, match=r"\(-2\)"):
                a.kmer_compare(b, 5)
        for kw in (dict(k=0), dict(k=33), dict(k=21, n_bins=1), dict(k=21, n_bins=1025), dict(k=21, sel=(3, 2, 0, INF)), dict(k=21, sel=(0, INF, 1, 0))):
            with pytest.raises(api.FmdError, match=r"\(-2\)"):
                d.kmer_compare_spectrum(d, **kw)
    finally:
        d.close()
        fwd.close()


# ---- 13. the command --------------------------------------------------------------------------------------------------------------------------------
def test_cli(gpu, want):
    fa, fb = gold("ctA"), gold("ctB")
    with Pair(gpu, "ctA", "ctB") as (a, b):
        hist, st = a.kmer_compare_spectrum(b, 21, n_bins=256)
        km, c0, c1, st2 = a.kmer_compare(b, 21, sel=(3, INF, 0, 0))
    p = subprocess.run([AMD, "kcmp", "-k21", fa, fb], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.decode() == hostlib.kcmp_hist_text(hist) == "".join("%d\t%d\t%d\n" % (i, j, hist[i, j]) for i in range(256) for j in range(256) if hist[i, j])
    line = "[M::main_kcmp] k=21 distinct=%d only0=%d only1=%d shared=%d total0=%d total1=%d parts=" % tuple(st[f] for f in ("n_kmers", "n_only0", "n_only1", "n_shared", "n_total0", "n_total1"))
    assert line.encode() in p.stderr
    q = subprocess.run([AMD, "kcmp", "-k21", "-d", "-a3", "-B0", fa, fb], capture_output=True, timeout=120)
    assert q.returncode == 0 and len(km) == 206, q.stderr
    assert q.stdout.decode() == "".join("%s\t%d\t%d\n" % (hostlib.kmer_text(x, 21), u, v) for x, u, v in zip(km.tolist(), c0.tolist(), c1.tolist()))
    assert ("[M::main_kcmp] k=21 distinct=%d only0=%d only1=0 shared=0 " % (len(km), len(km))).encode() in q.stderr
    assert subprocess.run([AMD, "kcmp", "-k21", "-g", "0", fa, fb], capture_output=True, timeout=120).stdout == p.stdout
    assert subprocess.run([AMD, "kcmp", "-k21", "-d", "-a3", "-B0", "-g", "0", fa, fb], capture_output=True, timeout=120).stdout == q.stdout
    small = subprocess.run([AMD, "kcmp", "-k6", "-n", "8", fa, gold("sub.empty")], capture_output=True, timeout=120)   # a label of n - 1: that many or more; an empty second file
    w = want.joint("ctA", "empty", 6).answer(UNION, 8)[3]
    assert small.returncode == 0 and small.stdout.decode() == hostlib.kcmp_hist_text(w) and "\n7\t0\t" in "\n" + small.stdout.decode()
