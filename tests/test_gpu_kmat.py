"""GPU: kmat (fmd_kmat / fmd_kmat_part_dev, api.kmer_matrix_spectrum / kmer_matrix, `fermi-amd kmat`) against brute force over the sequences as indexed:
per read set the canonical form of every N-free k-window of the forward sequences, counted with numpy (the helper of test_gpu_kcmp.py, `build`'s palindrome
trim applied), the sets joined on the union.  The kernels compute the other form of the same numbers -- occ(W) on N indexes of both strands, each halved for
a k-mer that is its own reverse complement -- so the two meet only if both are right.  Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib
from test_gpu_kcmp import GUARD, DevMem, Wants, gold, packed_revcomp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
INF = api.KMAT_NO_MAX
EIGHT = ("ctA", "ctB", "cnA", "cnB", "tiny", "repeat", "palin", "special")
THREE, FIVE = ("ctA", "ctB", "cnA"), ("ctA", "ctB", "cnA", "tiny", "palin")
EMPTY = "sub.empty"
SUMS = ("n_kmers", "n_total", "n_present")


class Matrix:
    """N sets joined on the union of their canonical k-mers: km ascending, c[n, N]"""

    def __init__(self, wants, names, k):
        per = [wants.set("empty" if n == EMPTY else n).counts(k) for n in names]
        self.k, self.n_idx = k, len(names)
        self.km = np.unique(np.concatenate([p[0] for p in per] + [np.zeros(0, dtype=np.uint64)]))
        self.c = np.zeros((len(self.km), len(names)), dtype=np.uint64)
        for i, (km, ct) in enumerate(per):
            self.c[np.searchsorted(self.km, km), i] = ct
        self.pal = packed_revcomp(self.km, k) == self.km

    def answer(self, sel=None, present=1):
        """(kmers, counts[n, N], hist[2^N], the sums of the stat) as fmd_kmat defines them; sel = up to N pairs (min, max), max None = no bound"""
        keep = np.ones(len(self.km), dtype=bool)
        for i, (lo, hi) in enumerate(sel or []):
            keep &= self.c[:, i] >= np.uint64(lo)
            if hi is not None and hi != INF:
                keep &= self.c[:, i] <= np.uint64(hi)
        km, c = self.km[keep], self.c[keep]
        here = c >= np.uint64(present)
        pat = (here.astype(np.int64) << np.arange(self.n_idx, dtype=np.int64)).sum(axis=1)
        hist = np.bincount(pat, minlength=1 << self.n_idx).astype(np.uint64)
        sums = dict(n_kmers=len(km), n_total=[int(v) for v in c.sum(axis=0)], n_present=[int(v) for v in here.sum(axis=0)])
        return km, c, hist, sums


class Mats:
    def __init__(self, gpu):
        self.wants, self.mats = Wants(gpu), {}

    def get(self, names, k):
        if (names, k) not in self.mats:
            self.mats[(names, k)] = Matrix(self.wants, names, k)
        return self.mats[(names, k)]

    def set(self, name):
        return self.wants.set(name)


@pytest.fixture(scope="module")
def mats(gpu):
    """per tuple of golden read sets and k the brute force, filled in as the tests ask and shared among them"""
    return Mats(gpu)


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


def check_all(idx, m, sel=None, present=1, cap=0):
    """spectrum and list of one selection against brute force, exactly -> (stat of the spectrum, stat of the list)"""
    km, c, hist, sums = m.answer(sel, present)
    got_hist, st = api.kmer_matrix_spectrum(idx, m.k, sel=sel, present=present, cap=cap)
    assert got_hist.shape == (1 << m.n_idx,) and np.array_equal(got_hist, hist), (m.k, sel, present, got_hist[got_hist != hist], hist[got_hist != hist])
    assert {f: st[f] for f in SUMS} == sums and st["overflow"] == 0, (m.k, sel, st, sums)
    if present == 1:
        assert got_hist[0] == 0
    assert (st["n_parts"] >= 1 and st["n_retries"] < st["n_parts"] and st["n_ext"] > 0) or (m.k == 1 and st["n_parts"] == 0) or len(m.km) == 0 or len(km) == 0
    got_km, got_c, st2 = api.kmer_matrix(idx, m.k, sel=sel, present=present, cap=cap)
    assert got_km.dtype == np.uint64 and got_c.dtype == np.uint32 and got_c.shape == (len(km), m.n_idx)
    assert np.array_equal(got_km, km) and np.array_equal(got_c.astype(np.uint64), c), (m.k, sel)
    assert {f: st2[f] for f in SUMS} == sums and st2["overflow"] == 0
    return st, st2


# ---- 1. all eight ---------------------------------------------------------------------------------------------------------------------------------
def test_fixture_numbers(mats):
    """the cases hit what they aim at: many patterns at k = 21 and 32, one at k = 4, a trio selection that is not empty, palindromes where they are asked for"""
    m = mats.get(EIGHT, 21)
    assert int((m.answer()[2] != 0).sum()) >= 10 and 50000 < len(m.km) < 60000
    assert int((mats.get(EIGHT, 32).answer()[2] != 0).sum()) >= 10
    m = mats.get(EIGHT, 4)
    hist = m.answer()[2]
    assert len(m.km) == 136 and hist[255] == 136 and int(hist.sum()) == 136
    m = mats.get(THREE, 21)
    assert 150 < len(m.answer([(2, None), (0, 0), (0, 0)])[0]) < 260
    for k in (4, 20, 32):
        m = mats.get(("ctA", "palin", "special"), k)
        assert (m.pal & (m.c[:, 1] > 0)).any(), k


@pytest.mark.parametrize("k", [4, 21, 32])
def test_all_eight(gpu, mats, k):
    """the 256-cell spectrum, the sums and the list with eight columns; k = 32: the shift by 0 of the reverse complement"""
    m = mats.get(EIGHT, k)
    with Open(gpu, EIGHT) as idx:
        st, _ = check_all(idx, m)
        assert st["n_total"] == [mats.set(n).n_windows(k) for n in EIGHT]       # every N-free k-window of each set, once
        assert st["n_present"] == [len(mats.set(n).counts(k)[0]) for n in EIGHT]


# ---- 2. odd N: the last side alone in its round; N = 1 and 2 are kcount and kcmp ----------------------------------------------------------------------
@pytest.mark.parametrize("names", [THREE, FIVE, THREE + ("cnB",), FIVE + ("special",), FIVE + ("special", "repeat")], ids=lambda n: "N%d" % len(n))
def test_other_n(gpu, mats, names):
    with Open(gpu, names) as idx:
        for k in (6, 21):
            check_all(idx, mats.get(names, k))


def test_one_is_kcount(gpu):
    with Open(gpu, ("ctA",)) as (a,):
        for k in (1, 2, 6, 21, 32):
            km0, ct0, st0 = a.kmer_counts(k)
            km, c, st = api.kmer_matrix([a], k)
            assert np.array_equal(km, km0) and c.shape == (len(km0), 1) and np.array_equal(c[:, 0], ct0)
            assert st["n_kmers"] == st0["n_kmers"] and st["n_total"] == [st0["n_total"]] and st["n_present"] == [st0["n_kmers"]]
            hist, st = api.kmer_matrix_spectrum([a], k)
            assert hist.tolist() == [0, st0["n_kmers"]] and st["n_total"] == [st0["n_total"]]
            km3, ct3, _ = a.kmer_counts(k, min_occ=3)
            km, c, st = api.kmer_matrix([a], k, sel=[(3, None)])
            assert np.array_equal(km, km3) and np.array_equal(c[:, 0], ct3)


def test_two_is_kcmp(gpu):
    with Open(gpu, ("ctA", "ctB")) as (a, b):
        for k, sel in ((21, (0, None, 0, None)), (6, (0, None, 0, None)), (21, (3, None, 0, 0)), (32, (1, None, 1, None)), (2, (0, None, 0, None)), (1, (0, None, 0, None))):
            km0, c0, c1, st0 = a.kmer_compare(b, k, sel=sel)
            msel = [(sel[0], sel[1]), (sel[2], sel[3])]
            km, c, st = api.kmer_matrix([a, b], k, sel=msel)
            assert np.array_equal(km, km0) and np.array_equal(c[:, 0], c0) and np.array_equal(c[:, 1], c1)
            hist, st = api.kmer_matrix_spectrum([a, b], k, sel=msel)
            assert hist.tolist() == [0, st0["n_only0"], st0["n_only1"], st0["n_shared"]]
            assert st["n_total"] == [st0["n_total0"], st0["n_total1"]] and st["n_kmers"] == st0["n_kmers"]
            if k > 1:
                assert st["n_ext"] == a.kmer_compare_spectrum(b, k, sel=sel)[1]["n_ext"]


# ---- 3. a permutation of the handles permutes the columns and the pattern bits, and nothing else --------------------------------------------------------
def test_permutation(gpu, mats):
    perm = (3, 0, 4, 1, 2)
    with Open(gpu, FIVE) as idx:
        sel = [(0, None), (0, 5), (1, None), (0, None), (0, None)]
        for k, s in ((21, None), (21, sel), (6, None)):
            km, c, st = api.kmer_matrix(idx, k, sel=s)
            hist, _ = api.kmer_matrix_spectrum(idx, k, sel=s)
            km2, c2, st2 = api.kmer_matrix([idx[p] for p in perm], k, sel=None if s is None else [s[p] for p in perm])
            hist2, _ = api.kmer_matrix_spectrum([idx[p] for p in perm], k, sel=None if s is None else [s[p] for p in perm])
            assert np.array_equal(km2, km) and np.array_equal(c2, c[:, list(perm)])
            assert st2["n_total"] == [st["n_total"][p] for p in perm] and st2["n_present"] == [st["n_present"][p] for p in perm] and st2["n_ext"] == st["n_ext"]
            want = np.zeros_like(hist)
            for pat in range(32):                                                  # bit j of the new pattern is bit perm[j] of the old one
                want[sum((pat >> p & 1) << j for j, p in enumerate(perm))] += hist[pat]
            assert np.array_equal(hist2, want)


# ---- 4. one handle N times ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 8])
def test_one_handle_n_times(gpu, n):
    with Open(gpu, ("tiny",)) as (a,):
        for k in (6, 21):
            km0, ct0, _ = a.kmer_counts(k)
            km, c, st = api.kmer_matrix([a] * n, k)
            assert np.array_equal(km, km0) and all(np.array_equal(c[:, i], ct0) for i in range(n))
            hist, st = api.kmer_matrix_spectrum([a] * n, k)
            assert hist[(1 << n) - 1] == len(km0) and int(hist.sum()) == len(km0) and st["n_present"] == [len(km0)] * n


# ---- 5. the empty index as first, middle and last side -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [0, 1, 3])
def test_empty_side(gpu, mats, at):
    rest = THREE
    names = rest[:at] + (EMPTY,) + rest[at:]
    with Open(gpu, names) as idx:
        assert int(idx[at].mcnt[0]) == 0
        for k in (2, 21):
            st, _ = check_all(idx, mats.get(names, k))
            km, c, _ = api.kmer_matrix(idx, k)
            hist, _ = api.kmer_matrix_spectrum(idx, k)
            assert not c[:, at].any() and st["n_total"][at] == 0 and st["n_present"][at] == 0
            assert not hist[[p for p in range(16) if p >> at & 1]].any()
            without = [d for i, d in enumerate(idx) if i != at]
            km3, c3, st3 = api.kmer_matrix(without, k)
            assert np.array_equal(km, km3) and np.array_equal(np.delete(c, at, axis=1), c3) and st["n_ext"] == st3["n_ext"]
        km, c, st = api.kmer_matrix([idx[at]] * 3, 21)
        assert len(km) == 0 and c.shape == (0, 3) and st["n_kmers"] == 0
        check_all(idx, mats.get(names, 1))


# ---- 6. palindromes: every side is halved on its own ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 20, 32, 7])
def test_palindromes(gpu, mats, k):
    """a k-mer that is its own reverse complement occurs occ = 2 count times in an index: with c = m it must be gone at min = m + 1 <= occ, although every
    inner level -- which sees occ -- lets it through; its neighbours are untouched (an odd k has none: the same checks run dry)"""
    names = ("ctA", "palin", "special")
    m = mats.get(names, k)
    assert m.pal.any() == (k % 2 == 0)
    with Open(gpu, names) as idx:
        check_all(idx, m)
        side = 1
        seen = 0
        for v in sorted(set(int(x) for x in m.c[m.pal & (m.c[:, side] > 0), side]))[:3]:
            sel = [(0, None), (v + 1, None), (0, None)]
            km, c, st = api.kmer_matrix(idx, k, sel=sel)
            gone = m.km[m.pal & (m.c[:, side] == v)]
            assert len(gone) > 0 and not np.isin(gone, km).any() and np.isin(m.km[m.c[:, side] > v], km).all()
            check_all(idx, m, sel)
            km, c, st = api.kmer_matrix(idx, k, sel=[(0, None), (v, v), (0, None)])
            assert np.isin(gone, km).all() and (c[:, side] == v).all()
            seen += 1
        assert (seen > 0) == (k % 2 == 0)


# ---- 7. selections --------------------------------------------------------------------------------------------------------------------------------------
def test_selections(gpu, mats):
    m = mats.get(THREE, 21)
    with Open(gpu, THREE) as idx:
        full, _ = check_all(idx, m)
        trio = [(2, None), (0, 0), (0, 0)]
        st, _ = check_all(idx, m, trio)
        assert st["n_kmers"] > 0 and st["n_present"] == [st["n_kmers"], 0, 0] and st["n_ext"] < full["n_ext"]
        st, _ = check_all(idx, m, [(1, None)] * 3)                                 # the core
        assert st["n_kmers"] > 0 and st["n_ext"] < full["n_ext"]
        st, _ = check_all(idx, m, [(0, 1), (0, 2), (0, 0)])                         # upper bounds prune nothing
        assert st["n_kmers"] > 0 and st["n_ext"] == full["n_ext"]
        st, _ = check_all(idx, m, [(0, None), (3, 7)])                              # trailing entries left out
        assert st["n_ext"] < full["n_ext"]
        top = int(m.c[:, 0].max())
        st, _ = check_all(idx, m, [(top + 1, None), (0, None), (0, None)])          # nothing meets it
        assert st["n_kmers"] == 0 and st["n_ext"] < full["n_ext"]
        st, _ = check_all(idx, m, [(top, None), (0, 0), (1, None)])
    m8 = mats.get(EIGHT, 21)
    with Open(gpu, EIGHT) as idx:
        st, _ = check_all(idx, m8, [(1, None), (1, None), (0, None), (0, None), (0, 0), (0, None), (0, None), (0, 0)])
        assert st["n_kmers"] > 0


# ---- 8. the presence threshold ----------------------------------------------------------------------------------------------------------------------------
def test_present_3(gpu, mats):
    for names in (THREE, EIGHT):
        m = mats.get(names, 21)
        with Open(gpu, names) as idx:
            check_all(idx, m, present=3)
            hist, st = api.kmer_matrix_spectrum(idx, 21, present=3)
            assert hist[0] > 0 and int(hist.sum()) == st["n_kmers"] == len(m.km)
            km1, c1, _ = api.kmer_matrix(idx, 21)
            km3, c3, _ = api.kmer_matrix(idx, 21, present=3)
            assert np.array_equal(km1, km3) and np.array_equal(c1, c3)
            check_all(idx, m, [(2, None)], present=3)


# ---- 9. the split -----------------------------------------------------------------------------------------------------------------------------------------
def test_split_gives_the_same(gpu, mats):
    """a capacity far below the frontier: parts overflow, are discarded and cut; spectrum, sums and list do not change, and the sink sees ascending slices"""
    m = mats.get(EIGHT, 21)
    with Open(gpu, EIGHT) as idx:
        hist0, st0 = api.kmer_matrix_spectrum(idx, 21)
        km0, c0, _ = api.kmer_matrix(idx, 21)
        assert np.array_equal(km0, m.km)
        for cap in (api.KMAT_MIN_CAP, 16384):
            hist, st = api.kmer_matrix_spectrum(idx, 21, cap=cap)
            assert np.array_equal(hist, hist0) and {f: st[f] for f in SUMS} == {f: st0[f] for f in SUMS}
            assert st["n_parts"] > 1 and st["n_retries"] >= 1
            slices = []
            km, c, st = api.kmer_matrix(idx, 21, cap=cap, slices=slices)
            assert st["n_parts"] > 1 and st["n_retries"] >= 1 and len(slices) > 1 and sum(slices) == len(km0)
            assert np.array_equal(km, km0) and np.array_equal(c, c0) and (km[1:] > km[:-1]).all()   # ascending as they came: nothing was sorted here
        check_all(idx, m, [(2, None), (0, 0)], cap=api.KMAT_MIN_CAP)
        for bad in (1, api.KMAT_MIN_CAP - 1, api.KMAT_MAX_CAP + 1):
            with pytest.raises(api.FmdError, match=r"\(-2\)"):
                api.kmer_matrix_spectrum(idx, 21, cap=bad)


# ---- 10. large counts in one column -------------------------------------------------------------------------------------------------------------------------
def test_dup32_large_counts(gpu, mats):
    names = ("tiny", "dup32", "palin")
    m = mats.get(names, 21)
    assert int(m.c[:, 1].max()) >= 40000
    with Open(gpu, names) as idx:
        check_all(idx, m)
        check_all(idx, m, [(0, None), (1000, None)])
        check_all(idx, m, present=1000)


# ---- 11. the part entry -------------------------------------------------------------------------------------------------------------------------------------
def roots_of(idx, root_len):
    """the entries of every string of root_len bases: [kmer, 0, x0[N], size[N]] as uint64 words"""
    n = len(idx)
    if root_len == 1:
        strings = [[c] for c in (1, 2, 3, 4)]
    else:
        strings = [[1 + (v >> 2 * (root_len - 1 - j) & 3) for j in range(root_len)] for v in range(4 ** root_len)]
    roots = np.zeros((len(strings), 2 * (n + 1)), dtype=np.uint64)
    for r, s in enumerate(strings):
        roots[r, 0] = sum((b - 1) << 2 * (root_len - 1 - j) for j, b in enumerate(s))
    for i, d in enumerate(idx):
        if root_len == 1:
            beg = np.array([d.cnt[c] for c in (1, 2, 3, 4)], dtype=np.uint64)
            cnt = np.array([d.cnt[c + 1] - d.cnt[c] for c in (1, 2, 3, 4)], dtype=np.uint64)
        else:
            cnt, beg, _ = d.backward_search([np.array(s, dtype=np.uint8) for s in strings])
        roots[:, 2 + n + i] = cnt
        roots[:, 2 + i] = np.where(cnt > 0, beg, 0)
    return roots


def part_dev(gpu, idx, mem, k, sel, cap, out_cap, root_len=1, listed=True, present=1):
    """one fmd_kmat_part_dev call from the roots of one length, on buffers of exactly the stated sizes with guard words behind each"""
    L = gpu.lib()
    n = len(idx)
    wb = L.fmd_kmat_work_bytes(n, cap)
    assert wb % 16 == 0 and L.fmd_kmat_node_bytes(n) == 16 * (n + 1)
    cells = 1 << n
    work = np.full(wb // 8 + 8, GUARD, dtype=np.uint64)
    hist = np.zeros(cells + 4, dtype=np.uint64); hist[cells:] = GUARD
    kmer = np.full(out_cap + 4, GUARD, dtype=np.uint64)
    count = np.full(n * out_cap + 4, 0x5A5A5A5A, dtype=np.uint32)
    stat = np.full(22 + 4, GUARD, dtype=np.uint64)
    roots = roots_of(idx, root_len)
    hs = (C.c_void_p * n)(*[d.h for d in idx])
    d_work, d_hist, d_kmer, d_count, d_stat = mem.put(work), mem.put(hist), mem.put(kmer), mem.put(count), mem.put(stat)
    gpu.check(L.fmd_kmat_part_dev(n, hs, None, k, api.kmat_sel(n, sel, present).ctypes.data, root_len, len(roots), mem.put(roots), cap, d_hist,
                                  d_kmer if listed else None, d_count if listed else None, out_cap, d_stat, d_work, wb))
    idx[0].sync()
    assert (mem.get(d_work, work)[wb // 8:] == GUARD).all()
    mem.get(d_hist, hist); mem.get(d_kmer, kmer); mem.get(d_count, count); mem.get(d_stat, stat)
    assert (hist[cells:] == GUARD).all() and (kmer[out_cap:] == GUARD).all() and (count[n * out_cap:] == 0x5A5A5A5A).all() and (stat[22:] == GUARD).all()
    st = stat[:22].view(api.KMAT_STAT_DT)[0]
    sums = dict(n_kmers=int(st["n_kmers"]), n_total=[int(v) for v in st["n_total"][:n]], n_present=[int(v) for v in st["n_present"][:n]])
    assert not st["n_total"][n:].any() and not st["n_present"][n:].any()
    return hist[:cells], kmer[:out_cap], count[:n * out_cap].reshape(n, out_cap).T, {f: int(st[f]) for f in ("n_ext", "overflow", "widest_level", "n_parts", "n_retries")}, sums


def test_part_entry(gpu, mats):
    k = 21
    m = mats.get(THREE, k)
    km, c, hist, sums = m.answer()
    n = len(km)
    mem = DevMem(gpu)
    try:
        with Open(gpu, THREE) as idx:
            cap = 1 << 18
            for root_len in (1, 3):
                h, gk, gc, st, gs = part_dev(gpu, idx, mem, k, None, cap, n, root_len=root_len)   # a list of exactly the answer
                assert st["overflow"] == 0 and gs == sums and st["n_parts"] == 1 and st["n_ext"] > n
                order = np.argsort(gk)
                assert np.array_equal(gk[order], km) and np.array_equal(gc[order].astype(np.uint64), c) and np.array_equal(h, hist)
            h, gk, gc, st, gs = part_dev(gpu, idx, mem, k, None, cap, 37)                  # a tiny list: the flag, and nothing past the end (part_dev looks at the guards)
            assert st["overflow"] == 1 and np.isin(gk, km).all() and np.array_equal(gc.astype(np.uint64), c[np.searchsorted(km, gk)])
            h, gk, gc, st, gs = part_dev(gpu, idx, mem, k, None, cap, 8, listed=False)     # no list: out_cap means nothing
            assert st["overflow"] == 0 and gs == sums and np.array_equal(h, hist) and (gk == GUARD).all() and (gc == 0x5A5A5A5A).all()
            trio = [(2, None), (0, 0), (0, 0)]
            wk, wc, wh, ws = m.answer(trio, 3)
            h, gk, gc, st, gs = part_dev(gpu, idx, mem, k, trio, cap, len(wk), root_len=3, present=3)
            assert st["overflow"] == 0 and np.array_equal(np.sort(gk), wk) and np.array_equal(h, wh) and gs == ws
            h, gk, gc, st, gs = part_dev(gpu, idx, mem, k, None, api.KMAT_MIN_CAP, n)       # a frontier that does not fit: the flag, the work area's guards intact
            assert st["overflow"] == 1
        with Open(gpu, ("ctA", "ctB")) as idx:                                             # the leaf on the roots
            wk, wc, wh, ws = mats.get(("ctA", "ctB"), 2).answer()
            h, gk, gc, st, gs = part_dev(gpu, idx, mem, 2, None, api.KMAT_MIN_CAP, len(wk))
            assert st["overflow"] == 0 and np.array_equal(np.sort(gk), wk) and np.array_equal(h, wh) and gs == ws
    finally:
        mem.free()


def test_part_entry_arguments(gpu):
    L = gpu.lib()
    fwd = gpu.DevIndex.from_bwt(gpu.build_bwt_strands([np.array([1, 1, 1, 2, 1, 3, 1, 1, 2, 1], dtype=np.uint8)], strands=api.STRAND_FWD))
    mem = DevMem(gpu)
    try:
        with Open(gpu, THREE) as idx:
            cap = api.KMAT_MIN_CAP
            wb = L.fmd_kmat_work_bytes(3, cap)
            buf = mem.put(np.zeros(wb // 8 + 2, dtype=np.uint64))
            small = mem.put(np.zeros(1024, dtype=np.uint64))
            ok = dict(n=3, h=[d.h for d in idx], k=21, sel=api.kmat_sel(3), root_len=1, n_roots=4, roots=small, cap=cap, hist=small, stat=small, work=buf, wb=wb)

            def call(**kw):
                v = dict(ok, **kw)
                hs = (C.c_void_p * 8)(*v["h"]) if v["h"] is not None else None
                return L.fmd_kmat_part_dev(v["n"], hs, None, v["k"], v["sel"].ctypes.data if v["sel"] is not None else None, v["root_len"], v["n_roots"], v["roots"],
                                           v["cap"], v["hist"], None, None, 0, v["stat"], v["work"], v["wb"])
            bad_p = api.kmat_sel(3); bad_p["present"] = 0
            for kw in (dict(n=0), dict(n=9), dict(k=1), dict(k=33), dict(root_len=0), dict(root_len=21), dict(cap=api.KMAT_MIN_CAP - 1), dict(cap=api.KMAT_MAX_CAP + 1),
                       dict(wb=wb - 1), dict(n_roots=cap + 1), dict(h=None), dict(h=[idx[0].h, None, idx[2].h]), dict(hist=None), dict(stat=None), dict(work=None),
                       dict(work=C.c_void_p(buf.value + 8)), dict(sel=None), dict(sel=api.kmat_sel(3, [(3, 2)])), dict(sel=api.kmat_sel(3, [(0, None), (0, None), (1, 0)])),
                       dict(sel=bad_p), dict(h=[fwd.h, idx[1].h, idx[2].h]), dict(h=[idx[0].h, idx[1].h, fwd.h])):
                assert call(**kw) == api.FMD_E_ARG, kw
            for kw in (dict(k=0), dict(k=33), dict(k=21, sel=[(3, 2)]), dict(k=21, present=0), dict(k=21, cap=5)):
                with pytest.raises(api.FmdError, match=r"\(-2\)"):
                    api.kmer_matrix_spectrum(idx, **kw)
            for bad in ([], [idx[0]] * 9, [idx[0], fwd]):
                with pytest.raises(api.FmdError, match=r"\(-2\)"):
                    api.kmer_matrix(bad, 21)
            assert L.fmd_kmat_work_bytes(3, cap - 1) == 0 and L.fmd_kmat_work_bytes(0, cap) == 0 and L.fmd_kmat_work_bytes(9, cap) == 0
    finally:
        mem.free()
        fwd.close()


# ---- 12. the extensions: one per (node, non-empty side) -------------------------------------------------------------------------------------------------------
def test_n_ext(gpu, mats):
    k = 12
    with Open(gpu, THREE) as idx:
        _, st = api.kmer_matrix_spectrum(idx, k)
        assert st["n_retries"] == 0
        assert st["n_ext"] == sum(mats.set(n).n_strings(d) for n in THREE for d in range(1, k))   # the strings of 1 .. k - 1 bases of each set


# ---- 13. handles without tables --------------------------------------------------------------------------------------------------------------------------------
def test_handles_without_tables(gpu, mats):
    m = mats.get(THREE, 21)
    with Open(gpu, THREE, opener=lambda n: gpu.DevIndex.open_bare(gold(n))) as idx:
        check_all(idx, m)
        st, _ = check_all(idx, m, [(2, None), (0, 1)], cap=api.KMAT_MIN_CAP)       # the split asks fmd_extend_batch for a root's children
        assert st["n_retries"] > 0


# ---- 14. the command -------------------------------------------------------------------------------------------------------------------------------------------
def test_cli(gpu, mats):
    names = ("ctA", "ctB", "cnA", EMPTY)
    files = [gold(n) for n in names]
    with Open(gpu, names) as idx:
        hist, st = api.kmer_matrix_spectrum(idx, 21)
        km, c, st2 = api.kmer_matrix(idx, 21, sel=[(3, None), (0, 0), (0, 0)])
        hist3, st3 = api.kmer_matrix_spectrum(idx, 21, sel=[(0, None), (1, 9)], present=2)
    p = subprocess.run([AMD, "kmat", "-k21"] + files, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    want = "".join("PT\t%s\t%d\n" % ("".join("1" if v >> i & 1 else "0" for i in range(4)), hist[v]) for v in range(16) if hist[v])
    want += "".join("SM\t%d\t%d\t%d\n" % (i, st["n_present"][i], st["n_total"][i]) for i in range(4))
    assert p.stdout.decode() == want == hostlib.kmat_pt_text(hist) + hostlib.kmat_sm_text(st["n_present"], st["n_total"])
    assert "PT\t1000\t" in want and "PT\t0001\t" not in want and ("[M::main_kmat] k=21 n=4 distinct=%d parts=" % st["n_kmers"]).encode() in p.stderr
    q = subprocess.run([AMD, "kmat", "-k21", "-d", "-s", "3:,0:0,0:0"] + files, capture_output=True, timeout=120)
    assert q.returncode == 0 and len(km) > 0, q.stderr
    assert q.stdout.decode() == "".join("%s\t%s\n" % (hostlib.kmer_text(x, 21), "\t".join(str(v) for v in row)) for x, row in zip(km.tolist(), c.tolist()))
    lines = [ln.split("\t")[0] for ln in q.stdout.decode().splitlines()]
    assert lines == sorted(lines) and len(set(lines)) == len(lines)
    r = subprocess.run([AMD, "kmat", "-k21", "-p2", "-s", ":,1:9", "-g", "0"] + files, capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout.decode() == hostlib.kmat_pt_text(hist3) + hostlib.kmat_sm_text(st3["n_present"], st3["n_total"])


# ---- 15. k = 1: the marginal counts; k = 2: the leaf on the roots ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_shortest_k(gpu, mats, k):
    with Open(gpu, FIVE) as idx:
        m = mats.get(FIVE, k)
        st, _ = check_all(idx, m)
        assert st["n_parts"] == (0 if k == 1 else 1)
        check_all(idx, m, [(0, None), (0, None), (0, None), (0, None), (int(m.c[:, 4].min()) + 1, None)])
        check_all(idx, m, present=int(m.c[:, 3].min()) + 1)
        check_all(idx, m, [(0, int(m.c[:, 0].max()) - 1)])
