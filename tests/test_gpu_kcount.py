"""GPU: kcount (fmd_kcount / fmd_kcount_part_dev, DevIndex.kmer_spectrum / kmer_counts, `fermi-amd kcount`) against brute force over the sequences as
indexed: the canonical form of every N-free k-window of the forward sequences, counted with numpy.  The kernel computes the other form of the same
number -- occ(W) on the index of both strands, halved for a k-mer that is its own reverse complement -- so the two meet only if both are right."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib
from harvest_ref import forward_as_indexed, revcomp      # the golden reads as `build` indexed them

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
GUARD = 0x5A5A5A5A5A5A5A5A


# ---- the forward sequences as indexed, and brute force over them --------------------------------------------------------------------------------
def canonical_windows(seqs, k):
    """the canonical packed k-mer of every N-free k-window of seqs, in no order"""
    sh = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    out = [np.zeros(0, dtype=np.uint64)]
    for r in seqs:
        if len(r) < k:
            continue
        base = (r.astype(np.uint64) - np.uint64(1)) & np.uint64(3)
        w = np.lib.stride_tricks.sliding_window_view(base, k)
        good = np.lib.stride_tricks.sliding_window_view((r >= 1) & (r <= 4), k).all(axis=1)
        fw = np.bitwise_or.reduce(w << sh, axis=1)
        rc = np.bitwise_or.reduce((np.uint64(3) - w[:, ::-1]) << sh, axis=1)
        out.append(np.minimum(fw, rc)[good])
    return np.concatenate(out)


class Want:
    """brute force for one read set, per k computed once"""

    def __init__(self, seqs):
        self.seqs, self.by_k = seqs, {}

    def counts(self, k):
        if k not in self.by_k:
            self.by_k[k] = np.unique(canonical_windows(self.seqs, k), return_counts=True)
        return self.by_k[k]

    def answer(self, k, min_occ, n_bins):
        """(kmers, counts, hist, n_kmers, n_total) as fmd_kcount defines them"""
        km, ct = self.counts(k)
        keep = ct >= min_occ
        km, ct = km[keep], ct[keep].astype(np.uint64)
        hist = np.bincount(np.minimum(ct, np.uint64(n_bins - 1)).astype(np.int64), minlength=n_bins).astype(np.uint64)
        return km, ct, hist, len(km), int(ct.sum())

    def palindromes(self, k):
        km, ct = self.counts(k)
        sh = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
        bases = (km[:, None] >> sh) & np.uint64(3)
        rc = np.bitwise_or.reduce((np.uint64(3) - bases[:, ::-1]) << sh, axis=1)
        return km[rc == km], ct[rc == km]


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


def check_all(d, w, k, min_occ, n_bins=1024, cap=0):
    """spectrum and list of one (k, min_occ) against brute force, exactly -> (stat of the spectrum, stat of the list)"""
    km, ct, hist, n_kmers, n_total = w.answer(k, min_occ, n_bins)
    got_hist, st = d.kmer_spectrum(k, min_occ=min_occ, n_bins=n_bins, cap=cap)
    assert np.array_equal(got_hist, hist), (k, min_occ, n_bins)
    assert st["n_kmers"] == n_kmers and st["n_total"] == n_total and st["overflow"] == 0 and got_hist[0] == 0
    got_km, got_ct, st2 = d.kmer_counts(k, min_occ=min_occ, cap=cap)
    assert got_km.dtype == np.uint64 and got_ct.dtype == np.uint32
    assert np.array_equal(got_km, km) and np.array_equal(got_ct.astype(np.uint64), ct), (k, min_occ)
    assert st2["n_kmers"] == n_kmers and st2["n_total"] == n_total
    return st, st2


# ---- 1. tiny ------------------------------------------------------------------------------------------------------------------------------------
def test_fixture_numbers(want):
    """the cases hit what they aim at: the numbers of the brute force itself"""
    t = want["tiny"]
    km, ct = t.counts(21)
    assert len(km) == 25547 and int((ct == 1).sum()) == 15448
    pk, pc = t.palindromes(6)
    assert len(pk) == 60 and int(t.counts(6)[1].max()) == 298
    assert len(want["special"].palindromes(20)[0]) == 1 and len(want["special"].palindromes(6)[0]) == 26
    assert len(want["palin"].palindromes(20)[0]) == 2 and len(want["palin"].palindromes(32)[0]) == 2 and len(want["palin"].palindromes(6)[0]) == 29


@pytest.mark.parametrize("k", [1, 2, 6, 21, 31, 32])
def test_tiny(gpu, want, k):
    d = gpu.DevIndex.open(os.path.join(GOLD, "tiny.fmd"))
    try:
        for min_occ in (1, 2, 5):
            st, _ = check_all(d, want["tiny"], k, min_occ)
            if min_occ == 1:                                                       # every N-free k-window of the forward sequences, once
                assert st["n_total"] == sum(max(len(r) - k + 1, 0) for r in want["tiny"].seqs)   # (tiny has no N)
    finally:
        d.close()


def test_tiny_rle(gpu, want):
    d = gpu.DevIndex.open(os.path.join(GOLD, "tiny.rle.fmd"))
    try:
        for min_occ in (1, 2, 5):
            check_all(d, want["tiny"], 21, min_occ)
    finally:
        d.close()


# ---- 2. special: N, short reads, palindromes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 6, 20, 21])
def test_special(gpu, want, k):
    w = want["special"]
    d = gpu.DevIndex.open(os.path.join(GOLD, "special.fmd"))
    try:
        for min_occ in (1, 2, 3):
            st, _ = check_all(d, w, k, min_occ)
            if min_occ == 1:
                assert st["n_total"] == len(canonical_windows(w.seqs, k))
    finally:
        d.close()


def test_special_palindrome_drops_out_below_its_halved_count(gpu, want):
    """a k-mer that is its own reverse complement occurs occ = 2 count times in the index: at min_occ = count + 1 <= occ it must be gone,
    although every inner level -- which sees occ -- lets it through"""
    w = want["special"]
    pk, pc = w.palindromes(6)
    assert len(pk) > 0
    d = gpu.DevIndex.open(os.path.join(GOLD, "special.fmd"))
    try:
        seen = 0
        for min_occ in sorted(set(int(c) + 1 for c in pc))[:4]:
            km, ct, st = d.kmer_counts(6, min_occ=min_occ)
            gone = pk[pc == min_occ - 1]                                           # occ = 2 min_occ - 2 >= min_occ for min_occ >= 2
            assert len(gone) > 0 and not np.isin(gone, km).any()
            assert np.isin(pk[pc >= min_occ], km).all()
            seen += int(min_occ >= 2)
        assert seen > 0
    finally:
        d.close()


# ---- 3. palin: palindromes at the top of the word ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 32])
def test_palin(gpu, want, k):
    d = gpu.DevIndex.open(os.path.join(GOLD, "palin.fmd"))
    try:
        for min_occ in (1, 2):
            check_all(d, want["palin"], k, min_occ)
    finally:
        d.close()


# ---- 4. large counts, the last bin --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [2, 8, 1024])
def test_dup32_large_counts(gpu, want, n_bins):
    w = want["dup32"]
    assert int(w.counts(21)[1].max()) >= 40000
    d = gpu.DevIndex.open(os.path.join(GOLD, "dup32.fmd"))
    try:
        st, _ = check_all(d, w, 21, 1, n_bins=n_bins)
        hist, _ = d.kmer_spectrum(21, n_bins=n_bins)
        assert hist[n_bins - 1] > 0
        check_all(d, w, 21, 1000, n_bins=n_bins)
    finally:
        d.close()


def test_repeat_counts_on_both_sides_of_the_last_bin(gpu, want):
    w = want["repeat"]
    ct = w.counts(21)[1]
    assert (ct < 15).any() and (ct >= 15).any()
    d = gpu.DevIndex.open(os.path.join(GOLD, "repeat.fmd"))
    try:
        check_all(d, w, 21, 1, n_bins=16)
        hist, _ = d.kmer_spectrum(21, n_bins=16)
        assert hist[15] == int((ct >= 15).sum()) and hist[1:15].sum() == int((ct < 15).sum())
    finally:
        d.close()


# ---- 5. the split -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 32])
def test_split_gives_the_same(gpu, want, k):
    """a capacity far below the frontier: parts overflow, are discarded and cut; histogram, list and sums do not change, and the sink sees
    ascending slices with no k-mer twice"""
    L = gpu.lib()
    d = gpu.DevIndex.open(os.path.join(GOLD, "tiny.fmd"))
    try:
        hist0, st0 = d.kmer_spectrum(k, n_bins=64)
        km0, ct0, _ = d.kmer_counts(k)
        for cap in (api.KCOUNT_MIN_CAP, 16384):
            hist, st = d.kmer_spectrum(k, n_bins=64, cap=cap)
            assert np.array_equal(hist, hist0) and st["n_kmers"] == st0["n_kmers"] and st["n_total"] == st0["n_total"]
            assert st["n_parts"] > 1
            if cap == api.KCOUNT_MIN_CAP:
                assert st["n_retries"] > 0
            slices = []
            km, ct, st = d.kmer_counts(k, cap=cap, slices=slices)
            assert st["n_parts"] > 1 and len(slices) > 1 and sum(slices) == len(km0)
            assert np.array_equal(km, km0) and np.array_equal(ct, ct0)             # ascending over the whole run as they came: nothing was sorted here
            assert (km[1:] > km[:-1]).all()
        hist, st = d.kmer_spectrum(k, min_occ=2, n_bins=64, cap=api.KCOUNT_MIN_CAP)
        w = want["tiny"].answer(k, 2, 64)
        assert np.array_equal(hist, w[2]) and st["n_kmers"] == w[3]
        for bad in (1, api.KCOUNT_MIN_CAP - 1, api.KCOUNT_MAX_CAP + 1):
            with pytest.raises(api.FmdError):
                d.kmer_spectrum(k, cap=bad)
        assert L.fmd_kcount_work_bytes(api.KCOUNT_MIN_CAP - 1) == 0 and L.fmd_kcount_work_bytes(api.KCOUNT_MIN_CAP) > 0
    finally:
        d.close()


# ---- 6. the part entry ------------------------------------------------------------------------------------------------------------------------
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


def part_dev(gpu, d, mem, k, min_occ, cap, n_bins, out_cap, listed=True):
    """one fmd_kcount_part_dev call from the four single-base roots, on buffers of exactly the stated sizes with guard words behind each"""
    L = gpu.lib()
    roots = np.zeros(4, dtype=api.INTV_DT)
    for i, c in enumerate((4, 3, 2, 1)):
        roots[i]["x"] = (d.cnt[c], d.cnt[5 - c], d.cnt[c + 1] - d.cnt[c]); roots[i]["info"] = c - 1
    wb = L.fmd_kcount_work_bytes(cap)
    assert wb % 16 == 0
    work = np.full(wb // 8 + 8, GUARD, dtype=np.uint64)
    hist = np.zeros(n_bins + 4, dtype=np.uint64); hist[n_bins:] = GUARD
    kmer = np.full(out_cap + 4, GUARD, dtype=np.uint64)
    count = np.full(out_cap + 4, 0x5A5A5A5A, dtype=np.uint32)
    d_work, d_hist, d_kmer, d_count, d_stat = mem.put(work), mem.put(hist), mem.put(kmer), mem.put(count), mem.put(np.zeros(7, dtype=np.uint64))
    gpu.check(L.fmd_kcount_part_dev(d.h, None, k, min_occ, 1, 4, mem.put(roots), cap, n_bins, d_hist, d_kmer if listed else None, d_count if listed else None,
                                    out_cap, d_stat, d_work, wb))
    d.sync()
    assert (mem.get(d_work, work)[wb // 8:] == GUARD).all()
    mem.get(d_hist, hist); mem.get(d_kmer, kmer); mem.get(d_count, count)
    assert (hist[n_bins:] == GUARD).all() and (kmer[out_cap:] == GUARD).all() and (count[out_cap:] == 0x5A5A5A5A).all()
    stat = mem.get(d_stat, np.zeros(1, dtype=api.KCOUNT_STAT_DT))[0]
    return hist[:n_bins], kmer[:out_cap], count[:out_cap], {f: int(stat[f]) for f in api.KCOUNT_STAT_DT.names}


def test_part_entry(gpu, want):
    L = gpu.lib()
    k, n_bins = 21, 32
    km, ct, hist, n_kmers, n_total = want["tiny"].answer(k, 1, n_bins)
    d = gpu.DevIndex.open(os.path.join(GOLD, "tiny.fmd"))
    mem = DevMem(gpu)
    try:
        cap = 1 << 18
        h, gk, gc, st = part_dev(gpu, d, mem, k, 1, cap, n_bins, n_kmers)          # a list of exactly the answer
        assert st["overflow"] == 0 and st["n_kmers"] == n_kmers and st["n_total"] == n_total and st["n_parts"] == 1 and st["n_ext"] > n_kmers
        order = np.argsort(gk)
        assert np.array_equal(gk[order], km) and np.array_equal(gc[order].astype(np.uint64), ct) and np.array_equal(h, hist)
        h, gk, gc, st = part_dev(gpu, d, mem, k, 1, cap, n_bins, n_kmers - 1)      # one short: the flag, and nothing past the end (part_dev looks at the guards)
        assert st["overflow"] == 1 and np.isin(gk, km).all()
        h, gk, gc, st = part_dev(gpu, d, mem, k, 1, cap, n_bins, 8, listed=False)  # no list: out_cap means nothing
        assert st["overflow"] == 0 and st["n_kmers"] == n_kmers and np.array_equal(h, hist) and (gk == GUARD).all()
        h, gk, gc, st = part_dev(gpu, d, mem, k, 1, api.KCOUNT_MIN_CAP, n_bins, n_kmers)   # a frontier that does not fit: the flag, the work area's guards intact
        assert st["overflow"] == 1
        # arguments
        wb = L.fmd_kcount_work_bytes(cap)
        buf = mem.put(np.zeros(wb // 8, dtype=np.uint64))
        small = mem.put(np.zeros(64, dtype=np.uint64))
        ok = dict(k=21, min_occ=1, root_len=1, n_roots=4, cap=cap, n_bins=n_bins, wb=wb, h=d.h, hist=small, stat=small, work=buf)

        def call(**kw):
            a = dict(ok, **kw)
            return L.fmd_kcount_part_dev(a["h"], None, a["k"], a["min_occ"], a["root_len"], a["n_roots"], small, a["cap"], a["n_bins"], a["hist"], None, None, 0,
                                         a["stat"], a["work"], a["wb"])
        for kw in (dict(k=1), dict(k=33), dict(min_occ=0), dict(n_bins=1), dict(root_len=0), dict(root_len=21), dict(cap=api.KCOUNT_MIN_CAP - 1), dict(wb=wb - 1),
                   dict(n_roots=cap + 1), dict(h=None), dict(hist=None), dict(stat=None), dict(work=None)):
            assert call(**kw) == api.FMD_E_ARG, kw
    finally:
        mem.free()
        d.close()


# ---- 7. no tables; 8. one strand --------------------------------------------------------------------------------------------------------------
def test_handle_without_tables(gpu, want):
    d = gpu.DevIndex.open_bare(os.path.join(GOLD, "tiny.fmd"))
    try:
        check_all(d, want["tiny"], 21, 1)
        hist, st = d.kmer_spectrum(21, n_bins=64, cap=api.KCOUNT_MIN_CAP)          # the split asks fmd_extend_batch for a root's children
        assert np.array_equal(hist, want["tiny"].answer(21, 1, 64)[2]) and st["n_retries"] > 0
    finally:
        d.close()


def test_one_strand_index_is_refused(gpu):
    reads = [np.array([1, 1, 1, 2, 1, 3, 1, 1, 2, 1], dtype=np.uint8), np.array([2, 2, 1, 2, 2, 3, 2, 1], dtype=np.uint8)]   # many A and C, no T
    d = gpu.DevIndex.from_bwt(gpu.build_bwt_strands(reads, strands=api.STRAND_FWD))
    try:
        with pytest.raises(api.FmdError, match=r"\(-2\)"):
            d.kmer_spectrum(5)
        with pytest.raises(api.FmdError, match=r"\(-2\)"):
            d.kmer_counts(5)
    finally:
        d.close()
    d = gpu.DevIndex.open(os.path.join(GOLD, "tiny.fmd"))
    try:
        for kw in (dict(k=0), dict(k=33), dict(k=21, min_occ=0), dict(k=21, n_bins=1)):
            with pytest.raises(api.FmdError, match=r"\(-2\)"):
                d.kmer_spectrum(**kw)
    finally:
        d.close()


# ---- 9. the command ---------------------------------------------------------------------------------------------------------------------------
def test_cli(gpu, want):
    fmd = os.path.join(GOLD, "tiny.fmd")
    d = gpu.DevIndex.open(fmd)
    try:
        hist, st = d.kmer_spectrum(21, n_bins=10001)
        km, ct, st2 = d.kmer_counts(21, min_occ=2)
    finally:
        d.close()
    a = subprocess.run([AMD, "kcount", "-k21", fmd], capture_output=True, timeout=120)
    assert a.returncode == 0, a.stderr
    assert a.stdout.decode() == "".join("%d\t%d\n" % (i, hist[i]) for i in range(len(hist)) if hist[i])
    assert ("[M::main_kcount] k=21 distinct=%d total=%d parts=" % (st["n_kmers"], st["n_total"])).encode() in a.stderr
    b = subprocess.run([AMD, "kcount", "-k21", "-d", "-o2", fmd], capture_output=True, timeout=120)
    assert b.returncode == 0, b.stderr
    assert b.stdout.decode() == "".join("%s\t%d\n" % (hostlib.kmer_text(x, 21), c) for x, c in zip(km.tolist(), ct.tolist()))
    assert subprocess.run([AMD, "kcount", "-k21", "-g", "0", fmd], capture_output=True, timeout=120).stdout == a.stdout
    assert subprocess.run([AMD, "kcount", "-k21", "-d", "-o2", "-g", "0", fmd], capture_output=True, timeout=120).stdout == b.stdout
    small = subprocess.run([AMD, "kcount", "-k6", "-b", "100", fmd], capture_output=True, timeout=120)   # counts up to 298: the last bin is labelled b - 1
    w = want["tiny"].answer(6, 1, 100)[2]
    assert small.returncode == 0 and small.stdout.decode() == "".join("%d\t%d\n" % (i, w[i]) for i in range(100) if w[i]) and small.stdout.decode().split("\n")[-2].startswith("99\t")
