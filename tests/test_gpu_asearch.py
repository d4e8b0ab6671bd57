"""GPU: asearch (fmd_asearch_bound_dev / fmd_asearch_dev / fmd_asearch_batch, DevIndex.approx_search / approx_bound, `fermi-amd asearch`) against brute
force in numpy over the sequences as indexed: every window of the query's length without a non-base, kept when it differs from the query in at most d
places, grouped by content.  The expected interval of a pattern is what the exact search (backward_search) gives for it on the same handle."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from fermi_amd import api, hostlib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
GUARD = 0x5A5A5A5A5A5A5A5A


# ---- the sequences as indexed, and brute force over them (revcomp, strands_of, fastq_names_reads: as in test_gpu_locate.py) ---------------------
def revcomp(s):
    out = s[::-1].copy()
    m = (out >= 1) & (out <= 4)
    out[m] = 5 - out[m]
    return out


def strands_of(reads, trim):
    """sequence 2 i = read i (an even-length read that is its own reverse complement loses its last base where `build` trims), 2 i + 1 = its reverse complement"""
    out = []
    for r in reads:
        r = np.ascontiguousarray(r, dtype=np.uint8)
        if trim:
            r = r[:hostlib.trim_palindrome(r)]
        out += [r, revcomp(r)]
    return out


def fastq_names_reads(name):
    tab = np.full(256, 5, dtype=np.uint8)
    for ch, v in zip(b"ACGTacgt", [1, 2, 3, 4, 1, 2, 3, 4]):
        tab[ch] = v
    with gzip.open(os.path.join(GOLD, name + ".fq.gz"), "rb") as f:
        lines = f.read().split(b"\n")
    return [lines[i][1:].split()[0].decode() for i in range(0, len(lines) - 1, 4)], [tab[np.frombuffer(lines[i], dtype=np.uint8)] for i in range(1, len(lines) - 1, 4)]


class Brute:
    """every sequence after the other with a 0 between them; mult = every sequence stands for that many copies"""

    def __init__(self, seqs, mult=1):
        self.text = np.frombuffer(b"\0".join(s.tobytes() for s in seqs) + b"\0", dtype=np.uint8)
        self.bytes = self.text.tobytes()
        self.bad = np.concatenate([[0], np.cumsum((self.text < 1) | (self.text > 4))])
        self.mult = mult

    def hits(self, q, d):
        """{pattern bytes: (n_sub, count)} of the patterns within d substitutions of q; the mismatches are counted six columns at a time over the windows still in"""
        q = np.asarray(q, dtype=np.uint8)
        L = len(q)
        if L == 0 or L > len(self.text):
            return {}
        win = sliding_window_view(self.text, L)
        idx = np.flatnonzero(self.bad[L:] - self.bad[:-L] == 0)                    # windows of bases only
        mm = np.zeros(len(idx), dtype=np.int64)
        for c in range(0, L, 6):
            mm += (win[idx, c:c + 6] != q[c:c + 6]).sum(axis=1)
            keep = mm <= d
            idx, mm = idx[keep], mm[keep]
        if len(idx) == 0:
            return {}
        pats, first, counts = np.unique(win[idx], axis=0, return_index=True, return_counts=True)
        return {pats[j].tobytes(): (int(mm[first[j]]), int(counts[j]) * self.mult) for j in range(len(pats))}

    def bound(self, q):
        """the restatement of k_asearch_bound: greedy disjoint substrings that do not occur, an N costs one"""
        lb, z, s = np.zeros(len(q), dtype=np.uint8), 0, 0
        for p in range(len(q)):
            if not 1 <= q[p] <= 4 or self.bytes.find(np.asarray(q[s:p + 1], dtype=np.uint8).tobytes()) < 0:
                z, s = z + 1, p + 1
            lb[p] = min(z, 255)
        return lb


def make_queries(strands, rng, n_sub, n_n, n_rand, lens):
    """n_sub substrings of strands with 0..3 bases changed, n_n with an N put in, n_rand random strings; lengths from `lens`"""
    qs = []
    for j in range(n_sub + n_n):
        ln = int(lens[j % len(lens)])
        while True:
            r = strands[int(rng.integers(len(strands)))]
            if len(r) >= ln:
                break
        at = int(rng.integers(0, len(r) - ln + 1))
        q = np.array(r[at:at + ln], dtype=np.uint8)
        for p in rng.integers(0, ln, size=int(rng.integers(0, 4))):
            q[p] = 1 + (int(q[p]) + int(rng.integers(0, 3))) % 4 if 1 <= q[p] <= 4 else int(rng.integers(1, 5))
        if j >= n_sub:
            q[int(rng.integers(ln))] = 5
        qs.append(q)
    qs += [rng.integers(1, 5, size=int(rng.integers(20, 46))).astype(np.uint8) for _ in range(n_rand)]
    return qs


class Set:
    """queries on one handle, the brute force per query and budget (filled in as asked, kept), the exact interval of every pattern seen"""

    def __init__(self, d, brute, qs):
        self.d, self.brute, self.qs, self.memo, self.beg = d, brute, qs, {}, {}

    def want(self, i, dmax):
        if (i, dmax) not in self.memo:
            self.memo[(i, dmax)] = self.brute.hits(self.qs[i], dmax) if 0 < len(self.qs[i]) <= api.ASEARCH_MAX_LEN else {}
        return self.memo[(i, dmax)]

    def begs(self, pats):
        new = sorted(set(p for p in pats if p not in self.beg))
        if new:
            cnt, beg, _ = self.d.backward_search([np.frombuffer(p, dtype=np.uint8) for p in new])
            for p, c, b in zip(new, cnt.tolist(), beg.tolist()):
                self.beg[p] = (c, b)
        return self.beg

    def check(self, strata, hits, dmax, which=None, listed=None, best=False):
        """strata and hits of approx_search(qs or qs[which], max_sub=dmax) against brute force: per query the set of (pattern, n_sub, cnt, beg); listed[i] =
        False: the query is truncated, its strata exact and no hit listed; best: only the lowest stratum with a hit -> the brute-force hit counts"""
        which = list(range(len(self.qs))) if which is None else which
        assert strata.shape == (len(which), dmax + 1, 2)
        key = list(zip(hits["query"].tolist(), hits["n_sub"].tolist(), hits["beg"].tolist()))
        assert key == sorted(key)                                                  # the order fmd_asearch_batch promises
        cut = np.searchsorted(hits["query"], np.arange(len(which) + 1))
        n_want = []
        for k, i in enumerate(which):
            w = self.want(i, dmax)
            if best and w:
                lo = min(v[0] for v in w.values())
                w = {p: v for p, v in w.items() if v[0] == lo}
            n_want.append(len(w))
            exp = np.zeros((dmax + 1, 2), dtype=np.uint64)
            for ns, c in w.values():
                exp[ns] += np.array([1, c], dtype=np.uint64)
            assert np.array_equal(strata[k], exp), (i, self.qs[i], strata[k], exp)
            got = hits[cut[k]:cut[k + 1]]
            if listed is not None and not listed[k]:
                assert len(got) == 0, i
                continue
            begs = self.begs(w.keys())
            exp_set = sorted((p, v[0], v[1], begs[p][1]) for p, v in w.items())
            assert all(begs[p][0] == v[1] for p, v in w.items()), i                # the exact search counts what brute force counts
            got_set = sorted((hostlib.asearch_pattern(self.qs[i], h).tobytes(), int(h["n_sub"]), int(h["cnt"]), int(h["beg"])) for h in got)
            assert got_set == exp_set, (i, self.qs[i])                             # (asearch_pattern raises unless sub[] is descending and 0xffff-padded)
            for h in got:
                assert np.array_equal(api.approx_pattern(self.qs[i], h), hostlib.asearch_pattern(self.qs[i], h))
            iv = sorted((int(h["beg"]), int(h["cnt"])) for h in got)
            assert all(a[0] + a[1] <= b[0] for a, b in zip(iv, iv[1:])), i         # distinct hits, disjoint intervals
        return n_want


@pytest.fixture(scope="module")
def main(gpu):
    """a 2 000-base genome, 300 reads of 40-60 bases from both strands with 2 % substitutions, 5 reads with an N, 3 reads 40 times over and one read of 60 A
    (intervals that stay wider than 63 deep into the walk): ~3 x 10^4 symbols.  200 queries of 0 .. 70 bases, mixed in one batch."""
    rng = np.random.default_rng(2024)
    genome = rng.integers(1, 5, size=2000).astype(np.uint8)
    reads = []
    for _ in range(300):
        ln = int(rng.integers(40, 61)); at = int(rng.integers(0, 2000 - ln + 1))
        r = genome[at:at + ln].copy()
        if rng.random() < 0.5:
            r = revcomp(r)
        for p in np.flatnonzero(rng.random(ln) < 0.02):
            r[p] = 1 + (int(r[p]) + int(rng.integers(0, 3))) % 4
        reads.append(r)
    for r in reads[:5]:
        r[int(rng.integers(len(r)))] = 5
    reads += [reads[i].copy() for i in (10, 20, 30) for _ in range(40)]
    reads.append(np.full(60, 1, dtype=np.uint8))
    strands = strands_of(reads, trim=False)
    lens = np.concatenate([np.arange(1, 46)] * 5)
    qs = make_queries(strands, rng, 178, 10, 10, lens)
    qs += [np.zeros(0, dtype=np.uint8), rng.integers(1, 5, size=70).astype(np.uint8)]     # one empty, one longer than every read
    assert len(qs) == 200 and sorted(set(len(q) for q in qs[:178])) == list(range(1, 46))
    d = gpu.DevIndex.from_bwt(gpu.build_bwt(reads))
    assert 30000 < d.n < 50000 and d.mcnt[2] == d.mcnt[5] and d.mcnt[3] == d.mcnt[4]
    s = Set(d, Brute(strands), qs)
    s.reads, s.rand = reads, list(range(188, 198))
    yield s
    d.close()


def search(s, dmax, which=None, **kw):
    qs = s.qs if which is None else [s.qs[i] for i in which]
    return s.d.approx_search(qs, max_sub=dmax, with_stat=True, **kw)


# ---- 1. no substitution: the exact search -------------------------------------------------------------------------------------------------------------
def test_max_sub_0_is_the_exact_search(gpu, main):
    """max_sub = 0: one hit with the interval backward_search gives, or none -- for every query, misses included.  (A query that holds an N has none by the
    semantics stated in the header -- an N equals no pattern base -- whatever the exact search, which matches an N of the index, finds.)"""
    strata, hits, st = search(main, 0, max_hits=1)
    cnt, beg, _ = main.d.backward_search(main.qs)
    has_n = np.array([bool((q == 5).any()) for q in main.qs])
    cnt[has_n] = 0
    assert (cnt > 0).sum() > 40 and (cnt == 0).sum() > 60
    assert np.array_equal(strata[:, 0, 0], (cnt > 0).astype(np.uint64)) and np.array_equal(strata[:, 0, 1], cnt)
    found = np.flatnonzero(cnt > 0)
    assert np.array_equal(hits["query"], found) and np.array_equal(hits["cnt"], cnt[found]) and np.array_equal(hits["beg"], beg[found])
    assert (hits["n_sub"] == 0).all() and (hits["sub"] == 0xFFFF).all()
    assert st["n_hits"] == len(found) and st["n_occ"] == int(cnt.sum()) and st["n_skipped"] == 1 and st["n_truncated"] == 0 and st["overflow"] == 0


# ---- 2. brute force -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dmax", [1, 2, 3])
def test_equals_brute_force(gpu, main, dmax):
    strata, hits, st = search(main, dmax, max_hits=10 ** 6)
    n_want = main.check(strata, hits, dmax)
    assert st["n_hits"] == len(hits) == sum(n_want) == int(strata[:, :, 0].sum()) and st["n_occ"] == int(strata[:, :, 1].sum()) == int(hits["cnt"].sum())
    assert st["n_skipped"] == 1 and st["n_truncated"] == 0 and st["n_unfinished"] == 0 and st["overflow"] == 0 and st["widest_level"] > 64 and st["n_ext"] > 0
    assert int(hits["cnt"].max()) > 63 and int((hits["n_sub"] == dmax).sum()) > 50


# ---- 3. the budget covers the whole query: level 0 is the last level -------------------------------------------------------------------------------------
def test_short_queries_every_lmer(gpu, main):
    rng = np.random.default_rng(5)
    qs = [rng.integers(1, 6, size=L).astype(np.uint8) for L in (1, 2, 3) for _ in range(3)]
    s = Set(main.d, main.brute, qs)
    strata, hits = main.d.approx_search(qs, max_sub=4, max_hits=1000)
    s.check(strata, hits, 4)
    for k, q in enumerate(qs):                                                     # every L-mer of bases that occurs, whatever the query
        L = len(q)
        occurring = set(main.brute.hits(np.ones(L, dtype=np.uint8), L))
        assert set(hostlib.asearch_pattern(q, h).tobytes() for h in hits[hits["query"] == k]) == occurring and len(occurring) >= 4 ** L - 2


# ---- 4. an N in the query costs one ---------------------------------------------------------------------------------------------------------------------
def test_n_costs_one(gpu, main):
    nnn = [np.full(3, 5, dtype=np.uint8)]
    strata, hits = main.d.approx_search(nnn, max_sub=2)
    assert len(hits) == 0 and not strata.any()
    strata, hits = main.d.approx_search(nnn, max_sub=3)
    assert len(hits) == int(strata[0, 3, 0]) == len(main.brute.hits(np.array([1, 1, 1]), 3)) >= 60 and not strata[0, :3].any()
    assert (hits["n_sub"] == 3).all() and np.array_equal(hits["sub"][:, :3] >> 2, np.tile([2, 1, 0], (len(hits), 1))) and (hits["sub"][:, 3] == 0xFFFF).all()
    Set(main.d, main.brute, nnn).check(strata, hits, 3)


# ---- 5. the bound -----------------------------------------------------------------------------------------------------------------------------------------
def test_bound(gpu, main):
    lb = main.d.approx_bound(main.qs)
    some = 0
    for q, got in zip(main.qs, lb):
        want = main.brute.bound(q)
        assert np.array_equal(got, want), (q, got, want)
        some += int(want[-1]) if len(want) else 0
    assert some > 100 and max(int(x.max()) for x in lb if len(x)) >= 4
    assert main.d.approx_bound([]) == []


def test_one_strand_index(gpu, main):
    """an index of the forward strands only: the bound is all zero (its test of both strands fails), the search still equals brute force over that strand"""
    d = gpu.DevIndex.from_bwt(gpu.build_bwt_strands(main.reads, gpu.STRAND_FWD))
    try:
        assert d.mcnt[2] != d.mcnt[5]
        which = list(range(0, 200, 3))
        qs = [main.qs[i] for i in which]
        assert all(not x.any() for x in d.approx_bound(qs))
        s = Set(d, Brute([np.ascontiguousarray(r, dtype=np.uint8) for r in main.reads]), qs)
        strata, hits = d.approx_search(qs, max_sub=2, max_hits=10 ** 6)
        assert sum(s.check(strata, hits, 2)) > 100
    finally:
        d.close()


# ---- 6. pruning changes nothing but the work ---------------------------------------------------------------------------------------------------------------
def test_pruning_changes_nothing(gpu, main):
    a = search(main, 2, max_hits=10 ** 6)
    b = search(main, 2, max_hits=10 ** 6, prune=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2]["n_hits"] == b[2]["n_hits"]
    assert a[2]["n_ext"] <= b[2]["n_ext"]
    ra = search(main, 2, which=main.rand)
    rb = search(main, 2, which=main.rand, prune=False)
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2]["n_ext"] < rb[2]["n_ext"]


# ---- the _dev form on buffers of exactly the stated sizes -----------------------------------------------------------------------------------------------------
class DevMem:
    def __init__(self, gpu):
        self.gpu, self.L, self.ptrs = gpu, gpu.lib(), []

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.gpu.check(self.L.fmd_dev_malloc(0, max(int(nbytes), 16), C.byref(p)))
        self.ptrs.append(p)
        return p

    def put(self, a):
        p = self.alloc(a.nbytes)
        if a.nbytes:
            self.gpu.check(self.L.fmd_memcpy_h2d(p, a.ctypes.data, a.nbytes, None))
        return p

    def get(self, p, a):
        self.gpu.check(self.L.fmd_memcpy_d2h(a.ctypes.data, p, a.nbytes, None))
        return a

    def free(self):
        for p in self.ptrs:
            self.L.fmd_dev_free(p)


def asearch_dev(gpu, d, mem, qs, max_sub, max_hits, levels, hit_cap, cap, prune=True):
    """one fmd_asearch_dev call -> (hits stored, strata, stat); guard words behind d_hits[hit_cap] and behind the work area are checked"""
    L = gpu.lib()
    flat, off = api.flatten_reads(qs)
    n = len(qs)
    d_seqs, d_off = mem.put(flat), mem.put(off)
    d_lb = None
    if prune:
        d_lb = mem.put(np.zeros(len(flat), dtype=np.uint8))
        gpu.check(L.fmd_asearch_bound_dev(d.h, None, n, d_seqs, d_off, d_lb))
    wb = L.fmd_asearch_work_bytes(n, cap)
    assert wb > 0 and wb % 16 == 0
    hits = np.full(hit_cap * 4 + 8, GUARD, dtype=np.uint64)
    work = np.full(wb // 8 + 8, GUARD, dtype=np.uint64)
    strata = np.full(n * (max_sub + 1) * 2 + 8, GUARD, dtype=np.uint64)
    d_hits, d_work, d_strata, d_stat = mem.put(hits), mem.put(work), mem.put(strata), mem.put(np.zeros(8, dtype=np.uint64))
    gpu.check(L.fmd_asearch_dev(d.h, None, n, d_seqs, d_off, d_lb, max_sub, max_hits, levels, d_hits if hit_cap else None, hit_cap, d_strata, d_stat, d_work, wb))
    d.sync()
    mem.get(d_hits, hits); mem.get(d_strata, strata)
    assert (hits[hit_cap * 4:] == GUARD).all() and (strata[n * (max_sub + 1) * 2:] == GUARD).all() and (mem.get(d_work, work)[wb // 8:] == GUARD).all()
    stat = mem.get(d_stat, np.zeros(1, dtype=api.ASEARCH_STAT_DT))[0]
    stat = {f: int(stat[f]) for f in api.ASEARCH_STAT_DT.names}
    stored = min(stat["n_hits"] + stat["n_truncated"] * max_hits, hit_cap)
    return hits[:hit_cap * 4].view(api.ASEARCH_HIT_DT)[:stored], strata[:n * (max_sub + 1) * 2].reshape(n, max_sub + 1, 2), stat


def by_query(hits):
    order = np.lexsort((hits["beg"], hits["n_sub"], hits["query"]))
    return hits[order]


# ---- 7. every capacity gives the same result ---------------------------------------------------------------------------------------------------------------------
def test_every_cap_the_same(gpu, main):
    a = search(main, 3, max_hits=10 ** 6)
    b = search(main, 3, max_hits=10 ** 6, cap=api.ASEARCH_MIN_CAP)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert {k: v for k, v in a[2].items() if k not in ("n_ext", "widest_level")} == {k: v for k, v in b[2].items() if k not in ("n_ext", "widest_level")}
    assert b[2]["n_ext"] > a[2]["n_ext"] and b[2]["widest_level"] > api.ASEARCH_MIN_CAP   # parts were discarded and cut: their work was done all the same
    c = search(main, 3, max_hits=10 ** 6, cap=1 << 14)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    mem = DevMem(gpu)
    try:
        n_all = int(a[2]["n_hits"])
        # the whole batch in the smallest work area: the flag, nothing written past the area
        hits, strata, st = asearch_dev(gpu, main.d, mem, main.qs, 3, 10 ** 6, 69, n_all, api.ASEARCH_MIN_CAP)
        assert st["overflow"] & 1 and st["widest_level"] > api.ASEARCH_MIN_CAP
        # room for everything: the whole answer, in any order
        hits, strata, st = asearch_dev(gpu, main.d, mem, main.qs, 3, 10 ** 6, 69, n_all, 1 << 16)
        assert st["overflow"] == 0 and st["n_unfinished"] == 0 and st["n_hits"] == n_all and st["n_skipped"] == 1 and np.array_equal(strata, a[0])
        assert np.array_equal(by_query(hits), a[1])
        # a hit array one short: the flag, and what was stored is part of the answer
        hits, strata, st = asearch_dev(gpu, main.d, mem, main.qs, 3, 10 ** 6, 69, n_all - 1, 1 << 16)
        assert st["overflow"] == 2 and np.array_equal(strata, a[0]) and len(hits) == n_all - 1
        assert set(h.tobytes() for h in hits) < set(h.tobytes() for h in a[1])
    finally:
        mem.free()


# ---- 8. max_hits ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_max_hits(gpu, main):
    full = search(main, 2, max_hits=10 ** 6)
    n_hits = full[0][:, :, 0].sum(axis=1)
    listed = n_hits <= 5
    assert 10 < (~listed).sum() < 190
    strata, hits, st = search(main, 2, max_hits=5)
    main.check(strata, hits, 2, listed=listed)
    assert np.array_equal(strata, full[0]) and np.array_equal(hits, full[1][listed[full[1]["query"]]])
    assert st["n_truncated"] == int((~listed).sum()) and st["n_hits"] == len(hits) == int(n_hits[listed].sum()) and st["n_occ"] == int(hits["cnt"].sum())
    # count only
    s0, h0, st0 = search(main, 2, max_hits=5, count_only=True)
    assert np.array_equal(s0, full[0]) and len(h0) == 0 and st0["n_truncated"] == st["n_truncated"] and st0["n_hits"] == st["n_hits"]
    mem = DevMem(gpu)
    try:
        hits_d, strata_d, st_d = asearch_dev(gpu, main.d, mem, main.qs, 2, 5, 69, 0, 1 << 16)
        assert np.array_equal(strata_d, full[0]) and st_d["overflow"] == 0 and st_d["n_truncated"] == st["n_truncated"] and st_d["n_hits"] == st["n_hits"]
        # listed through the _dev form: max_hits of every truncated query beside the hits of the others
        hits_d, strata_d, st_d = asearch_dev(gpu, main.d, mem, main.qs, 2, 5, 69, 200 * 5, 1 << 16)
        assert len(hits_d) == st["n_hits"] + 5 * st["n_truncated"] and np.array_equal(np.bincount(hits_d["query"], minlength=200), np.minimum(n_hits, 5))
        assert np.array_equal(by_query(hits_d[listed[hits_d["query"]]]), hits)
    finally:
        mem.free()
    # more hits than the hit buffer of a wave holds (128), all of one query
    six = [main.qs[5][:6]] if len(main.qs[5]) >= 6 else [main.qs[50][:6]]
    s = Set(main.d, main.brute, six)
    strata, hits = main.d.approx_search(six, max_sub=3, max_hits=10 ** 6)
    assert s.check(strata, hits, 3)[0] == len(hits) > 128


# ---- 9. the best stratum only ------------------------------------------------------------------------------------------------------------------------------------------
def test_best_stratum(gpu, main):
    strata, hits, st = search(main, 3, max_hits=10 ** 6, best=True)
    main.check(strata, hits, 3, best=True)
    assert ((strata[:, :, 0] > 0).sum(axis=1) <= 1).all() and sorted(set(hits["n_sub"].tolist())) == [0, 1, 2, 3]
    assert st["n_hits"] == len(hits) and st["n_skipped"] == 1


# ---- 10. fewer levels than the longest query ------------------------------------------------------------------------------------------------------------------------------
def test_levels(gpu, main):
    full = search(main, 2, max_hits=10 ** 6)
    mem = DevMem(gpu)
    try:
        for levels in (0, 1, 20):
            hits, strata, st = asearch_dev(gpu, main.d, mem, main.qs, 2, 10 ** 6, levels, len(full[1]), 1 << 16)
            done = np.array([len(q) - 1 <= levels for q in main.qs])                # L - 1 levels finish a query of L bases
            assert st["n_unfinished"] > 0 and st["overflow"] == 0
            assert np.array_equal(by_query(hits), full[1][done[full[1]["query"]]])
            assert np.array_equal(strata[done], full[0][done]) and not strata[~done].any()
        hits, strata, st = asearch_dev(gpu, main.d, mem, main.qs, 2, 10 ** 6, 69, len(full[1]), 1 << 16, prune=False)
        assert st["n_unfinished"] == 0 and np.array_equal(by_query(hits), full[1]) and np.array_equal(strata, full[0])
    finally:
        mem.free()


# ---- 11. the golden indexes ---------------------------------------------------------------------------------------------------------------------------------------------------
def fixture_strands(gpu, gold, name):
    if name == "dup32":                                                            # one read 40 000 times over (it has no FASTQ): brute force over one copy
        read = np.array([b"$ACGTN".index(c) for c in gold.npz("dup32_vectors.npz")["read"].tobytes()], dtype=np.uint8)
        return [read, revcomp(read)], 40000
    return strands_of(fastq_names_reads(name)[1], trim=True), 1


@pytest.mark.parametrize("name", ["tiny", "special", "palin", "repeat", "dup32"])
def test_golden_indexes(gpu, gold, name):
    strands, mult = fixture_strands(gpu, gold, name)
    rng = np.random.default_rng(len(name) * 7 + 1)
    longest = min(45, max(len(s) for s in strands))
    qs = make_queries(strands, rng, 50, 5, 5, rng.integers(1, longest + 1, size=55))
    want = None
    s = Set(None, Brute(strands, mult), qs)                                        # (the brute force once; the intervals from each handle)
    for opener in (gpu.DevIndex.open, gpu.DevIndex.open_bare):
        d = opener(gold.path(name + ".fmd"))
        try:
            assert int(d.mcnt[1]) == len(strands) * mult
            s.d, s.beg = d, {}
            strata, hits = d.approx_search(qs, max_sub=2, max_hits=10 ** 6)
            assert sum(s.check(strata, hits, 2)) > 50                               # (dup32 is two sequences of 100 bases: few patterns, counts of 40 000)
            if name == "dup32":
                assert int(hits["cnt"].min()) >= 32
            if want is not None:
                assert np.array_equal(strata, want[0]) and np.array_equal(hits, want[1])
            want = (strata, hits)
        finally:
            d.close()


def test_nothing_to_do_and_bad_arguments(gpu, gold, main):
    d = main.d
    L = gpu.lib()
    strata, hits, st = d.approx_search([], max_sub=2, with_stat=True)
    assert strata.shape == (0, 3, 2) and len(hits) == 0 and not any(st.values())
    # only queries that are skipped: empty, and longer than FMD_ASEARCH_MAX_LEN
    exact = main.reads[50][:30].copy()                                            # a piece of a read as it is: it occurs
    long_q = np.tile(exact, api.ASEARCH_MAX_LEN // len(exact) + 1)
    strata, hits, st = d.approx_search([np.zeros(0, np.uint8), long_q, long_q[:api.ASEARCH_MAX_LEN], exact], max_sub=1, with_stat=True)
    assert st["n_skipped"] == 2 and not strata[:3].any() and strata[3, 0, 0] == 1 and set(hits["query"].tolist()) == {3}
    assert [len(x) for x in d.approx_bound([long_q, exact])] == [len(long_q), len(exact)]
    mem = DevMem(gpu)
    try:
        hits, strata, st = asearch_dev(gpu, d, mem, [np.zeros(0, np.uint8), long_q, exact], 1, 100, len(long_q), 100, api.ASEARCH_MIN_CAP)
        assert st["n_skipped"] == 2 and st["n_unfinished"] == 0 and st["overflow"] == 0 and set(hits["query"].tolist()) == {2} and not strata[:2].any()
        flat, off = api.flatten_reads(main.qs[:10])
        wb = L.fmd_asearch_work_bytes(10, api.ASEARCH_MIN_CAP)
        d_seqs, d_off, d_strata, d_stat, d_work = mem.put(flat), mem.put(off), mem.alloc(10 * 3 * 16), mem.alloc(64), mem.alloc(wb + 16)
        call = lambda work, nbytes, max_sub=2, n=10: L.fmd_asearch_dev(d.h, None, n, d_seqs, d_off, None, max_sub, 10, 5, None, 0, d_strata, d_stat, work, nbytes)
        assert call(d_work, wb) == api.FMD_OK
        assert call(d_work, wb - 64) == api.FMD_E_ARG                               # too small for the smallest capacity
        assert call(C.c_void_p(d_work.value + 8), wb) == api.FMD_E_ARG              # misaligned
        assert call(d_work, wb, max_sub=5) == api.FMD_E_ARG and call(d_work, wb, max_sub=-1) == api.FMD_E_ARG
        assert call(None, wb) == api.FMD_E_ARG and call(d_work, wb, n=2 ** 32) == api.FMD_E_ARG
        assert call(None, 0, n=0) == api.FMD_OK                                     # n = 0 is a no-op
        d.sync()
        st = np.zeros(1, dtype=api.ASEARCH_STAT_DT)
        s2 = np.zeros(10 * 3 * 2, dtype=np.uint64)
        batch = lambda max_sub, cap, flags=0: L.fmd_asearch_batch(d.h, 10, flat.ctypes.data, off.ctypes.data, max_sub, 10, flags, cap, None, None, s2.ctypes.data, st.ctypes.data)
        assert batch(2, 0) == api.FMD_OK and s2.any()
        assert batch(5, 0) == api.FMD_E_ARG and batch(2, api.ASEARCH_MIN_CAP - 1) == api.FMD_E_ARG and batch(2, api.ASEARCH_MAX_CAP + 1) == api.FMD_E_ARG and batch(2, 0, flags=8) == api.FMD_E_ARG
    finally:
        mem.free()
    with pytest.raises(api.FmdError):
        d.approx_search(main.qs[:3], max_sub=5)


# ---- 12. the command -------------------------------------------------------------------------------------------------------------------------------------------------------------
def render(qs, names, strata, hits, max_hits):
    out, cut = [], np.searchsorted(hits["query"], np.arange(len(qs) + 1))
    for i, q in enumerate(qs):
        nh = int(strata[i, :, 0].sum())
        out.append("SQ\t%s\t%d\t%d\t%d\t%d\t%s" % (names[i], len(q), nh, int(strata[i, :, 1].sum()), nh <= max_hits, ",".join(str(int(v)) for v in strata[i, :, 0])))
        for h in hits[cut[i]:cut[i + 1]]:
            pat = hostlib.asearch_pattern(q, h)
            subs = ",".join("%d:%s>%s" % (v >> 2, "$ACGTN"[q[v >> 2]], "ACGT"[v & 3]) for v in sorted(int(x) for x in h["sub"][:int(h["n_sub"])]))
            out.append("AH\t%d\t%s\t%d\t%s" % (h["n_sub"], "".join("$ACGTN"[c] for c in pat), h["cnt"], subs or "*"))
        out.append("//")
    return out


def test_cli(gpu, gold, tmp_path):
    _, reads = fastq_names_reads("ctA")
    strands = strands_of(reads, trim=True)
    rng = np.random.default_rng(12)
    qs = make_queries(strands, rng, 24, 3, 3, rng.integers(12, 46, size=27))
    names = ["q%d" % i for i in range(len(qs))]
    fa = tmp_path / "q.fa"
    fa.write_text("".join(">%s\n%s\n" % (nm, "".join("$ACGTN"[c] for c in q)) for nm, q in zip(names, qs)))
    fmd, rank = gold.path("ctA.fmd"), gold.path("ctA.rank")
    d = gpu.DevIndex.open(fmd)
    try:
        strata, hits = d.approx_search(qs, max_sub=2, max_hits=1000)
        assert sum(Set(d, Brute(strands), qs).check(strata, hits, 2)) > 30
        best = d.approx_search(qs, max_sub=2, max_hits=1000, best=True)
        few = d.approx_search(qs, max_sub=2, max_hits=1)
    finally:
        d.close()
    run = lambda args: subprocess.run([AMD, "asearch"] + args + [fmd, str(fa)], capture_output=True, timeout=120)
    p = run(["-d", "2", "-l", "-r", rank])
    assert p.returncode == 0, p.stderr
    lines = p.stdout.decode().splitlines()
    assert [ln for ln in lines if not ln.startswith("OC")] == render(qs, names, strata, hits, 1000)
    # the OC lines behind every AH: what `locate` prints for that pattern
    pats = [ln.split("\t")[2] for ln in lines if ln.startswith("AH")]
    pf = tmp_path / "p.fa"
    pf.write_text("".join(">p%d\n%s\n" % (j, s) for j, s in enumerate(pats)))
    loc = subprocess.run([AMD, "locate", "-m", "1000", "-r", rank, fmd, str(pf)], capture_output=True, timeout=120)
    assert loc.returncode == 0, loc.stderr
    want_oc = [[ln for ln in blk.splitlines() if ln.startswith("OC")] for blk in loc.stdout.decode().split("//\n")[:-1]]
    got_oc = []
    for ln in lines:
        if ln.startswith("AH"):
            got_oc.append([])
        elif ln.startswith("OC"):
            got_oc[-1].append(ln)
    assert len(pats) == len(hits) and got_oc == want_oc and sum(map(len, got_oc)) >= int(hits["cnt"][hits["cnt"] <= 1000].sum()) > 100
    # without -l no OC line; -b and -m as the flags of the library
    p = run(["-d", "2"])
    assert p.returncode == 0 and p.stdout.decode().splitlines() == render(qs, names, strata, hits, 1000)
    p = run(["-d", "2", "-b"])
    assert p.returncode == 0 and p.stdout.decode().splitlines() == render(qs, names, best[0], best[1], 1000)
    p = run(["-d", "2", "-m", "1"])
    assert p.returncode == 0 and p.stdout.decode().splitlines() == render(qs, names, few[0], few[1], 1)
    assert any(ln.split("\t")[5] == "0" for ln in p.stdout.decode().splitlines() if ln.startswith("SQ"))
