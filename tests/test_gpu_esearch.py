"""GPU: esearch (fmd_esearch_dev / fmd_esearch_batch, DevIndex.edit_search / edit_patterns, `fermi-amd esearch`) against brute force in numpy over the
sequences as indexed: the full edit-distance table of text[s : s + L + 4] against the query for EVERY start s at once (no trie), the distance of every length
read off its last column, windows of bases only, grouped by content.  It runs once per query at budget 4; its hits at distance <= d are the answer for
budget d.  The expected interval of a pattern is what the exact search (backward_search) gives for it on the same handle."""
import ctypes as C
import gzip
import os
import re
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
DMAX = api.ESEARCH_MAX_EDIT


# ---- the sequences as indexed, and brute force over them (revcomp, strands_of, fastq_names_reads: as in test_gpu_asearch.py) --------------------
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
    """every sequence after the other with a 0 behind each; mult = every sequence stands for that many copies"""

    def __init__(self, seqs, mult=1):
        self.text = np.frombuffer(b"".join(s.tobytes() + b"\0" for s in seqs), dtype=np.uint8)
        self.mult = mult

    def hits(self, q, d=DMAX):
        """{pattern bytes: (edit distance, count)} of the patterns within d edits of q.  Row r of the table, for all starts s at once: T[r][c] = ed(text[s : s + r],
        q[:c]); the term T[r][c - 1] + 1 is a running minimum along the row.  A start leaves when text[s + r - 1] is no base (the window would span a non-base) or
        when its whole row exceeds d (the row minimum never decreases)."""
        q = np.asarray(q, dtype=np.uint8)
        L = len(q)
        if L == 0:
            return {}
        text = self.text
        qb = np.where((q >= 1) & (q <= 4), q, 0).astype(np.uint8)                # an N of the query equals no base
        s = np.flatnonzero((text >= 1) & (text <= 4))
        cols = np.arange(L + 1, dtype=np.int16)
        T = np.tile(cols, (len(s), 1))
        found = []
        for r in range(1, L + d + 1):
            ch = text[s + r - 1]                                                   # (every sequence ends in a 0: a start is gone before it could run off the text)
            ok = (ch >= 1) & (ch <= 4)
            s, T, ch = s[ok], T[ok], ch[ok]
            if len(s) == 0:
                break
            X = np.empty_like(T)
            X[:, 0] = r
            X[:, 1:] = np.minimum(T[:, :-1] + (ch[:, None] != qb[None, :]), T[:, 1:] + 1)
            T = np.minimum.accumulate(X - cols, axis=1) + cols
            keep = T.min(axis=1) <= d
            s, T = s[keep], T[keep]
            hit = T[:, L] <= d
            if hit.any():
                found.append((r, s[hit], T[hit, L]))
        out = {}
        for r, ss, dist in found:
            pats, first, counts = np.unique(sliding_window_view(text, r)[ss], axis=0, return_index=True, return_counts=True)
            for j in range(len(pats)):
                out[pats[j].tobytes()] = (int(dist[first[j]]), int(counts[j]) * self.mult)
        return out


def edited(r, rng, n_edit):
    """r with n_edit random edits: a base changed, a base inserted, a base deleted"""
    q = list(int(x) for x in r)
    for _ in range(n_edit):
        kind, at = int(rng.integers(3)), int(rng.integers(len(q)))
        if kind == 0:
            q[at] = 1 + (q[at] + int(rng.integers(0, 3))) % 4 if 1 <= q[at] <= 4 else int(rng.integers(1, 5))
        elif kind == 1:
            q.insert(at, int(rng.integers(1, 5)))
        elif len(q) > 1:
            del q[at]
    return np.array(q, dtype=np.uint8)


def piece(strands, rng, ln):
    while True:
        r = strands[int(rng.integers(len(strands)))]
        if len(r) >= ln:
            at = int(rng.integers(0, len(r) - ln + 1))
            return np.array(r[at:at + ln], dtype=np.uint8)


def make_queries(strands, rng, n_edit, n_n, n_rand, lens):
    """n_edit pieces of strands with 0..3 edits of all three kinds, n_n with an N put in, n_rand random strings; lengths from `lens`"""
    qs = []
    for j in range(n_edit + n_n):
        q = edited(piece(strands, rng, int(lens[j % len(lens)])), rng, j % 4)
        if j >= n_edit:
            q[int(rng.integers(len(q)))] = 5
        qs.append(q)
    qs += [rng.integers(1, 5, size=int(rng.integers(20, 46))).astype(np.uint8) for _ in range(n_rand)]
    return qs


class Set:
    """queries on one handle, the brute force per query (once, at budget 4, kept), the exact interval of every pattern seen"""

    def __init__(self, d, brute, qs, dmax=DMAX):
        self.d, self.brute, self.qs, self.dmax, self.memo, self.beg = d, brute, qs, dmax, {}, {}

    def want(self, i, dmax):
        assert dmax <= self.dmax
        if i not in self.memo:
            self.memo[i] = self.brute.hits(self.qs[i], self.dmax) if 0 < len(self.qs[i]) <= api.ESEARCH_MAX_LEN else {}
        return {p: v for p, v in self.memo[i].items() if v[0] <= dmax}

    def begs(self, pats):
        new = sorted(set(p for p in pats if p not in self.beg))
        if new:
            cnt, beg, _ = self.d.backward_search([np.frombuffer(p, dtype=np.uint8) for p in new])
            for p, c, b in zip(new, cnt.tolist(), beg.tolist()):
                self.beg[p] = (c, b)
        return self.beg

    def check(self, strata, hits, dmax, which=None, listed=None, best=False):
        """strata and hits of edit_search(qs or qs[which], max_edit=dmax) against brute force: per query the set of (pattern, n_edit, cnt, beg, len), the patterns
        read back from the index (edit_patterns); listed[i] = False: the query is truncated, its strata exact and no hit listed; best: only the lowest stratum with
        a hit.  -> the brute-force hit counts"""
        which = list(range(len(self.qs))) if which is None else which
        assert strata.shape == (len(which), dmax + 1, 2)
        key = list(zip(hits["query"].tolist(), hits["n_edit"].tolist(), hits["beg"].tolist(), hits["len"].tolist()))
        assert key == sorted(key) and len(set(key)) == len(key)                    # the order fmd_esearch_batch promises; no hit twice
        assert not hits["reserved"].any()
        pats = [p.tobytes() for p in self.d.edit_patterns(hits)]
        cut = np.searchsorted(hits["query"], np.arange(len(which) + 1))
        n_want = []
        for k, i in enumerate(which):
            w = self.want(i, dmax)
            if best and w:
                lo = min(v[0] for v in w.values())
                w = {p: v for p, v in w.items() if v[0] == lo}
            n_want.append(len(w))
            exp = np.zeros((dmax + 1, 2), dtype=np.uint64)
            for ne, c in w.values():
                exp[ne] += np.array([1, c], dtype=np.uint64)
            assert np.array_equal(strata[k], exp), (i, self.qs[i], strata[k], exp)
            got = hits[cut[k]:cut[k + 1]]
            if listed is not None and not listed[k]:
                assert len(got) == 0, i
                continue
            begs = self.begs(w.keys())
            assert all(begs[p][0] == v[1] for p, v in w.items()), i                # the exact search counts what brute force counts
            exp_set = sorted((p, v[0], v[1], begs[p][1], len(p)) for p, v in w.items())
            got_set = sorted((pats[cut[k] + j], int(h["n_edit"]), int(h["cnt"]), int(h["beg"]), int(h["len"])) for j, h in enumerate(got))
            assert got_set == exp_set, (i, self.qs[i])                             # every distinct pattern once, with its exact distance
        return n_want


def build_main(gpu, rng):
    """a 2 000-base genome, 300 reads of 40-60 bases from both strands with 2 % substitutions, 5 reads with an N, 3 reads 40 times over, one read of 60 A
    (intervals that stay wider than 63 deep into the walk) and 12 reads with one base inserted or deleted: ~3 x 10^4 symbols"""
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
    for j in range(12):
        at = int(rng.integers(0, 1950)); r = list(genome[at:at + 50]); p = int(rng.integers(5, 45))
        if j % 2:
            del r[p]
        else:
            r.insert(p, int(rng.integers(1, 5)))
        reads.append(np.array(r, dtype=np.uint8))
    return reads


@pytest.fixture(scope="module")
def main(gpu):
    """the index of build_main and 64 queries, mixed in one batch: 36 pieces of the strands with 0..3 edits, 12 .. 45 bases; 1 .. 5 bases (<= budget, <= budget + 1);
    25 A (inside the homopolymer) and 62 A (beyond it); 6 with an N; 8 random strings; one empty, one longer than every read"""
    rng = np.random.default_rng(2025)
    reads = build_main(gpu, rng)
    strands = strands_of(reads, trim=False)
    qs = make_queries(strands, rng, 36, 6, 8, rng.integers(12, 46, size=42))
    short = [piece(strands, rng, L) for L in (1, 2, 3, 4, 5)] + [rng.integers(1, 5, size=L).astype(np.uint8) for L in (2, 3, 4, 5)] + [np.array([5, 2], dtype=np.uint8)]
    qs += short + [np.full(25, 1, dtype=np.uint8), np.full(62, 1, dtype=np.uint8)]
    qs += [np.zeros(0, dtype=np.uint8), rng.integers(1, 5, size=70).astype(np.uint8)]
    assert len(qs) == 64
    d = gpu.DevIndex.from_bwt(gpu.build_bwt(reads))
    assert 30000 < d.n < 50000 and d.mcnt[2] == d.mcnt[5] and d.mcnt[3] == d.mcnt[4]
    s = Set(d, Brute(strands), qs)
    s.reads, s.rand, s.short, s.homo = reads, list(range(42, 50)), list(range(50, 60)), 60
    yield s
    d.close()


def search(s, dmax, which=None, **kw):
    qs = s.qs if which is None else [s.qs[i] for i in which]
    return s.d.edit_search(qs, max_edit=dmax, with_stat=True, **kw)


@pytest.fixture(scope="module")
def full(main):
    """the whole set at every budget, nothing truncated: computed once, shared, left unchanged"""
    return {dmax: search(main, dmax, max_hits=10 ** 6) for dmax in range(DMAX + 1)}


# ---- 1. brute force ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dmax", [1, 2, 3, 4])
def test_equals_brute_force(gpu, main, full, dmax):
    strata, hits, st = full[dmax]
    n_want = main.check(strata, hits, dmax)
    assert st["n_hits"] == len(hits) == sum(n_want) == int(strata[:, :, 0].sum()) and st["n_occ"] == int(strata[:, :, 1].sum()) == int(hits["cnt"].sum())
    assert st["n_skipped"] == 1 and st["n_truncated"] == 0 and st["n_unfinished"] == 0 and st["overflow"] == 0 and st["widest_level"] > 64 and st["n_ext"] > 0
    qlen = np.array([len(q) for q in main.qs])[hits["query"]]
    assert (hits["len"] > qlen).sum() > 20 and (hits["len"] < qlen).sum() > 20 and int(hits["cnt"].max()) > 63 and int((hits["n_edit"] == dmax).sum()) > 50
    assert (hits["len"] >= np.maximum(1, qlen - dmax)).all() and (hits["len"] <= qlen + dmax).all()
    # a pattern that several alignments reach is listed once: 24 A against 25 A -- any of the 25 could be the one left out
    h = hits[(hits["query"] == main.homo) & (hits["len"] == 24)]
    assert len(h) == 1 and h["n_edit"][0] == 1 and main.d.edit_patterns(h)[0].tolist() == [1] * 24


# ---- 2. no edit: the exact search -------------------------------------------------------------------------------------------------------------------------
def test_max_edit_0_is_the_exact_search(gpu, main, full):
    """max_edit = 0: one hit with the interval backward_search gives, or none -- for every query, misses included.  A query that holds an N has none: an N
    equals no pattern base, whatever the exact search, which matches an N of the index, finds."""
    strata, hits, st = full[0]
    cnt, beg, _ = main.d.backward_search(main.qs)
    has_n = np.array([bool((q == 5).any()) for q in main.qs])
    assert has_n.sum() >= 7
    cnt[has_n] = 0
    assert (cnt > 0).sum() > 10 and (cnt == 0).sum() > 30
    assert np.array_equal(strata[:, 0, 0], (cnt > 0).astype(np.uint64)) and np.array_equal(strata[:, 0, 1], cnt)
    found = np.flatnonzero(cnt > 0)
    assert np.array_equal(hits["query"], found) and np.array_equal(hits["cnt"], cnt[found]) and np.array_equal(hits["beg"], beg[found])
    assert (hits["n_edit"] == 0).all() and np.array_equal(hits["len"], np.array([len(q) for q in main.qs])[found])
    assert st["n_hits"] == len(found) and st["n_occ"] == int(cnt.sum()) and st["n_skipped"] == 1 and st["n_truncated"] == 0 and st["overflow"] == 0
    main.check(strata, hits, 0)


# ---- 3. every hit of asearch is a hit here, at most as far away -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dmax", [1, 2, 3])
def test_contains_asearch(gpu, main, full, dmax):
    _, ahits = main.d.approx_search(main.qs, max_sub=dmax, max_hits=10 ** 6)
    _, hits, _ = full[dmax]
    mine = {(int(h["query"]), int(h["beg"]), int(h["len"])): int(h["n_edit"]) for h in hits}
    assert len(ahits) > 100
    closer = 0
    for h in ahits:
        k = (int(h["query"]), int(h["beg"]), len(main.qs[int(h["query"])]))
        assert k in mine and mine[k] <= int(h["n_sub"]), k
        closer += mine[k] < int(h["n_sub"])
    assert closer > 0 or dmax < 3                                                  # (one insertion and one deletion undo a shift that costs three substitutions or more, never fewer)


# ---- 4. queries no longer than the budget -------------------------------------------------------------------------------------------------------------------
def test_short_queries(gpu, main, full):
    """L <= d: the empty pattern would be within budget and is no hit; lengths go down to 1 and up to L + d, so levels beyond L run"""
    _, hits, _ = full[4]
    seen = 0
    for i in main.short:
        L = len(main.qs[i])
        got = hits[hits["query"] == i]
        if L <= 4:
            assert int(got["len"].min()) == 1 and int(got["len"].max()) > L and len(got) > 1000
            assert int(got["len"].max()) == L + 4 or (main.qs[i] == 5).any()      # (beside an N the budget buys one base less)
            seen += 1
    assert seen >= 7


# ---- 5. pruning changes nothing but the work ------------------------------------------------------------------------------------------------------------------
def test_pruning_changes_nothing(gpu, main, full):
    for dmax in (1, 2, 4):
        a = full[dmax]
        b = search(main, dmax, max_hits=10 ** 6, prune=False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2]["n_hits"] == b[2]["n_hits"]
        assert a[2]["n_ext"] < b[2]["n_ext"]
    ra = search(main, 2, which=main.rand)
    rb = search(main, 2, which=main.rand, prune=False)
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2]["n_ext"] < rb[2]["n_ext"]


def test_one_strand_index(gpu, main):
    """an index of the forward strands only: the bound is all zero (its test of both strands fails), so the walk is unpruned, and still equals brute force"""
    d = gpu.DevIndex.from_bwt(gpu.build_bwt_strands(main.reads, gpu.STRAND_FWD))
    try:
        assert d.mcnt[2] != d.mcnt[5]
        which = list(range(0, 64, 2))
        qs = [main.qs[i] for i in which]
        s = Set(d, Brute([np.ascontiguousarray(r, dtype=np.uint8) for r in main.reads]), qs, dmax=2)
        a = d.edit_search(qs, max_edit=2, max_hits=10 ** 6, with_stat=True)
        b = d.edit_search(qs, max_edit=2, max_hits=10 ** 6, with_stat=True, prune=False)
        assert sum(s.check(a[0], a[1], 2)) > 100
        assert np.array_equal(a[1], b[1]) and a[2]["n_ext"] == b[2]["n_ext"]
    finally:
        d.close()


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


def esearch_dev(gpu, d, mem, qs, max_edit, max_hits, levels, hit_cap, cap, prune=True):
    """one fmd_esearch_dev call -> (hits stored, strata, stat); guard words behind d_hits[hit_cap], d_strata and the work area are checked"""
    L = gpu.lib()
    flat, off = api.flatten_reads(qs)
    n = len(qs)
    d_seqs, d_off = mem.put(flat), mem.put(off)
    d_lb = None
    if prune:
        d_lb = mem.put(np.zeros(len(flat), dtype=np.uint8))
        gpu.check(L.fmd_asearch_bound_dev(d.h, None, n, d_seqs, d_off, d_lb))
    wb = L.fmd_esearch_work_bytes(n, cap)
    assert wb > 0 and wb % 16 == 0
    hits = np.full(hit_cap * 4 + 8, GUARD, dtype=np.uint64)
    work = np.full(wb // 8 + 8, GUARD, dtype=np.uint64)
    strata = np.full(n * (max_edit + 1) * 2 + 8, GUARD, dtype=np.uint64)
    d_hits, d_work, d_strata, d_stat = mem.put(hits), mem.put(work), mem.put(strata), mem.put(np.zeros(8, dtype=np.uint64))
    gpu.check(L.fmd_esearch_dev(d.h, None, n, d_seqs, d_off, d_lb, max_edit, max_hits, levels, d_hits if hit_cap else None, hit_cap, d_strata, d_stat, d_work, wb))
    d.sync()
    mem.get(d_hits, hits); mem.get(d_strata, strata)
    assert (hits[hit_cap * 4:] == GUARD).all() and (strata[n * (max_edit + 1) * 2:] == GUARD).all() and (mem.get(d_work, work)[wb // 8:] == GUARD).all()
    stat = mem.get(d_stat, np.zeros(1, dtype=api.ESEARCH_STAT_DT))[0]
    stat = {f: int(stat[f]) for f in api.ESEARCH_STAT_DT.names}
    stored = min(stat["n_hits"] + stat["n_truncated"] * max_hits, hit_cap)
    return hits[:hit_cap * 4].view(api.ESEARCH_HIT_DT)[:stored], strata[:n * (max_edit + 1) * 2].reshape(n, max_edit + 1, 2), stat


def by_query(hits):
    return hits[np.lexsort((hits["len"], hits["beg"], hits["n_edit"], hits["query"]))]


LEVELS = 70 + DMAX - 1                                                             # the longest query has 70 bases


# ---- 6. every capacity gives the same result -------------------------------------------------------------------------------------------------------------------
def test_every_cap_the_same(gpu, main, full):
    a = full[2]
    b = search(main, 2, max_hits=10 ** 6, cap=api.ESEARCH_MIN_CAP)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert {k: v for k, v in a[2].items() if k not in ("n_ext", "widest_level")} == {k: v for k, v in b[2].items() if k not in ("n_ext", "widest_level")}
    assert b[2]["n_ext"] > a[2]["n_ext"] and b[2]["widest_level"] > api.ESEARCH_MIN_CAP   # parts were discarded and cut: their work was done all the same
    c = search(main, 2, max_hits=10 ** 6, cap=1 << 14)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    mem = DevMem(gpu)
    try:
        # the short queries at budget 4 in the smallest work area: the flag, nothing written past the area
        short = [main.qs[i] for i in main.short]
        hits, strata, st = esearch_dev(gpu, main.d, mem, short, 4, 10 ** 6, 9, 1 << 17, api.ESEARCH_MIN_CAP)
        assert st["overflow"] & 1 and st["widest_level"] > api.ESEARCH_MIN_CAP
        # room for everything: the whole answer, in any order
        n_all = int(a[2]["n_hits"])
        hits, strata, st = esearch_dev(gpu, main.d, mem, main.qs, 2, 10 ** 6, LEVELS, n_all, 1 << 16)
        assert st["overflow"] == 0 and st["n_unfinished"] == 0 and st["n_hits"] == n_all and st["n_skipped"] == 1 and np.array_equal(strata, a[0])
        assert np.array_equal(by_query(hits), a[1])
        # a hit array one short: the flag, and what was stored is part of the answer
        hits, strata, st = esearch_dev(gpu, main.d, mem, main.qs, 2, 10 ** 6, LEVELS, n_all - 1, 1 << 16)
        assert st["overflow"] == 2 and np.array_equal(strata, a[0]) and len(hits) == n_all - 1
        assert set(h.tobytes() for h in hits) < set(h.tobytes() for h in a[1])
    finally:
        mem.free()


# ---- 7. max_hits ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_max_hits(gpu, main, full):
    n_hits = full[2][0][:, :, 0].sum(axis=1)
    listed = n_hits <= 5
    assert 10 < (~listed).sum() < 60
    strata, hits, st = search(main, 2, max_hits=5)
    main.check(strata, hits, 2, listed=listed)
    assert np.array_equal(strata, full[2][0]) and np.array_equal(hits, full[2][1][listed[full[2][1]["query"]]])
    assert st["n_truncated"] == int((~listed).sum()) and st["n_hits"] == len(hits) == int(n_hits[listed].sum()) and st["n_occ"] == int(hits["cnt"].sum())
    # count only
    s0, h0, st0 = search(main, 2, max_hits=5, count_only=True)
    assert np.array_equal(s0, full[2][0]) and len(h0) == 0 and st0["n_truncated"] == st["n_truncated"] and st0["n_hits"] == st["n_hits"]
    mem = DevMem(gpu)
    try:
        hits_d, strata_d, st_d = esearch_dev(gpu, main.d, mem, main.qs, 2, 5, LEVELS, 0, 1 << 16)
        assert np.array_equal(strata_d, full[2][0]) and st_d["overflow"] == 0 and st_d["n_truncated"] == st["n_truncated"] and st_d["n_hits"] == st["n_hits"]
        # listed through the _dev form: exactly max_hits of every truncated query beside the hits of the others
        hits_d, strata_d, st_d = esearch_dev(gpu, main.d, mem, main.qs, 2, 5, LEVELS, 64 * 5, 1 << 16)
        assert len(hits_d) == st["n_hits"] + 5 * st["n_truncated"] and np.array_equal(np.bincount(hits_d["query"], minlength=64), np.minimum(n_hits, 5))
        assert np.array_equal(by_query(hits_d[listed[hits_d["query"]]]), hits)
    finally:
        mem.free()


# ---- 8. the best stratum only ------------------------------------------------------------------------------------------------------------------------------------------
def test_best_stratum(gpu, main):
    strata, hits, st = search(main, 3, max_hits=10 ** 6, best=True)
    main.check(strata, hits, 3, best=True)
    assert ((strata[:, :, 0] > 0).sum(axis=1) <= 1).all() and sorted(set(hits["n_edit"].tolist())) == [0, 1, 2, 3]
    assert st["n_hits"] == len(hits) and st["n_skipped"] == 1


# ---- 9. fewer levels than the longest pattern ---------------------------------------------------------------------------------------------------------------------------
def test_levels(gpu, main, full):
    a = full[2]
    mem = DevMem(gpu)
    try:
        for levels in (0, 1, 20):
            hits, strata, st = esearch_dev(gpu, main.d, mem, main.qs, 2, 10 ** 6, levels, len(a[1]), 1 << 16)
            assert st["n_unfinished"] > 0 and st["overflow"] == 0
            assert np.array_equal(by_query(hits), a[1][a[1]["len"] <= levels + 1])        # level 0 and `levels` levels: the patterns of up to levels + 1 bases
            done = np.array([len(q) + 2 - 1 <= levels for q in main.qs])                    # L + max_edit - 1 levels finish a query of L bases
            assert np.array_equal(strata[done], a[0][done])
        hits, strata, st = esearch_dev(gpu, main.d, mem, main.qs, 2, 10 ** 6, LEVELS, len(a[1]), 1 << 16, prune=False)
        assert st["n_unfinished"] == 0 and np.array_equal(by_query(hits), a[1]) and np.array_equal(strata, a[0])
    finally:
        mem.free()


# ---- 10. the golden indexes ---------------------------------------------------------------------------------------------------------------------------------------------------
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
    qs = make_queries(strands, rng, 24, 3, 3, rng.integers(1, longest + 1, size=27))
    want = None
    s = Set(None, Brute(strands, mult), qs, dmax=1)                               # (the brute force once; the intervals from each handle)
    for opener in (gpu.DevIndex.open, gpu.DevIndex.open_bare):
        d = opener(gold.path(name + ".fmd"))
        try:
            assert int(d.mcnt[1]) == len(strands) * mult
            s.d, s.beg = d, {}
            strata, hits = d.edit_search(qs, max_edit=1, max_hits=10 ** 6)
            assert sum(s.check(strata, hits, 1)) > 20
            if name == "dup32":                                                    # two sequences 40 000 times over: one hit with count 40 000 per duplicate
                assert (hits["cnt"] % 40000 == 0).all() and int(hits["cnt"].min()) == 40000
            if want is not None:
                assert np.array_equal(strata, want[0]) and np.array_equal(hits, want[1])
            want = (strata, hits)
        finally:
            d.close()


def test_nothing_to_do_and_bad_arguments(gpu, gold, main):
    d = main.d
    L = gpu.lib()
    strata, hits, st = d.edit_search([], max_edit=2, with_stat=True)
    assert strata.shape == (0, 3, 2) and len(hits) == 0 and not any(st.values())
    # only queries that are skipped: empty, and longer than FMD_ESEARCH_MAX_LEN
    exact = main.reads[50][:30].copy()                                            # a piece of a read as it is: it occurs
    long_q = np.tile(exact, api.ESEARCH_MAX_LEN // len(exact) + 1)
    strata, hits, st = d.edit_search([np.zeros(0, np.uint8), long_q, long_q[:api.ESEARCH_MAX_LEN], exact], max_edit=1, with_stat=True)
    assert st["n_skipped"] == 2 and not strata[:3].any() and strata[3, 0, 0] == 1 and set(hits["query"].tolist()) == {3}
    mem = DevMem(gpu)
    try:
        flat, off = api.flatten_reads(main.qs[:10])
        wb = L.fmd_esearch_work_bytes(10, api.ESEARCH_MIN_CAP)
        d_seqs, d_off, d_strata, d_stat, d_work = mem.put(flat), mem.put(off), mem.alloc(10 * 3 * 16), mem.alloc(64), mem.alloc(wb + 16)
        call = lambda work, nbytes, max_edit=2, n=10: L.fmd_esearch_dev(d.h, None, n, d_seqs, d_off, None, max_edit, 10, 5, None, 0, d_strata, d_stat, work, nbytes)
        assert call(d_work, wb) == api.FMD_OK
        assert call(d_work, wb - 64) == api.FMD_E_ARG                               # too small for the smallest capacity
        assert call(C.c_void_p(d_work.value + 8), wb) == api.FMD_E_ARG              # misaligned
        assert call(d_work, wb, max_edit=5) == api.FMD_E_ARG and call(d_work, wb, max_edit=-1) == api.FMD_E_ARG
        assert call(None, wb) == api.FMD_E_ARG and call(d_work, wb, n=2 ** 32) == api.FMD_E_ARG
        assert call(None, 0, n=0) == api.FMD_OK                                     # n = 0 is a no-op
        d.sync()
        st = np.zeros(1, dtype=api.ESEARCH_STAT_DT)
        s2 = np.zeros(10 * 3 * 2, dtype=np.uint64)
        batch = lambda max_edit, cap, flags=0: L.fmd_esearch_batch(d.h, 10, flat.ctypes.data, off.ctypes.data, max_edit, 10, flags, cap, None, None, s2.ctypes.data, st.ctypes.data)
        assert batch(2, 0) == api.FMD_OK and s2.any()
        assert batch(5, 0) == api.FMD_E_ARG and batch(2, api.ESEARCH_MIN_CAP - 1) == api.FMD_E_ARG and batch(2, api.ESEARCH_MAX_CAP + 1) == api.FMD_E_ARG and batch(2, 0, flags=8) == api.FMD_E_ARG
    finally:
        mem.free()
    with pytest.raises(api.FmdError):
        d.edit_search(main.qs[:3], max_edit=5)


# ---- 11. the command -------------------------------------------------------------------------------------------------------------------------------------------------------------
def cigar_cost(cigar, q, p):
    """walks query and pattern (nt6 lists) along the CIGAR: '=' equal bases, 'X' unequal, 'I' a query base alone, 'D' a pattern base alone -> the operations that
    are not '='; AssertionError unless it turns exactly this query into exactly this pattern"""
    assert re.fullmatch(r"(\d+[=XID])+", cigar), cigar
    i = j = cost = 0
    for n, op in re.findall(r"(\d+)([=XID])", cigar):
        for _ in range(int(n)):
            if op in "=X":
                assert (q[i] == p[j] and 1 <= p[j] <= 4) == (op == "="), (cigar, i, j)
                i, j = i + 1, j + 1
            elif op == "I":
                i += 1
            else:
                j += 1
            cost += op != "="
    assert i == len(q) and j == len(p), cigar
    return cost


def test_cli(gpu, gold, tmp_path):
    _, reads = fastq_names_reads("ctA")
    strands = strands_of(reads, trim=True)
    rng = np.random.default_rng(12)
    qs = make_queries(strands, rng, 20, 2, 2, rng.integers(12, 46, size=22))
    names = ["q%d" % i for i in range(len(qs))]
    fa = tmp_path / "q.fa"
    fa.write_text("".join(">%s\n%s\n" % (nm, "".join("$ACGTN"[c] for c in q)) for nm, q in zip(names, qs)))
    fmd, rank = gold.path("ctA.fmd"), gold.path("ctA.rank")
    d = gpu.DevIndex.open(fmd)
    try:
        strata, hits = d.edit_search(qs, max_edit=2, max_hits=1000)
        assert sum(Set(d, Brute(strands), qs, dmax=2).check(strata, hits, 2)) > 30
        pats = ["".join("$ACGTN"[c] for c in p) for p in d.edit_patterns(hits)]
        few = d.edit_search(qs, max_edit=2, max_hits=1, best=True)
    finally:
        d.close()

    def parse(out):
        """-> per query (the SQ fields, [(n_edit, pattern, count, cigar)], the OC lines per EH)"""
        recs = []
        for ln in out.decode().splitlines():
            f = ln.split("\t")
            if f[0] == "SQ":
                recs.append((f[1:], [], []))
            elif f[0] == "EH":
                recs[-1][1].append((int(f[1]), f[2], int(f[3]), f[4])); recs[-1][2].append([])
            elif f[0] == "OC":
                recs[-1][2][-1].append(ln)
            else:
                assert ln == "//"
        return recs

    def expect_sq(strata, max_hits):
        return [[names[i], str(len(q)), str(int(strata[i, :, 0].sum())), str(int(strata[i, :, 1].sum())), str(int(strata[i, :, 0].sum() <= max_hits)),
                 ",".join(str(int(v)) for v in strata[i, :, 0])] for i, q in enumerate(qs)]

    run = lambda args: subprocess.run([AMD, "esearch"] + args + [fmd, str(fa)], capture_output=True, timeout=120)
    p = run(["-e", "2", "-l", "-r", rank])
    assert p.returncode == 0, p.stderr
    recs = parse(p.stdout)
    assert [r[0] for r in recs] == expect_sq(strata, 1000)
    cut = np.searchsorted(hits["query"], np.arange(len(qs) + 1))
    n_edits = 0
    for i, (_, ehs, _) in enumerate(recs):                                         # patterns, distances and counts: those of edit_search, in its order
        got = hits[cut[i]:cut[i + 1]]
        assert [(e, pt, c) for e, pt, c, _ in ehs] == [(int(h["n_edit"]), pats[cut[i] + j], int(h["cnt"])) for j, h in enumerate(got)]
        for e, pt, _, cigar in ehs:                                                # every CIGAR turns the query into the pattern with exactly n_edit operations that are not '='
            assert cigar_cost(cigar, qs[i].tolist(), ["$ACGTN".index(ch) for ch in pt]) == e
            n_edits += e
    assert n_edits > 30
    # the OC lines behind every EH: what `locate` prints for that pattern
    pf = tmp_path / "p.fa"
    pf.write_text("".join(">p%d\n%s\n" % (j, s) for j, s in enumerate(pats)))
    loc = subprocess.run([AMD, "locate", "-m", "1000", "-r", rank, fmd, str(pf)], capture_output=True, timeout=120)
    assert loc.returncode == 0, loc.stderr
    want_oc = [[ln for ln in blk.splitlines() if ln.startswith("OC")] for blk in loc.stdout.decode().split("//\n")[:-1]]
    got_oc = [oc for r in recs for oc in r[2]]
    assert len(pats) == len(hits) == len(got_oc) and got_oc == want_oc and sum(map(len, got_oc)) >= int(hits["cnt"][hits["cnt"] <= 1000].sum()) > 100
    # without -l no OC line; -b and -m as the flags of the library
    p = run(["-e", "2", "-b", "-m", "1"])
    assert p.returncode == 0 and b"\nOC\t" not in p.stdout
    assert [r[0] for r in parse(p.stdout)] == expect_sq(few[0], 1) and sum(len(r[1]) for r in parse(p.stdout)) == len(few[1]) >= 5   # (the five queries cut from the reads as they are have one hit at distance 0)
