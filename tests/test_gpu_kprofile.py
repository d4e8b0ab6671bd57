"""GPU: kprofile (fmd_kprofile_dev / fmd_kprofile_batch, DevIndex.kmer_profile, `fermi-amd kprofile`) against brute force over the forward sequences as
indexed, independent of any index code: for k <= 32 the canonical form of every N-free k-window, counted with numpy (what tests/test_gpu_kcount.py
does, restated here); for k > 32 a Python dict over the byte strings of the windows of every sequence and its reverse complement, a hit on a window
that is its own reverse complement halved.  Every window of every query is compared exactly, on every path the library has."""
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
GUARD32 = 0x5A5A5A5A
# every path the library has: its own choice and the plain path.  (A shared path -- groups of consecutive windows searching their common bases once --
# was a third entry here while it was measured; it lost and left the library)
FLAGS = [0, api.KPROFILE_PLAIN]
FLAG_IDS = ["default", "plain"]


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


def windows_packed(r, k):
    """(canonical packed k-mer, N-free?, own reverse complement?) of every k-window of r, k <= 32"""
    sh = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    base = (r.astype(np.uint64) - np.uint64(1)) & np.uint64(3)
    w = np.lib.stride_tricks.sliding_window_view(base, k)
    good = np.lib.stride_tricks.sliding_window_view((r >= 1) & (r <= 4), k).all(axis=1)
    fw = np.bitwise_or.reduce(w << sh, axis=1)
    rc = np.bitwise_or.reduce((np.uint64(3) - w[:, ::-1]) << sh, axis=1)
    return np.minimum(fw, rc), good, (fw == rc) & good


class Want:
    """brute force for one read set, per k computed once and never changed"""

    def __init__(self, seqs):
        self.seqs, self.by_k = seqs, {}

    def table(self, k):
        """identical sequences are walked once and weighed by how often they occur (dup32 is one read 40 000 times)"""
        if k not in self.by_k:
            uniq, mult = np.unique(np.array([s.tobytes() for s in self.seqs] + [b""], dtype=object), return_counts=True)
            if k <= 32:
                parts, wts = [np.zeros(0, dtype=np.uint64)], [np.zeros(0, dtype=np.float64)]
                for b, n in zip(uniq, mult):
                    if len(b) >= k:
                        c, good, _ = windows_packed(np.frombuffer(b, dtype=np.uint8), k)
                        parts.append(c[good]); wts.append(np.full(int(good.sum()), float(n)))
                km, inv = np.unique(np.concatenate(parts), return_inverse=True)
                self.by_k[k] = (km, np.bincount(inv.reshape(-1), weights=np.concatenate(wts), minlength=len(km)).astype(np.int64))
            else:
                d = {}
                for b, n in zip(uniq, mult):
                    r = np.frombuffer(b, dtype=np.uint8)
                    for s in (b, revcomp(r).tobytes()):
                        for j in range(len(s) - k + 1):
                            w = s[j:j + k]
                            d[w] = d.get(w, 0) + int(n)
                self.by_k[k] = d
        return self.by_k[k]

    def profile(self, queries, k):
        """(counts, woff, N-free, own reverse complement) of every window of every query, as fmd_kprofile defines them"""
        tab = self.table(k)
        woff = np.zeros(len(queries) + 1, dtype=np.uint64)
        cs, gs, ps = [np.zeros(0, np.uint32)], [np.zeros(0, bool)], [np.zeros(0, bool)]
        for i, q in enumerate(queries):
            q = np.asarray(q, dtype=np.uint8)
            nw = max(0, len(q) - k + 1)
            woff[i + 1] = woff[i] + np.uint64(nw)
            if nw == 0:
                continue
            if k <= 32:
                km, ct = tab
                c, good, pal = windows_packed(q, k)
                at = np.minimum(np.searchsorted(km, c), max(len(km) - 1, 0))
                cnt = np.where(good & (km[at] == c), ct[at], 0) if len(km) else np.zeros(nw, np.int64)
            else:
                b, rb = q.tobytes(), revcomp(q).tobytes()
                good = np.lib.stride_tricks.sliding_window_view((q >= 1) & (q <= 4), k).all(axis=1)
                pal = np.array([good[j] and b[j:j + k] == rb[len(b) - j - k:len(b) - j] for j in range(nw)], dtype=bool)
                cnt = np.array([(tab.get(b[j:j + k], 0) >> int(pal[j])) if good[j] else 0 for j in range(nw)], dtype=np.int64)
            cs.append(np.minimum(cnt, 2 ** 32 - 1).astype(np.uint32)); gs.append(good); ps.append(pal)
        return np.concatenate(cs), woff, np.concatenate(gs), np.concatenate(ps)


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


def table_depth(d, asked):
    """the depth of the handle's prefix table for FMD_PTAB_DEPTH = asked: as asked, but no deeper than the index has symbols for (fmd_index.hip)"""
    depth = min(asked, 15)
    while depth > 2 and 4 ** depth > int(d.mcnt[0]):
        depth -= 1
    return depth


def check(d, w, queries, k, flags, depth, all_hit=False):
    """one profile of `queries` against brute force, every window, and the statistics; depth = the handle's table depth (0: none) -> (counts, woff, stat)"""
    cnt, woff, good, pal = w.profile(queries, k)
    got, gwoff, st = d.kmer_profile(queries, k, flags=flags, with_stat=True)
    assert got.dtype == np.uint32 and gwoff.dtype == np.uint64 and np.array_equal(gwoff, woff)
    assert np.array_equal(got, cnt), (k, flags, np.flatnonzero(got != cnt)[:8])
    assert st["n_windows"] == len(cnt) and st["n_valid"] == int(good.sum()) and st["n_hit"] == int((cnt > 0).sum())
    if all_hit:
        assert good.all() and (cnt > 0).all()
    from_table = depth > 0 and k >= depth
    assert st["n_table"] == (st["n_valid"] if from_table else 0)
    assert st["n_ext"] <= st["n_valid"] * max(0, k - (depth if from_table else 1))
    if all_hit:
        assert st["n_ext"] == st["n_valid"] * max(0, k - (depth if from_table else 1))   # nobody stops early
    return got, woff, st


def open_tiny(gpu, monkeypatch, cfg):
    """tiny with a prefix table of depth 4 or 8, or without tables -> (handle, its table depth)"""
    fn = os.path.join(GOLD, "tiny.fmd")
    if cfg == "bare":
        return gpu.DevIndex.open_bare(fn), 0
    monkeypatch.setenv("FMD_PTAB_DEPTH", str(cfg))
    d = gpu.DevIndex.open(fn)
    return d, table_depth(d, cfg)


# ---- 1. the k sweep -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("cfg", [4, 8, "bare"])
def test_k_sweep_on_tiny(gpu, want, monkeypatch, cfg, flags):
    w = want["tiny"]
    queries = w.seqs[:200]
    assert all(len(q) == 100 for q in queries)
    d, depth = open_tiny(gpu, monkeypatch, cfg)
    try:
        assert depth == (0 if cfg == "bare" else cfg)
        ks = sorted(set(k for k in (1, 2, depth - 1, depth, depth + 1, depth + 2, 21, 31, 32, 33, 55, 100, 101) if k >= 1))
        for k in ks:
            got, woff, st = check(d, w, queries, k, flags, depth, all_hit=k <= 100)   # the queries are indexed reads without an N: every window occurs
            assert len(got) == 200 * (101 - k)
        # k = 101: no window at all -- woff is written, all zero, and there is no array
        flat, off = api.flatten_reads(queries)
        woff = np.full(201, 7, dtype=np.uint64)
        p = C.c_void_p(1)
        stat = np.zeros(1, dtype=api.KPROFILE_STAT_DT)
        assert gpu.lib().fmd_kprofile_batch(d.h, 200, flat.ctypes.data, off.ctypes.data, 101, flags, woff.ctypes.data, C.byref(p), stat.ctypes.data) == 0
        assert p.value is None and not woff.any()
        woff[:] = 7
        assert gpu.lib().fmd_kprofile_batch(d.h, 0, None, None, 21, flags, woff.ctypes.data, C.byref(p), stat.ctypes.data) == 0 and woff[0] == 0 and p.value is None
    finally:
        d.close()


# ---- 2. misses at every depth -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_misses_at_every_depth(gpu, want, monkeypatch, flags):
    """one stretch of 2k bases, once per position with a substitution there and once with an N there: the windows over the position turn into misses
    in every step of the walk; with the N they are 0 without a search"""
    w = want["tiny"]
    k = 21
    stretch = w.seqs[3][30:30 + 2 * k].copy()
    subs, ns = [], []
    for p in range(2 * k):
        s = stretch.copy(); s[p] = s[p] % 4 + 1; subs.append(s)
        s = stretch.copy(); s[p] = 5; ns.append(s)
    d, depth = open_tiny(gpu, monkeypatch, 8)
    try:
        got, woff, st = check(d, w, subs + ns, k, flags, depth)
        nw = k + 1
        clean, _, _, _ = w.profile([stretch], k)
        assert (clean > 0).all()
        n_missed = 0
        for p in range(2 * k):
            over = np.array([j <= p < j + k for j in range(nw)])
            a = got[(2 * k + p) * nw:(2 * k + p + 1) * nw]                          # with the N: 0 over p, the stretch's own counts elsewhere
            assert not a[over].any() and np.array_equal(a[~over], clean[~over])
            b = got[p * nw:(p + 1) * nw]                                           # with the substitution: the same elsewhere
            assert np.array_equal(b[~over], clean[~over])
            n_missed += int((b[over] == 0).sum())
        assert n_missed > k * (k + 1) // 2                                         # (of the k (k + 1) substituted windows most occur nowhere)
        assert st["n_valid"] == 2 * k * nw + sum(nw - sum(1 for j in range(nw) if j <= p < j + k) for p in range(2 * k))
    finally:
        d.close()


# ---- 3. seams: the _dev form on buffers of exactly the stated sizes -----------------------------------------------------------------------------
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


def profile_dev(gpu, d, mem, queries, k, flags):
    """fmd_kprofile_dev with a caller-made woff; the count array is followed by poisoned guard words that must come back untouched -> (counts, woff, stat)"""
    flat, off = api.flatten_reads(queries)
    woff = np.zeros(len(queries) + 1, dtype=np.uint64)
    np.cumsum([max(0, len(q) - k + 1) for q in queries], out=woff[1:])
    W = int(woff[-1])
    count = np.full(W + 4, GUARD32, dtype=np.uint32)
    d_count, d_stat = mem.put(count), mem.put(np.zeros(1, dtype=api.KPROFILE_STAT_DT))
    gpu.check(gpu.lib().fmd_kprofile_dev(d.h, None, len(queries), mem.put(flat), mem.put(off), mem.put(woff), k, flags, d_count, d_stat))
    d.sync()
    mem.get(d_count, count)
    assert (count[W:] == GUARD32).all()
    stat = mem.get(d_stat, np.zeros(1, dtype=api.KPROFILE_STAT_DT))[0]
    return count[:W], woff, {f: int(stat[f]) for f in api.KPROFILE_STAT_DT.names}


def seam_queries(w, k):
    """lengths k - 1 .. k + 17 (many sequences in one wave, their bases at every alignment) with an empty sequence in the middle and at the end,
    and one sequence of 5000 bases (many waves, many chunk starts)"""
    text = np.concatenate(w.seqs[:60])
    qs, at = [], 0
    for ln in range(k - 1, k + 2 * 8 + 2):
        qs.append(text[at:at + ln].copy()); at += ln + 3
        if ln == k + 8:
            qs.append(np.zeros(0, dtype=np.uint8))
    qs.append(text[at:at + 5000].copy())
    qs.append(np.zeros(0, dtype=np.uint8))
    return qs


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_seams(gpu, want, flags):
    w = want["tiny"]
    k = 21
    d = gpu.DevIndex.open(os.path.join(GOLD, "tiny.fmd"))
    mem = DevMem(gpu)
    try:
        text = np.concatenate(w.seqs[100:110])
        sets = [seam_queries(w, k)]
        for n_win in (1, 63, 64, 65):                                              # one sequence, and the same windows over sequences of 1 .. 3 windows
            sets.append([text[:k - 1 + n_win].copy()])
            lens, left = [], n_win
            while left:
                lens.append(min(left, 1 + len(lens) % 3)); left -= lens[-1]
            sets.append([text[7 * j:7 * j + k - 1 + ln].copy() for j, ln in enumerate(lens)])
        sets.append([q for q in seam_queries(w, k) if len(q) < 5000] * 3)           # a total that is no multiple of 64
        for qs in sets:
            cnt, woff, good, pal = w.profile(qs, k)
            got, gwoff, st = profile_dev(gpu, d, mem, qs, k, flags)
            assert np.array_equal(gwoff, woff) and np.array_equal(got, cnt), (len(qs), np.flatnonzero(got != cnt)[:8])
            assert st["n_windows"] == len(cnt) and st["n_valid"] == int(good.sum()) and st["n_hit"] == int((cnt > 0).sum())
            got2, woff2 = d.kmer_profile(qs, k, flags=flags)                        # the _batch form gives the same
            assert np.array_equal(got2, got) and np.array_equal(woff2, woff)
        assert int(w.profile(sets[-1], k)[1][-1]) % 64 != 0 and len(w.profile(sets[0], k)[0]) > 4980
    finally:
        mem.free()
        d.close()


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_large_k_many_short_sequences(gpu, want, flags):
    """sequences of one or two windows at a large k: the bases of a wave's 64 windows do not fit its LDS together, and the wave takes them in passes"""
    w = want["tiny"]
    k = 97
    qs = [w.seqs[j][j % 3:j % 3 + k + j % 2].copy() for j in range(150)]
    d = gpu.DevIndex.open(os.path.join(GOLD, "tiny.fmd"))
    try:
        got, woff, st = check(d, w, qs, k, flags, depth_of_default(d), all_hit=True)
        assert len(got) == sum(1 + j % 2 for j in range(150))
        text = np.concatenate(w.seqs[30:38])                                       # the largest k: no read is that long, so nothing occurs -- and nothing is read past a sequence
        for kk in (api.KPROFILE_MAX_K - 1, api.KPROFILE_MAX_K):
            got, woff, st = check(d, w, [text[:700].copy(), text[100:100 + kk].copy(), text[5:5 + kk - 1].copy(), text[3:3 + kk + 70].copy()], kk, flags, depth_of_default(d))
            assert len(got) == 700 - kk + 1 + 1 + 71 and not got.any() and st["n_valid"] == len(got)
    finally:
        d.close()


def depth_of_default(d):
    """the depth fmd_dev_open_file gives the prefix table without FMD_PTAB_DEPTH: as deep as keeps 4^depth <= n / 8, between 2 and 14 (fmd_index.hip)"""
    depth = 2
    while depth < 14 and 4 ** (depth + 1) <= int(d.mcnt[0]) // 8:
        depth += 1
    return depth


# ---- 4. palindromes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("k", [20, 32, 21])
def test_palindromes(gpu, want, k, flags):
    """even k: the windows of the indexed reads that are their own reverse complement count half their interval; odd k: there is none"""
    w = want["palin"]
    d = gpu.DevIndex.open(os.path.join(GOLD, "palin.fmd"))
    try:
        cnt, woff, good, pal = w.profile(w.seqs, k)
        assert (int(pal.sum()) > 0) == (k % 2 == 0)
        got, _, _ = check(d, w, w.seqs, k, flags, depth_of_default(d))
        assert np.array_equal(got[pal], cnt[pal]) and (cnt[pal] > 0).all()
    finally:
        d.close()


# ---- 5. large counts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("k", [21, 55])
def test_dup32_large_counts(gpu, want, k, flags):
    w = want["dup32"]
    uniq, n_of = np.unique(np.array([s.tobytes() for s in w.seqs], dtype=object), return_counts=True)
    dup = np.frombuffer(uniq[int(np.argmax(n_of))], dtype=np.uint8)
    assert int(n_of.max()) >= 10000 and len(dup) >= k
    d = gpu.DevIndex.open(os.path.join(GOLD, "dup32.fmd"))
    try:
        got, _, _ = check(d, w, [dup, w.seqs[0], w.seqs[-1]], k, flags, depth_of_default(d))
        assert int(got.max()) >= 10000
    finally:
        d.close()


# ---- 6. agreement with kcount -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_agrees_with_kcount_on_repeat(gpu, want, flags):
    w = want["repeat"]
    k = 21
    d = gpu.DevIndex.open(os.path.join(GOLD, "repeat.fmd"))
    try:
        got, woff = d.kmer_profile(w.seqs, k, flags=flags)
        canon, good = [], []
        for r in w.seqs:
            if len(r) >= k:
                c, g, _ = windows_packed(r, k)
                canon.append(c); good.append(g)
        canon, good = np.concatenate(canon), np.concatenate(good)
        assert len(canon) == len(got) and not got[~good].any()
        pairs = np.unique(np.stack([canon[good], got[good].astype(np.uint64)], axis=1), axis=0)
        km, ct, _ = d.kmer_counts(k, 1)
        assert np.array_equal(pairs[:, 0], km) and np.array_equal(pairs[:, 1], ct.astype(np.uint64))   # every k-mer with ONE count, and kcount's
    finally:
        d.close()


# ---- 7. special: N in indexed reads, short reads ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("k", [6, 20])
def test_special(gpu, want, k, flags):
    """queries with N, shorter than k, and palindromes; an N of a query never matches an N of a read"""
    w = want["special"]
    assert any((r == 5).any() for r in w.seqs) and (k < 20 or any(len(r) < k for r in w.seqs))   # (the shortest read has 8 bases)
    d = gpu.DevIndex.open(os.path.join(GOLD, "special.fmd"))
    try:
        check(d, w, w.seqs, k, flags, depth_of_default(d))
    finally:
        d.close()


# ---- 8. arguments, one strand, an empty index ---------------------------------------------------------------------------------------------------
def test_arguments(gpu, want):
    L = gpu.lib()
    w = want["tiny"]
    qs = w.seqs[:4]
    flat, off = api.flatten_reads(qs)
    d = gpu.DevIndex.open(os.path.join(GOLD, "tiny.fmd"))
    mem = DevMem(gpu)
    try:
        woff = np.zeros(5, dtype=np.uint64)
        np.cumsum([len(q) - 20 for q in qs], out=woff[1:])
        ok = dict(h=d.h, n=4, seqs=mem.put(flat), off=mem.put(off), woff=mem.put(woff), k=21, flags=0, count=mem.put(np.zeros(int(woff[-1]), np.uint32)))

        def call(**kw):
            a = dict(ok, **kw)
            return L.fmd_kprofile_dev(a["h"], None, a["n"], a["seqs"], a["off"], a["woff"], a["k"], a["flags"], a["count"], None)
        assert call() == 0                                                         # (without a stat)
        d.sync()
        for kw in (dict(k=0), dict(k=-1), dict(k=api.KPROFILE_MAX_K + 1), dict(flags=2), dict(flags=3), dict(flags=4), dict(flags=16), dict(flags=1 << 31),   # (2: the flag of the shared path that is not there)
                   dict(h=None), dict(seqs=None), dict(off=None), dict(woff=None), dict(count=None), dict(n=2 ** 32)):
            assert call(**kw) == api.FMD_E_ARG, kw
        assert call(n=0, seqs=None, off=None, woff=None, count=None) == 0          # nothing to do
        assert len(d.kmer_profile(qs, api.KPROFILE_MAX_K)[0]) == 0                 # the largest k: no sequence here is that long
        for kw in (dict(k=0), dict(k=api.KPROFILE_MAX_K + 1), dict(flags=3), dict(flags=16)):
            with pytest.raises(api.FmdError, match=r"\(-2\)"):
                d.kmer_profile(qs, **dict(dict(k=21, flags=0), **kw))
    finally:
        mem.free()
        d.close()


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_one_strand_index_is_refused_and_an_empty_one_counts_nothing(gpu, want, flags):
    reads = [np.array([1, 1, 1, 2, 1, 3, 1, 1, 2, 1], dtype=np.uint8), np.array([2, 2, 1, 2, 2, 3, 2, 1], dtype=np.uint8)]   # many A and C, no T
    d = gpu.DevIndex.from_bwt(gpu.build_bwt_strands(reads, strands=api.STRAND_FWD))
    mem = DevMem(gpu)
    try:
        with pytest.raises(api.FmdError, match=r"\(-2\)"):
            d.kmer_profile(reads, 5, flags=flags)
        flat, off = api.flatten_reads(reads)
        woff = np.array([0, 6, 10], dtype=np.uint64)
        assert gpu.lib().fmd_kprofile_dev(d.h, None, 2, mem.put(flat), mem.put(off), mem.put(woff), 5, flags, mem.put(np.zeros(10, np.uint32)), None) == api.FMD_E_ARG
    finally:
        mem.free()
        d.close()
    d = gpu.DevIndex.open(os.path.join(GOLD, "sub.empty.fmd"), empty_ok=True)
    try:
        qs = want["tiny"].seqs[:5] + [np.array([1, 5, 2], dtype=np.uint8)]
        for k in (1, 21):
            got, woff, st = d.kmer_profile(qs, k, flags=flags, with_stat=True)
            assert len(got) == sum(max(0, len(q) - k + 1) for q in qs) and not got.any()
            assert st["n_windows"] == len(got) and st["n_hit"] == 0 and st["n_ext"] == 0
    finally:
        d.close()


# ---- 9. the command -----------------------------------------------------------------------------------------------------------------------------
def test_cli(gpu, want, tmp_path):
    w = want["tiny"]
    k = 21
    qs = [w.seqs[j].copy() for j in range(12)] + [want["special"].seqs[j].copy() for j in range(6)]
    qs[2][40] = 5                                                                  # an N
    qs[5] = qs[5][:k - 1]                                                          # no window
    qs[7] = qs[7][:k]                                                              # one
    qs.append(np.concatenate(w.seqs[20:24]))
    text = ["".join("?ACGTN"[c] for c in q) for q in qs]
    fa = tmp_path / "q.fa"
    fa.write_text("".join(">q%d\n%s\n" % (i, s) for i, s in enumerate(text)))
    lower = tmp_path / "lower.fa"
    lower.write_text("".join(">q%d\n%s\n" % (i, s.lower()) for i, s in enumerate(text)))
    fmds = [os.path.join(GOLD, "tiny.fmd"), os.path.join(GOLD, "special.fmd")]
    idx = [gpu.DevIndex.open(f) for f in fmds]
    try:
        prof = [d.kmer_profile(qs, k) for d in idx]
        exp, exp_s = [], []
        for i, q in enumerate(qs):
            nw = max(0, len(q) - k + 1)
            head = "SQ\tq%d\t%d\t%d\n" % (i, len(q), nw)
            exp.append(head); exp_s.append(head)
            for j, (cnt, woff) in enumerate(prof):
                c = cnt[int(woff[i]):int(woff[i + 1])]
                exp.append("KP\t%d\t%s\n" % (j, ",".join(str(int(v)) for v in c) if nw else "*"))
                good = np.lib.stride_tricks.sliding_window_view((q >= 1) & (q <= 4), k).all(axis=1) if nw else np.zeros(0, bool)
                v = np.sort(c[good])
                exp_s.append("KS\t%d\t%d\t%d\t" % (j, len(v), int((v == 0).sum())) +
                             ("%d\t%d\t%d\t%.3f\n" % (v[0], v[(len(v) - 1) // 2], v[-1], float(v.astype(np.float64).sum()) / len(v)) if len(v) else "*\t*\t*\t*\n"))
            exp.append("//\n"); exp_s.append("//\n")
        a = subprocess.run([AMD, "kprofile", "-k", str(k), str(fa)] + fmds, capture_output=True, timeout=120)
        assert a.returncode == 0, a.stderr
        assert a.stdout.decode() == "".join(exp)
        assert "KP\t0\t" in a.stdout.decode() and "KP\t1\t" in a.stdout.decode()
        b = subprocess.run([AMD, "kprofile", "-k", str(k), str(lower)] + fmds, capture_output=True, timeout=120)
        assert b.returncode == 0 and b.stdout == a.stdout                         # lower case counts as upper case
        s = subprocess.run([AMD, "kprofile", "-k", str(k), "-s", str(fa)] + fmds, capture_output=True, timeout=120)
        assert s.returncode == 0 and s.stdout.decode() == "".join(exp_s)
        # a batch of queries ends wherever the next sequence would take it past its size: the same lines from batches of 150 bases (a sequence of 400 is its own)
        handles = [d.h for d in idx]
        assert hostlib.kprofile_run(str(fa), handles, k) == a.stdout.decode()
        assert hostlib.kprofile_run(str(fa), handles, k, batch_bases=150) == a.stdout.decode()
        assert hostlib.kprofile_run(str(fa), handles, k, "s", batch_bases=1) == s.stdout.decode()
        # -q: FASTQ whose quality line carries the counts, as cnt2qual reads it
        q = subprocess.run([AMD, "kprofile", "-k", str(k), "-q", str(lower), fmds[0]], capture_output=True, timeout=120)
        assert q.returncode == 0, q.stderr
        cnt, woff = prof[0]
        want_fq = "".join("@q%d\n%s\n+\n%s\n" % (i, text[i].lower(), hostlib.kprofile_qual_text(len(qs[i]), k, cnt[int(woff[i]):int(woff[i + 1])])) for i in range(len(qs)))
        assert q.stdout.decode() == want_fq
        assert hostlib.kprofile_run(str(lower), handles[:1], k, "q", batch_bases=150) == want_fq
        fq = tmp_path / "counts.fq"
        fq.write_bytes(q.stdout)
        c2q = subprocess.run([AMD, "cnt2qual", str(fq), "2"], capture_output=True, timeout=60)
        assert c2q.returncode == 0
        recs = c2q.stdout.decode().split("\n")
        assert [recs[4 * i + 1] for i in range(len(qs))] == [t.lower() for t in text] and all(len(recs[4 * i + 3]) == len(text[i]) for i in range(len(qs)))
    finally:
        for d in idx:
            d.close()
