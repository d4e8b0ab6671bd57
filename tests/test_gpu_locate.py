"""GPU: locate (fmd_locate_dev / fmd_locate_batch, DevIndex.locate_rows / locate, `fermi-amd locate`) -- against brute force over the reads, and against
`retrieve` of every row of the same intervals, the independent row-by-row walk."""
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
U32_MAX = 2 ** 32 - 1


# ---- the reads as indexed, and brute force over them ------------------------------------------------------------------------------------
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
    """every sequence after the other with a 0 between them: one bytes.find walk per query finds its occurrences in all of them"""

    def __init__(self, strands):
        self.start = np.zeros(len(strands) + 1, dtype=np.int64)
        np.cumsum([len(s) + 1 for s in strands], out=self.start[1:])
        self.text = b"\0".join(s.tobytes() for s in strands) + b"\0"

    def hits(self, q):
        """sorted (id, offset) of every occurrence of q"""
        q = np.asarray(q, dtype=np.uint8).tobytes()
        ats, at = [], self.text.find(q)
        while at >= 0:
            ats.append(at)
            at = self.text.find(q, at + 1)
        ats = np.array(ats, dtype=np.int64)
        i = np.searchsorted(self.start, ats, side="right") - 1
        return sorted(zip(i.tolist(), (ats - self.start[i]).tolist()))


def queries(reads, n, seed, max_len=60):
    """substrings of reads, 1 .. max_len bases, 40 % with one base changed"""
    rng = np.random.default_rng(seed)
    qs = []
    for _ in range(n):
        r = reads[int(rng.integers(len(reads)))]
        ln = int(rng.integers(1, min(max_len, len(r)) + 1)); at = int(rng.integers(0, len(r) - ln + 1))
        q = np.array(r[at:at + ln], dtype=np.uint8)
        if rng.random() < 0.4:
            p = int(rng.integers(ln))
            q[p] = 1 + (int(q[p]) + int(rng.integers(0, 3))) % 4 if 1 <= q[p] <= 4 else int(rng.integers(1, 5))
        qs.append(q)
    return qs


def hits_of(res, i):
    cnt, located, hit_off, hit_id, hit_pos = res
    return list(zip(hit_id[hit_off[i]:hit_off[i + 1]].tolist(), hit_pos[hit_off[i]:hit_off[i + 1]].tolist()))


def expand(runs):
    """runs -> sorted (query, rank, offset) of every row"""
    out = []
    for r in runs:
        out += [(int(r["query"]), int(r["rank"]) + j, int(r["off"])) for j in range(int(r["n"]))]
    return sorted(out)


def row_by_row(d, beg, cnt, keep=None):
    """the yardstick: fm_retrieve of every row of the intervals -> sorted (query, rank, len)"""
    qi = [i for i in range(len(cnt)) if cnt[i] and (keep is None or keep[i])]
    rows = np.concatenate([np.arange(int(beg[i]), int(beg[i]) + int(cnt[i]), dtype=np.uint64) for i in qi] + [np.zeros(0, dtype=np.uint64)])
    q = np.concatenate([np.full(int(cnt[i]), i, dtype=np.int64) for i in qi] + [np.zeros(0, dtype=np.int64)])
    _, ln, rank = d.retrieve(rows, stride=1)
    return sorted(zip(q.tolist(), rank.astype(np.int64).tolist(), ln.astype(np.int64).tolist()))


@pytest.fixture(scope="module")
def golden_sets(gpu):
    """per golden read set: names, reads, sequences as indexed, the 400 queries and what brute force finds for each -- computed once"""
    sets = {}
    for name, seed in (("ctA", 101), ("cnA", 102)):
        names, reads = fastq_names_reads(name)
        strands = strands_of(reads, trim=True)
        qs = queries(strands, 400, seed)
        b = Brute(strands)
        sets[name] = dict(names=names, reads=reads, strands=strands, qs=qs, want=[b.hits(q) for q in qs],
                          rank=np.fromfile(os.path.join(GOLD, name + ".rank"), dtype=np.uint64))
    return sets


# ---- 1. brute force ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ctA", "cnA"])
def test_locate_equals_brute_force(gpu, golden_sets, name):
    """400 substrings of reads, 40 % with one base changed: the (sequence id, offset) pairs DevIndex.locate lists -- ids through the golden .rank map -- are
    those bytes.find finds over every read and its reverse complement"""
    s = golden_sets[name]
    d = gpu.DevIndex.open(os.path.join(GOLD, name + ".fmd"))
    try:
        cnt = d.backward_search(s["qs"])[0]
        res = d.locate(s["qs"], max_occ=int(cnt.max()) + 1, sorted_map=s["rank"])
        assert np.array_equal(res[0], cnt) and res[1][cnt > 0].all() and res[1].all()
        assert (cnt > 0).sum() > 200 and (cnt == 0).sum() > 20 and cnt.max() > 60
        for i, q in enumerate(s["qs"]):
            assert int(cnt[i]) == len(s["want"][i]), (i, q)
            assert hits_of(res, i) == s["want"][i], (i, q)
    finally:
        d.close()


# ---- 2. row by row ----------------------------------------------------------------------------------------------------------------------------
def check_rows(d, qs, max_occ=None):
    cnt, beg, _ = d.backward_search(qs)
    m = int(cnt.max()) + 1 if max_occ is None else max_occ
    runs, st = d.locate_rows(beg, cnt, max_occ=m)
    keep = cnt <= np.uint64(m)
    assert expand(runs) == row_by_row(d, beg, cnt, keep)
    assert st["n_runs"] == len(runs) and st["n_rows"] == int(cnt[keep].sum()) == int(runs["n"].sum()) and st["n_unfinished"] == 0 and st["overflow"] == 0
    assert st["n_skipped"] == int((~keep).sum())
    key = list(zip(runs["query"].tolist(), runs["off"].tolist(), runs["rank"].tolist()))
    assert key == sorted(key) and (runs["reserved"] == 0).all()                   # the order fmd_locate_batch promises
    return cnt, runs, st


def test_rows_ctA(gpu, golden_sets):
    d = gpu.DevIndex.open(os.path.join(GOLD, "ctA.fmd"))
    try:
        cnt, runs, st = check_rows(d, golden_sets["ctA"]["qs"])
        assert 0 < st["n_ext"] < sum(int(r["n"]) * int(r["off"] + 1) for r in runs)     # fewer extensions than rows x steps: the rows share their walk
        _, _, st20 = check_rows(d, golden_sets["ctA"]["qs"], max_occ=20)                # some intervals above max_occ, some below
        assert 0 < st20["n_skipped"] < (cnt > 0).sum()
    finally:
        d.close()


def test_rows_special_with_N(gpu):
    """reads with N: a walk goes through an N like through any base; a query that holds an N finds the reads that have one there"""
    _, reads = fastq_names_reads("special")
    strands = strands_of(reads, trim=True)
    qs = queries(strands, 300, 7, max_len=40)
    with_n = [r for r in strands if (r == 5).any()]
    assert len(with_n) >= 10
    for r in with_n[:10]:
        p = int(np.flatnonzero(r == 5)[0])
        qs.append(r[max(0, p - 3):p + 4].copy())                                   # the N inside the query
        qs.append(r[p + 1:].copy() if p + 1 < len(r) else r[p:].copy())            # the N just left of the match: the walk's next symbol
    d = gpu.DevIndex.open(os.path.join(GOLD, "special.fmd"))
    try:
        cnt, runs, _ = check_rows(d, qs)
        assert all(cnt[i] > 0 for i in range(300, len(qs)))
        res = d.locate(qs, max_occ=int(cnt.max()) + 1, sorted_map=np.fromfile(os.path.join(GOLD, "special.rank"), dtype=np.uint64))
        b = Brute(strands)
        for i in list(range(0, 300, 5)) + list(range(300, len(qs))):
            assert hits_of(res, i) == b.hits(qs[i]), i
    finally:
        d.close()


def test_rows_dup32_one_long_run(gpu, gold):
    """one read 40 000 times over: its rows walk as ONE item, and the '$' child is one run of all its copies; max_occ below the count: nothing is located"""
    read = np.array([b"$ACGTN".index(c) for c in gold.npz("dup32_vectors.npz")["read"].tobytes()], dtype=np.uint8)    # (stored as letters)
    qs = [read, read[37:], read[:50], read[20:45], revcomp(read)[5:30], read[88:], np.array([1, 2, 3, 4, 1, 2, 3, 4, 1, 1, 1, 2], dtype=np.uint8)]
    d = gpu.DevIndex.open(os.path.join(GOLD, "dup32.fmd"))
    try:
        cnt, runs, st = check_rows(d, qs)
        whole = runs[runs["query"] == 0]
        assert cnt[0] >= 1000 and len(whole) == 1 and whole[0]["n"] == cnt[0] and whole[0]["off"] == 0
        assert int(runs["n"].max()) >= 1000
        # below the count
        c1, b1, _ = d.backward_search(qs[:2])
        r1, s1 = d.locate_rows(b1[:1], c1[:1], max_occ=int(c1[0]) - 1)
        assert len(r1) == 0 and s1["n_skipped"] == 1 and s1["n_rows"] == 0 and s1["n_runs"] == 0 and s1["overflow"] == 0 and s1["n_ext"] == 0
        res = d.locate(qs[:1], max_occ=int(c1[0]) - 1)
        assert res[0][0] == c1[0] and not res[1][0] and res[2].tolist() == [0, 0] and len(res[3]) == 0
    finally:
        d.close()


def test_rows_merged_index(gpu):
    """merge.special_palin.fmd: the merged index of two read sets (palindromes, Ns, reads of 8 to 80 bases)"""
    _, a = fastq_names_reads("special")
    _, b = fastq_names_reads("palin")
    qs = queries(strands_of(a, True), 150, 21, max_len=40) + queries(strands_of(b, True), 150, 22)
    d = gpu.DevIndex.open(os.path.join(GOLD, "merge.special_palin.fmd"))
    try:
        check_rows(d, qs)
    finally:
        d.close()


# ---- 3. wide intervals ------------------------------------------------------------------------------------------------------------------------
def test_wide_intervals_cover_the_index(gpu, gold):
    """the 4 one-base and 16 two-base queries on tiny.fmd, nothing skipped: every row that starts with a base is walked to its sentinel, and the
    largest offset per sentinel rank + 1 is the sequence's length as `retrieve` reports it"""
    qs = [np.array([a], dtype=np.uint8) for a in range(1, 5)] + [np.array([a, b], dtype=np.uint8) for a in range(1, 5) for b in range(1, 5)]
    d = gpu.DevIndex.open(gold.path("tiny.fmd"))
    try:
        cnt, beg, _ = d.backward_search(qs)
        assert int(cnt[:4].sum()) == int(d.cnt[5] - d.cnt[1]) and (cnt > 63).all()
        runs, st = d.locate_rows(beg, cnt, max_occ=U32_MAX)
        assert st["n_rows"] == int(cnt.sum()) == int(runs["n"].sum()) and st["n_unfinished"] == 0 and st["n_skipped"] == 0 and st["overflow"] == 0
        n_seq = int(d.mcnt[1])
        one = runs[runs["query"] < 4]
        top = np.full(n_seq, -1, dtype=np.int64)
        two = np.full(n_seq, -1, dtype=np.int64)
        for r, t in ((one, top), (runs[runs["query"] >= 4], two)):
            ranks = np.repeat(r["rank"].astype(np.int64), r["n"]) + np.concatenate([np.arange(int(k)) for k in r["n"]])
            np.maximum.at(t, ranks, np.repeat(r["off"].astype(np.int64), r["n"]))
            per = np.bincount(ranks, minlength=n_seq)
            _, ln, rank = d.retrieve(np.arange(n_seq, dtype=np.uint64), stride=1)
            want = np.zeros(n_seq, dtype=np.int64); want[rank.astype(np.int64)] = ln
            if t is top:
                assert np.array_equal(t + 1, want) and np.array_equal(per, want)      # every base of every sequence once, the last one at offset len - 1
            else:
                assert np.array_equal(t + 2, want) and np.array_equal(per, want - 1)  # every pair of neighbours once
    finally:
        d.close()


# ---- 4. ragged reads, with and without tables -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(gpu):
    """3 000 reads of 30-120 bp with Ns and duplicates (the generator of test_gpu_msearch.py::whole), their BWT from build_bwt, queries and brute force"""
    from fermi_amd import synth
    rng = np.random.default_rng(11)
    gen = synth.genome(synth.DEFAULT_SEED + 5, 20000, 100, 10)
    reads = synth.ragged_reads(synth.DEFAULT_SEED + 77, 2700, gen, min_len=30, max_len=120, err=0.02)
    for r in reads[::9]:
        r[rng.integers(0, len(r), size=2)] = 5                                 # Ns
    reads += [reads[i].copy() for i in rng.integers(0, len(reads), size=300)]  # duplicates
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    assert len(reads) == 3000 and min(map(len, reads)) >= 30 and max(map(len, reads)) <= 120
    strands = strands_of(reads, trim=False)
    qs = queries(strands, 400, 33)
    b = Brute(strands)
    return gpu.build_bwt(reads), strands, qs, [b.hits(q) for q in qs]


@pytest.mark.parametrize("tables", [True, False])
def test_ragged_reads(gpu, ragged, tables):
    """the same index opened with and without FMD_OPEN_NO_TABLES: rows against `retrieve`, and hits against brute force through the map that `retrieve`
    of the sentinel rows gives (sentinel row x ends sequence x; the rank it returns is where that sequence sorts)"""
    bwt, strands, qs, want = ragged
    h = C.c_void_p()
    gpu.check(gpu.lib().fmd_dev_open_bwt_ex(0, bwt.ctypes.data, len(bwt), 0 if tables else 1, C.byref(h)))
    d = gpu.DevIndex(h)
    try:
        n_seq = int(d.mcnt[1])
        assert n_seq == len(strands)
        seqs, ln, rank = d.retrieve(np.arange(n_seq, dtype=np.uint64), stride=128)
        for x in range(0, n_seq, 7):
            assert np.array_equal(seqs[x, :ln[x]], strands[x]), x
        smap = np.zeros(n_seq, dtype=np.uint64)
        smap[rank.astype(np.int64)] = np.arange(n_seq, dtype=np.uint64) << np.uint64(2) | np.uint64(1)
        cnt, _, _ = check_rows(d, qs)
        res = d.locate(qs, max_occ=int(cnt.max()) + 1, sorted_map=smap)
        assert res[1].all()
        for i in range(len(qs)):
            # duplicates sort next to each other in an order of their own; brute force lists every copy, so the sets agree whatever that order is
            assert hits_of(res, i) == want[i], i
    finally:
        d.close()


# ---- 5. the _dev contract ---------------------------------------------------------------------------------------------------------------------
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


GUARD = 0x5A5A5A5A5A5A5A5A


def locate_dev(gpu, d, mem, beg, cnt, max_occ, levels, run_cap, total_rows, guard_words=6):
    """one fmd_locate_dev call on buffers of exactly the stated sizes + guard words after the runs -> (runs, stat, guards)"""
    L = gpu.lib()
    n = len(beg)
    wb = L.fmd_locate_work_bytes(n, total_rows)
    runs = np.zeros(run_cap * 3 + guard_words, dtype=np.uint64)
    runs[run_cap * 3:] = GUARD
    work = np.full(wb // 8 + 8, GUARD, dtype=np.uint64)                           # the work area is a multiple of 16 bytes; 64 guard bytes behind it
    assert wb % 16 == 0
    d_runs, d_stat, d_work = mem.put(runs), mem.put(np.zeros(6, dtype=np.uint64)), mem.put(work)
    gpu.check(L.fmd_locate_dev(d.h, None, n, mem.put(beg), mem.put(cnt), max_occ, levels, d_runs, run_cap, d_stat, d_work, wb))
    d.sync()
    mem.get(d_runs, runs)
    assert (mem.get(d_work, work)[wb // 8:] == GUARD).all()
    stat = mem.get(d_stat, np.zeros(1, dtype=api.LOCATE_STAT_DT))[0]
    return runs[:run_cap * 3].view(api.LOCATE_RUN_DT), {f: int(stat[f]) for f in api.LOCATE_STAT_DT.names}, runs[run_cap * 3:]


def test_dev_contract(gpu, golden_sets):
    s = golden_sets["ctA"]
    L = gpu.lib()
    d = gpu.DevIndex.open(os.path.join(GOLD, "ctA.fmd"))
    mem = DevMem(gpu)
    try:
        cnt, beg, _ = d.backward_search(s["qs"])
        few = cnt <= 1000                                  # (the one- and two-base queries have tens of thousands of rows each: test 1 and 2 walk those)
        cnt, beg = cnt[few], beg[few]
        total = int(cnt.sum())
        full = row_by_row(d, beg, cnt)
        longest = max(t[2] for t in full)
        assert longest >= 100
        # every level there is: the whole answer, in any order
        runs, st, guards = locate_dev(gpu, d, mem, beg, cnt, U32_MAX, longest + 1, total, total)
        assert st["overflow"] == 0 and st["n_unfinished"] == 0 and st["n_rows"] == total and (guards == GUARD).all()
        assert expand(runs[:st["n_runs"]]) == full
        # fewer levels than the longest walk: the rows at offsets >= levels are still walking, every run that was emitted is right
        for levels in (0, 1, 40):
            runs, st, guards = locate_dev(gpu, d, mem, beg, cnt, U32_MAX, levels, total, total)
            assert st["n_unfinished"] == sum(1 for t in full if t[2] >= levels) > 0 and st["overflow"] == 0
            assert expand(runs[:st["n_runs"]]) == [t for t in full if t[2] < levels] and st["n_rows"] == total - st["n_unfinished"]
        # a run array one short of what is needed
        need = st_need = locate_dev(gpu, d, mem, beg, cnt, U32_MAX, longest + 1, total, total)[1]["n_runs"]
        runs, st, guards = locate_dev(gpu, d, mem, beg, cnt, U32_MAX, longest + 1, need - 1, total)
        assert st["overflow"] == 1 and st["n_runs"] == st_need - 1 and (guards == GUARD).all()
        assert set(expand(runs[:st["n_runs"]])) < set(full)
        # a work area sized for fewer rows than there are: the flag, and nothing written past it (the area ends where the guards of the next allocation would be hit:
        # the library derives its capacity from work_bytes alone)
        runs, st, guards = locate_dev(gpu, d, mem, beg, cnt, U32_MAX, longest + 1, total, 0)
        assert (st["overflow"] == 1 or expand(runs[:st["n_runs"]]) == full) and (guards == GUARD).all()
        # all misses; cnt = 0 next to an interval above max_occ
        z = np.zeros(5, dtype=np.uint64)
        runs, st, _ = locate_dev(gpu, d, mem, z, z, 1000, 50, 4, 0)
        assert st == dict(n_runs=0, n_rows=0, n_skipped=0, n_unfinished=0, overflow=0, n_ext=0)
        big = int(np.argmax(cnt))
        runs, st, _ = locate_dev(gpu, d, mem, np.array([0, beg[big]], dtype=np.uint64), np.array([0, cnt[big]], dtype=np.uint64), int(cnt[big]) - 1, 50, 4, 0)
        assert st == dict(n_runs=0, n_rows=0, n_skipped=1, n_unfinished=0, overflow=0, n_ext=0)
        # an interval that reaches past the index is left out, not walked
        runs, st, _ = locate_dev(gpu, d, mem, np.array([d.n - 2], dtype=np.uint64), np.array([3], dtype=np.uint64), 1000, 5, 4, 3)
        assert st["n_skipped"] == 1 and st["n_runs"] == 0 and st["n_ext"] == 0
        # n = 0 is a no-op; argument errors
        assert L.fmd_locate_dev(d.h, None, 0, None, None, 1000, 10, None, 0, None, None, 0) == api.FMD_OK
        wb = L.fmd_locate_work_bytes(len(beg), total)
        assert wb > L.fmd_locate_work_bytes(len(beg), 0) > 0
        d_beg, d_cnt, d_runs, d_stat, d_work = mem.put(beg), mem.put(cnt), mem.alloc(24 * total), mem.alloc(48), mem.alloc(wb)
        short = L.fmd_locate_work_bytes(len(beg), 0) - 1
        assert L.fmd_locate_dev(d.h, None, len(beg), d_beg, d_cnt, 1000, 10, d_runs, total, d_stat, d_work, short) == api.FMD_E_ARG
        assert L.fmd_locate_dev(d.h, None, len(beg), None, d_cnt, 1000, 10, d_runs, total, d_stat, d_work, wb) == api.FMD_E_ARG
        assert L.fmd_locate_dev(d.h, None, len(beg), d_beg, d_cnt, 1000, 10, d_runs, total, None, d_work, wb) == api.FMD_E_ARG
        assert L.fmd_locate_dev(d.h, None, len(beg), d_beg, d_cnt, 1000, 10, d_runs, total, d_stat, None, wb) == api.FMD_E_ARG
        assert L.fmd_locate_dev(None, None, len(beg), d_beg, d_cnt, 1000, 10, d_runs, total, d_stat, d_work, wb) == api.FMD_E_ARG
        assert L.fmd_locate_dev(d.h, None, 2 ** 32, d_beg, d_cnt, 1000, 10, d_runs, total, d_stat, d_work, wb) == api.FMD_E_ARG
        d.sync()
        # the host form stops at max_len levels
        r40, s40 = d.locate_rows(beg, cnt, max_occ=U32_MAX, max_len=40)
        assert expand(r40) == [t for t in full if t[2] < 40] and s40["n_unfinished"] == sum(1 for t in full if t[2] >= 40)
        r0, s0 = d.locate_rows(np.zeros(0, np.uint64), np.zeros(0, np.uint64))
        assert len(r0) == 0 and s0["n_runs"] == 0
    finally:
        mem.free()
        d.close()


# ---- 6. the command ---------------------------------------------------------------------------------------------------------------------------
def test_cli_with_and_without_the_rank_file(gpu, golden_sets, tmp_path):
    """`fermi-amd locate -r ctA.rank` and the same with the map computed in the process print the same bytes: those the brute force of test 1 gives"""
    s = golden_sets["ctA"]
    fa = tmp_path / "q.fa"
    with open(fa, "w") as f:
        for i, q in enumerate(s["qs"]):
            f.write(">q%d\n%s\n" % (i, "".join("$ACGTN"[c] for c in q)))
    want = []
    for i, q in enumerate(s["qs"]):
        want.append("SQ\tq%d\t%d\t%d\t1\n" % (i, len(q), len(s["want"][i])))
        want += ["OC\t%d\t%s\t%d\n" % (sid >> 1, "+-"[sid & 1], pos) for sid, pos in s["want"][i]]
        want.append("//\n")
    want = "".join(want).encode()
    fmd = os.path.join(GOLD, "ctA.fmd")
    a = subprocess.run([AMD, "locate", "-m", "100000", "-r", os.path.join(GOLD, "ctA.rank"), fmd, str(fa)], capture_output=True, timeout=120)
    b = subprocess.run([AMD, "locate", "-m", "100000", fmd, str(fa)], capture_output=True, timeout=120)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout
    assert a.stdout == want
    # -m below a count: the query is reported, not listed
    c = subprocess.run([AMD, "locate", "-m", "3", "-r", os.path.join(GOLD, "ctA.rank"), fmd, str(fa)], capture_output=True, timeout=120)
    assert c.returncode == 0
    blocks = c.stdout.decode().split("//\n")[:-1]
    assert len(blocks) == len(s["qs"])
    for i, blk in enumerate(blocks):
        lines = blk.splitlines()
        n = len(s["want"][i])
        assert lines[0] == "SQ\tq%d\t%d\t%d\t%d" % (i, len(s["qs"][i]), n, n <= 3) and len(lines) == 1 + (n if n <= 3 else 0)
