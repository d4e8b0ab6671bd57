"""GPU: the paths of csrc/fmd_fltuniq.hip and of `fermi-amd fltuniq` that tests/test_gpu_fltuniq.py does not reach -- every k of the
window assembly, chunk seams (de Bruijn reads: every k-mer exactly once), the streamed entries through the C ABI in many batches,
the host forms and the command in many batches (fmd_fltuniq_batch_limits behind FMD_FLTUNIQ_TEST_HOOKS=1), the grid-stride loop and
offsets past 2^32.  The reference of every test is the numpy restatement of seq.c:164-199 (_np_kmers / _np_table of
tests/test_gpu_fltuniq.py; for a table too large to hold twice, the same k-mers and counts without the dense array), and every
comparison is exact: tables word for word, verdicts and output byte for byte.
k = 19 and 20 of "every k" are not run (tables of 64 and 256 GiB); k = 20 is run over the seam lengths where the device has the room."""
import ctypes as C
import functools
import gzip
import os
import re
import time

import numpy as np
import pytest

from test_gpu_fltuniq import GOLD, GUARD, _dev, _np_kmers, _np_table, _ragged, _run

gpu_test = pytest.mark.gpu
T_START = time.time()
ONCE, TWICE = np.uint64(0x5555555555555555), np.uint64(0xFFFFFFFFFFFFFFFF)
HOOK_VARS = ("FMD_FLTUNIQ_TEST_HOOKS", "FMD_FLTUNIQ_TEST_BATCH_BYTES", "FMD_FLTUNIQ_TEST_BATCH_READS")


# ---- inputs and references, computed once and left unchanged
@functools.lru_cache(maxsize=None)
def _case(seed, n, k):
    """ragged reads with non-bases, an empty read and one shorter than every k; between them 60 pairs of equal reads of 40 random
    bases at neighbouring places, whose k-mers occur exactly twice -> (reads, table, verdicts)"""
    reads = _ragged(seed, n)
    rng = np.random.default_rng(seed + 7)
    for i in rng.choice(np.arange(20, n - 2, 3), 60, replace=False):
        reads[i] = rng.integers(1, 5, 40).astype(np.uint8)
        reads[i + 1] = reads[i].copy()
    tab, verdict = _np_table(reads, k)
    tab.setflags(write=False); verdict.setflags(write=False)
    return reads, tab, verdict


def _np_sparse(reads, k):
    """_np_table without the dense array: (k-mers in increasing order, their states 1 / 3, verdicts)"""
    km = _np_kmers(reads, k)
    u, cnt = np.unique(np.concatenate([z for _, z in km] + [np.zeros(0, np.int64)]), return_counts=True)
    twice = set(u[cnt >= 2].tolist())
    verdict = np.array([ok and all(int(x) in twice for x in z) for ok, z in km], dtype=bool)
    return u, np.where(cnt >= 2, 3, 1).astype(np.uint64), verdict


def _np_window(u, state, first_word, n_words):
    """words [first_word, +n_words) of the table that holds `state` for the k-mers `u`"""
    tab = np.zeros(n_words, dtype=np.uint64)
    m = ((u >> 5) >= first_word) & ((u >> 5) < first_word + n_words)
    np.bitwise_or.at(tab, (u[m] >> 5) - first_word, state[m] << ((u[m].astype(np.uint64) & np.uint64(31)) << np.uint64(1)))
    return tab


def de_bruijn(k):
    """a linear de Bruijn sequence B(4, k) as nt6 codes: the Lyndon words whose length divides k, in order, and the first k - 1 bases
    again -- 4^k + k - 1 bases, every k-mer in exactly one window"""
    a, seq = [0] * (4 * k), []

    def db(t, p):
        if t > k:
            if k % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return (np.array(seq + seq[:k - 1], dtype=np.uint8) + 1).astype(np.uint8)


def _seam_positions(k, length):
    step = 65 - k
    return sorted({0, k - 1, step - 1, step, step + k - 2, 63, 64, length - 1})


def _with_non_base(seq, p):
    r = seq.copy()
    r[p] = 5
    return r


def _table_without(seq, k, p):
    """every k-mer of the de Bruijn read once, but those of the windows that cover position p"""
    w = np.int64(4) ** np.arange(k - 1, -1, -1, dtype=np.int64)
    tab = np.full(4 ** k // 32, ONCE, dtype=np.uint64)
    for s in range(max(0, p - k + 1), min(p, len(seq) - k) + 1):
        z = int(((seq[s:s + k].astype(np.int64) - 1) * w).sum())
        tab[z >> 5] &= ~(np.uint64(3) << np.uint64((z & 31) << 1))
    return tab


DB_K = [3, 4, 5, 6, 7]


@pytest.mark.parametrize("k", DB_K)
def test_reference_on_de_bruijn_reads(k):
    """(no GPU) the input condition of the seam tests: the numpy reference alone counts every k-mer of B(4, k) exactly once, and a
    non-base at p takes out exactly the windows that cover p"""
    seq = de_bruijn(k)
    assert len(seq) == 4 ** k + k - 1 == {3: 66, 4: 259, 5: 1028, 6: 4101, 7: 16390}[k]
    assert seq.min() == 1 and seq.max() == 4
    tab, verdict = _np_table([seq], k)
    assert len(tab) == 4 ** k // 32 and (tab == ONCE).all() and not verdict[0]
    tab, verdict = _np_table([seq, seq], k)
    assert (tab == TWICE).all() and verdict.all()
    for p in _seam_positions(k, len(seq)):
        tab, verdict = _np_table([_with_non_base(seq, p)], k)
        want = _table_without(seq, k, p)
        assert np.array_equal(tab, want) and not verdict[0]
        st = np.concatenate([(want >> np.uint64(2 * j)) & np.uint64(3) for j in range(32)])
        assert (st == 0).sum() == min(p, len(seq) - k) - max(0, p - k + 1) + 1 and ((st == 0) | (st == 1)).all()


def _cut(reads, max_bytes, max_reads):
    """the batches the limits allow, cut greedily in file order: [first, last) read numbers"""
    out, i = [], 0
    while i < len(reads):
        j, fill = i, 0
        while j < len(reads) and j - i < max_reads and fill + len(reads[j]) <= max_bytes:
            fill += len(reads[j]); j += 1
        assert j > i
        out.append((i, j)); i = j
    return out


def _split_kmers(reads, k, batches):
    """the k-mers that occur exactly twice, once in each of two neighbouring batches"""
    batch_of = np.zeros(len(reads), dtype=np.int64)
    for b, (i, j) in enumerate(batches):
        batch_of[i:j] = b
    km = _np_kmers(reads, k)
    z_all = np.concatenate([z for _, z in km])
    b_all = np.concatenate([np.full(len(z), batch_of[r]) for r, (_, z) in enumerate(km)])
    order = np.argsort(z_all, kind="stable")
    z_s, b_s = z_all[order], b_all[order]
    u, first, cnt = np.unique(z_s, return_index=True, return_counts=True)
    two = first[cnt == 2]
    return u[cnt == 2][np.abs(b_s[two] - b_s[two + 1]) == 1]


# ---- the streamed entries through the C ABI
class Stream:
    """fmd_fltuniq_t by hand: slot -> fill the pinned arrays -> count / test"""

    def __init__(self, gpu, k, max_bytes, max_reads, h=None):
        self.gpu, self.L, self.k, self.max_bytes, self.max_reads = gpu, gpu.lib(), k, max_bytes, max_reads
        self.h = h or C.c_void_p()
        if h is None:
            gpu.check(self.L.fmd_fltuniq_open(0, k, max_bytes, max_reads, C.byref(self.h)))
        self.words = self.L.fmd_fltuniq_table_bytes(k) // 8
        self.seqs = self.off = None

    def close(self):
        self.L.fmd_fltuniq_close(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def slot(self):
        s, o = C.c_void_p(), C.c_void_p()
        self.gpu.check(self.L.fmd_fltuniq_slot(self.h, C.byref(s), C.byref(o)))
        self.seqs = np.ctypeslib.as_array(C.cast(s, C.POINTER(C.c_uint8)), shape=(self.max_bytes,))
        self.off = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), shape=(self.max_reads + 1,))

    def fill(self, reads):
        self.off[0] = 0
        if len(reads):
            self.off[1:len(reads) + 1] = np.cumsum([len(r) for r in reads])
            flat = np.concatenate(reads)
            self.seqs[:len(flat)] = flat

    def cut(self, reads):
        return _cut(reads, self.max_bytes, self.max_reads)

    def count(self, reads):
        batches = self.cut(reads)
        for i, j in batches:
            self.slot()
            self.fill(reads[i:j])
            self.gpu.check(self.L.fmd_fltuniq_count(self.h, j - i))
        return batches

    def sync(self):
        ms = (C.c_double * 2)(-1.0, -1.0)
        self.gpu.check(self.L.fmd_fltuniq_sync(self.h, ms))
        return ms[0], ms[1]

    def export(self, first=0, n=None):
        n = self.words - first if n is None else n
        out = np.zeros(n, dtype=np.uint64)
        self.gpu.check(self.L.fmd_fltuniq_export(self.h, first, n, out.ctypes.data))
        return out


def _test_pass_checked(st, reads, verdict):
    """the test pass in batches into one verdict array at moving offsets; at every step the bytes of the batches in flight and of those
    to come still hold the pattern written before the run, the delivered ones hold the reference's verdicts, the guards stay"""
    n = len(reads)
    buf = np.full(n + 2 * GUARD, 0x5A, dtype=np.uint8)
    got, want = buf[GUARD:GUARD + n], verdict.astype(np.uint8)
    batches = st.cut(reads)
    for b, (i, j) in enumerate(batches):
        st.slot()                                        # batch b - 2 had this slot: its verdicts are delivered now, and nothing else
        done = batches[b - 2][1] if b >= 2 else 0
        assert np.array_equal(got[:done], want[:done]) and (got[done:] == 0x5A).all(), b
        st.fill(reads[i:j])
        st.gpu.check(st.L.fmd_fltuniq_test(st.h, j - i, got[i:].ctypes.data))
        assert np.array_equal(got[:done], want[:done]) and (got[done:] == 0x5A).all(), b     # (b - 1 and b are in flight)
    ms = st.sync()
    assert np.array_equal(got, want) and (buf[:GUARD] == 0x5A).all() and (buf[-GUARD:] == 0x5A).all()
    return batches, ms


@gpu_test
@pytest.mark.parametrize("max_bytes,max_reads", [(257, 1000), (1 << 20, 5)])
def test_streamed_run_in_many_batches(gpu, max_bytes, max_reads):
    k = 11
    reads, want, verdict = _case(55, 2000, k)
    with Stream(gpu, k, max_bytes, max_reads) as st:
        batches = st.cut(reads)
        assert len(batches) > 300 and max(j - i for i, j in batches) <= max_reads
        # consecutive count batches run on two streams at once: k-mers whose only two occurrences lie in neighbouring batches
        split = _split_kmers(reads, k, batches)
        assert len(split) >= 100, len(split)
        assert st.count(reads) == batches
        ms1 = st.sync()
        assert ms1[0] > 0 and ms1[1] == 0
        got = st.export()
        assert np.array_equal(got, want)
        state = (got[split >> 5] >> ((split.astype(np.uint64) & np.uint64(31)) << np.uint64(1))) & np.uint64(3)
        assert (state == 3).all()
        mid = st.words // 3 + 5
        assert np.array_equal(st.export(mid, 4099), want[mid:mid + 4099])
        assert len(st.export(st.words, 0)) == 0
        assert _test_pass_checked(st, reads, verdict)[0] == batches
        ms2 = st.sync()
        assert ms2[0] >= ms1[0] and ms2[1] > 0
        assert st.sync()[1] >= ms2[1]
        assert np.array_equal(st.export(), want)                       # the test pass only reads the table
        print("streamed, %d bytes / %d reads a slot: %d batches, %d k-mers seen once in each of two neighbouring batches; kernels %.3f + %.3f ms"
              % (max_bytes, max_reads, len(batches), len(split), ms2[0], ms2[1]))


@gpu_test
def test_streamed_argument_errors_leave_the_run_usable(gpu):
    L, k, E = gpu.lib(), 11, gpu.FMD_E_ARG
    reads, want, verdict = _case(55, 2000, k)
    h = C.c_void_p()
    for kk, mb, mr in ((2, 100, 10), (21, 100, 10), (k, 0, 10), (k, 100, 0)):
        assert L.fmd_fltuniq_open(0, kk, mb, mr, C.byref(h)) == E and not h.value
    assert L.fmd_fltuniq_open(0, k, 100, 10, None) == E
    L.fmd_fltuniq_close(None)
    assert L.fmd_fltuniq_sync(None, None) == E
    ms = (C.c_double * 2)(-1.0, -1.0)
    assert L.fmd_fltuniq_sync(None, ms) == E and ms[0] == -1.0
    ok = np.full(16, 0x5A, dtype=np.uint8)
    with Stream(gpu, k, 1000, 10) as st:
        assert L.fmd_fltuniq_count(st.h, 1) == E and L.fmd_fltuniq_test(st.h, 1, ok.ctypes.data) == E        # before any slot
        assert L.fmd_fltuniq_slot(st.h, None, None) == E
        st.slot()
        st.fill(reads[20:24])
        assert L.fmd_fltuniq_count(st.h, 11) == E                                                             # n_reads > max_reads
        st.off[0] = 1
        assert L.fmd_fltuniq_count(st.h, 4) == E and L.fmd_fltuniq_test(st.h, 4, ok.ctypes.data) == E         # off[0] != 0
        st.off[0] = 0
        keep = int(st.off[4])
        st.off[4] = 1001
        assert L.fmd_fltuniq_count(st.h, 4) == E and L.fmd_fltuniq_test(st.h, 4, ok.ctypes.data) == E         # off[n] > max_bytes
        st.off[4] = keep
        assert L.fmd_fltuniq_test(st.h, 4, None) == E                                                         # no place for the verdicts
        one = np.zeros(2, dtype=np.uint64)
        assert L.fmd_fltuniq_export(st.h, st.words, 1, one.ctypes.data) == E and L.fmd_fltuniq_export(st.h, st.words + 1, 0, one.ctypes.data) == E
        assert L.fmd_fltuniq_export(st.h, 0, st.words + 1, one.ctypes.data) == E and L.fmd_fltuniq_export(st.h, 0, 1, None) == E
        assert L.fmd_fltuniq_export(st.h, (1 << 64) - 1, 2, one.ctypes.data) == E
        assert L.fmd_fltuniq_export(None, 0, 1, one.ctypes.data) == E
        assert not st.export().any()                                                                          # none of these counted anything
        # no reads: fine, and the slot is not taken -- the same slot then takes a batch
        assert L.fmd_fltuniq_count(st.h, 0) == 0 and L.fmd_fltuniq_test(st.h, 0, ok.ctypes.data) == 0
        assert not st.export().any()
        gpu.check(L.fmd_fltuniq_count(st.h, 4))
        assert L.fmd_fltuniq_count(st.h, 4) == E                                                              # the slot is at work
        assert (ok == 0x5A).all()
        # the run is as good as new: the rest of the reads, then every verdict
        st.count(reads[:20] + reads[24:])
        assert np.array_equal(st.export(), want)
        _test_pass_checked(st, reads, verdict)


# ---- every k
@gpu_test
@pytest.mark.parametrize("k", list(range(3, 15)))
def test_every_k_table_and_verdicts(gpu, k):
    """k = 3..14, each its own sequence of lane shifts in fu_window (the powers of two and the all-ones 7 among them).  15..18 are the
    command's md5s of tests/test_gpu_fltuniq.py, 17 is below; 19 and 20 would need tables of 64 and 256 GiB and are not run here."""
    reads = _ragged(200 + k, 1500)
    want, verdict = _np_table(reads, k)
    got = gpu.fltuniq_table(reads, k)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    ok = gpu.fltuniq_pass(reads, k)
    assert ok.dtype == bool and np.array_equal(ok, verdict)
    assert ok[3] and 0 < ok.sum() < len(ok)


def _windows_equal(st, u, state, firsts, n_words=1024):
    for w0 in firsts:
        w0 = int(min(max(0, w0), st.words - n_words))
        assert np.array_equal(st.export(w0, n_words), _np_window(u, state, w0, n_words)), w0


@gpu_test
def test_k17_streamed_without_copying_the_table(gpu):
    """4 GiB of table: every verdict, and 1024-word windows of the table at both ends and around eight k-mers of the reads, half of
    them k-mers >= 2^32 (an all-A and an all-T read twice each make word 0 and the last word non-zero)"""
    k = 17
    reads = _ragged(317, 400)
    reads += [np.full(40, 1, np.uint8), np.full(40, 4, np.uint8), np.full(40, 1, np.uint8), np.full(40, 4, np.uint8)]
    u, state, verdict = _np_sparse(reads, k)
    assert u[0] == 0 and u[-1] == 4 ** k - 1 and state[0] == 3 and state[-1] == 3 and (state == 1).any() and verdict[-4:].all()
    picks = u[np.linspace(1, len(u) - 2, 8).astype(np.int64)]
    assert (picks >= 1 << 32).sum() >= 4 and (picks < 1 << 32).any()
    with Stream(gpu, k, 4000, 64) as st:
        assert st.words == 4 ** k // 32 == 1 << 29
        assert len(st.count(reads)) > 6
        _windows_equal(st, u, state, [0, st.words - 1024] + [int(z >> 5) - 512 for z in picks])
        assert (st.export(0, 1)[0] & np.uint64(3)) == 3 and st.export(st.words - 1, 1)[0] >> np.uint64(62) == 3
        _test_pass_checked(st, reads, verdict)
    assert 0 < verdict.sum() < len(verdict)


# ---- chunk seams
@gpu_test
@pytest.mark.parametrize("k", DB_K)
def test_de_bruijn_reads_cross_every_seam(gpu, k):
    """B(4, k) holds every k-mer once, in windows that cross every chunk seam of the read: a window counted by both chunks of a seam
    shows as state 3 and a window dropped as state 0, wherever it is"""
    seq = de_bruijn(k)
    got = gpu.fltuniq_table([seq], k)
    assert (got == ONCE).all(), np.flatnonzero(got != ONCE)[:8]
    assert not gpu.fltuniq_pass([seq], k)[0]
    assert (gpu.fltuniq_table([seq, seq], k) == TWICE).all()
    assert gpu.fltuniq_pass([seq, seq], k).all()
    with Stream(gpu, k, len(seq), 1) as st:                       # once in each of two calls on one table, the calls on two streams
        assert st.count([seq, seq]) == [(0, 1), (1, 2)]
        assert (st.export() == TWICE).all()
    for p in _seam_positions(k, len(seq)):
        r = _with_non_base(seq, p)
        assert np.array_equal(gpu.fltuniq_table([r], k), _table_without(seq, k, p)), p
        assert not gpu.fltuniq_pass([r], k)[0], p
        assert not gpu.fltuniq_pass([r, r], k).any(), p           # every window there is has state 3 now: the non-base alone fails them


def _seam_lengths(k):
    step = 65 - k
    return sorted({0, 1, k - 1, k, k + 1, 63, 64, 65, step + k - 2, step + k - 1, step + k, 2 * step + k - 1, 2 * step + k, 128, 129})


def _seam_reads(k):
    """every length around the seams once clean and once with a non-base at its last position (which only the chunk before the last
    seam sees when the tail is shorter than k) -> (the clean reads, the others)"""
    rng = np.random.default_rng(900 + k)
    clean = [rng.integers(1, 5, n).astype(np.uint8) for n in _seam_lengths(k)]
    return clean, [_with_non_base(rng.integers(1, 5, n).astype(np.uint8), n - 1) for n in _seam_lengths(k) if n]


@gpu_test
@pytest.mark.parametrize("k", [3, 8, 13, 16])
def test_lengths_around_the_seams(gpu, k):
    clean, other = _seam_reads(k)
    for reads in (clean + other, clean + other + clean):      # once: at k = 13 and 16 nearly every state is 1, a window counted twice shows;
        want, verdict = _np_table(reads, k)                   # the clean reads twice: they pass, through every chunk
        assert np.array_equal(gpu.fltuniq_table(reads, k), want)
        ok = gpu.fltuniq_pass(reads, k)
        assert np.array_equal(ok, verdict)
        if k == 13 and len(reads) == len(clean + other):
            st = np.concatenate([(want >> np.uint64(2 * j)) & np.uint64(3) for j in range(32)])
            assert (st == 1).sum() > 1000 and (st == 3).sum() == 0
    n = len(clean)
    assert ok[:n].all() and not ok[n:n + len(other)].any() and ok[n + len(other):].all()


@gpu_test
def test_lengths_around_the_seams_k20(gpu):
    """k = 20 where its table of 256 GiB fits the device beside what else runs there (k = 16 above stands in where it does not):
    verdicts, and table windows at both ends and around k-mers of the reads"""
    import torch
    k = 20
    need = gpu.lib().fmd_fltuniq_table_bytes(k)
    free, total = torch.cuda.mem_get_info(0)
    if free < need + (16 << 30):
        print("k = 20 not run: %.0f GiB free of %.0f, the table takes %.0f; k = 16 stands in" % (free / 2 ** 30, total / 2 ** 30, need / 2 ** 30))
        return
    clean, other = _seam_reads(k)
    reads = clean + other + clean[::2] + [np.full(30, 1, np.uint8), np.full(30, 4, np.uint8)] * 2
    u, state, verdict = _np_sparse(reads, k)
    t0 = time.time()
    h = C.c_void_p()
    rc = gpu.lib().fmd_fltuniq_open(0, k, 4096, 16, C.byref(h))
    if rc == gpu.FMD_E_NOMEM:
        print("k = 20 not run: the device has no 256 GiB in one piece; k = 16 stands in")
        return
    gpu.check(rc)
    with Stream(gpu, k, 4096, 16, h) as st:
        assert st.words == 1 << 35
        st.count(reads)
        picks = u[np.linspace(1, len(u) - 2, 8).astype(np.int64)]
        _windows_equal(st, u, state, [0, st.words - 1024] + [int(z >> 5) - 512 for z in picks])
        _test_pass_checked(st, reads, verdict)
    print("k = 20: %.1f s with a table of 256 GiB" % (time.time() - t0))


# ---- the host forms and the command in many batches
def _limits(gpu):
    b, r = C.c_uint64(), C.c_uint64()
    gpu.lib().fmd_fltuniq_batch_limits(C.byref(b), C.byref(r))
    return b.value, r.value


def _host_batches(reads, max_bytes, max_reads):
    return len(_cut(reads, max(max_bytes, max(len(r) for r in reads)), max_reads))     # (a limit below the longest read is raised to it)


@gpu_test
def test_host_forms_in_many_batches(gpu, monkeypatch):
    k = 11
    reads, want, verdict = _case(55, 2000, k)
    for v in HOOK_VARS:
        monkeypatch.delenv(v, raising=False)
    assert _limits(gpu) == (64 << 20, 1 << 20)
    monkeypatch.setenv("FMD_FLTUNIQ_TEST_BATCH_BYTES", "300")
    monkeypatch.setenv("FMD_FLTUNIQ_TEST_BATCH_READS", "7")
    assert _limits(gpu) == (64 << 20, 1 << 20)                      # without the gate the two are not read
    monkeypatch.setenv("FMD_FLTUNIQ_TEST_HOOKS", "0")
    assert _limits(gpu) == (64 << 20, 1 << 20)
    monkeypatch.setenv("FMD_FLTUNIQ_TEST_HOOKS", "1")
    assert _limits(gpu) == (300, 7)                                 # (read on every call: nothing is cached)
    monkeypatch.setenv("FMD_FLTUNIQ_TEST_BATCH_READS", "0")
    assert _limits(gpu) == (300, 1 << 20)
    monkeypatch.delenv("FMD_FLTUNIQ_TEST_BATCH_BYTES")
    assert _limits(gpu) == (64 << 20, 1 << 20)
    longest = max(len(r) for r in reads)
    for max_bytes, max_reads in ((300, 7), (longest - 30, 1000), (1 << 20, 1)):      # the second: below the longest read, raised to it
        monkeypatch.setenv("FMD_FLTUNIQ_TEST_BATCH_BYTES", str(max_bytes))
        monkeypatch.setenv("FMD_FLTUNIQ_TEST_BATCH_READS", str(max_reads))
        assert _limits(gpu) == (max_bytes, max_reads)
        n_batches = _host_batches(reads, max_bytes, max_reads)
        print("host forms with %d bytes / %d reads a batch: %d batches a pass" % (max_bytes, max_reads, n_batches))
        assert n_batches > 250
        assert np.array_equal(gpu.fltuniq_table(reads, k), want)
        assert np.array_equal(gpu.fltuniq_pass(reads, k), verdict)


def _cli(name, k, hooks=None, bytes_=None, reads=None):
    env = {a: b for a, b in os.environ.items() if a not in HOOK_VARS}
    env["FMD_TIMING"] = "1"
    if hooks is not None:
        env["FMD_FLTUNIQ_TEST_HOOKS"] = str(hooks)
    if bytes_ is not None:
        env["FMD_FLTUNIQ_TEST_BATCH_BYTES"] = str(bytes_)
    if reads is not None:
        env["FMD_FLTUNIQ_TEST_BATCH_READS"] = str(reads)
    p = _run(["fltuniq", "-k%d" % k, os.path.join(GOLD, name)], env=env)
    m = re.search(r"\[M::main_fltuniq\] batches: (\d+) in pass 1, (\d+) in pass 2\n", p.stderr.decode())
    return p, (int(m.group(1)), int(m.group(2))) if m else None


def _golden(name, k):
    return gzip.open(os.path.join(GOLD, "fltuniq.%s.k%d.out.gz" % (name, k))).read()


def _fastq_nt6(name):
    tab = np.full(256, 5, dtype=np.uint8)
    for ch, v in zip(b"ACGTacgt", [1, 2, 3, 4, 1, 2, 3, 4]):
        tab[ch] = v
    ln = gzip.open(os.path.join(GOLD, name)).read().split(b"\n")
    return [ln[i] for i in range(0, len(ln) - 1, 4)], [tab[np.frombuffer(ln[i], dtype=np.uint8)] for i in range(1, len(ln) - 1, 4)]


PAIRS_READ_LIMIT, PAIRS_ONE_MATE_FAILS, PAIRS_STRADDLING = 7, 25, 4


@gpu_test
def test_cli_pairs_in_many_batches(gpu):
    """1400 mates in batches of 7 reads: every seventh pair lies across a batch border, its first mate's verdict delivered a batch before
    its second's.  By the numpy verdicts 25 pairs have exactly one failing mate and 4 of those lie across a border, so the pairing
    machine must carry the name and the held record over."""
    names, reads = _fastq_nt6("pairs.cofq.fq.gz")
    n = len(reads)
    assert n == 1400 and all(names[i] == names[i + 1] for i in range(0, n, 2)) and len(set(names)) == n // 2
    _, verdict = _np_table(reads, 13)
    one = [i for i in range(0, n, 2) if verdict[i] != verdict[i + 1]]
    assert len(one) == PAIRS_ONE_MATE_FAILS
    assert sum(1 for i in one if (i + 1) % PAIRS_READ_LIMIT == 0) == PAIRS_STRADDLING
    assert {True, False} == {bool(verdict[i]) for i in one if (i + 1) % PAIRS_READ_LIMIT == 0}     # the failing mate on either side of a border
    p, batches = _cli("pairs.cofq.fq.gz", 13, hooks=1, reads=PAIRS_READ_LIMIT)
    assert p.returncode == 0, p.stderr.decode()
    print("fltuniq -k13 pairs.cofq.fq.gz, %d reads a batch: %s batches" % (PAIRS_READ_LIMIT, batches))
    assert batches == (200, 200) and min(batches) > 100
    assert p.stdout == _golden("pairs.cofq.fq.gz", 13)


@gpu_test
@pytest.mark.parametrize("limit", [1, 2, 3])
def test_cli_three_records_under_one_name_across_borders(gpu, limit):
    """the three records @a of the corner file (passes, holds an N, passes) in batches of 1, 2 and 3 reads: every place a border can have"""
    p, batches = _cli("readprep.corner.fx", 5, hooks=1, reads=limit)
    assert p.returncode == 0, p.stderr.decode()
    assert batches == (-(-14 // limit),) * 2
    assert p.stdout == _golden("readprep.corner.fx", 5)


@gpu_test
def test_cli_byte_limit_and_the_gate(gpu):
    want = _golden("special.fq.gz", 11)
    reads = _fastq_nt6("special.fq.gz")[1]
    assert len(reads) == 302 and max(len(r) for r in reads) == 60
    p, batches = _cli("special.fq.gz", 11, hooks=1, bytes_=256, reads=1 << 20)
    assert p.returncode == 0, p.stderr.decode()
    print("fltuniq -k11 special.fq.gz, 256 bytes a batch: %s batches" % (batches,))
    assert batches == (len(_cut(reads, 256, 1 << 20)),) * 2 and batches[0] > 50
    assert p.stdout == want
    p, batches = _cli("special.fq.gz", 11, hooks=1, bytes_=59)           # the longest record has 60 bases
    assert p.returncode == 1 and p.stdout == b"" and batches is None
    assert "[E::main_fltuniq] a sequence of 60 bases: longer than a batch\n" in p.stderr.decode()
    p, batches = _cli("special.fq.gz", 11, hooks=1, bytes_=60)
    assert p.returncode == 0 and p.stdout == want and batches == (len(_cut(reads, 60, 1 << 20)),) * 2 and batches[0] > 200
    for hooks in (None, 0):                                              # without the gate: one batch a pass, the same bytes
        p, batches = _cli("special.fq.gz", 11, hooks=hooks, bytes_=59, reads=1)
        assert p.returncode == 0 and batches == (1, 1) and p.stdout == want


# ---- the kernels: grid-stride loop, partial workgroups, offsets past 2^32
def _count_and_test_dev(gpu, k, d_seqs, off, n, want, verdict):
    L = gpu.lib()
    words = len(want)
    host = np.full(words + 2 * GUARD, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    hpass = np.full(n + 2 * GUARD, 0x5A, dtype=np.uint8)
    d_off, d_tab, d_pass = _dev(gpu, off), _dev(gpu, host), _dev(gpu, hpass)
    try:
        tab = C.c_void_p(d_tab.value + 8 * GUARD)
        gpu.check(L.fmd_memset_dev(tab, 0, words * 8, None))
        gpu.check(L.fmd_fltuniq_count_dev(0, None, k, d_seqs, d_off, n, tab))
        gpu.check(L.fmd_fltuniq_test_dev(0, None, k, d_seqs, d_off, n, tab, C.c_void_p(d_pass.value + GUARD)))
        gpu.check(L.fmd_memcpy_d2h(host.ctypes.data, d_tab, host.nbytes, None))
        gpu.check(L.fmd_memcpy_d2h(hpass.ctypes.data, d_pass, hpass.nbytes, None))
    finally:
        for p in (d_off, d_tab, d_pass):
            L.fmd_dev_free(p)
    assert np.array_equal(host[GUARD:-GUARD], want)
    assert (host[:GUARD] == 0xA5A5A5A5A5A5A5A5).all() and (host[-GUARD:] == 0xA5A5A5A5A5A5A5A5).all()
    assert np.array_equal(hpass[GUARD:-GUARD], verdict.astype(np.uint8))
    assert (hpass[:GUARD] == 0x5A).all() and (hpass[-GUARD:] == 0x5A).all()


@gpu_test
def test_grid_stride_loop_and_partial_workgroups(gpu):
    """more reads than the launch has waves (32 a CU), so r += n_waves takes a second turn and a third begins; then 1..5 reads, whose
    workgroups of four waves are not full"""
    import torch
    k, L = 9, gpu.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * 32 * cus + 5
    rng = np.random.default_rng(88)
    gen = rng.integers(1, 5, 3000).astype(np.uint8)
    lens, pos = rng.integers(1, 41, n), rng.integers(0, 3000 - 40, n)
    reads = [rng.integers(1, 5, 40).astype(np.uint8)] + [gen[p:p + ln].copy() for p, ln in zip(pos, lens)][1:]
    for i in 1 + rng.choice(n - 1, n // 10, replace=False):
        reads[i][rng.integers(0, len(reads[i]))] = 5
    few = [np.full(30, 1, np.uint8), reads[0], np.full(12, 2, np.uint8), _with_non_base(reads[1], 0), reads[0]]
    assert len(few[1]) == 40 and [_np_table(few[:m], k)[1].tolist() for m in (1, 2, 3, 4, 5)] == [
        [True], [True, False], [True, False, True], [True, False, True, False], [True, True, True, False, True]]
    for m in (n, 1, 2, 3, 4, 5):
        sub = reads if m == n else few[:m]
        want, verdict = _np_table(sub, k)
        flat, off = gpu.flatten_reads(sub)
        d_seqs = _dev(gpu, flat)
        try:
            _count_and_test_dev(gpu, k, d_seqs, off, m, want, verdict)
        finally:
            L.fmd_dev_free(d_seqs)
        if m == n:
            assert 0 < verdict.sum() < n and (want != 0).any()
    print("grid-stride: %d CUs, %d reads" % (cus, n))


@gpu_test
def test_offsets_past_4_gib(gpu):
    """off[] is absolute and 64-bit: reads that lie on both sides of the 4 GiB mark of d_seqs (nothing but the reads is copied there)"""
    k, L = 7, gpu.lib()
    rng = np.random.default_rng(99)
    gen = rng.integers(1, 5, 400).astype(np.uint8)
    reads = [gen[p:p + ln].copy() for p, ln in zip(rng.integers(0, 250, 20), rng.integers(60, 150, 20))]
    reads[5][17] = 5; reads[11] = reads[11][:3]; reads[12] = np.zeros(0, np.uint8)
    flat, off = gpu.flatten_reads(reads)
    base = (1 << 32) - 200
    off = off + np.uint64(base)
    assert off[0] < 1 << 32 < off[4] and off[-1] > (1 << 32) + 1500 and off[-1] <= (1 << 32) + 4096 - 16
    want, verdict = _np_table(reads, k)
    assert (want != 0).any() and 0 < verdict.sum() < len(reads)
    d_seqs = C.c_void_p()
    gpu.check(L.fmd_dev_malloc(0, (1 << 32) + 4096, C.byref(d_seqs)))
    try:
        gpu.check(L.fmd_memcpy_h2d(C.c_void_p(d_seqs.value + base), flat.ctypes.data, int(off[-1]) - base, None))
        _count_and_test_dev(gpu, k, d_seqs, off, len(reads), want, verdict)
    finally:
        L.fmd_dev_free(d_seqs)


@gpu_test
def test_zz_duration_of_this_file(gpu):
    print("tests/test_gpu_fltuniq_paths.py: %.1f s" % (time.time() - T_START))
