"""GPU: the k-mer harvest of `correct` (fmd_kmer_collect, _seeds, _part_dev: k_kmer_level, k_kmer_emit, the tile compaction, the regrowth loop, the
shards) against brute force over the reads (tests/harvest_ref.py, itself checked against the reference-made golden and the oracle in
tests/test_harvest_ref_host.py).  Every comparison is exact: the triples (bucket, key, val) in the order the entry promises, and cnt[]."""
import ctypes as C

import numpy as np
import pytest

import harvest_ref as hr
from fermi_amd import api, synth

pytestmark = pytest.mark.gpu

MIN_CAP = 1 << 16                  # the smallest capacity the entries take
SYNTH = (17, 1, 2)                 # (w, min_occ, suf_len) on the synthetic index


# ---- the indexes, opened once, and their brute force ----------------------------------------------------------------------------------------------
class Sets:
    def __init__(self, gpu, gold):
        self.gpu, self.gold, self.open, self.ref = gpu, gold, {}, {}

    def dev(self, name):
        if name not in self.open:
            self.open[name] = self.synth_index() if name == "synth" else self.cg_index() if name == "cg" else self.gpu.DevIndex.open(self.gold.path(name + ".fmd"))
        return self.open[name]

    def want(self, name):
        if name not in self.ref:
            if name == "dup32":                                                    # no FASTQ: its sequences are read back from the index
                d = self.dev(name)
                n_seq = int(d.mcnt[1])
                seqs, ln, _ = d.retrieve(np.arange(n_seq, dtype=np.uint64), stride=256)
                assert int(ln.max()) <= 256
                fwd = [seqs[x, :ln[x]] for x in range(0, n_seq, 2)]                # sequence 2 i + 1 is the reverse complement of sequence 2 i
                assert np.array_equal(seqs[1, :ln[1]], hr.revcomp(fwd[0]))
            elif name == "synth":
                fwd = list(self.synth_reads())
            elif name == "cg":
                fwd = self.cg_reads()
            else:
                fwd = hr.forward_as_indexed(name)
            self.ref[name] = hr.Harvest(fwd)
        return self.ref[name]

    @staticmethod
    def synth_reads():
        return synth.reads(synth.DEFAULT_SEED + 17, 3000, coverage=2, err=0.01)   # 3000 reads of 100 bases with 1 % errors, thinly spread: most 17-mers are distinct

    def synth_index(self):
        return self.gpu.DevIndex.from_bwt(self.gpu.build_bwt(self.synth_reads()))

    @staticmethod
    def cg_reads():
        """C and G only, odd lengths (no read is its own reverse complement): the seeds A and T are empty"""
        rng = np.random.default_rng(5)
        genome = rng.integers(2, 4, size=300).astype(np.uint8)
        return [genome[p:p + ln].copy() for ln in (31, 45, 31, 63, 33, 31, 51, 31) * 6 for p in [int(rng.integers(0, 300 - ln + 1))]]

    def cg_index(self):
        return self.gpu.DevIndex.from_bwt(self.gpu.build_bwt(self.cg_reads()))

    def close(self):
        for d in self.open.values():
            d.close()


@pytest.fixture(scope="module")
def sets(gpu, gold):
    s = Sets(gpu, gold)
    yield s
    s.close()


def same(got, want, cnt_want):
    """(bucket, key, val, cnt) of a host form against the triples in the order it promises"""
    b, k, v, cnt = got
    assert b.dtype == np.uint32 and k.dtype == np.uint32 and v.dtype == np.uint8
    assert len(b) == len(want[0]) and list(cnt) == list(cnt_want), (len(b), len(want[0]), list(cnt), cnt_want)
    assert np.array_equal(b, want[0]) and np.array_equal(k, want[1]) and np.array_equal(v, want[2])


# ---- 1. every read set, every corner of the arguments ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hr.CASES + [hr.EMPTY_CASE], ids=lambda c: "w%d_o%d_s%d" % c)
@pytest.mark.parametrize("name", hr.NAMES)
def test_every_read_set(sets, monkeypatch, name, case):
    """one pass: sorted by (bucket, key); four parts: one sorted run per last base, in the order A, C, G, T"""
    w, mo, sl = case
    d, a = sets.dev(name), sets.want(name).answer(w, mo, sl)
    if case == hr.EMPTY_CASE:
        assert a.n == 0 and a.cnt == [0, 0]
    else:
        assert a.n > 0
    monkeypatch.setenv("FMD_KMER_PARTS", "1")
    same(d.kmer_collect(w, mo, sl), (a.bucket, a.key, a.val), a.cnt)
    monkeypatch.setenv("FMD_KMER_PARTS", "4")
    same(d.kmer_collect(w, mo, sl), a.in_parts([1, 2, 4, 8]), a.cnt)


def test_default_suf_len_is_compute_SUF(sets, monkeypatch):
    monkeypatch.setenv("FMD_KMER_PARTS", "1")
    d, h = sets.dev("special"), sets.want("special")
    for w, sl in ((15, 1), (16, 1), (17, 2), (27, 12)):
        a = h.answer(w, 1, sl)
        same(d.kmer_collect(w, 1), (a.bucket, a.key, a.val), a.cnt)


# ---- 2. shards --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case", [("special", (16, 1, 1)), ("special", (5, 3, 2)), ("repeat", (17, 3, 2)), ("repeat", (17, 3, 16))],
                         ids=lambda x: x if isinstance(x, str) else "w%d_o%d_s%d" % x)
def test_shards(sets, name, case):
    """fmd_kmer_collect_seeds, what `correct -g a,b,..` runs on each GPU: every mask against the brute force kept to that mask, cnt per shard"""
    w, mo, sl = case
    d, h = sets.dev(name), sets.want(name)
    for mask in range(1, 16):
        a = h.answer(w, mo, sl, mask)
        assert a.n > 0
        same(d.kmer_collect_seeds(w, mo, sl, mask), a.in_parts([1 << p for p in range(4) if mask >> p & 1]), a.cnt)
    b, k, v, cnt = d.kmer_collect_seeds(w, mo, sl, 0)                              # no seed: FMD_OK and nothing
    assert len(b) == 0 and len(k) == 0 and len(v) == 0 and list(cnt) == [0, 0]
    for bad in (0x10, 0x1f, 0x100, -1):
        with pytest.raises(api.FmdError, match=r"\(-2\)"):
            d.kmer_collect_seeds(w, mo, sl, bad)


def test_shards_with_empty_seeds(sets):
    """an index without A and T: two of the four roots have size 0 and are not seeded"""
    d, h = sets.dev("cg"), sets.want("cg")
    assert int(d.cnt[2] - d.cnt[1]) == 0 and int(d.cnt[5] - d.cnt[4]) == 0 and int(d.cnt[3] - d.cnt[2]) > 0
    for w, mo, sl in ((9, 1, 3), (17, 2, 2)):
        a = h.answer(w, mo, sl)
        assert a.n > 0
        same(d.kmer_collect_seeds(w, mo, sl, 0xf), a.in_parts([1, 2, 4, 8]), a.cnt)
        same(d.kmer_collect(w, mo, sl), (a.bucket, a.key, a.val), a.cnt)
        same(d.kmer_collect_seeds(w, mo, sl, 0x9), tuple(x[:0] for x in (a.bucket, a.key, a.val)), [0, 0])


# ---- 3. the dev form at a chosen capacity ---------------------------------------------------------------------------------------------------------
GUARD_BYTES = 4096


class Guarded:
    """a torch buffer of exactly n bytes with a patterned guard region behind it"""

    def __init__(self, n):
        import torch
        self.n = n
        self.t = torch.full((n + GUARD_BYTES,), 0x5A, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()

    def intact(self):
        return bool((self.t[self.n:] == 0x5A).all().item())

    def host(self, dtype, count):
        return self.t[:count * np.dtype(dtype).itemsize].cpu().numpy().view(dtype).copy()


def part_dev(gpu, d, w, mo, sl, mask, cap):
    """one fmd_kmer_collect_part_dev call on buffers of exactly the stated sizes -> (bucket, key, val, status) sorted by (bucket, key), guards checked"""
    import torch
    L = gpu.lib()
    wb = L.fmd_kmer_work_bytes(cap)
    work, db, dk, dv, ds = Guarded(wb), Guarded(4 * cap), Guarded(4 * cap), Guarded(cap), Guarded(32)
    torch.cuda.synchronize()
    rc = L.fmd_kmer_collect_part_dev(d.h, None, w, mo, sl, mask, work.ptr, wb, cap, db.ptr, dk.ptr, dv.ptr, ds.ptr)
    torch.cuda.synchronize()
    assert rc == api.FMD_OK, rc
    for g in (work, db, dk, dv, ds):
        assert g.intact(), cap
    status = [int(x) for x in ds.host(np.uint64, 4)]
    assert status[0] <= cap, (status, cap)
    n = status[0]
    b, k, v = db.host(np.uint32, n), dk.host(np.uint32, n), dv.host(np.uint8, n)
    o = np.lexsort([k, b])
    return b[o], k[o], v[o], status


def test_dev_form_at_odd_capacities(gpu, sets):
    """grown as the host grows it, but through odd capacities: r_flag then sits at byte 9 cap and the tile kernels take their tail path"""
    w, mo, sl = SYNTH
    d, h = sets.dev("synth"), sets.want("synth")
    a = h.answer(w, mo, sl)
    widest = int(h.level_counts(w, mo, sl).max())
    assert widest > 3 * MIN_CAP, widest                                            # the reference's own level counts: the first capacity cannot hold it
    cap, log, fitted = MIN_CAP, [], 0
    for call, step in enumerate((0, 1, 3, 2047, 2049, 1, 3, 2047, 2049, 1)):
        if call:
            cap = 2 * cap + step
        b, k, v, status = part_dev(gpu, d, w, mo, sl, 0xf, cap)
        log.append((cap, status[1] != 0))
        if call == 0:
            assert status[1] != 0
        if status[1] == 0:
            assert cap >= widest
            assert np.array_equal(b, a.bucket) and np.array_equal(k, a.key) and np.array_equal(v, a.val) and status[2:] == a.cnt and status[0] == a.n, cap
            fitted += 1
            if fitted == 2:                                                        # the first capacity that fits, and the next odd one
                break
        else:
            assert fitted == 0, log                                                # what fitted once fits when larger
    print("capacities (cap, overflowed):", log)
    assert fitted == 2 and cap % 8 != 0, log


def test_dev_form_one_seed(gpu, sets):
    """_part_dev with a single seed at an odd capacity, and _dev (all seeds) at the same one"""
    w, mo, sl = (16, 1, 1)
    d, h = sets.dev("special"), sets.want("special")
    for mask in (0x4, 0xf):
        a = h.answer(w, mo, sl, mask)
        cap = MIN_CAP + 2049                                                       # every wave that finds a child takes a chunk of its own: a small capacity
        for _ in range(8):                                                         # may overflow on a small trie too, and says so
            b, k, v, status = part_dev(gpu, d, w, mo, sl, mask, cap)
            if status[1] == 0:
                break
            cap = 2 * cap + 3
        assert status[1] == 0 and status[0] == a.n and status[2:] == a.cnt, cap
        assert np.array_equal(b, a.bucket) and np.array_equal(k, a.key) and np.array_equal(v, a.val)
    import torch
    L = gpu.lib()
    wb = L.fmd_kmer_work_bytes(cap)
    work, db, dk, dv, ds = Guarded(wb), Guarded(4 * cap), Guarded(4 * cap), Guarded(cap), Guarded(32)
    torch.cuda.synchronize()
    assert L.fmd_kmer_collect_dev(d.h, None, w, mo, sl, work.ptr, wb, cap, db.ptr, dk.ptr, dv.ptr, ds.ptr) == api.FMD_OK
    torch.cuda.synchronize()
    status = [int(x) for x in ds.host(np.uint64, 4)]
    assert all(g.intact() for g in (work, db, dk, dv, ds)) and status == [a.n, 0] + a.cnt
    assert np.array_equal(np.sort(db.host(np.uint32, a.n).astype(np.uint64) << np.uint64(32) | dk.host(np.uint32, a.n)),
                          a.bucket.astype(np.uint64) << np.uint64(32) | a.key)


def test_dev_form_arguments(gpu, sets):
    import torch
    L = gpu.lib()
    d = sets.dev("special")
    cap = MIN_CAP
    wb = L.fmd_kmer_work_bytes(cap)
    work, db, dk, dv, ds = Guarded(wb), Guarded(4 * cap), Guarded(4 * cap), Guarded(cap), Guarded(32)
    ok = dict(w=17, mo=1, sl=2, mask=0xf, wb=wb, cap=cap, h=d.h, work=work.ptr, db=db.ptr, dk=dk.ptr, dv=dv.ptr, ds=ds.ptr)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.fmd_kmer_collect_part_dev(a["h"], None, a["w"], a["mo"], a["sl"], a["mask"], a["work"], a["wb"], a["cap"], a["db"], a["dk"], a["dv"], a["ds"])
        torch.cuda.synchronize()
        return rc
    assert call() == api.FMD_OK
    for kw in (dict(cap=MIN_CAP - 1), dict(wb=wb - 1), dict(mask=0), dict(mask=0x10), dict(sl=17), dict(sl=18), dict(w=17, sl=1), dict(w=27, sl=11), dict(w=1, sl=1),
               dict(w=1, sl=0), dict(w=28, sl=13), dict(w=28, sl=16), dict(mo=0), dict(sl=0), dict(h=None), dict(work=None), dict(db=None), dict(dk=None),
               dict(dv=None), dict(ds=None)):
        assert call(**kw) == api.FMD_E_ARG, kw
    assert call(w=27, sl=12) == api.FMD_OK and call(w=16, sl=1) == api.FMD_OK and call(w=2, sl=1) == api.FMD_OK
    assert all(g.intact() for g in (work, db, dk, dv, ds))


# ---- 4. a bucket wider than 32 bits is refused, by the harvest and by the table that takes its triples ------------------------------------------
@pytest.mark.parametrize("sl", [17, 26])
def test_suf_len_beyond_16_is_refused(gpu, sets, sl):
    """w - suf_len <= 15 alone let these through, and the kernel cut the bucket to its low 32 bits without a word"""
    L = gpu.lib()
    d = sets.dev("special")
    with pytest.raises(api.FmdError, match=r"\(-2\)"):
        d.kmer_collect(27, 1, sl)
    with pytest.raises(api.FmdError, match=r"\(-2\)"):
        d.kmer_collect_seeds(27, 1, sl, 0x3)
    cap = MIN_CAP
    wb = L.fmd_kmer_work_bytes(cap)
    work, db, dk, dv, ds = Guarded(wb), Guarded(4 * cap), Guarded(4 * cap), Guarded(cap), Guarded(32)
    assert L.fmd_kmer_collect_part_dev(d.h, None, 27, 1, sl, 0xf, work.ptr, wb, cap, db.ptr, dk.ptr, dv.ptr, ds.ptr) == api.FMD_E_ARG
    assert L.fmd_kmer_collect_dev(d.h, None, 27, 1, sl, work.ptr, wb, cap, db.ptr, dk.ptr, dv.ptr, ds.ptr) == api.FMD_E_ARG
    bucket, key, val = np.zeros(4, dtype=np.uint32), np.arange(4, dtype=np.uint32) << 2, np.full(4, 9, dtype=np.uint8)
    t = C.c_void_p()
    assert L.fmd_ectab_build(0, 27, sl, 4, bucket.ctypes.data, key.ctypes.data, val.ctypes.data, C.byref(t)) == api.FMD_E_ARG and not t.value
    assert L.fmd_ectab_build_dev(0, None, 27, sl, 4, db.ptr, dk.ptr, dv.ptr, C.byref(t)) == api.FMD_E_ARG and not t.value
    assert L.fmd_ectab_build(0, 27, 16, 4, bucket.ctypes.data, key.ctypes.data, val.ctypes.data, C.byref(t)) == api.FMD_OK and t.value   # the last that fits
    L.fmd_ectab_free(t)


# ---- 5. regrowth in the host form; 6. the other frontier ranges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [1, 4])
def test_host_form_regrows(sets, monkeypatch, parts):
    """FMD_KMER_CAP0 = 65536 is far below the widest level: km_collect_part_host grows to demand + demand / 5 + 1024, no multiple of 8 or 2048"""
    w, mo, sl = SYNTH
    d, h = sets.dev("synth"), sets.want("synth")
    a = h.answer(w, mo, sl)
    masks = [0xf] if parts == 1 else [1, 2, 4, 8]
    for m in masks:
        assert int(h.level_counts(w, mo, sl, m).max()) > MIN_CAP                   # every part overflows its first capacity
    want = a.in_parts(masks)
    monkeypatch.setenv("FMD_KMER_PARTS", str(parts))
    monkeypatch.delenv("FMD_KMER_CAP0", raising=False)
    whole = d.kmer_collect(w, mo, sl)
    same(whole, want, a.cnt)
    monkeypatch.setenv("FMD_KMER_CAP0", str(MIN_CAP))
    same(d.kmer_collect(w, mo, sl), want, a.cnt)
    monkeypatch.setenv("FMD_KMER_CAP0", "1")                                       # clamped to 1 << 16, not refused
    same(d.kmer_collect(w, mo, sl), want, a.cnt)
    if parts == 4:
        same(d.kmer_collect_seeds(w, mo, sl, 0xa), a.in_parts([2, 8]), h.answer(w, mo, sl, 0xa).cnt)


@pytest.mark.parametrize("name,case", [("repeat", (17, 3, 2)), ("repeat", (5, 3, 2)), ("synth", SYNTH)], ids=lambda x: x if isinstance(x, str) else "w%d_o%d_s%d" % x)
def test_plain_frontier_ranges(sets, monkeypatch, name, case):
    """FMD_KMER_XCD=0, read per call: one stride over the whole frontier instead of one range per XCD"""
    w, mo, sl = case
    d, a = sets.dev(name), sets.want(name).answer(w, mo, sl)
    monkeypatch.setenv("FMD_KMER_PARTS", "1")
    for xcd in ("0", "1", "0"):
        monkeypatch.setenv("FMD_KMER_XCD", xcd)
        same(d.kmer_collect(w, mo, sl), (a.bucket, a.key, a.val), a.cnt)
    if name == "synth":
        monkeypatch.setenv("FMD_KMER_CAP0", str(MIN_CAP))
        same(d.kmer_collect(w, mo, sl), (a.bucket, a.key, a.val), a.cnt)
