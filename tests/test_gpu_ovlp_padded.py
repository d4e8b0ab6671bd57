"""GPU: overlap discovery (and SMEM, locate, k-mer counts) on a small REAL read set whose index lies beyond 2^32 positions -- tests/padded.py puts M filler
reads A^100 in front of the read set S, so that every C-, G- and T-starting suffix of S moves up by 202 M rows, the A-starting ones by 2 M + j M with the
length j of their A-run, the counts of A and T cross 2^32 while those of C and G do not, and the two sides (x0, x1) of one candidate lie on both sides of
2^32.  The results for the strands of S do not depend on the filler (no strand of a random genome holds A^40): only ids (by 2 M) and sequence ranks
(padded.Padding.map_rank) move.  Every number of a record that names a row is such a rank -- tests/test_padded_host.py shows that with the oracle alone --,
so the records stay below 2^32; what crosses it is everything the kernels hold in between: candidates, resume entries, list words.

  size   M x Lf           symbols        sentinels    -> DevIndex   handle in HBM            the oracle's file
  p32    2.2*10^7 x 100   4.45*10^9      4.4*10^7     < 0.1 s       9.1 GB (2.05 B/symbol)   0.8 s, 32 MB
  p33    5*10^7 x 100     1.01*10^10     10^8         < 0.1 s       15.2 GB (1.50)           1.9 s, 72 MB
  p34s   1.3*10^8 x 100   2.63*10^10     2.6*10^8     0.1 s         32.6 GB (1.24)           5.1 s, 187 MB
(one MI355X; the string itself is in HBM in under 0.1 s once the allocation is there, up to 3.7 s with it; the oracle's records of all strands take 0.3 s.
Every case prints its own figures as `[padded]` lines: pytest -s.  The whole module: 127 tests in 45 s.)

HBM while an index opens: the string, 1 byte per symbol, beside the handle made from it, at most 2.05 bytes per symbol as measured above; the RLE\6
stream of the oracle's file (n / 31 bytes for the filler's runs), tables and the work area of a job of ~10^4 strands are the fixed 6 GiB of the layout
seams' rule.  need_bytes = 3.1 bytes per symbol + 6 GiB; p33 and p34s skip only when the card has less than that free; p32 never skips.

The oracle's file: rows A^k $ for every k above the longest run of A in S follow one another with no row of S between them, so the BWT holds ONE run of
about 93 M equal symbols -- 2.0 * 10^9 at p32, 4.65 * 10^9 at p33, 1.2 * 10^10 at p34s --, and a block of an RLD\2 file counts its symbols in 31 bits.  The
writer (fermi_amd/host/rld_writer.c) writes such a run as several codes of the same symbol, which a reader takes as one run; tests/test_padded_host.py
holds that to the closed form without a GPU.

References: (1) the oracle on the padded index, loaded from a run-length file written once per index -- it never sees the plain string; (2) the SAME
kernels on the index of S alone, ids shifted and ranks moved: S unpadded is the 32-bit class that the md5 tests hold to the reference.  Compared: every
field of a record but `reserved` and `lfork` against the oracle (its lfork is exact where the product's may know less: include/fmd_hip.h; `reserved` where
check_left ran; `flags` -- FORKED and FIXED -- on the rows that are not flagged OVERFLOW, which the oracle, having no capacities, never sets), ALL fields against (2) and between the ways to run; neighbours up to n_nei; rows up to len + ext_len.
A comparison leaves out only rows flagged OVLP_F_OVERFLOW, at most 1 % (test_padded_host.py: by the oracle none at MAX_NEI = 8)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import orcbind
import ovlp_diff
import padded
from test_gpu_nei_lists import ENTRIES, FIGURES, SLOTS, STATS, _reads, _stderr_of
from test_gpu_nei_inline import LANE
from test_padded_host import CAP_SHARE, moved, set_b, set_c, small_set

pytestmark = pytest.mark.gpu
U64 = np.uint64
I64 = np.int64
L = 100
TWO32 = 1 << 32
SIZES = {"p32": (22_000_000, 100), "p33": (50_000_000, 100), "p34s": (130_000_000, 100)}
ORACLE_FIELDS = ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei", "flags")
SWITCHES = {"FMD_OVLP_FAST": "the general group kernels alone", "FMD_WALK_CLS": "lists by k_ovl_classify", "FMD_LANE_INLINE": "the lane rounds without the short cuts",
            "FMD_NEI_LANE": "the group-form fast kernel"}


def report(tag, **kv):
    print("[padded] %s: %s" % (tag, ", ".join("%s = %s" % (k, v) for k, v in kv.items())), flush=True)


def need_bytes(n):
    return int(3.1 * n) + (6 << 30)


class Base:
    """a read set and what the kernels give for it on its own index (the 32-bit class)"""

    def __init__(self, gpu, name):
        self.name = name
        self.reads = _reads() if name == "a" else set_b()
        self.bwt = gpu.build_bwt(self.reads)
        self.ids = np.arange(2 * len(self.reads), dtype=U64)
        self.runs, self.msgs = {}, {}
        self.o = orcbind.OrcIndex(bwt=self.bwt)
        self.want = {mm: self.o.overlap_batch(self.ids, mm, L, 8, 16, check_left=True) for mm in (40, 50)}
        d = gpu.DevIndex.from_bwt(self.bwt)
        saved = os.environ.get("FMD_OVLP_STATS")
        os.environ["FMD_OVLP_STATS"] = "1"
        try:
            for mm in (40, 50):
                self.runs[mm], self.msgs[mm] = _stderr_of(lambda: d.overlap_sorted(self.ids, mm, L, 8, 0, check_left=True))
        finally:
            if saved is None:
                os.environ.pop("FMD_OVLP_STATS")
            else:
                os.environ["FMD_OVLP_STATS"] = saved
            d.close()


_bases = {}


def base_of(gpu, name):
    if name not in _bases:
        _bases[name] = Base(gpu, name)
    return _bases[name]


class Padded:
    """one padded index: the device handle, the oracle on the same string, the ids of S's strands on it"""

    def __init__(self, gpu, base, size, tmp):
        import torch
        from fermi_amd import workload
        M, Lf = SIZES[size]
        self.size, self.base = size, base
        n = len(base.bwt) + 2 * M * (Lf + 1)
        free_b, _ = torch.cuda.mem_get_info()
        if size != "p32" and free_b < need_bytes(n):
            pytest.skip("HBM: %d bytes free, %s needs %d" % (free_b, size, need_bytes(n)))
        t0 = time.time()
        s, self.pad = padded.padded_bwt_device(base.bwt, M, Lf, torch.device("cuda", 0))
        torch.cuda.synchronize()
        t1 = time.time()
        fn = str(tmp / ("%s_%s.fmd" % (size, base.name)))
        workload.write_fmd_from_device_bwt(s.data_ptr(), self.pad.n, fn)
        t2 = time.time()
        self.d = gpu.DevIndex.from_bwt_dev(s.data_ptr(), self.pad.n, 0)
        del s
        torch.cuda.empty_cache()
        self.d.sync()
        torch.cuda.synchronize()
        t3 = time.time()
        self.o = orcbind.OrcIndex(fn=fn)
        t4 = time.time()
        self.ids = base.ids + U64(self.pad.id_shift)
        self.want = {}
        report("%s/%s" % (size, base.name), generation="%.1f s" % (t1 - t0), file="%.1f s (%d bytes, the longest run %d)" % (t2 - t1, os.path.getsize(fn), self.pad.longest_fill()), open="%.1f s" % (t3 - t2),
               oracle_load="%.1f s" % (t4 - t3), hbm_bytes=self.d.hbm_bytes, bytes_per_symbol="%.3f" % (self.d.hbm_bytes / self.pad.n), **self.pad.counts())

    def oracle(self, mm):
        """the oracle's records of every strand of S on the padded index, check_left_simple included (eight neighbours: the first of them are those of any smaller table)"""
        if mm not in self.want:
            t = time.time()
            by_form = moved(self.base.want[mm], self.pad)        # (the oracle on S alone, moved by the closed form: the same thing, test_padded_host.py)
            self.want[mm] = self.o.overlap_batch(self.ids, mm, L, 8, 16, check_left=True)
            assert ovlp_diff.same(self.want[mm][0], self.want[mm][1], by_form[0], by_form[1]) and np.array_equal(self.want[mm][2], by_form[2]), \
                ovlp_diff.explain(self.want[mm][0], self.want[mm][1], by_form[0], by_form[1], self.ids, what="the oracle on the file against the oracle on S, moved")
            report("%s/%s oracle -l%d" % (self.size, self.base.name, mm), seconds="%.1f" % (time.time() - t))
        return self.want[mm]

    def close(self):
        self.d.close(); self.o.close()


@pytest.fixture(scope="module", params=[(s, b) for s in SIZES for b in "ab"], ids=lambda p: "%s-%s" % p)
def px(request, gpu, oracle_lib, tmp_path_factory):
    size, name = request.param
    p = Padded(gpu, base_of(gpu, name), size, tmp_path_factory.mktemp("padded"))
    yield p
    p.close()


# ---------------------------------------------------------------------------------------------------------------------------- comparisons
def against(gpu, got, want, ids, max_nei, what, fields=ORACLE_FIELDS, strict_rows=False, capped=True):
    """records, neighbours and rows of `got` against `want` on every row that `got` does not flag; the rows left out: only flagged ones, at most 1 %, and
    none that the reference says fit (strict_rows: none at all; capped=False: the caller has held the flagged rows to the reference's, one by one)"""
    rec, nei, seq = got
    wrec, wnei, wseq = want
    over = (rec["flags"] & gpu.OVLP_F_OVERFLOW) != 0
    ok = ~over
    fits = wrec["n_nei"] <= max_nei
    msg = lambda: ovlp_diff.explain(rec, nei, wrec, wnei[:, :max_nei], ids, fields=fields, rows=ok, what=what)     # noqa: E731
    assert over.sum() <= CAP_SHARE * len(rec) or max_nei == 1 or not capped, "%s: %d of %d rows flagged\n%s" % (what, over.sum(), len(rec), msg())
    assert not (over & fits).any() and not (strict_rows and over.any()), "%s: %d rows flagged that fit %d neighbours, the first id %d\n%s" % (
        what, (over & fits).sum(), max_nei, ids[np.nonzero(over & fits)[0][:1]].sum(), msg())
    assert ovlp_diff.same(rec, nei, wrec, wnei[:, :max_nei], fields=fields, rows=ok), msg()
    used = (wrec["len"] + np.maximum(wrec["ext_len"], 0)).astype(I64)
    m = (np.arange(seq.shape[1])[None, :] < used[:, None]) & (ok & (wrec["status"] == 0))[:, None]
    bad = np.nonzero((seq != wseq)[:, :wseq.shape[1]] & m)[0]
    assert len(bad) == 0, "%s: the bases of %d rows differ, the first id %d\n%s" % (what, len(np.unique(bad)), ids[bad[0]], msg())
    return ok


def same_bytes(a, b, ids, max_nei, what):
    """two ways to run the same kernels: whole records, neighbours up to n_nei, rows up to len + ext_len"""
    assert ovlp_diff.same(a[0], a[1], b[0], b[1]), ovlp_diff.explain(a[0], a[1], b[0], b[1], ids, what=what)
    used = (b[0]["len"] + np.maximum(b[0]["ext_len"], 0)).astype(I64)
    m = (np.arange(b[2].shape[1])[None, :] < used[:, None]) & (b[0]["status"] == 0)[:, None]
    bad = np.nonzero(((a[2] != b[2]) & m).any(axis=1))[0]
    assert len(bad) == 0, "%s: the bases of %d rows differ, the first id %d\n%s" % (what, len(bad), ids[bad[0]], ovlp_diff.explain(a[0], a[1], b[0], b[1], ids, rows=np.isin(np.arange(len(ids)), bad[:10]), what=what))


def cut(run, max_nei):
    """the reference for a smaller neighbour table: the same records, the first max_nei neighbours"""
    return run[0], run[1][:, :max_nei], run[2]


# ---------------------------------------------------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("name", ["fixed", "ragged"])
@pytest.mark.parametrize("Lf", [1, 7, 100])
@pytest.mark.parametrize("M", [1, 3, 64])
def test_device_form_equals_the_host_form(gpu, name, M, Lf):
    """padded_bwt_device against padded_bwt_host, which test_padded_host.py holds to the BWT by sorting: byte for byte, the sentinels' alternating rows
    and every segment's place included"""
    import torch
    _, bwt_S = small_set(name)
    want, pad = padded.padded_bwt_host(bwt_S, M, Lf)
    got, pad_d = padded.padded_bwt_device(bwt_S, M, Lf, torch.device("cuda", 0))
    got = got.cpu().numpy()
    assert pad_d.n == pad.n == len(got) and np.array_equal(pad_d.ins, pad.ins)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%d rows differ, the first at %d: got %d, want %d" % (len(bad), bad[0], got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------------------------------------------------------------------- the index itself
def test_index_is_the_padded_one(px):
    """counts by the closed form; positions beyond 2^32 and below it in the same job; the oracle reads the same string"""
    pad, d = px.pad, px.d
    cnt_S = np.bincount(px.base.bwt, minlength=6).astype(I64)
    want = cnt_S + np.array([2 * pad.M, pad.M * pad.Lf, 0, 0, pad.M * pad.Lf, 0])
    assert d.n == pad.n and [int(v) for v in d.mcnt[1:7]] == want.tolist() and [int(v) for v in px.o.mcnt[1:7]] == want.tolist()
    assert pad.n > TWO32 and want[1] > TWO32 // 2 and want[2] < TWO32 and want[3] < TWO32
    rows = pad.map_pos(np.arange(pad.n_S)).astype(I64)
    # the C-, G- and T-starting rows of S lie behind the sentinels and every A^k $: M (Lf + 2) rows up.  That is beyond 2^32 at p33 and p34s; at p32 (2.24 * 10^9)
    # it is beyond 2^31, and only rows of the filler lie beyond 2^32
    edge = TWO32 if pad.M * (pad.Lf + 2) >= TWO32 else TWO32 // 2
    below, beyond = int((rows < edge).sum()), int((rows >= edge).sum())
    report("%s/%s rows of S" % (px.size, px.base.name), edge=edge, below=below, beyond=beyond)
    assert below > 1000 and beyond > pad.n_S // 2
    at = np.concatenate([np.arange(0, pad.n_S, max(1, pad.n_S // 5000)), [pad.n_S - 1]]).astype(I64)
    ok, sym = d.rank1a(rows[at].astype(U64))
    wk, ws = px.base.o.rank1a(at.astype(U64))                    # rank on S and the filler's rows in front, by the closed form
    wk = wk.astype(I64) + pad.occ_filler(at)
    assert np.array_equal(ok.astype(I64), wk) and np.array_equal(sym, ws)
    fk, fs = px.o.rank1a(rows[at].astype(U64))                   # ... and the oracle on the file
    assert np.array_equal(fk.astype(I64), wk) and np.array_equal(fs, ws)


# ---------------------------------------------------------------------------------------------------------------------------- overlap discovery
@pytest.mark.parametrize("max_nei", [8, 1])
@pytest.mark.parametrize("mm", [40, 50])
def test_sorted_job_and_id_order_equal_the_oracle(gpu, px, mm, max_nei):
    want = cut(px.oracle(mm), max_nei)
    got = px.d.overlap_sorted(px.ids, mm, L, max_nei, 0)
    tag = "%s/%s -l%d, %d neighbours" % (px.size, px.base.name, mm, max_nei)
    ok = against(gpu, got, want, px.ids, max_nei, tag + ", sorted job", strict_rows=max_nei == 8)
    one = px.d.overlap(px.ids, mm, L, max_nei, check_left=False)
    against(gpu, one, want, px.ids, max_nei, tag + ", id order")
    same_bytes(one, got, px.ids, max_nei, tag + ": id order against the sorted job")
    over = ~ok
    if max_nei == 1:                                             # the flag itself: a row is flagged exactly when it has a second neighbour
        assert np.array_equal(over, want[0]["n_nei"] > 1), "%s: %d rows flagged, %d have more than one neighbour" % (tag, over.sum(), (want[0]["n_nei"] > 1).sum())
        assert over.sum() > 100
    assert (want[0]["n_nei"] > 0).sum() > len(px.ids) // 4


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_every_way_to_run_equals_the_oracle(gpu, px, monkeypatch, switch):
    """FMD_OVLP_FAST=0, FMD_WALK_CLS=0, FMD_LANE_INLINE=0, FMD_NEI_LANE=0: each against the oracle, not merely against the default"""
    monkeypatch.setenv(switch, "0")
    # the switch is a switch: what FMD_OVLP_STATS says of one job under it (FMD_WALK_CLS chooses who fills the lists, which no figure shows)
    monkeypatch.setenv("FMD_OVLP_STATS", "1")
    _, msg = _stderr_of(lambda: px.d.overlap_sorted(px.ids, 40, L, 8, 0))
    monkeypatch.delenv("FMD_OVLP_STATS")
    fig, lane = [int(v) for v in STATS.findall(msg)[0]], [int(v) for v in LANE.findall(msg)[0]]
    if switch == "FMD_OVLP_FAST":
        assert fig[1] == 0 and lane[0] == 0, msg                  # nothing to the unforked path
    elif switch == "FMD_NEI_LANE":
        assert fig[1] > 0 and lane[0] == 0, msg                   # the unforked path without the lane kernel
    elif switch == "FMD_LANE_INLINE":
        assert lane[0] > 0 and lane[3] == 0 and lane[4] == 0 and lane[5] > 0, msg   # no self-end round inline, no closing past the loops
    for mm, max_nei in ((40, 8), (50, 8), (40, 1), (50, 1)):
        got = px.d.overlap_sorted(px.ids, mm, L, max_nei, 0)
        against(gpu, got, cut(px.oracle(mm), max_nei), px.ids, max_nei, "%s/%s -l%d, %d neighbours, %s=0 (%s)" % (px.size, px.base.name, mm, max_nei, switch, SWITCHES[switch]))


@pytest.mark.parametrize("mm", [40, 50])
def test_check_left_equals_the_oracle(gpu, px, mm):
    want = px.oracle(mm)
    got = px.d.overlap_sorted(px.ids, mm, L, 8, 0, check_left=True)
    tag = "%s/%s -l%d, check_left" % (px.size, px.base.name, mm)
    against(gpu, got, want, px.ids, 8, tag, fields=ORACLE_FIELDS + ("reserved",), strict_rows=True)
    assert (want[0]["reserved"] == 1).sum() > 0 and (want[0]["reserved"] == 0).sum() > 0


@pytest.mark.parametrize("mm", [40, 50])
def test_padding_moves_ids_and_ranks_only(gpu, px, mm):
    """the second reference: the same kernels on the index of S alone -- every field, flags and lfork included"""
    want = moved(px.base.runs[mm], px.pad)
    got = px.d.overlap_sorted(px.ids, mm, L, 8, 0, check_left=True)
    tag = "%s/%s -l%d against the index of S alone" % (px.size, px.base.name, mm)
    assert not ((want[0]["flags"] | got[0]["flags"]) & gpu.OVLP_F_OVERFLOW).any(), tag
    same_bytes(got, want, px.ids, 8, tag)


def test_flagged_rows_run_again_into_a_side_table(gpu, px):
    """room for 4 neighbours, then fmd_ovlp_rerun_overflow_dev with room for 16: the flagged rows are exactly those with more than 4 neighbours by the oracle,
    the side table holds exactly them, none is flagged again, and its rows are the oracle's"""
    Lb = gpu.lib()
    mm, max_nei, side_nei, side_cap = 40, 4, 16, 4096
    want = px.oracle(mm)
    ids, n = px.ids, len(px.ids)
    stride = 2 * L
    wb = max(Lb.fmd_ovlp_sorted_work_bytes(n, 0, L, mm), Lb.fmd_ovlp_side_work_bytes(side_cap, L, mm))
    rec = np.zeros(n, dtype=gpu.OVLP_DT); nei = np.zeros((n, max_nei), dtype=gpu.INTV_DT); seq = np.zeros((n, stride), dtype=np.uint8)
    s_ids = np.zeros(side_cap, dtype=U64); s_rows = np.zeros(side_cap, dtype=np.uint32); s_rec = np.zeros(side_cap, dtype=gpu.OVLP_DT)
    s_nei = np.zeros((side_cap, side_nei), dtype=gpu.INTV_DT); s_seq = np.zeros((side_cap, stride), dtype=np.uint8)
    host = [ids, rec, nei, seq, s_ids, s_rows, s_rec, s_nei, s_seq]
    ptrs = []
    try:
        for a in host + [None]:
            p = C.c_void_p()
            gpu.check(Lb.fmd_dev_malloc(px.d.device, wb if a is None else max(a.nbytes, 16), C.byref(p)))
            ptrs.append(p)
        for p, a in zip(ptrs, host):
            gpu.check(Lb.fmd_memcpy_h2d(p, a.ctypes.data, a.nbytes, None))
        d_ids, d_rec, d_nei, d_seq, d_sids, d_srows, d_srec, d_snei, d_sseq, d_work = ptrs
        gpu.check(Lb.fmd_ovlp_sorted_dev(px.d.h, None, n, d_ids, mm, L, max_nei, d_rec, d_nei, d_seq, stride, d_work, wb, 0))
        ns, still = C.c_uint64(), C.c_uint64()
        gpu.check(Lb.fmd_ovlp_rerun_overflow_dev(px.d.h, None, n, d_ids, d_rec, mm, L, side_nei, side_cap, d_sids, d_srows, d_srec, d_snei, d_sseq, stride, d_work, wb,
                                                 C.byref(ns), C.byref(still)))
        gpu.check(Lb.fmd_dev_sync(px.d.h, None))
        for p, a in zip(ptrs[1:], host[1:]):
            gpu.check(Lb.fmd_memcpy_d2h(a.ctypes.data, p, a.nbytes, None))
    finally:
        for p in ptrs:
            Lb.fmd_dev_free(p)
    tag = "%s/%s -l%d, 4 neighbours and the side table" % (px.size, px.base.name, mm)
    flagged = (rec["flags"] & gpu.OVLP_F_OVERFLOW) != 0
    more = want[0]["n_nei"] > max_nei
    assert more.sum() > 50 and want[0]["n_nei"].max() <= side_nei
    assert np.array_equal(flagged, more), "%s: %d rows flagged, %d have more than 4 neighbours by the oracle; ids flagged without: %s, not flagged with: %s" % (
        tag, flagged.sum(), more.sum(), ids[flagged & ~more][:10], ids[more & ~flagged][:10])
    k = int(ns.value)
    assert k == flagged.sum() and still.value == 0, (tag, k, int(flagged.sum()), still.value)
    order = np.argsort(s_rows[:k])
    rows = s_rows[:k][order].astype(I64)
    assert np.array_equal(rows, np.nonzero(flagged)[0]) and np.array_equal(s_ids[:k][order], ids[rows])
    against(gpu, cut((rec, nei, seq), max_nei), cut(want, max_nei), ids, max_nei, tag + ": the main table", capped=False)
    side = (s_rec[:k][order], s_nei[:k][order], s_seq[:k][order])
    w = (want[0][rows], np.concatenate([want[1][rows], np.zeros((k, side_nei - 8), dtype=gpu.INTV_DT)], axis=1), want[2][rows])
    assert want[0]["n_nei"][rows].max() <= 8                     # (the oracle was asked for eight)
    against(gpu, side, w, ids[rows], side_nei, tag + ": the side table", strict_rows=True)


def test_strands_take_the_paths_they_take_unpadded(px, monkeypatch):
    """FMD_OVLP_STATS: which list a strand goes to depends on its candidates' count, form and width -- none of which the padding changes -- so every figure
    about the lists' contents equals the unpadded run's, and every kind of list is reached"""
    monkeypatch.setenv("FMD_OVLP_STATS", "1")
    back = 0
    for mm in (40, 50):
        _, msg = _stderr_of(lambda: px.d.overlap_sorted(px.ids, mm, L, 8, 0, check_left=True))
        base_msg = px.base.msgs[mm]
        got, want = {}, {}
        for out, text in ((got, msg), (want, base_msg)):
            s, e, ln = STATS.findall(text), ENTRIES.findall(text), LANE.findall(text)
            assert len(s) == 1 and len(e) == 1 and len(ln) == 1, text
            out["figures"] = [int(v) for v in s[0]]; out["entries"] = [int(v) for v in e[0]]; out["lane"] = [int(v) for v in ln[0]]
        report("%s/%s -l%d paths" % (px.size, px.base.name, mm), padded=got, unpadded=want)
        for i, name in enumerate(FIGURES):
            if i != SLOTS:                                       # (slots count the holes of the chunked hand-over: they vary from run to run, test_gpu_nei_lists.py)
                assert got["figures"][i] == want["figures"][i], (name, got, want)
        assert got["entries"] == want["entries"] and got["lane"] == want["lane"], (got, want)
        n, unforked, handed_on, _, lane_at_once, handed_back, _ = got["figures"]
        assert n == len(px.ids) and unforked > 0 and handed_on > 0, got
        back += handed_back
        assert got["lane"][0] > 0                                 # admitted
        if px.base.name == "a":                                   # (set b has no window of more than 31 rows and no strand with more than 32 candidates on its own index either)
            assert got["lane"][1] > 0 and lane_at_once > 0 and got["entries"][0] > 0 and sum(got["entries"][1:]) > 0, (got, want)
    assert back > 0 or px.base.name == "b"                        # (handed back to the lane-per-strand kernel: a few strands of set a, none of set b on its own index either)


def test_forks_and_fix_ups_are_the_oracles(gpu, oracle_lib):
    """FORKED and FIXED on ragged reads with errors, where fake forks are fixed up (sets a and b have none; no padding here): the sorted job, the job in id
    order and the general group kernels alone against the oracle, whole records but `reserved` and `lfork` -- the comparison a benchmark leg makes when the
    reference binaries did not travel with the tree"""
    reads = set_c()
    bwt = gpu.build_bwt(reads)
    d = gpu.DevIndex.from_bwt(bwt)
    o = orcbind.OrcIndex(bwt=bwt)
    ids = np.arange(2 * len(reads), dtype=U64)
    try:
        for mm in (40, 30):
            want = o.overlap_batch(ids, mm, L, 8, 16, check_left=False)
            assert (want[0]["flags"] == 5).sum() > 10 and (want[0]["flags"] == 1).sum() > 100
            for what, got in (("sorted job", d.overlap_sorted(ids, mm, L, 8, 0)), ("id order", d.overlap(ids, mm, L, 8, check_left=False))):
                ok = against(gpu, got, want, ids, 8, "ragged reads with errors -l%d, %s" % (mm, what))
                g2 = got[0].copy(); g2["reserved"] = want[0]["reserved"]; g2["lfork"] = want[0]["lfork"]
                assert g2[ok].tobytes() == want[0][ok].tobytes() and got[1][ok].tobytes() == want[1][ok].tobytes(), \
                    ovlp_diff.explain(g2, got[1], want[0], want[1], ids, rows=ok, what="ragged reads with errors -l%d, %s, whole records and every neighbour slot" % (mm, what))
    finally:
        d.close(); o.close()


# ---------------------------------------------------------------------------------------------------------------------------- the other search kernels
@pytest.mark.parametrize("kernel", ["smem", "locate", "kmer_counts"])
def test_other_search_kernels_on_the_padded_handle(gpu, px, kernel):
    reads = px.base.reads
    rng = np.random.default_rng(11)
    if kernel == "smem":                                          # test_smem_vs_oracle_ragged's comparison, the oracle on the padded file
        qs = [r[int(rng.integers(0, 50)):][:int(rng.integers(1, 100))].copy() for r in reads[:300]]
        for q in qs[::3]:
            q[int(rng.integers(len(q)))] = int(rng.integers(1, 5))
        got = px.d.smem(qs, 0, max_mem=64)
        n_far = 0
        for q, m in zip(qs, got):
            w = px.o.smem(q, 0)
            assert m.tobytes() == w.tobytes(), "smem of %s: got %s, want %s" % (q.tolist(), m, w)
            n_far += int((w["x"][:, :2] >= U64(TWO32 if px.size != "p32" else TWO32 // 2)).any(axis=1).sum())
        report("%s/%s smem" % (px.size, px.base.name), matches_with_an_end_beyond_the_edge=n_far)
        assert n_far > len(qs) // 2                               # interval ends beyond 2^32 (p32: 2^31, where no row of S lies beyond 2^32)
    elif kernel == "locate":                                      # brute force over the strands of S; a sequence is named by its rank, which the oracle's records give
        from test_gpu_locate import Brute, hits_of
        strands = padded.strands_of(reads)
        b = Brute(strands)
        rank_of = px.oracle(40)[0]["rank"].astype(I64)
        qs = []
        for _ in range(200):
            r = strands[int(rng.integers(len(strands)))]
            ln = int(rng.integers(16, 61)); at = int(rng.integers(0, L - ln + 1))
            q = r[at:at + ln].copy()
            if rng.random() < 0.3:
                q[int(rng.integers(ln))] = int(rng.integers(1, 5))
            qs.append(q)
        cnt = px.d.backward_search(qs)[0]
        res = px.d.locate(qs, max_occ=int(cnt.max()) + 1)
        assert (cnt > 1).sum() > 100 and res[1].all()
        for i, q in enumerate(qs):
            want = sorted((int(rank_of[s]), p) for s, p in b.hits(q))
            assert int(cnt[i]) == len(want) and hits_of(res, i) == want, (i, q.tolist(), hits_of(res, i)[:5], want[:5])
    else:                                                         # the k-mers of S by brute force; the filler adds A^k alone (canonical: T^k is the same k-mer, packed 0), excluded by name
        from test_gpu_kcount import canonical_windows
        k = 24
        km, ct = np.unique(canonical_windows(list(reads), k), return_counts=True)
        assert not (km == 0).any()
        for min_occ in (1, 3):
            g_km, g_ct, st = px.d.kmer_counts(k, min_occ=min_occ)
            assert st["overflow"] == 0
            keep = g_km != 0
            assert (~keep).sum() == 1                             # A^24, from the filler
            w = ct >= min_occ
            assert np.array_equal(g_km[keep], km[w]) and np.array_equal(g_ct[keep].astype(I64), ct[w].astype(I64)), (k, min_occ)
