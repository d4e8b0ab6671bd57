"""GPU: the paths of k_ecfix (csrc/fmd_ecfix.hip) that the fixture's reads at w 17 do not reach -- lanes that take read after read from the ticket
queue (FMD_ECFIX_TEST_WAVES behind FMD_ECFIX_TEST_HOOKS=1), launches of fewer lanes than the gates wait for, other k-mer lengths and steps (the
batched hop's branches), reads round the staging limit at every alignment, a queue that fills and a trace that overflows on staged reads
(FMD_ECFIX_TEST_TRACE), the seams of the table's lines and the one triple the table cannot hold.  The reference of every test is the oracle's
ec_fix (oracle/ecfix_oracle.c, pinned to the reference's own function at these parameters by tests/test_ref_ecfix.py), and every comparison is
exact: bases, qualities and info words.  That the inputs reach the path a test is named after is asserted from the oracle's side (the largest
queue and trace of a read, orcbind.ec_fix(stats=True)), never from the kernel's."""
import ctypes as C

import numpy as np
import pytest

import orcbind
from test_gpu_parity import _odd_reads

pytestmark = pytest.mark.gpu
HOOK_VARS = ("FMD_ECFIX_TEST_HOOKS", "FMD_ECFIX_TEST_WAVES", "FMD_ECFIX_TEST_TRACE")
TRACE_FULL = np.int32(-2147483648)   # FMD_ECFIX_TRACE_FULL (include/fmd_hip.h)
_CACHE = {}


def _once(key, make):
    """inputs and the oracle's results: computed once, shared, left unchanged"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _flat(seqs, quals, spare=8):
    n = len(seqs)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in seqs], out=off[1:])
    s = np.concatenate([np.asarray(x, dtype=np.uint8) for x in seqs] + [np.zeros(spare, np.uint8)])
    q = np.concatenate([np.asarray(x, dtype=np.uint8) for x in quals] + [np.zeros(spare, np.uint8)])
    return s, q, off


class _Tab:
    """a device table of (bucket, key, val) triples and the two forms of the correction pass over it"""
    def __init__(self, gpu, w, bucket, key, val, lib=None):
        self.gpu, self.L, self.t = gpu, lib or gpu.lib(), C.c_void_p()
        bucket = np.ascontiguousarray(bucket, dtype=np.uint32); key = np.ascontiguousarray(key, dtype=np.uint32); val = np.ascontiguousarray(val, dtype=np.uint8)
        gpu.check(self.L.fmd_ectab_build(0, w, w - 15 if w > 15 else 1, len(key), bucket.ctypes.data, key.ctypes.data, val.ctypes.data, C.byref(self.t)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.L.fmd_ectab_free(self.t)

    def batch(self, seqs, quals, step, skip=0):
        """fmd_ecfix_batch over reads [skip, n): offsets that do not start at 0"""
        s, q, off = _flat(seqs, quals)
        n = len(seqs) - skip
        info = np.zeros(n, dtype=np.int32)
        self.gpu.check(self.L.fmd_ecfix_batch(self.t, n, s.ctypes.data, q.ctypes.data, off.ctypes.data + 8 * skip, step, info.ctypes.data))
        return s[: int(off[-1])], q[: int(off[-1])], off, info

    def dev(self, seqs, quals, step, trace_cap):
        """fmd_ecfix_dev on device arrays: no re-runs, a read whose trace does not fit gets FMD_ECFIX_TRACE_FULL"""
        import torch
        s, q, off = _flat(seqs, quals, spare=16)
        n = len(seqs)
        ds, dq, doff = torch.from_numpy(s).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        info = torch.zeros(n, dtype=torch.int32, device="cuda")
        wb = self.L.fmd_ecfix_work_bytes(self.t, n, trace_cap)
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.gpu.check(self.L.fmd_ecfix_dev(self.t, None, n, ds.data_ptr(), dq.data_ptr(), doff.data_ptr(), step, trace_cap, info.data_ptr(), work.data_ptr(), wb))
        torch.cuda.synchronize()
        return ds.cpu().numpy()[: int(off[-1])], dq.cpu().numpy()[: int(off[-1])], off, info.cpu().numpy()


def _same(got, want, what):
    assert np.array_equal(got[3], want[3]), (what, "info", np.flatnonzero(got[3] != want[3])[:8])
    assert np.array_equal(got[0], want[0]), (what, "bases")
    assert np.array_equal(got[1], want[1]), (what, "qualities")


def _same_reads(got, want, sel, what):
    """the reads `sel` (a mask) of two results over the same offsets"""
    off = want[2]
    byte = np.repeat(sel, np.diff(off).astype(np.int64))
    assert np.array_equal(got[3][sel], want[3][sel]), (what, "info")
    assert np.array_equal(got[0][byte], want[0][byte]) and np.array_equal(got[1][byte], want[1][byte]), (what, "bases / qualities")


def _hooks(monkeypatch, waves=None, trace=None):
    for k in HOOK_VARS:
        monkeypatch.delenv(k, raising=False)
    if waves is not None or trace is not None:
        monkeypatch.setenv("FMD_ECFIX_TEST_HOOKS", "1")
    if waves is not None:
        monkeypatch.setenv("FMD_ECFIX_TEST_WAVES", str(waves))
    if trace is not None:
        monkeypatch.setenv("FMD_ECFIX_TEST_TRACE", str(trace))


def _w17(gold):
    v = _once("solid", lambda: gold.npz("tiny_solid.npz"))
    return v["w17_o3_bucket"], v["w17_o3_key"], v["w17_o3_val"]


def _tiny_reads(gold):
    from test_oracle_golden import _fastq_records
    return _once("tiny", lambda: (gold.fastq_nt6("tiny.fq.gz"), [np.frombuffer(r[2], dtype=np.uint8) for r in _fastq_records(gold.text_gz("tiny.fq.gz"))]))


def _mixed(gold):
    """the 600 odd reads of test_ecfix_kernel_odd_reads_vs_oracle and the first 600 reads of tiny.fq, shuffled: short, all-N, seedless, 300-base
    and plain reads next to each other in ticket order"""
    def make():
        base, bq = _tiny_reads(gold)
        seqs, quals = _odd_reads(base)
        seqs, quals = seqs + [r.copy() for r in base[:600]], quals + [q.copy() for q in bq[:600]]
        order = np.random.default_rng(11).permutation(len(seqs))
        return [seqs[i] for i in order], [quals[i] for i in order]
    return _once("mixed", make)


def _mixed_want(gold, step):
    return _once(("mixed_want", step), lambda: orcbind.ec_fix(17, *_w17(gold), *_mixed(gold), step))


# ---------------------------------------------------------------------------------------------------------------- refill
@pytest.mark.parametrize("step", [5, 0])
def test_lanes_take_read_after_read(gpu, gold, oracle_lib, monkeypatch, step):
    """1, 2 and 3 waves for 1200 reads: every lane takes ~19, ~9, ~6 reads of every kind one after another (what a lane carries from one read to
    the next: staged / unstaged, the quality window, the trace piece, the first strand's word, the kept path, its slice of the queue), and the gates
    see lanes at different stages of different reads.  == the oracle == the uncapped run of the same process."""
    seqs, quals = _mixed(gold)
    want = _mixed_want(gold, step)
    with _Tab(gpu, 17, *_w17(gold)) as t:
        _hooks(monkeypatch)
        free = t.batch(seqs, quals, step)
        _same(free, want, "uncapped")
        for waves in (1, 2, 3):
            assert len(seqs) > 64 * waves * 4                      # every lane takes more than four reads
            _hooks(monkeypatch, waves=waves)
            got = t.batch(seqs, quals, step)
            _same(got, want, "waves %d" % waves)
            _same(got, free, "waves %d vs uncapped" % waves)
        # the cap is what sizes the launch: the work area is so many waves' slices (+ 256 bytes of alignment); with the gate shut the cap is not read
        def slices():
            return t.L.fmd_ecfix_work_bytes(t.t, len(seqs), 1024) - 256
        _hooks(monkeypatch)
        n_waves = (len(seqs) + 63) // 64
        per_wave = slices() // n_waves
        assert slices() == n_waves * per_wave and per_wave >= 64 * (1024 * 8 + 256 * 16)
        for waves in (1, 2, 3):
            _hooks(monkeypatch, waves=waves)
            assert slices() == waves * per_wave
        monkeypatch.setenv("FMD_ECFIX_TEST_HOOKS", "0")
        assert slices() == n_waves * per_wave


# ---------------------------------------------------------------------------------------------------------------- tiny launches
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 63, 64, 65])
def test_launches_smaller_than_the_gates(gpu, gold, oracle_lib, monkeypatch, n):
    """fewer lanes with work than EC_GATE_IN / EC_GATE_CL wait for (the gates must open when nobody is searching), one wave more or less full,
    one read beyond it: uncapped (two waves at n = 65) and with one wave (the 65th read is a refill)"""
    seqs, quals = _mixed(gold)
    full = _mixed_want(gold, 5)
    end = int(full[2][n])
    want = (full[0][:end], full[1][:end], full[2][: n + 1], full[3][:n])   # (reads are independent: the first n of the oracle's batch)
    with _Tab(gpu, 17, *_w17(gold)) as t:
        for waves in (None, 1):
            _hooks(monkeypatch, waves=waves)
            _same(t.batch(seqs[:n], quals[:n], 5), want, "n %d waves %s" % (n, waves))


# ---------------------------------------------------------------------------------------------------------------- k and step
def _table_of(gold, w):
    if w in (17, 21, 23):
        v = _once("solid", lambda: gold.npz("tiny_solid.npz"))
        tag = "w%d_o%d" % (w, 2 if w == 23 else 3)
        return v[tag + "_bucket"], v[tag + "_key"], v[tag + "_val"]

    def make():
        sl = w - 15 if w > 15 else 1
        o = orcbind.OrcIndex(gold.path("tiny.fmd"))
        B, K, V, _ = o.ec_range(w, 3, sl, 0, 1 << (2 * sl), 2)
        o.close()
        return B, K, V
    return _once(("table", w), make)


@pytest.mark.parametrize("w", [17, 21, 23, 11, 27])
def test_other_kmer_lengths_and_steps(gpu, gold, oracle_lib, w):
    """shift = 2 (w - 1) and the key packing x << 10 up to their limit at w 27; step 1 (no hop), 8 (the batched hop's full mask), 9 and 16
    (not batched), 0, 2 and 5, on 400 reads of tiny.fq and 100 of the odd kinds"""
    base, bq = _tiny_reads(gold)
    odd = _odd_reads(base)
    seqs, quals = base[:400] + odd[0][:100], bq[:400] + odd[1][:100]
    B, K, V = _table_of(gold, w)
    otab = _once(("otab", w), lambda: orcbind.ec_tab_new(w, B, K, V))     # (the oracle's table of w 27 has 2^24 buckets: built once)
    with _Tab(gpu, w, B, K, V) as t:
        for step in (0, 1, 2, 5, 8, 9, 16):
            want = orcbind.ec_fix(w, B, K, V, seqs, quals, step, tab=otab)
            fixed = want[3] & 0xffff
            assert ((fixed != 0) & (fixed != 0xffff)).sum() >= 20, (w, step)    # the cell corrects something
            _same(t.batch(seqs, quals, step), want, "w %d step %d" % (w, step))


# ---------------------------------------------------------------------------------------------------------------- lengths round the staging limit
def test_lengths_round_the_staging_limit_at_every_alignment(gpu, oracle_lib):
    """reads of 120..136 bases (EC_LDS_BASES = 128: staged up to 128, unstaged beyond) and of 16, 17, 18, 19, 33 (w = 17: too short, one
    k-mer, a few), in length order so that they start at every residue mod 16 (ec_stage_words' funnel shift, the 16-byte quality window, the
    batched hop's second word at base 127), 1 % substitutions and a few Ns; once more with offsets that do not start at 0"""
    from fermi_amd import synth
    rng = np.random.default_rng(23)
    src = synth.reads(synth.DEFAULT_SEED + 5, 660, 160, 40, 0.0)
    bwt = gpu.build_bwt(src)
    o = orcbind.OrcIndex(bwt=bwt)
    B, K, V, _ = o.ec_range(17, 3, 2, 0, 16, 2)
    o.close()
    assert len(B) > 2000
    lens = sorted(list(range(120, 137)) + [16, 17, 18, 19, 33])
    seqs, quals = [], []
    for i, ln in enumerate(np.repeat(lens, len(src) // len(lens))):
        a = int(rng.integers(0, 160 - ln + 1))
        r = src[i][a:a + ln].copy()
        flip = rng.random(ln) < 0.01
        r[flip] = (r[flip] - 1 + rng.integers(1, 4, int(flip.sum()))) % 4 + 1       # another base
        if i % 9 == 0:
            r[int(rng.integers(0, ln))] = 5
        seqs.append(r); quals.append(rng.integers(33, 78, ln).astype(np.uint8))
    off = np.concatenate([[0], np.cumsum([len(r) for r in seqs])])
    long_ = np.array([len(r) >= 120 for r in seqs])
    assert set((off[:-1][long_] % 16).tolist()) == set(range(16)) and set((off[:-1] % 4).tolist()) == set(range(4))
    with _Tab(gpu, 17, B, K, V) as t:
        for step in (5, 8):
            want = orcbind.ec_fix(17, B, K, V, seqs, quals, step)
            fixed = want[3] & 0xffff
            assert ((fixed != 0) & (fixed != 0xffff) & long_).sum() >= 100
            _same(t.batch(seqs, quals, step), want, "step %d" % step)
            got = t.batch(seqs, quals, step, skip=37)
            cut = int(want[2][37])
            assert np.array_equal(got[3], want[3][37:]) and np.array_equal(got[0][cut:], want[0][cut:]) and np.array_equal(got[1][cut:], want[1][cut:])
            s0, q0, _ = _flat(seqs[:37], quals[:37], spare=0)
            assert np.array_equal(got[0][:cut], s0) and np.array_equal(got[1][:cut], q0)     # the reads before the first offset are not touched


# ---------------------------------------------------------------------------------------------------------------- full queue, short trace
RECIPES = ["staged", "unstaged", "second"]


def _hard(gold, recipe):
    """the golden w 17 triples with the best base of a random 60 % replaced by another one, and reads with qualities uniform in 33..77: searches
    that fill the queue and need traces of thousands of entries.  staged: the first 300 reads of tiny.fq; unstaged: of the first 150, r, r reversed,
    r (300 bases: not staged in LDS); second: the staged reads, and half of the depth bytes say that a second base was seen 4..7 times -- the price
    of leaving the read's base (correct.c:164-171) is then often below the quality, and only then does the budget of correct.c:173-175 decide about
    the SECOND push too (the golden depth bytes price it at 39 and more, above every quality: that push always happens)"""
    def make():
        rng = np.random.default_rng(41)
        B, K, V = _w17(gold)
        K = K.copy()
        sel = rng.random(len(K)) < 0.6
        K[sel] = (K[sel] & ~np.uint32(3)) | ((K[sel] & np.uint32(3)) + rng.integers(1, 4, int(sel.sum())).astype(np.uint32)) % np.uint32(4)
        base = _tiny_reads(gold)[0]
        seqs = [np.concatenate([r, r[::-1], r]) for r in base[:150]] if recipe == "unstaged" else [r.copy() for r in base[:300]]
        quals = [rng.integers(33, 78, len(r)).astype(np.uint8) for r in seqs]
        if recipe == "second":
            rng = np.random.default_rng(43)
            V = V.copy()
            sel = rng.random(len(V)) < 0.5
            V[sel] = (V[sel] & 0xf8) | rng.integers(4, 8, int(sel.sum())).astype(np.uint8)
        return (B, K, V), seqs, quals
    return _once(("hard", recipe), make)


def _hard_want(gold, recipe, step):
    def make():
        tab, seqs, quals = _hard(gold, recipe)
        return orcbind.ec_fix(17, *tab, seqs, quals, step, stats=True)
    return _once(("hard_want", recipe, step), make)


def _assert_hard_floors(want):
    tmax, hmax = want[4], want[5]
    assert (hmax >= 255).sum() >= 50 and (tmax > 1024).sum() >= 50 and (tmax > 4096).sum() >= 20, \
        ((hmax >= 255).sum(), (tmax > 1024).sum(), (tmax > 4096).sum(), tmax.max())


@pytest.mark.parametrize("recipe", RECIPES)
def test_full_queue_and_long_trace_batch_form(gpu, gold, oracle_lib, monkeypatch, recipe):
    """the queue leaves LDS and reaches EC_MAX_HEAP (the budget rule of correct.c:173-175), the walk back crosses hundreds of trace pieces,
    fmd_ecfix_batch runs reads again: on reads staged in LDS, and on 300-base reads that are not.  (On the third recipe an oracle that applies the
    budget to the second push as the queue stood BEFORE the first one gives other bases or info words on 3 reads at step 5 and 7 at step 0, and
    other trace lengths on 109 and 111; on the first two it gives the same: measured when the test was written.)"""
    tab, seqs, quals = _hard(gold, recipe)
    _hooks(monkeypatch)
    with _Tab(gpu, 17, *tab) as t:
        for step in {"staged": (5, 2, 0), "unstaged": (5,), "second": (5, 0)}[recipe]:
            want = _hard_want(gold, recipe, step)
            if step == 5:
                _assert_hard_floors(want)
            _same(t.batch(seqs, quals, step), want, "step %d" % step)


@pytest.mark.parametrize("recipe", RECIPES)
def test_trace_overflow_with_refill(gpu, gold, oracle_lib, monkeypatch, recipe):
    """a first trace of 16 entries (re-runs at 64 .. 16 384 and beyond) on two waves: a lane that gave a read up must start the next one clean"""
    tab, seqs, quals = _hard(gold, recipe)
    want = _hard_want(gold, recipe, 5)
    _assert_hard_floors(want)
    assert len(seqs) > 64 * 2 and (want[4] > 16).sum() >= len(seqs) * 5 // 6      # lanes refill, and nearly every first attempt overflows
    with _Tab(gpu, 17, *tab) as t:
        _hooks(monkeypatch, waves=2, trace=16)
        _same(t.batch(seqs, quals, 5), want, "trace 16, 2 waves")
    if recipe != "staged":
        return
    # that the first capacity is indeed the hook's: the instrumented build probes more table slots when every read starts over three more times
    Lc = gpu.count_lib()
    assert Lc is not None, "libfmdhip_count.so is not built"
    probed = []
    with _Tab(gpu, 17, *tab, lib=Lc) as t:
        for trace in (None, 16):
            _hooks(monkeypatch, trace=trace)
            buf, counting = (C.c_uint64 * 3)(), C.c_int(0)
            gpu.check(Lc.fmd_ectab_line_count(t.t, buf, 1, C.byref(counting)))
            _same(t.batch(seqs, quals, 5), want, "instrumented build, trace %s" % trace)
            gpu.check(Lc.fmd_ectab_line_count(t.t, buf, 1, C.byref(counting)))
            assert counting.value == 1
            probed.append(int(buf[0]))
    assert probed[1] > probed[0] > 0, probed


def _tight_caps(want, n):
    """the trace of n reads whose queue was full, spread over them, rounded up to whole pieces of four entries"""
    full_q = np.flatnonzero(want[5] >= 255)
    picks = full_q[np.linspace(0, len(full_q) - 1, n).astype(np.int64)]
    return tuple(sorted({(int(want[4][i]) + 3) & ~3 for i in picks}))


@pytest.mark.parametrize("recipe", RECIPES)
def test_trace_full_word_of_the_device_form(gpu, gold, oracle_lib, monkeypatch, recipe):
    """fmd_ecfix_dev at trace_cap 16, 64, 1024: exactly the reads whose trace (root included) is longer than that, by the oracle's count, get
    FMD_ECFIX_TRACE_FULL; every other read is the oracle's"""
    tab, seqs, quals = _hard(gold, recipe)
    want = _hard_want(gold, recipe, 5)
    _assert_hard_floors(want)
    _hooks(monkeypatch)
    long_reads = recipe == "unstaged"
    with _Tab(gpu, 17, *tab) as t:
        caps = (16, 64, 1024) + ((65536,) if long_reads else (8192,))  # (every 300-base read of the recipe needs more than 16 384 entries, none 65 536)
        # ... and capacities that this or that read whose queue was full just fits (its trace rounded up to whole pieces of four entries): a path
        # pushed or dropped against the budget rule of correct.c:173-175 moves the read's trace count, whether or not it changes the read's result
        tight = _tight_caps(want, 2 if long_reads else 24)
        assert len(tight) >= (2 if long_reads else 12)
        for cap in caps + tight:
            got = t.dev(seqs, quals, 5, cap)
            over = want[4] > cap
            if cap in caps:
                assert (~over).sum() >= 10 if cap == caps[-1] else over.sum() >= 10, (cap, over.sum())
            assert np.array_equal(got[3] == TRACE_FULL, over), (cap, np.flatnonzero((got[3] == TRACE_FULL) != over)[:8])
            _same_reads(got, want, ~over, "cap %d" % cap)


def test_trace_capacity_is_rounded_down_to_whole_pieces(gpu, gold, oracle_lib, monkeypatch):
    """fmd_ecfix_dev at capacities that are no multiple of four: c + 1, c + 2, c + 3 over four of the tight values c of the test above (the
    first recipe, step 5; the work area sized by the number passed).  The kernel's capacity is that number rounded DOWN to whole trace pieces:
    exactly the reads whose oracle trace is longer than cap & ~3 get FMD_ECFIX_TRACE_FULL, every other read is the oracle's (a piece is four entries,
    EC_TR_LINE, in the build that ships: a variant built with another piece length rounds otherwise and fails here).  The values c are
    chosen from the oracle's counts so that the rounding is observed: first those with a read whose trace is longer than c but no longer than
    c + 3 -- a read that the unrounded capacity would have passed --, then others up to four."""
    tab, seqs, quals = _hard(gold, "staged")
    want = _hard_want(gold, "staged", 5)
    _assert_hard_floors(want)
    _hooks(monkeypatch)
    tmax = want[4].astype(np.int64)
    tight = _tight_caps(want, 24)
    between = [c for c in tight if ((tmax > c) & (tmax <= c + 3)).any()]
    cs = between + [c for c in tight if c not in between][: max(0, 4 - len(between))]
    caps = [c + k for c in cs for k in (1, 2, 3)]
    assert len(cs) >= 4 and all(c % 4 == 0 for c in cs)
    assert sum(bool(((tmax > (cap & ~3)) & (tmax <= cap)).any()) for cap in caps) >= 2, "no capacity whose rounding decides about a read"
    with _Tab(gpu, 17, *tab) as t:
        for cap in caps:
            got = t.dev(seqs, quals, 5, cap)
            over = tmax > (cap & ~3)
            assert np.array_equal(got[3] == TRACE_FULL, over), (cap, np.flatnonzero((got[3] == TRACE_FULL) != over)[:8])
            _same_reads(got, want, ~over, "cap %d" % cap)


# ---------------------------------------------------------------------------------------------------------------- table seams
def _np_ec_hash(x):
    """ec_hash (fmd_ecfix.hip): the splitmix64 finaliser"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return x ^ (x >> np.uint64(31))


def _seam_case():
    """w 11, 512 triples in 1024 slots = 128 lines of eight: 20 k-mers whose home line is the last one (they spill through line 0 into line 1),
    12 each at home in line 0 and line 63, the rest at random; 200 reads of 100 bases made of table k-mers, each behind a copy of its own first
    base (the base the look-up of that k-mer is compared with), every seam k-mer in >= 3 reads"""
    def make():
        rng = np.random.default_rng(53)
        allx = np.arange(1 << 22, dtype=np.uint64)
        home = (_np_ec_hash(allx) & np.uint64(127)).astype(np.int64)
        seam = np.concatenate([rng.choice(allx[home == 127], 20, replace=False), rng.choice(allx[home == 0], 12, replace=False), rng.choice(allx[home == 63], 12, replace=False)])
        rest = rng.choice(np.setdiff1d(allx, seam), 512 - len(seam), replace=False)
        x = np.concatenate([seam, rest])
        first = (x >> np.uint64(20)).astype(np.uint32)                              # the k-mer's first base (the last one shifted in)
        best = np.where(np.arange(len(x)) % 2 == 0, first, (first + rng.integers(1, 4, len(x)).astype(np.uint32)) % 4)
        val = rng.integers(0, 256, len(x)).astype(np.uint8)
        deep = np.arange(len(x)) % 4 < 2
        val[deep] = (rng.integers(5, 32, int(deep.sum())) << 3).astype(np.uint8)     # val & 7 == 0, depth >= 5: hops start
        B = (x & np.uint64(3)).astype(np.uint32)
        K = ((x >> np.uint64(2)).astype(np.uint32) << np.uint32(2)) | best.astype(np.uint32)
        bases = ((x[:, None] >> (np.uint64(2) * np.arange(10, -1, -1, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.uint8) + 1   # in read order
        seqs, quals, uses = [], [], np.zeros(len(x), dtype=np.int64)
        for r in range(200):
            pick = rng.integers(0, len(x), 8)
            pick[0], pick[4] = (2 * r) % len(seam), (2 * r + 1) % len(seam)
            uses[pick] += 1
            unit = [np.concatenate([bases[k][:1], bases[k]]) for k in pick]
            seqs.append(np.concatenate(unit + [rng.integers(1, 5, 4).astype(np.uint8)]))
            quals.append(rng.integers(33, 78, 100).astype(np.uint8))
        return (B, K, val), x, home[x.astype(np.int64)], len(seam), uses, seqs, quals
    return _once("seam", make)


def test_table_line_seams_and_wrap(gpu, oracle_lib):
    """look-ups that go on from a full line to the next, and from the last line round to line 0 ((ln + 1) & lmask)"""
    tab, x, home, n_seam, uses, seqs, quals = _seam_case()
    assert len(x) == 512 and len(np.unique(x)) == 512                               # 1024 slots: 128 lines
    assert (home == 127).sum() >= 17 and (home == 0).sum() >= 9 and (home == 63).sum() >= 9
    assert (uses[:n_seam] >= 3).all() and all(len(r) == 100 for r in seqs)
    with _Tab(gpu, 11, *tab) as t:
        for step in (5, 0):
            want = orcbind.ec_fix(11, *tab, seqs, quals, step)
            s0, _, off = _flat(seqs, quals, spare=0)
            changed = np.add.reduceat((want[0] != s0).astype(np.int64), off[:-1].astype(np.int64)) > 0
            assert changed.sum() >= 100, changed.sum()
            bare = orcbind.ec_fix(11, *(a[n_seam:] for a in tab), seqs, quals, step)         # the seam entries are observed: without them ...
            assert ((bare[3] != want[3]) | (np.add.reduceat((bare[0] != want[0]).astype(np.int64), off[:-1].astype(np.int64)) > 0)).sum() >= 50
            _same(t.batch(seqs, quals, step), want, "step %d" % step)


# ---------------------------------------------------------------------------------------------------------------- the triple the table cannot hold
def _poly_case(gold):
    """w 27: every 100th triple of the oracle's table of tiny.fmd, the 27-mer of 27 As, and the 27-mer of 27 Ts with best base T and depth byte
    255 (table A: the one entry that equals EC_EMPTY, kept as a flag) or 254 (table B: an ordinary entry); 64 reads of tiny.fq with a run of
    28..40 Ts and 64 with a run of As (the other strand's Ts) in them, low qualities round the runs"""
    def make():
        rng = np.random.default_rng(67)
        B, K, V = _table_of(gold, 27)
        B, K, V = B[::100], K[::100], V[::100]
        assert 150 <= len(B) <= 250
        tabs = []
        for v_t in (255, 254):
            tabs.append((np.concatenate([B, [0, (1 << 24) - 1]]).astype(np.uint32), np.concatenate([K, [0, 0xffffffff]]).astype(np.uint32),
                         np.concatenate([V, [5 << 3, v_t]]).astype(np.uint8)))
        base = _tiny_reads(gold)[0]
        seqs, quals = [], []
        for i in range(128):
            r = base[1000 + i].copy()
            run = int(rng.integers(28, 41))
            a = int(rng.integers(1, len(r) - run - 1))
            r[a:a + run] = 4 if i < 64 else 1
            r[a - 1] = 1 + (i % 3) if i < 64 else 2 + (i % 3)                        # the run ends there
            r[a + run] = 1 + ((i + 1) % 3) if i < 64 else 2 + ((i + 1) % 3)
            seqs.append(r); quals.append(rng.integers(33, 78, len(r)).astype(np.uint8))
        return tabs, seqs, quals
    return _once("poly", make)


def test_the_triple_that_equals_the_empty_slot(gpu, gold, oracle_lib):
    """EC_FULL_FLAG: the all-T 27-mer with depth byte 255 and best base T is answered from the flag, with 254 from its slot; the all-A 27-mer
    is x = 0, the smallest entry"""
    tabs, seqs, quals = _poly_case(gold)
    wants = [orcbind.ec_fix(27, *tab, seqs, quals, 5) for tab in tabs]
    differ = (wants[0][3] != wants[1][3]) | (np.add.reduceat((wants[0][0] != wants[1][0]).astype(np.int64), wants[0][2][:-1].astype(np.int64)) > 0)
    assert differ.sum() >= 1, "the depth byte of the all-T k-mer is not observed"
    for tab, want, name in zip(tabs, wants, "AB"):
        with _Tab(gpu, 27, *tab) as t:
            _same(t.batch(seqs, quals, 5), want, "table " + name)
