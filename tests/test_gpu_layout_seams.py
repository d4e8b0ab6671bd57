"""GPU: the three places of the device index where a wider number is packed into a narrower field, each crossed in seconds and compared with a closed form.

  1. bits 32..39 of the per-block symbol counts (fmd_wave.h: one byte each for $, A, C, G in meta_5, T's in meta_6; unpacked by hand in fmd_block_rank6,
     fmd_block_rank1, fmd_block_rank1z and pair_abs of fmd_pair.hip).  Below 2^32 occurrences of every symbol all five are zero, and on an index of uniform
     composition (tests/test_gpu_cfg5.py, tools/huge_index_check.py) the four bases' bytes are equal almost everywhere: reading C's byte for G, or shifting
     by the wrong multiple of 8, passes there.  Case A makes ONE symbol cross 2^32 while the others stay below it.
  2. the 28-bit pair counts of a two-base block and pair_tab's row per superblock of 2^28 positions (written by k_pair_counts; decoded again by
     k_bsearch_pair, by the overlap walk and by k_pair_check).  Case B crosses five superblock ends with a pair whose count sets bit 27 of its field;
     case C makes all sixteen counts differ.
  3. the checks of those fields that existed compare device code with device code (fmd_dev_check_rank, fmd_dev_check_pairs).

The reference is tests/periodic.py: the index is made from a periodic string that is not the BWT of anything, whose counts are exact arithmetic -- rank, LF,
fm6_extend and the backward-search recurrence do not care.  Every case prints its wall times and the counts of its input conditions (pytest -s shows them)."""
import ctypes as C
import time

import numpy as np
import pytest

import periodic
from periodic import Periodic

pytestmark = pytest.mark.gpu
U64 = np.uint64
I64 = np.int64
SB = 1 << 28                                  # positions of a pair superblock (FMD_PAIR_SB_SHIFT + 5)
TWO32 = 1 << 32
N_PATTERNS = 200_000
NAMES = "$ACGTN"

N_A = -(-(TWO32 * 16 * 100) // (15 * 85))     # ceil(2^32 / (15/16) / 0.85): the heavy symbol's count crosses 2^32 at about 85 % of the string
N_B = 5 * SB + 12345                          # five full superblocks and a short sixth
N_C = 2 * SB + 12345


def table_depth(n):
    """the depth of the prefix table an index of n symbols gets (build_ptab, fmd_index.hip): a search of at least that many bases starts that far in"""
    d = 2
    while d < 14 and (1 << (2 * (d + 1))) <= n // 8 and n < (1 << (64 - 2 * (d + 1))) - 1:
        d += 1
    return d


class Case:
    """one index: the string, the patterns searched in it, and what the reference says about both (no GPU: the input conditions are checked here)"""

    def __init__(self, kind, c):
        self.kind, self.c = kind, c
        if kind == "A":
            shares, self.n = periodic.heavy_shares(c, 15 / 16), N_A
        elif kind == "B":
            shares, self.n = periodic.heavy_shares(c, 0.75), N_B
        else:
            shares, self.n = np.array([0.4, 0.3, 0.2, 0.1, 0.0]), N_C
        seed = {"A": 100, "B": 200, "C": 300}[kind] + c
        self.per = Periodic(periodic.make_pattern(shares, seed), self.n)
        self.pairs = not (kind == "A" and c == 5)               # the N-heavy string is ranked and extended only
        self.ref = None
        if self.pairs:
            rng = np.random.default_rng(seed + 1000)
            self.pats, self.lens = periodic.draw_patterns(rng, N_PATTERNS, self.per.comp[1:5])
            # eligible steps by the hand-over rule alone, and those among them that the device can take (its searches start `table_depth` bases in)
            self.ref_rule = self.per.backward_search(self.pats, self.lens)
            self.ref = self.per.backward_search(self.pats, self.lens, table_depth=table_depth(self.n))
            assert all(np.array_equal(self.ref[k], self.ref_rule[k]) for k in ("hit", "k", "l"))

    def need_bytes(self):
        """HBM this case wants free: string + rank blocks ~2 bytes per symbol; with two-base blocks 4 more per symbol, ~0.75 for their construction, and
        what fmd_pairs_ensure keeps clear beside them (the index once more, 8 GiB); the tables and work areas: 6 GiB"""
        b = 2 * self.n + (6 << 30)
        if self.pairs:
            b = max(b, int(6.75 * self.n) + (14 << 30))
        return b


_cases = {}


def case(kind, c):
    if (kind, c) not in _cases:
        _cases[(kind, c)] = Case(kind, c)
    return _cases[(kind, c)]


def report(tag, **kv):
    print("[layout seams] %s: %s" % (tag, ", ".join("%s = %s" % (k, v) for k, v in kv.items())), flush=True)


class Clock:
    def __init__(self):
        self.t = time.time(); self.parts = {}

    def lap(self, name):
        import torch
        torch.cuda.synchronize()
        now = time.time()
        self.parts[name] = self.parts.get(name, 0.0) + now - self.t
        self.t = now

    def __str__(self):
        return ", ".join("%s %.1f s" % kv for kv in self.parts.items()) + ", all %.1f s" % sum(self.parts.values())


def open_index(gpu, cs, clock):
    """the case's string in HBM -> DevIndex; the string is gone before anything is checked.  The only skip of this file: the card (shared) is short of memory."""
    import torch
    free_b, _ = torch.cuda.mem_get_info()
    if free_b < cs.need_bytes():
        pytest.skip("HBM: %d bytes free, the case needs %d" % (free_b, cs.need_bytes()))
    dev = torch.device("cuda", 0)
    s = cs.per.device_string(dev)
    clock.lap("generation")
    d = gpu.DevIndex.from_bwt_dev(s.data_ptr(), cs.n, 0)
    del s
    torch.cuda.empty_cache()
    clock.lap("open")
    return d


def check_counts(d, per):
    assert [int(v) for v in d.mcnt] == [per.n] + [int(v) for v in per.mcnt]
    assert [int(v) for v in d.cnt] == [int(v) for v in per.cnt]


def windows(per, centres, w):
    return np.concatenate([np.arange(max(0, p - w), min(per.n - 1, p + w) + 1, dtype=I64) for p in centres])


def check_rank1a(d, per, ks):
    ok, sym = d.rank1a(ks.astype(U64))
    want = per.occ(ks)
    bad = np.nonzero((ok.astype(I64) != want).any(axis=1))[0]
    assert len(bad) == 0, "rank1a: %d of %d positions differ, the first at %d: got %s, want %s" % (len(bad), len(ks), ks[bad[0]], ok[bad[0]], want[bad[0]])
    assert np.array_equal(sym.astype(np.uint8), per.sym(ks)), "rank1a: the symbol"
    return want


FIXED_GAPS = np.array([0, 1, 31, 32, 33, 63, 64, 95, 96, 97], dtype=I64)


def check_rank2a(d, per, ks, ls, what):
    gk, gl = d.rank2a(ks.astype(U64), ls.astype(U64))
    for side, got, pos in (("k", gk, ks), ("l", gl, ls)):
        want = per.occ(pos)
        bad = np.nonzero((got.astype(I64) != want).any(axis=1))[0]
        assert len(bad) == 0, "rank2a (%s), %s side: %d of %d differ, the first at k = %d, l = %d: got %s, want %s" % (
            what, side, len(bad), len(ks), ks[bad[0]], ls[bad[0]], got[bad[0]], want[bad[0]])


def check_extend(gpu, d, per, x0, x1, rng):
    m = len(x0)
    x = np.zeros((m, 3), dtype=I64)
    x[:, 2] = rng.integers(1, 101, m)
    x[:, 0] = np.minimum(x0, per.n - x[:, 2])                   # the interval ends inside the string
    x[:, 1] = np.minimum(x1, per.n - x[:, 2])
    is_back = rng.integers(0, 2, m).astype(np.uint8)
    iks = np.zeros(m, dtype=gpu.INTV_DT)
    iks["x"] = x.astype(U64)
    got = d.extend(iks, is_back)["x"].astype(I64)
    want = per.extend(x, is_back)
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert len(bad) == 0, "extend: %d of %d differ, the first: x = %s, is_back = %d, got %s, want %s" % (len(bad), m, x[bad[0]], is_back[bad[0]], got[bad[0]], want[bad[0]])


def check_search(d, cs, what):
    ref = cs.ref
    reads = [cs.pats[i, :cs.lens[i]] for i in range(len(cs.lens))]
    cnt, beg, end = d.backward_search(reads)
    hit = ref["hit"]
    wrong = np.nonzero((cnt > 0) != hit)[0]
    assert len(wrong) == 0, "backward search (%s): %d of %d patterns hit where they must not or the reverse, the first: %d" % (what, len(wrong), len(hit), wrong[0])
    bad = np.nonzero(hit & ((beg.astype(I64) != ref["k"]) | (end.astype(I64) != ref["l"]) | (cnt.astype(I64) != ref["l"] - ref["k"] + 1)))[0]
    assert len(bad) == 0, "backward search (%s): %d of %d hits have another interval, the first: pattern %d, got [%d, %d], want [%d, %d]" % (
        what, len(bad), int(hit.sum()), bad[0], beg[bad[0]], end[bad[0]], ref["k"][bad[0]], ref["l"][bad[0]])


def check_searches_and_pairs(gpu, d, cs, monkeypatch, clock):
    """the same patterns without the two-base blocks and with them, and every row's pair step against two single steps"""
    monkeypatch.setenv("FMD_PAIR", "0")
    check_search(d, cs, "FMD_PAIR=0")
    clock.lap("checks")
    monkeypatch.setenv("FMD_PAIR", "1")
    assert d.build_pairs() is True
    clock.lap("pairs")
    check_search(d, cs, "FMD_PAIR=1")
    assert d.check_pairs() == (0, 0)
    clock.lap("checks")


def pair_lines_of_the_counting_build(gpu, cs, monkeypatch):
    """the FMD_PAIR=1 search once more on a handle of the instrumented build: the number of two-base blocks its kernels asked for (None: no such build here)"""
    import torch
    Lc = gpu.count_lib()
    if Lc is None:
        return None
    monkeypatch.setenv("FMD_PAIR", "1")
    s = cs.per.device_string(torch.device("cuda", 0))
    h = C.c_void_p()
    assert Lc.fmd_dev_open_bwt_dev(0, s.data_ptr(), cs.n, C.byref(h)) == 0
    del s
    torch.cuda.empty_cache()
    try:
        buf, counting, built = (C.c_uint64 * 3)(), C.c_int(0), C.c_int(0)
        assert Lc.fmd_dev_build_pairs(h, C.byref(built)) == 0 and built.value
        assert Lc.fmd_dev_line_count3(h, buf, 1, C.byref(counting)) == 0 and counting.value
        flat, off = gpu.flatten_reads([cs.pats[i, :cs.lens[i]] for i in range(len(cs.lens))])
        m = len(off) - 1
        cnt, beg, end = (np.zeros(m, dtype=U64) for _ in range(3))
        assert Lc.fmd_bsearch_batch(h, m, flat.ctypes.data, off.ctypes.data, cnt.ctypes.data, beg.ctypes.data, end.ctypes.data) == 0
        assert Lc.fmd_dev_line_count3(h, buf, 1, C.byref(counting)) == 0
        assert np.array_equal(cnt > 0, cs.ref["hit"])
        return int(buf[2])
    finally:
        Lc.fmd_dev_close(h)


# ------------------------------------------------------------------------------------------------------------ case A: the high count bytes
@pytest.mark.parametrize("c", [1, 2, 3, 4, 5], ids=list("ACGTN"))
def test_one_symbol_beyond_2_to_32(gpu, monkeypatch, c):
    """15/16 of the string is symbol c: its count crosses 2^32 at ~85 % of the string and its high byte is 1 from there, all others stay 0 -- rank1a,
    rank2a and extend against the closed form at random positions and around the crossing, position 2^32 and both ends; for a base, backward search
    without and with the two-base blocks (built by pair_abs from counts beyond 2^32) and fmd_dev_check_pairs."""
    cs = case("A", c)
    per, n = cs.per, cs.n
    cross = per.crossing(c, TWO32)
    assert cross is not None and 0.8 * n < cross < 0.9 * n
    assert all(int(per.mcnt[b]) < TWO32 for b in range(6) if b != c)          # c's byte is 1 where every other one is 0
    beyond = None
    if cs.pairs:
        hits = int(cs.ref["hit"].sum())
        beyond_rule = int((cs.ref_rule["step_k"] >= cross).sum())
        beyond = int((cs.ref["step_k"] >= cross).sum())
        report("A/%s inputs" % NAMES[c], n=n, crossing=cross, hits="%d of %d" % (hits, N_PATTERNS), eligible_steps=len(cs.ref_rule["step_k"]),
               eligible_beyond_the_crossing=beyond_rule, behind_the_prefix_table=len(cs.ref["step_k"]), those_beyond_the_crossing=beyond)
        assert hits >= N_PATTERNS // 4
        if c == 1:
            assert beyond_rule >= 50_000 and beyond >= 50_000
    clock = Clock()
    d = open_index(gpu, cs, clock)
    try:
        check_counts(d, per)
        rng = np.random.default_rng(10 + c)
        near = np.concatenate([windows(per, [cross, TWO32, n - 1], 200), np.arange(0, 3001, dtype=I64)])
        ks = np.concatenate([rng.integers(0, n, 1_000_000), near]).astype(I64)
        want = check_rank1a(d, per, ks)
        n_high = int((want[:, c] >= TWO32).sum())
        # rank2a: at the same k, every fixed gap at every position of the windows, fixed and random gaps at the random positions
        gap = np.where(np.arange(len(ks)) % 2 == 0, FIXED_GAPS[(np.arange(len(ks)) // 2) % len(FIXED_GAPS)], rng.integers(0, 5001, len(ks)))
        check_rank2a(d, per, ks, np.minimum(ks + gap, n - 1), "random positions and the windows")
        kk = np.repeat(near, len(FIXED_GAPS)); ll = np.minimum(kk + np.tile(FIXED_GAPS, len(near)), n - 1)
        check_rank2a(d, per, kk, ll, "every fixed gap at every position of the windows")
        # extend: half of the ends from the windows
        m = 200_000
        x0, x1 = (np.where(rng.random(m) < 0.5, rng.choice(near, m), rng.integers(0, n, m)) for _ in range(2))
        check_extend(gpu, d, per, x0, x1, rng)
        clock.lap("checks")
        if cs.pairs:
            check_searches_and_pairs(gpu, d, cs, monkeypatch, clock)
    finally:
        d.close()
    report("A/%s" % NAMES[c], times=clock, rank1a_positions=len(ks), with_count_of_c_at_least_2_to_32=n_high)
    assert n_high > 100_000 and (want[:, c] < TWO32).sum() > 500_000


# ------------------------------------------------------------------------------------------------------------ cases B and C: the pair fields
def superblock_conditions(cs, cc_pair=None):
    """from the reference alone: where the pair-eligible steps the device can take start"""
    k = cs.ref["step_k"]
    sbs = np.bincount(k // SB, minlength=(cs.n - 1) // SB + 1)
    out = {"hits": "%d of %d" % (int(cs.ref["hit"].sum()), N_PATTERNS), "eligible_steps": len(cs.ref_rule["step_k"]), "behind_the_prefix_table": len(k),
           "per_superblock": sbs.tolist()}
    if cc_pair is not None:
        for name, ref in (("rule", cs.ref_rule), ("device", cs.ref)):
            cc = (ref["step_c1"] == cc_pair) & (ref["step_c2"] == cc_pair)
            out["cc_steps_" + name] = int(cc.sum())
            out["cc_late_" + name] = int((cc & (ref["step_k"] % SB >= 0.9 * SB)).sum())
    return sbs, out


def run_pair_case(gpu, monkeypatch, cs, tag):
    per, n = cs.per, cs.n
    clock = Clock()
    d = open_index(gpu, cs, clock)
    try:
        check_counts(d, per)
        check_rank1a(d, per, windows(per, [j * SB for j in range(0, (n - 1) // SB + 1)] + [n - 1], 100))
        clock.lap("checks")
        check_searches_and_pairs(gpu, d, cs, monkeypatch, clock)
    finally:
        d.close()
    lines = pair_lines_of_the_counting_build(gpu, cs, monkeypatch)
    clock.lap("counting build")
    report(tag, times=clock, two_base_blocks_requested=lines)
    assert lines is None or lines > 0                                          # (no counting build: the eligible-step counts are the guard)


@pytest.mark.parametrize("c", [1, 2, 3, 4], ids=list("ACGT"))
def test_pair_counts_across_superblocks_with_bit_27_set(gpu, monkeypatch, c):
    """3/4 of the string is base c: near the end of every superblock the count of the pair (c, c) is ~0.5625 * 2^28, bit 27 of its 28-bit field; the pairs
    (A, A), (C, C), (G, G), (T, T) sit at shifts 0, 12, 24 and 4 of their count words (both branches of `sh > 4`, and the clamped last word of k_bsearch_pair)."""
    cs = case("B", c)
    sbs, cond = superblock_conditions(cs, c)
    report("B/%s inputs" % NAMES[c], n=cs.n, **cond)
    assert int(cs.ref["hit"].sum()) >= N_PATTERNS // 4
    assert len(sbs) == 6 and (sbs[:5] > 0).all()
    assert cond["cc_late_rule"] >= 2500 and cond["cc_late_device"] >= 2500
    run_pair_case(gpu, monkeypatch, cs, "B/%s" % NAMES[c])


def test_sixteen_unequal_pair_counts(gpu, monkeypatch):
    """base shares 0.4, 0.3, 0.2, 0.1: all sixteen pair counts differ, so a neighbour's field is a wrong answer and not a near miss; two superblock ends"""
    cs = case("C", 0)
    sbs, cond = superblock_conditions(cs)
    report("C inputs", n=cs.n, **cond)
    assert int(cs.ref["hit"].sum()) >= N_PATTERNS // 4
    assert len(sbs) == 3 and (sbs[:2] > 0).all()
    run_pair_case(gpu, monkeypatch, cs, "C")
