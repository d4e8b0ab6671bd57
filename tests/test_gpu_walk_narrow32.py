"""GPU: the walk's narrow turn (k_ovl_walk, fmd_ovlp_walk.hip) at the seams of its window: records, n_ovlp, neighbours and sequence rows of ALL ids against the
oracle, for the sorted job and the job in id order, on read sets chosen for the narrow turn in two widths (profiles/walk_narrow32/narrow32.patch: 32-bit words
while no narrow lane of a wave holds more than 31 positions, the 64-position window otherwise; measured, not in the tree) and kept for whatever form the block
takes next: every size at most 31 in pass 2 (a), sizes around 31 / 32 at depth 32, both sides of that seam in one wave (b), wider than the window first and
through 63 and 31 in mid-read, the widest candidates of 32 .. 63 occurrences still in the narrow form (c), ragged lengths and reads with an N (d).

That the read sets reach the seams is asserted, not hoped for: the oracle alone walks every fourth strand of (a), (b) and (c) base by base (retrieve for the
bases, rank for the row, extend for the interval) and the steps from depth 32 on must include every residue of x0 mod 64, the sizes 1, 31, 32, 33 and 63, a
window that starts at offset 64 of its block, a 32-bit window that ends at offset 95 and k at the last position of its window.  Which set shows what: (a) at
15-fold has no size above 22, so the sizes 31, 32, 33 and the window that ends at offset 95 (it must start at 64 and hold 31) come from (b); 45-fold reads of
100 bases have Poisson(31) occurrences at depth 32 and a size of 63 has a probability of 10^-7 there -- it comes from (c), whose 80-fold set starts wider than
that.  Every item is asserted of the set that can show it, and all of them of the three together."""
import re

import numpy as np
import pytest

import orcbind
from fermi_amd import synth

pytestmark = pytest.mark.gpu
U64 = np.uint64
L = 100
SPLIT = 32                                            # FMD_WALK_SPLIT: pass 2 of the sorted job begins here
CASES = {"a": (15, 50, 4000), "b": (45, 32, 6000), "c": (80, 45, 6000)}       # coverage, -l, reads


def _reads(case, err=0.0):
    cov, _, n = CASES[case]
    return synth.reads(synth.DEFAULT_SEED + 3 * L + cov, n, L, cov, err)


def _ragged_with_n(reads):
    """(d): the reads of (b), a third of them cut to 40 .. 100 bases from either end, an N in one read of twelve"""
    rng = np.random.default_rng(20261019)
    out = []
    for r in reads:
        r = r.copy()
        u = rng.random()
        if u < 0.17:
            r = r[: rng.integers(40, 101)]
        elif u < 0.34:
            r = r[L - rng.integers(40, 101):]
        if rng.random() < 1 / 12:
            r[rng.integers(0, len(r))] = 5
        out.append(r)
    return out


class _Set:
    def __init__(self, gpu, reads):
        self.bwt = gpu.build_bwt(reads)
        self.d = gpu.DevIndex.from_bwt(self.bwt)
        self.o = orcbind.OrcIndex(bwt=self.bwt)
        self.ids = np.arange(2 * len(reads), dtype=U64)

    def close(self):
        self.d.close(); self.o.close()


@pytest.fixture(scope="module")
def sets(gpu, oracle_lib):
    """the error-free read sets of (a), (b), (c): index, oracle and the oracle's records of all ids, made once"""
    made = {}

    def get(case):
        if case not in made:
            s = _Set(gpu, _reads(case))
            s.want = s.o.overlap_batch(s.ids, CASES[case][1], L, 8, 4, check_left=False)
            made[case] = s
        return made[case]
    yield get
    for s in made.values():
        s.close()


def _against_oracle(gpu, got, want, min_ok):
    rec, nei, seq = got
    wrec, wnei, wseq = want
    ok = (rec["flags"] & gpu.OVLP_F_OVERFLOW) == 0    # (more than max_nei neighbours: the caller runs those again, larger)
    assert ok.sum() >= min_ok, ok.sum()
    for f in ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei"):
        assert np.array_equal(rec[f][ok], wrec[f][ok]), f
    for j in range(nei.shape[1]):
        mj = ok & (wrec["n_nei"] > j)
        assert nei[mj, j].tobytes() == wnei[mj, j].tobytes(), j
    used = (wrec["len"] + np.maximum(wrec["ext_len"], 0)).astype(np.int64)
    m = (np.arange(seq.shape[1])[None, :] < used[:, None]) & (ok & (wrec["status"] == 0))[:, None]
    assert np.array_equal(seq[m], wseq[m])


def _both_jobs(gpu, monkeypatch, s, mm, want, min_ok):
    """the sorted job (k_ovl_walk<WALK_HEAD>, <WALK_TAIL2>) and the job in id order (<WALK_WHOLE>), each against the oracle; returns the sorted job's result"""
    got = s.d.overlap_sorted(s.ids, mm, L, 8, 0)
    _against_oracle(gpu, got, want, min_ok)
    monkeypatch.setenv("FMD_OVLP_SORT", "0")
    plain = s.d.overlap_sorted(s.ids, mm, L, 8, 0)
    monkeypatch.delenv("FMD_OVLP_SORT")
    _against_oracle(gpu, plain, want, min_ok)
    assert plain[0].tobytes() == got[0].tobytes()     # (flags and lfork too, which the oracle has no opinion on)
    return got


def _oracle_steps(o, sids):
    """What the walk of the strands `sids` (equal lengths L) sees at the top of its step at every depth SPLIT .. L, from the oracle alone: x0 and size of
    the interval of the last `depth` bases and the row k of the strand's own suffix inside it."""
    sids = np.ascontiguousarray(sids, dtype=U64)
    seqs, ln, _ = o.retrieve(sids, stride=L + 4)
    assert (ln == L).all()
    cnt = o.cnt.astype(U64)
    n, at = len(sids), np.arange(len(sids))
    k = sids.copy()
    ik = np.zeros(n, dtype=orcbind.INTV_DT)
    x0s, szs, ks = [], [], []
    for d in range(L + 1):
        if d >= SPLIT:
            x0s.append(ik["x"][:, 0].copy()); szs.append(ik["x"][:, 2].copy()); ks.append(k.copy())
        if d == L:
            break
        c = seqs[:, L - 1 - d].astype(np.int64)
        rk, sym = o.rank1a(k)
        assert (sym == c).all()
        k = cnt[c] + rk[at, c] - U64(1)
        if d == 0:
            ik["x"][:, 0] = cnt[c]; ik["x"][:, 1] = cnt[5 - c]; ik["x"][:, 2] = cnt[c + 1] - cnt[c]
        else:
            ik = o.extend(ik, np.ones(n, dtype=np.uint8))[at, c].copy()
        assert ((k >= ik["x"][:, 0]) & (k < ik["x"][:, 0] + ik["x"][:, 2])).all()
    return np.concatenate(x0s).astype(np.int64), np.concatenate(szs).astype(np.int64), np.concatenate(ks).astype(np.int64)


def _seen(x0, sz, k):
    start = ((x0 - 1) & 63) + 1                       # offset of the window's first position in the block of x0 - 1: 1 .. 64
    # ends_at_95: the end is EXCLUSIVE -- positions 64 .. 94, the furthest a 32-bit window reaches (it starts at 64 and holds 31)
    return {"residues": set(np.unique(x0 & 63).tolist()), "sizes": set(np.unique(sz).tolist()), "max_size": int(sz.max()),
            "starts_at_64": bool(((start == 64) & (sz <= 31)).any()), "ends_at_95": bool(((start + sz == 95) & (sz <= 31)).any()),
            "k_last": bool(((k - x0 == sz - 1) & (sz > 1) & (sz <= 31)).any())}


@pytest.fixture(scope="module")
def seen(sets):
    """the steps of every fourth strand of (a), (b), (c), walked by the oracle once"""
    return {case: _seen(*_oracle_steps(sets(case).o, sets(case).ids[::4])) for case in CASES}


def test_read_sets_reach_the_seams(seen):
    a, b, c = seen["a"], seen["b"], seen["c"]
    for s in (a, b, c):
        assert s["residues"] == set(range(64))
        assert s["starts_at_64"] and s["k_last"] and 1 in s["sizes"]
    assert a["max_size"] <= 31                        # (a): every turn of pass 2 in the 32-bit form
    assert {31, 32, 33} <= b["sizes"] and b["ends_at_95"]      # (b): both sides of the seam at once
    assert {31, 32, 33, 63} <= c["sizes"] and c["max_size"] > 63 and c["ends_at_95"]      # (c): wide first, through the seam in mid-read
    assert {1, 31, 32, 33, 63} <= (a["sizes"] | b["sizes"] | c["sizes"])


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_both_widths_against_the_oracle(gpu, sets, seen, monkeypatch, capfd, case):
    s = sets(case)
    _, mm, n = CASES[case]
    if case == "c":
        monkeypatch.setenv("FMD_OVLP_STATS", "1")
        capfd.readouterr()
        s.d.overlap_sorted(s.ids, mm, L, 8, 0)
        msg = capfd.readouterr().err
        monkeypatch.delenv("FMD_OVLP_STATS")
        # the widest candidates (32 .. 63 occurrences) stayed in the narrow form: their strands still go to the unforked path
        took = [int(t) for t, _ in re.findall(r"(\d+) to the unforked path \((\d+) of them handed on\)", msg)]
        assert took and sum(took) > n // 2, msg
    got = _both_jobs(gpu, monkeypatch, s, mm, s.want, 2 * n - n // 20)
    assert (got[0]["n_nei"] > 0).sum() > n // 2 and (got[0]["len"] == L).all()


def test_reads_with_errors_through_the_seam(gpu, oracle_lib, monkeypatch):
    """(c) with 0.5 % substitutions: intervals that shrink by steps, strands of one wave on either side of 31 for many steps"""
    cov, mm, n = CASES["c"]
    s = _Set(gpu, _reads("c", 0.005))
    want = s.o.overlap_batch(s.ids, mm, L, 8, 4, check_left=False)
    _both_jobs(gpu, monkeypatch, s, mm, want, 2 * n - n // 20)
    s.close()


def test_ragged_lengths_and_ambiguous_bases(gpu, oracle_lib, monkeypatch):
    """(d): the lanes of a wave close in different steps and come back with new strands while others are in mid-read; an N takes the rank's other branch"""
    _, mm, n = CASES["b"]
    s = _Set(gpu, _ragged_with_n(_reads("b")))
    want = s.o.overlap_batch(s.ids, mm, L, 8, 4, check_left=False)
    got = _both_jobs(gpu, monkeypatch, s, mm, want, 2 * n - n // 20)
    assert (got[0]["len"] < L).sum() > n // 2 and (got[0]["n_nei"] > 0).sum() > n // 4
    s.close()
