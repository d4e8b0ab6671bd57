"""The closed-form reference of the layout-seam tests (tests/periodic.py) against brute force over the materialised string: np.cumsum and counting, at
sizes of a few thousand symbols -- n not a multiple of the period, k = -1 and k = n - 1, a pattern that lacks a base -- and its int64 arithmetic
against Python integers at the largest n the device layout takes.  No GPU."""
import numpy as np
import pytest

import periodic
from periodic import Periodic

I64 = np.int64


def _cases():
    rng = np.random.default_rng(7)
    return {
        "prime_period": Periodic(periodic.make_pattern([0.4, 0.3, 0.2, 0.1, 0.0], 1), 5 * 1009 + 333),
        "heavy_g": Periodic(periodic.make_pattern(periodic.heavy_shares(3, 0.75), 2), 3 * 1009 + 1),
        "no_c": Periodic(periodic.make_pattern([0.5, 0.0, 0.3, 0.2, 0.0], 3), 4 * 1009 - 1),       # a pattern that lacks one of the bases
        "heavy_n": Periodic(periodic.make_pattern(periodic.heavy_shares(5, 15 / 16), 4), 2 * 1009 + 77),
        "short_period": Periodic(rng.integers(0, 6, 37).astype(np.uint8), 4001),
        "whole_periods": Periodic(periodic.make_pattern([0.25, 0.25, 0.25, 0.25, 0.0], 5, P=101), 30 * 101),
        "less_than_a_period": Periodic(periodic.make_pattern([0.25, 0.25, 0.25, 0.25, 0.0], 6), 700),
    }


CASES = _cases()


class Brute:
    """the same quantities by counting"""

    def __init__(self, per):
        self.s = per.materialise()
        self.n = len(self.s)
        self.cum = np.zeros((self.n + 1, 6), dtype=I64)          # cum[i] = counts of s[:i]
        np.cumsum(self.s[:, None] == np.arange(6)[None, :], axis=0, out=self.cum[1:])
        self.mcnt = self.cum[self.n]
        self.cnt = np.concatenate([[0], np.cumsum(self.mcnt)]).astype(I64)

    def occ(self, k):
        return self.cum[np.asarray(k, dtype=I64) + 1]

    def search(self, pat):
        """fm_backward_search (exact.c:7-23) -> (hit, k, l)"""
        c = int(pat[-1])
        k, l = int(self.cnt[c]), int(self.cnt[c + 1]) - 1
        for c in pat[-2::-1]:
            if k > l:
                break
            c = int(c)
            k, l = int(self.cnt[c] + self.cum[k, c]), int(self.cnt[c] + self.cum[l + 1, c]) - 1
        return k <= l, k, l


@pytest.fixture(scope="module", params=sorted(CASES))
def pair(request):
    per = CASES[request.param]
    return per, Brute(per)


def test_the_pattern_rules():
    pat = periodic.make_pattern(periodic.heavy_shares(2, 15 / 16), 11)
    assert len(pat) == 1009 and pat[0] == 0 and pat[1] == 5
    assert (pat == 0).sum() == 1 and (pat == 5).sum() == 1 and (pat == 2).sum() > 900
    assert np.array_equal(pat, periodic.make_pattern(periodic.heavy_shares(2, 15 / 16), 11))
    assert (CASES["no_c"].pat == 2).sum() == 0 and CASES["no_c"].mcnt[2] == 0
    assert (CASES["heavy_n"].pat == 5).sum() > 900


def test_occ_counts_and_symbols(pair):
    per, br = pair
    k = np.arange(-1, per.n, dtype=I64)                          # every position, k = -1 and k = n - 1 among them
    assert np.array_equal(per.occ(k), br.occ(k))
    assert not per.occ(-1).any() and np.array_equal(per.occ(per.n - 1), br.mcnt)
    assert np.array_equal(per.mcnt, br.mcnt) and np.array_equal(per.cnt, br.cnt) and per.cnt[6] == per.n
    assert np.array_equal(per.sym(k[1:]), br.s)
    c = br.s.astype(np.intp)
    assert np.array_equal(per.occ1(k[1:], c), br.cum[1:][np.arange(per.n), c])
    for kk in (-1, 0, min(per.P, per.n) - 1, min(per.P, per.n - 1), per.n - 1):
        assert per.occ_int(kk) == [int(v) for v in br.occ(kk)]
    assert per.occ(k.reshape(1, -1)[:, :50]).shape == (1, 50, 6)


def test_lf(pair):
    per, br = pair
    p = np.arange(per.n, dtype=I64)
    c = br.s.astype(np.intp)
    want = br.cnt[c] + br.cum[1:][p, c] - 1
    assert np.array_equal(per.lf(p), want)
    assert np.array_equal(np.sort(want), p)                      # LF is a permutation of the rows whatever the string


def test_crossing(pair):
    per, br = pair
    for c in range(6):
        m = int(br.mcnt[c])
        assert per.crossing(c, m + 1) is None
        for v in sorted({1, 2, m // 3, m // 2, m - 1, m} - {0, -1}):
            if v < 1 or v > m:
                continue
            want = int(np.argmax(br.cum[1:, c] >= v))            # the first position at which the count has reached v
            assert per.crossing(c, v) == want, (c, v)


def test_extend(pair):
    per, br = pair
    rng = np.random.default_rng(3)
    m = 3000
    x = np.zeros((m, 3), dtype=I64)
    x[:, 2] = rng.integers(1, 101, m)
    x[:, 0] = rng.integers(0, per.n - x[:, 2] + 1)
    x[:, 1] = rng.integers(0, per.n - x[:, 2] + 1)
    x[:4, 0] = x[:4, 1] = 0                                      # rank of position -1
    x[4:8, 0] = x[4:8, 1] = per.n - x[4:8, 2]                    # ... and of n - 1
    is_back = rng.integers(0, 2, m).astype(np.uint8)
    got = per.extend(x, is_back)
    for i in range(m):                                           # fm6_extend, exact.c:72-88, line by line
        b = int(is_back[i])
        a = int(x[i, 1 - b])                                     # ik->x[!is_back]
        tk, tl = br.cum[a], br.cum[a + x[i, 2]]
        ok = np.zeros((6, 3), dtype=I64)
        for c in range(6):
            ok[c, 1 - b] = br.cnt[c] + tk[c]
            ok[c, 2] = tl[c] - tk[c]
        ok[0, b] = x[i, b]
        ok[4, b] = ok[0, b] + ok[0, 2]
        ok[3, b] = ok[4, b] + ok[4, 2]
        ok[2, b] = ok[3, b] + ok[3, 2]
        ok[1, b] = ok[2, b] + ok[2, 2]
        ok[5, b] = ok[1, b] + ok[1, 2]
        assert np.array_equal(got[i], ok), i
    assert (got[:, :, 2].sum(axis=1) == x[:, 2]).all()


def _patterns(per, rng, m):
    """half drawn as the GPU tests draw theirs, half cut from the string read backwards along LF-free positions (so that long ones hit too)"""
    sh = np.maximum(per.comp[1:5], 0).astype(np.float64)
    pats, lens = periodic.draw_patterns(rng, m, sh if sh.sum() else np.ones(4), max_len=12)
    lens[: m // 4] = rng.integers(1, 4, m // 4)                  # plenty of short ones: wide intervals, odd and even numbers of bases
    return pats, lens


def test_backward_search(pair):
    per, br = pair
    rng = np.random.default_rng(5)
    pats, lens = _patterns(per, rng, 4000)
    got = per.backward_search(pats, lens)
    hits = 0
    steps = set()
    for i in range(len(lens)):
        p = pats[i, :lens[i]]
        hit, k, l = br.search(p)
        assert bool(got["hit"][i]) == hit, i
        if hit:
            hits += 1
            assert (int(got["k"][i]), int(got["l"][i])) == (k, l), i
        # the states of this search one symbol at a time, and which of them are pair-eligible
        c = int(p[-1])
        k, l = int(br.cnt[c]), int(br.cnt[c + 1]) - 1
        left = int(lens[i]) - 1
        while k <= l and left >= 1:
            if left >= 2 and left % 2 == 0 and l - k < 64:
                steps.add((i, left, k, l, int(p[left - 1]), int(p[left - 2])))
            c = int(p[left - 1])
            k, l = int(br.cnt[c] + br.cum[k, c]), int(br.cnt[c] + br.cum[l + 1, c]) - 1
            left -= 1
    assert hits > 400 and hits < len(lens) - 400
    have = set(zip(*(got["step_" + key].tolist() for key in ("pat", "left", "k", "l", "c1", "c2"))))
    assert have == steps and len(have) == len(got["step_pat"]) and len(steps) > 200
    # from a table of depth D: the same answers, and only the states behind the table are steps
    D = 5
    tab = per.backward_search(pats, lens, table_depth=D)
    assert all(np.array_equal(tab[key], got[key]) for key in ("hit", "k", "l"))
    acgt = np.array([lens[i] >= D and ((pats[i, lens[i] - D:lens[i]] >= 1) & (pats[i, lens[i] - D:lens[i]] <= 4)).all() for i in range(len(lens))])
    want = {s for s in steps if not acgt[s[0]] or s[1] <= lens[s[0]] - D}
    assert set(zip(*(tab["step_" + key].tolist() for key in ("pat", "left", "k", "l", "c1", "c2")))) == want and 0 < len(want) < len(steps)


def test_backward_search_takes_symbols_that_are_not_bases():
    """a '$' or an 'N' inside a pattern is a symbol like any other to the recurrence"""
    per = CASES["short_period"]
    br = Brute(per)
    rng = np.random.default_rng(9)
    lens = rng.integers(1, 6, 1500).astype(I64)
    pats = rng.integers(0, 6, (1500, 5)).astype(np.uint8)
    got = per.backward_search(pats, lens, table_depth=3)
    for i in range(len(lens)):
        hit, k, l = br.search(pats[i, :lens[i]])
        assert bool(got["hit"][i]) == hit and (not hit or (int(got["k"][i]), int(got["l"][i])) == (k, l))
    assert 100 < got["hit"].sum() < 1400


def test_int64_path_at_the_largest_index():
    """n = 2^40 - 1 (one below what fmd_dev_open_* refuses): the int64 path equals Python integers, and its largest intermediate is a count"""
    n = (1 << 40) - 1
    for seed, sh in ((1, periodic.heavy_shares(1, 15 / 16)), (2, [0.4, 0.3, 0.2, 0.1, 0.0]), (3, periodic.heavy_shares(5, 15 / 16))):
        per = Periodic(periodic.make_pattern(sh, seed), n)
        rng = np.random.default_rng(seed)
        ks = np.concatenate([[-1, 0, 1, per.P - 1, per.P, n - 2, n - 1, (1 << 32) - 1, 1 << 32, (1 << 39) + 12345], rng.integers(0, n, 300)]).astype(I64)
        got = per.occ(ks)
        assert got.dtype == I64
        for k, g in zip(ks.tolist(), got):
            w = per.occ_int(k)
            assert [int(v) for v in g] == w and sum(w) == k + 1 and max(w) < (1 << 40)
        assert [int(v) for v in per.mcnt] == per.occ_int(n - 1) and int(per.cnt[6]) == n
        # every intermediate of occ is bounded by the number of symbols counted: (k + 1) // P * comp[c] <= k + 1 < 2^40
        assert ((ks + 1) // per.P * int(per.comp.max()) <= ks + 1).all()
        c = int(np.argmax(per.comp))
        v = int(per.mcnt[c]) - 5
        p = per.crossing(c, v)
        assert per.occ_int(p)[c] == v and per.occ_int(p - 1)[c] == v - 1
        assert np.array_equal(per.lf(ks[1:]), [int(per.cnt[int(per.pat[k % per.P])]) + per.occ_int(k)[int(per.pat[k % per.P])] - 1 for k in ks[1:].tolist()])
