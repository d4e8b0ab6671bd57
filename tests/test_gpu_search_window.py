"""GPU: the 16-base read window of the backward-search kernels (k_bsearch<0/1/2>, k_bsearch_pair, k_multi_bsearch) at its seams, on purpose.  A lane
reads its query backwards through the 16-byte block of the flat read buffer that holds the current base and never touches a dword above it; what can go
wrong depends on where the query's first and last byte sit in such a block.  So: every start residue r = 0..15 (a filler query in front moves the
next query's first byte to flat offset = r mod 16) times every length in LENS (one base, around one block, two, three), and in every (r, L) cell a hit,
a late miss (one base changed near the start: the search runs backwards) and a query with an N.  Queries are substrings of the reads of tiny.fq.gz and
special.fq.gz (real Ns).  One batch, one launch per index; all of it with the prefix-table start and, under FMD_PTAB_DEPTH=0, from the last base."""
import os

import numpy as np
import pytest

import orcbind

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
LENS = (1, 2, 3, 4, 5, 15, 16, 17, 18, 31, 32, 33, 34, 47, 48, 49)
HIT, LATE, WITH_N, FILL = 0, 1, 2, 3


def _sub(rng, reads, ln):
    r = reads[int(rng.integers(len(reads)))]
    at = int(rng.integers(0, len(r) - ln + 1))
    return r[at:at + ln].copy()


@pytest.fixture(scope="module")
def batch(gold, oracle_lib):
    """queries, and per query: kind, cell residue, length; the oracle's answers on tiny.fmd (computed once, shared, never written to)"""
    rng = np.random.default_rng(16)
    tiny, special = gold.fastq_nt6("tiny.fq.gz"), gold.fastq_nt6("special.fq.gz")
    with_n = [r for r in special if (r == 5).any()]
    assert with_n and min(map(len, tiny)) >= max(LENS)
    qs, kind, res = [], [], []
    at = 0                                                 # flat offset of the next query's first byte

    def put(q, k, r):
        nonlocal at
        qs.append(q); kind.append(k); res.append(r)
        at += len(q)

    for r in range(16):
        for ln in LENS:
            for k in (HIT, LATE, WITH_N):
                put(_sub(rng, tiny, (r - at) % 16), FILL, r)
                assert at % 16 == r
                odd = (r + ln + k) & 1                     # which fixture the query that is no hit comes from
                src = [x for x in (special if odd else tiny) if len(x) >= ln]
                if k == HIT:
                    q = _sub(rng, tiny, ln)
                elif k == LATE:
                    q = _sub(rng, src, ln)
                    p = int(rng.integers(0, min(3, ln)))
                    q[p] = (q[p] % 4) + 1 if q[p] <= 4 else 1
                else:
                    real = [x for x in with_n if len(x) >= ln]
                    if odd and real:                       # a window of a read of `special` around one of its own Ns
                        x = real[int(rng.integers(len(real)))]
                        n_at = int(rng.choice(np.flatnonzero(x == 5)))
                        lo = int(rng.integers(max(0, n_at - ln + 1), min(n_at, len(x) - ln) + 1))
                        q = x[lo:lo + ln].copy()
                    else:
                        q = _sub(rng, src, ln)
                        q[int(rng.integers(ln))] = 5
                    assert (q == 5).any()
                put(q, k, r)
    kind, res = np.array(kind), np.array(res)
    lens = np.array([len(q) for q in qs])
    assert len(qs) == 2 * 3 * 16 * len(LENS) < 2000
    o = orcbind.OrcIndex(os.path.join(GOLD, "tiny.fmd"))
    want = [np.zeros(len(qs), np.uint64) for _ in range(3)]
    for ln in sorted(set(lens.tolist()) - {0}):
        sel = np.flatnonzero(lens == ln)
        for w, g in zip(want, o.backward_search(np.array([qs[i] for i in sel], dtype=np.uint8))):
            w[sel] = g
    o.close()
    hit = want[0] > 0
    for r in range(16):                                    # no cell passes without testing anything
        for ln in LENS:
            cell = (res == r) & (lens == ln) & (kind != FILL)
            assert cell.sum() >= 3 and (hit & cell).any(), (r, ln)
    assert hit[kind == HIT].all() and (~hit[kind == WITH_N]).all() and (~hit[(kind == LATE) & (lens >= 15)]).mean() > 0.9
    for w in want:
        w.setflags(write=False)
    return qs, kind, res, lens, tuple(want)


def _same(got, want, what):
    cnt, beg, end = got
    assert np.array_equal(cnt, want[0]), (what, "cnt", np.flatnonzero(cnt != want[0])[:5])
    hit = want[0] > 0
    assert np.array_equal(beg[hit], want[1][hit]) and np.array_equal(end[hit], want[2][hit]), (what, "beg/end")


@pytest.mark.parametrize("table", [True, False], ids=["table", "last_base"])
def test_window_seams(gpu, batch, monkeypatch, table):
    qs, kind, res, lens, want = batch
    monkeypatch.delenv("FMD_PAIR", raising=False)
    monkeypatch.delenv("FMD_PAIR_USE", raising=False)
    if table:
        monkeypatch.delenv("FMD_PTAB_DEPTH", raising=False)
    else:
        monkeypatch.setenv("FMD_PTAB_DEPTH", "0")
    t = gpu.DevIndex.open(os.path.join(GOLD, "tiny.fmd"))
    s = gpu.DevIndex.open(os.path.join(GOLD, "special.fmd"))
    m = gpu.DevIndex.open(os.path.join(GOLD, "merge.tiny_special.fmd"))
    try:
        # k_bsearch<0> against the oracle
        single = t.backward_search(qs)
        _same(single, want, "k_bsearch<0>")
        # one part = the single search; two parts = the search on the merged file
        _same(gpu.multi_backward_search([t], qs), single, "multi [tiny]")
        _same(gpu.multi_backward_search([t, s], qs), m.backward_search(qs), "multi [tiny, special]")
        # the same handle with two-base blocks: k_bsearch<1> -> k_bsearch_pair -> k_bsearch<2>
        monkeypatch.setenv("FMD_PAIR", "1")
        assert t.build_pairs()
        paired = t.backward_search(qs)
        _same(paired, want, "two-base blocks")
        long_hit = (paired[0] > 0) & (lens > 34)
        assert (long_hit & (lens % 2 == 1)).any() and (long_hit & (lens % 2 == 0)).any()   # narrow long before the end: handed over, odd and even
    finally:
        for x in (t, s, m):
            x.close()
