"""GPU: the link stage of `scaf` (fmd_scaf_links, fermi_amd/csrc/fmd_scaf.hip) against the restatement of collect_nei (scaf.c:189-254)
in tests/scaf_restate.py, written with Python dictionaries: the dictionary of reads that occur once, the join of every entry with itself and its mate, the
groups per (own end, mate's end).  Every output word is compared.  Shapes: the smallest at which a step can go wrong -- nothing, one
entry, one pair, repeats, the distance bound, an excluded unitig, ids beyond 2^32, runs that cross waves (64, 65),
several blocks (70 001), the grid-stride loop (the grid is capped at 2^18 threads: 262 921), one end with 40 neighbours."""
import numpy as np
import pytest

from scaf_restate import NONE, restate

pytestmark = pytest.mark.gpu


def check(gpu, x, span, utig, length, excluded, max_dist):
    x = np.asarray(x, dtype=np.uint64); span = np.asarray(span, dtype=np.uint64); utig = np.asarray(utig, dtype=np.uint32)
    got = gpu.scaf_links(x, span, utig, length, excluded, max_dist)
    want = restate(x, span, utig, length, excluded, max_dist)
    for name, g, w in zip(("self", "mate", "gkey", "gval", "n_nei"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    return got


def sp(b, e):
    return b << 32 | e


LEN = [1000, 1000, 1000]
NOEXC = [0, 0, 0]


def test_nothing_and_one_entry(gpu):
    got = check(gpu, [], [], [], LEN, NOEXC, 360)
    assert len(got[2]) == 0 and not got[4].any()
    got = check(gpu, [10 << 1], [sp(800, 870)], [1], LEN, NOEXC, 360)
    assert got[0][0] == (1 << 1 | 1) << 32 | 200 and got[1][0] == NONE and len(got[2]) == 0
    check(gpu, [], [], [], [], [], 360)


def test_one_pair(gpu):
    # read 10 forward near the right end of unitig 0, its mate 11 reverse near the left end of unitig 1
    got = check(gpu, [10 << 1, 11 << 1 | 1], [sp(800, 870), sp(50, 120)], [0, 1], LEN, NOEXC, 360)
    assert list(got[2]) == [(1 << 32) | 2, (2 << 32) | 1] and list(got[3]) == [1 << 40 | 320] * 2 and list(got[4]) == [0, 1, 1, 0, 0, 0]
    # both mates on one unitig: each finds the other, no link
    got = check(gpu, [10 << 1, 11 << 1 | 1], [sp(800, 870), sp(50, 120)], [2, 2], LEN, NOEXC, 360)
    assert len(got[2]) == 0 and got[1][0] != NONE and got[1][1] != NONE
    # the reference's "deleted" mark: a reverse read that ends at base 0 of unitig 0 has the value 0 and is lost
    got = check(gpu, [10 << 1 | 1, 11 << 1], [sp(0, 0), sp(900, 970)], [0, 1], LEN, NOEXC, 360)
    assert got[0][0] == NONE and len(got[2]) == 0


def test_repeats_bound_and_excluded(gpu):
    x = [10 << 1, 10 << 1, 11 << 1 | 1,                       # a read listed twice, and its mate
         20 << 1, 20 << 1, 20 << 1, 21 << 1 | 1,              # three times
         30 << 1, 31 << 1 | 1,                                # dist == max_dist on one side
         40 << 1, 41 << 1 | 1,                                # max_dist + 1
         50 << 1, 51 << 1 | 1,                                # the mate's unitig is excluded
         60 << 1, 60 << 1, 61 << 1 | 1]                       # listed twice, once too far away: that listing does not count, but finds the other's value
    span = [sp(800, 870), sp(810, 880), sp(50, 120), sp(800, 870), sp(805, 875), sp(700, 770), sp(10, 80), sp(640, 710), sp(290, 360),
            sp(639, 709), sp(10, 80), sp(900, 970), sp(10, 80), sp(900, 970), sp(100, 170), sp(10, 80)]
    utig = [0, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 2, 0, 1, 1]
    got = check(gpu, x, span, utig, LEN, [0, 0, 1], 360)
    assert got[0][0] == NONE and got[0][2] != NONE and got[1][2] == NONE
    assert got[0][7] != NONE and got[0][8] != NONE and got[0][9] == NONE and got[1][10] == NONE
    assert got[0][11] != NONE and got[1][11] == NONE and got[0][12] == NONE
    assert got[0][13] == got[0][14] != NONE                  # entry 14 (dropped itself) reads entry 13's value, as scaf.c:223 does


def test_ids_above_2_to_32(gpu):
    big = (1 << 40) + 6
    check(gpu, [big << 1, (big ^ 1) << 1 | 1, (big + 2) << 1, (big + 3) << 1 | 1], [sp(800, 870), sp(50, 120), sp(900, 960), sp(0, 70)], [0, 1, 1, 2], LEN, NOEXC, 360)


def random_case(rng, n, n_utig=50, n_reads=None):
    n_reads = n_reads or max(4, n)
    length = rng.integers(200, 3000, n_utig).astype(np.int32)
    excluded = (rng.random(n_utig) < 0.1).astype(np.uint8)
    utig = rng.integers(0, n_utig, n).astype(np.uint32)
    x = (rng.integers(0, n_reads, n).astype(np.uint64) << np.uint64(1)) | rng.integers(0, 2, n).astype(np.uint64)
    b = (rng.random(n) * length[utig]).astype(np.int64)
    b = np.where(rng.random(n) < 0.5, np.minimum(b, 300), np.maximum(length[utig] - 300 - b % 300, 0))   # most entries near an end
    e = np.minimum(b + 70, length[utig])
    return x, (b.astype(np.uint64) << np.uint64(32)) | e.astype(np.uint64), utig, length, excluded


@pytest.mark.parametrize("n", [64, 65, 70001, 262921])
def test_random_entries(gpu, n):
    rng = np.random.default_rng(n)
    got = check(gpu, *random_case(rng, n), 360)
    if n > 1000:
        assert len(got[2]) > 1000 and (got[3] >> np.uint64(40)).max() > 1 and (got[0] == np.uint64(NONE)).any()


def test_forty_neighbours_of_one_end(gpu):
    x, span, utig = [], [], []
    for j in range(40):
        for k in range(1 + j % 3):
            r = 100 * j + 2 * k
            x += [r << 1, (r + 1) << 1 | 1]; span += [sp(900 - k, 970 - k), sp(10 + j, 80 + j)]; utig += [0, 1 + j]
    got = check(gpu, x, span, utig, [1000] * 41, [0] * 41, 360)
    assert got[4][1] == 40 and (got[4][2::2] == 1).all()
