"""GPU: the two short cuts of k_ovl_nei_lane (fmd_ovlp_lane.hip) -- the self-end round (round 0) done in the lane's own step and left pending on its column,
and the closing round taken past the loops of the full round code ("closing" in the counters) -- against the same kernel without them (FMD_LANE_INLINE=0) and against the group form (FMD_NEI_LANE=0), byte for byte: records, neighbours up to n_nei, rows up
to len + ext_len; and the default against the oracle's records, with the floor on compared rows from the oracle alone (as test_gpu_walk_phase32.py).

That a read set takes the paths it is here for is asserted from the lane kernels' own counters (the third line FMD_OVLP_STATS prints), not hoped for:
  a  6000 error-free reads of 100 bases at 45-fold, -l50 and -l32, one batch and batches of 1000: both inline rounds dominate
  b  20 and 33 reads: a partly filled wave, the drained queue with the self-end round pending
  c  every read three to five times: popc(ends) > 1 in round 0, candidate 0 larger than 1, windows of more than 31 positions (the 64-bit instantiations)
  d  ragged lengths, an N in one read of twelve: shorter reads end among the strand's own rows (popc(ends) > dmin), candidate 0 is not the first neighbour,
     contained reads, strands that close without a neighbour -- the full round, some of them with the self-end round still to apply to the column
  e  1 % substitutions: rounds with two bases, strands with several neighbours, and strands handed on (FMD_LIST_RESUME) after a pending self-end round
  f  set d with room for one neighbour -- and set e, because no strand of set d has a second neighbour (without a fork a strand's first neighbour masks
     the rest: the oracle gives at most one on all 12000), so only set e overflows: the overflow is the full round's and the general kernels'
  g  pairs of reads that overlap nobody else: one candidate, which is the widest too -- the neighbour test and the child test read the same entry"""
import re

import numpy as np
import pytest

import orcbind
from fermi_amd import synth

pytestmark = pytest.mark.gpu
U64 = np.uint64
L = 100
MAX_NEI = 8

LANE = re.compile(r"one lane per strand: (\d+) strands admitted \((\d+) with 64-bit masks\), lane rounds: (\d+) quiet, (\d+) self-end inline, (\d+) closing past the loops, "
                  r"(\d+) through the loops of the full round \((\d+) of them applied a pending self-end round first\)")
HANDED = re.compile(r"(\d+) to the unforked path \((\d+) of them handed on\)")
FIELDS = ("admitted", "admitted64", "quiet", "self_end", "closing", "full", "applied")


def _same(a, b, max_nei):
    rec0, nei0, seq0 = a; rec1, nei1, seq1 = b
    assert rec1.tobytes() == rec0.tobytes()
    for j in range(max_nei):
        mj = rec0["n_nei"] > j
        assert nei1[mj, j].tobytes() == nei0[mj, j].tobytes(), j
    used = (rec0["len"] + np.maximum(rec0["ext_len"], 0)).astype(np.int64)
    m = (np.arange(seq0.shape[1])[None, :] < used[:, None]) & (rec0["status"] == 0)[:, None]
    assert np.array_equal(seq1[m], seq0[m])


def _against_oracle(gpu, got, want, max_nei):
    rec, nei, seq = got
    wrec, wnei, wseq = want
    ok = (rec["flags"] & gpu.OVLP_F_OVERFLOW) == 0    # (more than max_nei neighbours: the caller runs those again, larger)
    floor = int((wrec["n_nei"] <= max_nei).sum())     # the oracle alone: these rows fit the neighbour table
    print("rows compared %d of %d, floor %d" % (ok.sum(), len(ok), floor))
    assert ok.sum() >= floor, (ok.sum(), floor)
    for f in ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei"):
        assert np.array_equal(rec[f][ok], wrec[f][ok]), f
    for j in range(max_nei):
        mj = ok & (wrec["n_nei"] > j)
        assert nei[mj, j].tobytes() == wnei[mj, j].tobytes(), j
    used = (wrec["len"] + np.maximum(wrec["ext_len"], 0)).astype(np.int64)
    m = (np.arange(seq.shape[1])[None, :] < used[:, None]) & (ok & (wrec["status"] == 0))[:, None]
    assert np.array_equal(seq[m], wseq[m])


class _Set:
    def __init__(self, gpu, reads):
        self.bwt = gpu.build_bwt(reads)
        self.d = gpu.DevIndex.from_bwt(self.bwt)
        self.o = orcbind.OrcIndex(bwt=self.bwt)
        self.ids = np.arange(2 * len(reads), dtype=U64)
        self.want = {}

    def oracle(self, mm, max_nei=MAX_NEI):
        if (mm, max_nei) not in self.want:
            self.want[mm, max_nei] = self.o.overlap_batch(self.ids, mm, L, max_nei, 4, check_left=False)
        return self.want[mm, max_nei]

    def close(self):
        self.d.close(); self.o.close()


def _three_ways(gpu, monkeypatch, capfd, s, mm, batch=0, max_nei=MAX_NEI):
    """the sorted job with the inline rounds (counted), without them, and in the group form: equal byte for byte, the first the oracle's.
    Returns the rows and what the lanes counted, summed over the batches, with the strands handed on."""
    monkeypatch.setenv("FMD_OVLP_STATS", "1")
    capfd.readouterr()
    got = s.d.overlap_sorted(s.ids, mm, L, max_nei, batch)
    msg = capfd.readouterr().err
    monkeypatch.setenv("FMD_LANE_INLINE", "0")
    capfd.readouterr()
    plain = s.d.overlap_sorted(s.ids, mm, L, max_nei, batch)
    msg_plain = capfd.readouterr().err
    monkeypatch.delenv("FMD_OVLP_STATS")
    uncounted = s.d.overlap_sorted(s.ids, mm, L, max_nei, batch)      # (the shipped instantiations, which hold no counter)
    monkeypatch.delenv("FMD_LANE_INLINE")
    monkeypatch.setenv("FMD_NEI_LANE", "0")
    group = s.d.overlap_sorted(s.ids, mm, L, max_nei, batch)
    monkeypatch.delenv("FMD_NEI_LANE")
    shipped = s.d.overlap_sorted(s.ids, mm, L, max_nei, batch)
    lines, lines_plain = LANE.findall(msg), LANE.findall(msg_plain)
    assert lines and len(lines) == len(lines_plain), msg
    c = dict(zip(FIELDS, (sum(int(l[i]) for l in lines) for i in range(len(FIELDS)))))
    p = dict(zip(FIELDS, (sum(int(l[i]) for l in lines_plain) for i in range(len(FIELDS)))))
    c["handed"] = sum(int(h) for _, h in HANDED.findall(msg))
    print("inline  ", c)
    print("switched off", p)
    # the switch is a switch, and every round is counted once either way: the rounds the inline paths took are the full round's without them
    assert p["self_end"] == 0 and p["closing"] == 0 and p["applied"] == 0 and p["admitted"] == c["admitted"]
    assert c["applied"] <= c["self_end"] and c["applied"] <= c["full"]
    assert p["full"] + p["quiet"] == c["full"] + c["quiet"] + c["self_end"] + c["closing"]
    for other in (plain, uncounted, group, shipped):
        _same(got, other, max_nei)
    _against_oracle(gpu, got, s.oracle(mm, max_nei), max_nei)
    return got, c


@pytest.fixture(scope="module")
def set_a(gpu, oracle_lib):
    s = _Set(gpu, synth.reads(synth.DEFAULT_SEED + 3 * L + 45, 6000, L, 45, 0.0))
    yield s
    s.close()


@pytest.mark.parametrize("mm,batch", [(50, 0), (50, 1000), (32, 0)])
def test_error_free_reads_take_both_inline_rounds(gpu, monkeypatch, capfd, set_a, mm, batch):
    got, c = _three_ways(gpu, monkeypatch, capfd, set_a, mm, batch)
    assert (got[0]["n_nei"] > 0).sum() > 3000 and (got[0]["len"] == L).all()
    # both dominate: most strands admitted take the self-end round inline, most close inline, and the full round is the exception
    assert c["admitted"] > (1000 if mm == 50 else 100), c            # (at 45-fold most strands of -l32 have more than 21 candidates: the group form's)
    assert 2 * c["self_end"] > c["admitted"] and 2 * c["closing"] > c["admitted"], c
    assert c["full"] < c["self_end"] + c["closing"], c


@pytest.mark.parametrize("n_reads", [20, 33])
def test_partly_filled_wave(gpu, oracle_lib, monkeypatch, capfd, n_reads):
    """40 strands: lanes that never get a strand beside lanes with a pending self-end round; 66: a full wave and two lanes"""
    s = _Set(gpu, synth.reads(synth.DEFAULT_SEED + 3 * L + 10 + n_reads, n_reads, L, 10, 0.0))     # (10-fold: a genome of 200 and 330 bases)
    got, c = _three_ways(gpu, monkeypatch, capfd, s, 50)
    assert (got[0]["len"] == L).all()
    assert c["admitted"] > n_reads // 2 and c["self_end"] > n_reads // 2 and c["closing"] > 0, c
    s.close()


def test_copies_of_every_read_and_wide_windows(gpu, oracle_lib, monkeypatch, capfd):
    """800 distinct reads at 15-fold, each three to five times: the strand's copies end with it in round 0, every candidate holds the copies of its read,
    and a window holds about 4 x 7.6 rows -- more than 31 for many strands, of at most 21 candidates"""
    uniq = synth.reads(synth.DEFAULT_SEED + 3 * L + 15, 800, L, 15, 0.0)
    copies = 3 + (synth.rnd(synth.DEFAULT_SEED, 77, np.arange(len(uniq), dtype=U64)) % U64(3)).astype(np.int64)
    s = _Set(gpu, np.repeat(uniq, copies, axis=0))
    got, c = _three_ways(gpu, monkeypatch, capfd, s, 50)
    want = s.oracle(50)[0]
    assert (want["n_ovlp"] > 0).sum() > 2000
    assert c["admitted64"] > 100 and c["admitted"] > c["admitted64"] + 100, c
    assert c["self_end"] > 0 and c["closing"] > 0, c
    s.close()


def _ragged_with_n(reads):
    """the recipe of test_gpu_walk_narrow32.py's (d): a third of the reads cut to 40 .. 100 bases from either end, an N in one read of twelve"""
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


@pytest.fixture(scope="module")
def set_d(gpu, oracle_lib):
    s = _Set(gpu, _ragged_with_n(synth.reads(synth.DEFAULT_SEED + 3 * L + 45, 6000, L, 45, 0.0)))
    yield s
    s.close()


def test_ragged_reads_go_through_the_full_round(gpu, monkeypatch, capfd, set_d):
    got, c = _three_ways(gpu, monkeypatch, capfd, set_d, 32)
    rec = got[0]
    want = set_d.oracle(32)[0]
    assert (rec["len"] < L).sum() > 3000
    ok = want["status"] == 0
    assert (ok & (want["n_ovlp"] > 0) & (want["n_nei"] == 0)).sum() > 0                       # strands that close without a neighbour
    assert c["full"] > 1000 and c["applied"] > 0, c                                             # ... in the full round, some with the self-end round pending
    assert c["self_end"] > 0 and c["closing"] > 0, c


def test_room_for_one_neighbour(gpu, monkeypatch, capfd, set_d):
    got, c = _three_ways(gpu, monkeypatch, capfd, set_d, 32, max_nei=1)
    want = set_d.oracle(32, 1)[0]
    assert not (got[0]["flags"] & gpu.OVLP_F_OVERFLOW).any() and (want["n_nei"] <= 1).all()
    assert c["closing"] > 0, c


@pytest.fixture(scope="module")
def set_e(gpu, oracle_lib):
    s = _Set(gpu, synth.reads(synth.DEFAULT_SEED + 3 * L + 31, 4000, L, 30, 0.01))
    yield s
    s.close()


def test_room_for_one_neighbour_where_strands_have_several(gpu, monkeypatch, capfd, set_e):
    got, c = _three_ways(gpu, monkeypatch, capfd, set_e, 40, max_nei=1)
    want = set_e.oracle(40, 1)[0]
    over = (got[0]["flags"] & gpu.OVLP_F_OVERFLOW) != 0
    assert (want["n_nei"] > 1).sum() > 0 and over.sum() > 0 and not (over & (want["n_nei"] <= 1)).any()
    assert c["closing"] > 0, c


def test_reads_with_errors_hand_on_with_a_round_pending(gpu, monkeypatch, capfd, set_e):
    got, c = _three_ways(gpu, monkeypatch, capfd, set_e, 40)
    assert (set_e.oracle(40)[0]["n_nei"] > 1).sum() > 0
    assert c["handed"] > 100 and c["applied"] > 0 and c["self_end"] > 0, c


def test_one_candidate_is_the_widest_too(gpu, oracle_lib, monkeypatch, capfd):
    """20 genomes of 140 bases, from each the reads [0, 100) and [40, 140): the forward strand of the first and the reverse strand of the second have one
    candidate, which closes them -- candidate 0 ends as the widest, so nothing shows a child and lfork comes from the full round"""
    reads = []
    for k in range(20):
        g = (1 + (synth.rnd(synth.DEFAULT_SEED + 7, 100 + k, np.arange(140, dtype=U64)) >> U64(62))).astype(np.uint8)
        reads += [g[:L], g[40:]]
    s = _Set(gpu, np.stack(reads))
    got, c = _three_ways(gpu, monkeypatch, capfd, s, 50)
    want = s.oracle(50)[0]
    assert ((want["n_ovlp"] == 1) & (want["n_nei"] == 1)).sum() == 40, np.bincount(want["n_ovlp"])
    assert c["admitted"] == 40 and c["self_end"] == 40 and c["closing"] == 0 and c["applied"] == 40, c
    s.close()
