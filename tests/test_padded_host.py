"""No GPU: tests/padded.py's closed form of the BWT of filler + S equals the BWT by sorting, byte for byte; what the padding does to an overlap record is what
padded.Padding says (the oracle on S and on filler + S); and the read sets of test_gpu_ovlp_padded.py leave fewer than 1 % of their rows out of a comparison."""
import numpy as np
import pytest

import orcbind
import padded
from test_build_host import bwt_by_sorting
from test_gpu_nei_lists import _bwt_on_the_host, _reads

U64 = np.uint64
CAP_SHARE = 0.01          # rows a comparison may leave out (flagged OVLP_F_OVERFLOW): the cap of test_repeat_rich...


def set_a():
    return _reads()


def set_b():
    """the reads with errors of test_gpu_nei_inline.py (set_e)"""
    from fermi_amd import synth
    return synth.reads(synth.DEFAULT_SEED + 3 * 100 + 31, 4000, 100, 30, 0.01)


def set_c():
    """ragged reads with errors: a fork whose second branch ends in a read that ends -- the fake forks that fm6_get_nei fixes up (unitig.c:158-176)"""
    from fermi_amd import synth
    rng = np.random.default_rng(99)
    reads = []
    for r in synth.reads(synth.DEFAULT_SEED + 41, 3000, 100, 40, 0.01):
        u = rng.random()
        if u < 0.3:
            r = r[: rng.integers(45, 100)]
        elif u < 0.6:
            r = r[rng.integers(0, 50):]
        reads.append(r.copy())
    return reads


_sets = {}


def small_set(name):
    """(strands, their BWT by sorting): `fixed` = the reads of test_gpu_nei_lists.py cut to 400, `ragged` = padded.ragged_reads()"""
    if name not in _sets:
        if name == "fixed":
            reads = _reads()[:400]
            strands = padded.strands_of(reads)
            bwt = _bwt_on_the_host(reads)
            both = np.zeros((len(strands), 101), dtype=np.uint8)
            both[:, :100] = np.stack(strands)
            assert np.array_equal(bwt_by_sorting(both), bwt)
            assert np.array_equal(padded.strands_bwt_by_sorting(strands), bwt)      # the sorter used below on unequal lengths is the two that exist
        else:
            strands = padded.strands_of(padded.ragged_reads())
            bwt = padded.strands_bwt_by_sorting(strands)
        _sets[name] = (strands, bwt)
    return _sets[name]


def test_ragged_set_hits_the_tie_rule():
    strands, _ = small_set("ragged")
    as_bytes = [bytes(s) for s in strands]
    for k in range(1, 10):
        for c in (padded.A, padded.T):
            run = bytes([c]) * k
            assert run in as_bytes                                                    # a suffix of S EQUAL to a filler suffix
            assert any(s.endswith(run) and len(s) > k and s[-k - 1] != c for s in as_bytes)
            assert any(run in s[1:-1] for s in as_bytes)
    assert len(set(len(s) for s in strands)) > 20


@pytest.mark.parametrize("name", ["fixed", "ragged"])
@pytest.mark.parametrize("Lf", [1, 7, 100])
@pytest.mark.parametrize("M", [1, 3, 64])
def test_closed_form_equals_sorting(name, M, Lf):
    strands, bwt_S = small_set(name)
    want = padded.strands_bwt_by_sorting(padded.filler_strands(M, Lf) + strands)
    got, pad = padded.padded_bwt_host(bwt_S, M, Lf)
    assert len(got) == len(want) == pad.n
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%d rows differ, the first at %d: got %d, want %d" % (len(bad), bad[0], got[bad[0]], want[bad[0]])
    # the position map: the rows of S, in order, are where it says, and every other row is the filler's
    at = pad.map_pos(np.arange(pad.n_S)).astype(np.int64)
    assert (np.diff(at) > 0).all() and np.array_equal(got[at], bwt_S)
    rest = np.ones(pad.n, dtype=bool); rest[at] = False
    assert rest.sum() == 2 * M * (Lf + 1) and np.array_equal(np.bincount(got[rest], minlength=5)[[0, 1, 4]], [2 * M, M * Lf, M * Lf])
    assert pad.id_shift == 2 * M


@pytest.fixture(scope="module")
def oracle_runs(oracle_lib):
    """the oracle's records of every strand of both read sets, -l40 and -l50"""
    out = {}
    for name, reads in (("a", set_a()), ("b", set_b())):
        bwt = _bwt_on_the_host(reads)
        o = orcbind.OrcIndex(bwt=bwt)
        ids = np.arange(2 * len(reads), dtype=U64)
        out[name] = {"bwt": bwt, "ids": ids}
        for mm in (40, 50):
            out[name][mm] = o.overlap_batch(ids, mm, 100, 8, 4, check_left=True)
        o.close()
    return out


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("mm", [40, 50])
def test_rows_left_out_stay_under_the_cap(oracle_runs, name, mm):
    """MAX_NEI = 8 on both sets: the share of rows with more neighbours, or more candidates than the list capacity max_len - min_match + 8
    (fmd_ovlp_list_cap), by the oracle alone.  (MAX_NEI = 1 is compared flag and first neighbour, MAX_NEI = 4 is the re-run's: neither leaves rows out.)"""
    rec = oracle_runs[name][mm][0]
    over = (rec["n_nei"] > 8) | (rec["n_ovlp"] > 100 - mm + 8)
    print("set %s -l%d: %d of %d rows beyond a capacity; n_nei > 4: %d, > 1: %d; back-bifurcations %d" % (
        name, mm, over.sum(), len(rec), (rec["n_nei"] > 4).sum(), (rec["n_nei"] > 1).sum(), (rec["reserved"] == 1).sum()))
    assert over.mean() < CAP_SHARE
    assert (rec["n_nei"] > 4).sum() > 0 and (rec["n_nei"] > 1).sum() > 100 and (rec["reserved"] == 1).sum() > 0


@pytest.mark.parametrize("name", ["a", "b"])
def test_padding_moves_ranks_and_nothing_else(oracle_lib, oracle_runs, name):
    """the oracle on filler + S (M = 5) against the oracle on S: every number of a record or a neighbour that names a row is a sequence RANK (a row
    among the sentinels', a count of `$` before a row) and moves by Padding.map_rank; sizes, lengths, flags, verdicts and bases stay"""
    run = oracle_runs[name]
    bwt, pad = padded.padded_bwt_host(run["bwt"], 5, 100)
    o = orcbind.OrcIndex(bwt=bwt)
    got = o.overlap_batch(run["ids"] + U64(pad.id_shift), 40, 100, 8, 4, check_left=True)
    o.close()
    want = moved(run[40], pad)
    for f in want[0].dtype.names:
        assert np.array_equal(got[0][f], want[0][f]), f
    for j in range(8):
        m = want[0]["n_nei"] > j
        assert got[1][m, j].tobytes() == want[1][m, j].tobytes(), j
    assert np.array_equal(got[2], want[2])


def moved(run, pad):
    """(rec, nei, seq) of strands of S on the index of S -> what they are on the padded index"""
    rec, nei, seq = (a.copy() for a in run)
    rec["rank"] = pad.map_rank(rec["rank"])
    has = rec["status"] != -1                                    # (a short strand has no interval)
    for j in (0, 1):
        rec["k"][has, j] = pad.map_rank(rec["k"][has, j])
    for j in range(nei.shape[1]):
        m = rec["n_nei"] > j
        for c in (0, 1):
            nei["x"][m, j, c] = pad.map_rank(nei["x"][m, j, c])
    return rec, nei, seq


def test_the_oracle_reports_forks_and_fix_ups(oracle_lib, oracle_runs):
    """flags of the oracle's records: FORKED (1) where a round of fm6_get_nei left more than one category, FIXED (4) where the fix-up ran -- that is a forked
    strand that closed with ONE neighbour, and nothing else; never OVERFLOW (2).  Set c is there for the fix-ups: sets a and b have none."""
    o = orcbind.OrcIndex(bwt=padded.strands_bwt_by_sorting(padded.strands_of(set_c())))
    rec_c = o.overlap_batch(np.arange(o.mcnt[1], dtype=U64), 40, 100, 8, 4, check_left=False)[0]
    o.close()
    for rec in (oracle_runs["a"][40][0], oracle_runs["b"][50][0], rec_c):
        assert set(np.unique(rec["flags"]).tolist()) <= {0, 1, 5}
        assert np.array_equal(rec["flags"] == 5, (rec["n_nei"] == 1) & ((rec["flags"] & 1) != 0))
        assert not ((rec["n_nei"] > 1) & (rec["flags"] == 0)).any()          # two neighbours: two categories closed, the strand forked
    assert (oracle_runs["a"][40][0]["flags"] == 1).sum() > 1000 and (rec_c["flags"] == 5).sum() > 10 and (rec_c["flags"] == 1).sum() > 100


def test_a_run_beyond_2_31_is_written_as_several_codes(oracle_lib, tmp_path):
    """A block of an RLD\\2 file counts its symbols in 31 bits.  The writer cuts a run of 2^30 symbols or more into codes of 2^27 (one-thread and sliced
    encoder alike: a slice that meets such a run sends the whole input through the one-thread encoder); the oracle reads the file back with the counts and
    ranks of the closed form.  The string: C G, 2.7 * 10^9 A, T, 1.5 * 10^9 C, G $ -- 4.2 * 10^9 symbols in 136 MB of RLE\\6 bytes (a byte holds a run of up to 31)."""
    from fermi_amd import hostlib
    runs = [(2, 1), (3, 1), (1, 2_700_000_001), (4, 1), (2, 1_500_000_000), (3, 1), (0, 1)]
    parts = []
    for c, n in runs:
        parts.append(np.full(n // 31, 31 << 3 | c, dtype=np.uint8))
        if n % 31:
            parts.append(np.array([(n % 31) << 3 | c], dtype=np.uint8))
    stream = np.concatenate(parts)
    start = np.concatenate([[0], np.cumsum([n for _, n in runs])]).astype(np.int64)
    ks = np.unique(np.concatenate([start[:-1], start[1:] - 1, start[2] + (np.arange(1, 21) << 27) - 1, start[2] + (np.arange(1, 21) << 27),
                                   np.random.default_rng(3).integers(0, start[-1], 2000)])).astype(np.int64)
    want = np.zeros((len(ks), 6), dtype=np.int64)                 # symbols of each kind among rows 0 .. k
    for j, (c, n) in enumerate(runs):
        want[:, c] += np.clip(ks + 1 - start[j], 0, n)
    files = []
    for threads in ("1", "16"):
        fn = str(tmp_path / ("long_%s.fmd" % threads))
        import os
        os.environ["FMD_RLD_THREADS"] = threads
        try:
            hostlib.write_rld_from_rle6(stream, fn)
        finally:
            del os.environ["FMD_RLD_THREADS"]
        files.append(open(fn, "rb").read())
        o = orcbind.OrcIndex(fn=fn)
        assert [int(v) for v in o.mcnt[:6]] == [int(start[-1]), 1, 2_700_000_001, 1_500_000_001, 2, 1]
        got, sym = o.rank1a(ks.astype(U64))
        o.close()
        bad = np.nonzero((got.astype(np.int64) != want).any(axis=1))[0]
        assert len(bad) == 0, "%d of %d positions differ, the first at %d: got %s, want %s" % (len(bad), len(ks), ks[bad[0]], got[bad[0]], want[bad[0]])
    assert files[0] == files[1]
