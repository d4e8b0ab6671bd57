"""GPU: pass 2 of the sorted overlap job (k_ovl_walk<WALK_TAIL2>: a strand closes in the step after its last -- the record in one piece, the row,
the work list -- and candidates leave in two stores) leaves the bytes the job in id order leaves -- records incl. lfork, neighbours, sequences +
appended bases -- on a dense tiling (strands of one minimizer at every offset 0..16 and exact duplicates in every wave), on fewer strands than a
wave has lanes, on ragged reads with Ns and on reads with errors, where the oracle has the last word.  (The cases are those set for starting the
strands of one minimizer in phase on the genome, which was measured and not kept -- profiles/walk_phase; they hold the close that was kept.)"""
import numpy as np
import pytest

import orcbind
from fermi_amd import synth

pytestmark = pytest.mark.gpu
U64 = np.uint64


def _same(a, b, max_nei):
    """the rule of test_gpu_sorted.py: whole records; neighbours up to n_nei; the sequence and its appended bases where the record is complete"""
    rec0, nei0, seq0 = a; rec1, nei1, seq1 = b
    assert rec1.tobytes() == rec0.tobytes()
    for j in range(max_nei):
        mj = rec0["n_nei"] > j
        assert nei1[mj, j].tobytes() == nei0[mj, j].tobytes(), j
    used = (rec0["len"] + np.maximum(rec0["ext_len"], 0)).astype(np.int64)
    m = (np.arange(seq0.shape[1])[None, :] < used[:, None]) & (rec0["status"] == 0)[:, None]
    assert np.array_equal(seq1[m], seq0[m])


def _both_ways(d, ids, mm, max_len, batch):
    """id order and the sorted job: the same; returns the sorted job's result"""
    want = d.overlap(ids, mm, max_len, 8, check_left=False)
    got = d.overlap_sorted(ids, mm, max_len, 8, batch)
    _same(want, got, 8)
    return got


@pytest.fixture(scope="module")
def tiling(gpu):
    """a 100-base read at every start position of a random genome of 600 bases, and its reverse complement: every key group of the sort
    holds consecutive offsets, every strand is there twice"""
    g = np.random.default_rng(20261018).integers(1, 5, 600).astype(np.uint8)
    reads = [g[s:s + 100].copy() for s in range(501)]
    reads += [(5 - r[::-1]).astype(np.uint8) for r in reads]
    d = gpu.DevIndex.from_bwt(gpu.build_bwt(reads))
    yield d, 2 * len(reads)
    d.close()


@pytest.mark.parametrize("mm", [50, 32])          # 32: the first candidate is pushed in the strand's first step
# batch 100 is no multiple of 64: every batch is a launch of its own, whose last wave gets 36 strands
@pytest.mark.parametrize("batch", [0, 100])
def test_dense_tiling(tiling, mm, batch):
    d, n_seq = tiling
    got = _both_ways(d, np.arange(n_seq, dtype=U64), mm, 100, batch)
    assert (got[0]["n_nei"] > 0).sum() > n_seq // 2 and (got[0]["len"] == 100).all()


@pytest.mark.parametrize("n", [40, 65])
def test_fewer_strands_than_lanes(tiling, n):
    """lanes that never get a strand (40: one wave, part of it; 65: a second wave with one strand)"""
    d, _ = tiling
    _both_ways(d, np.arange(n, dtype=U64), 50, 100, 0)


def test_ragged_short_and_ambiguous_reads(gpu):
    """the recipe of test_sorted_job_ragged_short_and_ambiguous_reads at N = 3000: reads that end inside the head, Ns inside and outside the first 32 bases (keys without a minimizer; rows by k_ovl_seq_redo), ragged lengths (the lanes of a wave close in different steps), an arbitrary subset of ids in arbitrary order"""
    rng = np.random.default_rng(99)
    N = 3000
    base = synth.reads(synth.DEFAULT_SEED + 41, N, 100, 40, 0.004)
    reads = []
    for i in range(N):
        r = base[i].copy()
        u = rng.random()
        if u < 0.06:
            r = r[: rng.integers(1, 40)]
        elif u < 0.16:
            r = r[rng.integers(0, 45):]
        if rng.random() < 0.05:
            r[rng.integers(0, len(r))] = 5
        if rng.random() < 0.02 and len(r) > 8:
            r[len(r) - 1 - rng.integers(0, 8)] = 5
        reads.append(r)
    reads += reads[:50]
    d = gpu.DevIndex.from_bwt(gpu.build_bwt(reads))
    n_seq = 2 * len(reads)
    ids = rng.permutation(n_seq)[: n_seq - 123].astype(U64)
    for mm, batch in ((50, 0), (60, 1000)):
        got = _both_ways(d, ids, mm, 100, batch)
    assert (got[0]["status"] == -1).sum() > 25 and (got[0]["len"] < 32).sum() > 25
    d.close()


def test_reads_with_errors_and_the_oracle(gpu, oracle_lib):
    """2 % errors: forks, so the work lists fill in another order and the group kernels take the hand-overs; the oracle on 500 ids"""
    N, L, mm = 8000, 100, 50
    reads = synth.reads(synth.DEFAULT_SEED + 77, N, L, 30, 0.02)
    bwt = gpu.build_bwt(reads)
    d = gpu.DevIndex.from_bwt(bwt)
    ids = np.arange(2 * N, dtype=U64)
    got = _both_ways(d, ids, mm, L, 0)
    o = orcbind.OrcIndex(bwt=bwt)
    sub = np.sort(np.random.default_rng(5).choice(len(ids), 500, replace=False)).astype(U64)
    wrec, wnei, _ = o.overlap_batch(sub, mm, L, 8, 4, check_left=False)
    si = sub.astype(np.int64)
    ok = (got[0]["flags"][si] & gpu.OVLP_F_OVERFLOW) == 0
    assert ok.sum() > 450
    # (every field the oracle has an opinion on: `flags` and `lfork` are the product's own, and are held to the job in id order byte for byte above)
    for f in ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei"):
        assert np.array_equal(got[0][f][si][ok], wrec[f][ok]), f
    for j in range(8):
        mj = ok & (wrec["n_nei"] > j)
        assert got[1][si][mj, j].tobytes() == wnei[mj, j].tobytes(), j
    d.close(); o.close()
