"""GPU: pass 2 of the sorted overlap job with the strands of one minimizer in phase on the genome (k_ovl_walk<WALK_TAIL2> with the sort keys at hand,
fmd_ovlp_walk.hip: generations of 64 consecutive strands of the sorted order, a strand whose minimizer lies o bases from its end starts omax - o steps late,
the close in company) against the free-running admission (FMD_WALK_PHASE=0) byte for byte -- records, neighbours up to n_nei, rows up to len + ext_len --
and both against the oracle's records.

What the read sets are for is asserted from the keys' definition, not hoped for: the sort key of every strand is recomputed here from the oracle's
retrieved bases (park_hash and the minimizer rule of fmd_ovlp_sort.hip) and the generations from the stable sort of those keys, batch by batch.
  1  one generation, partly filled (40 strands), and one full generation plus one of two lanes (66 strands)
  2  several generations, in one batch and in batches of 1000 (no multiple of 64: keys + b must follow sorted + b); at -l32 a strand pushes in its first
     step while its neighbours still wait; minimizers with strands at three and more offsets, a generation whose offsets span 12 and more
  3  more generations than resident waves (the CU count is read from the device): a wave resets its state and runs a second generation
  4  ragged lengths, reads with an N, reads shorter than 32 bases (key ~0: ended inside the head, skipped) and reads whose last 32 bases hold no 16-mer
     without an N (key 0xfffffffe: waits for nobody, its row comes from the redo list); the strands of a generation finish in different steps
  5  a generation in which no key has a minimizer: omax is 0 and nobody waits

The floor on the rows compared comes from the oracle alone: a row the oracle gives at most MAX_NEI neighbours cannot overflow the neighbour table."""
import numpy as np
import pytest

import orcbind
from fermi_amd import synth

pytestmark = pytest.mark.gpu
U64 = np.uint64
L = 100
SPLIT = 32                                            # FMD_WALK_SPLIT
PARK_K = 16                                           # bases per k-mer of the minimizer (fmd_ovlp_sort.hip)
MAX_NEI = 8
KEY_NOMIN, KEY_ENDED = 0xFFFFFFFE, 0xFFFFFFFF


def _park_hash(v):
    v = v.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    v = (v * np.uint64(0x9E3779B1)) & m; v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x85EBCA77)) & m; v ^= v >> np.uint64(13)
    return v


def _keys(o, ids):
    """k_ovl_park_keys from the oracle's bases: hash of the smallest-hashing 16-mer among the strand's last 32 bases (27 bits) | its offset from the
    strand's end (5 bits); 0xfffffffe when every 16-mer holds an ambiguous base, ~0 for a strand shorter than the head."""
    seqs, ln, _ = o.retrieve(ids, stride=L + 4)
    n = len(ids)
    ln = ln.astype(np.int64)
    parked = ln >= SPLIT
    best = np.full(n, KEY_ENDED, dtype=np.uint64)
    v = np.zeros(n, dtype=np.uint64); bad = np.zeros(n, dtype=np.uint64)
    at = np.arange(n)
    for j in range(SPLIT):
        c = seqs[at, np.maximum(ln - 1 - j, 0)].astype(np.uint64)      # base j from the strand's end
        v = ((v << np.uint64(2)) | ((c - np.uint64(1)) & np.uint64(3))) & np.uint64(0xFFFFFFFF)
        bad = ((bad << np.uint64(1)) | ((c < 1) | (c > 4)).astype(np.uint64)) & np.uint64(0xFFFF)
        if j + 1 >= PARK_K:
            h = (_park_hash(v) & ~np.uint64(31)) | np.uint64(j + 1 - PARK_K)
            best = np.where((bad == 0) & (h < best), h, best)
    key = np.where(best == KEY_ENDED, np.uint64(KEY_NOMIN), best)
    return np.where(parked, key, np.uint64(KEY_ENDED))


def _generations(keys, batch):
    """the keys of every generation: 64 consecutive strands of the sorted order (a stable sort: equal keys in id order), batch by batch"""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    n = len(sk)
    batch = batch if 0 < batch < n else n
    return [sk[g:min(g + 64, b + batch, n)] for b in range(0, n, batch) for g in range(b, min(b + batch, n), 64)]


def _same(a, b):
    rec0, nei0, seq0 = a; rec1, nei1, seq1 = b
    assert rec1.tobytes() == rec0.tobytes()
    for j in range(MAX_NEI):
        mj = rec0["n_nei"] > j
        assert nei1[mj, j].tobytes() == nei0[mj, j].tobytes(), j
    used = (rec0["len"] + np.maximum(rec0["ext_len"], 0)).astype(np.int64)
    m = (np.arange(seq0.shape[1])[None, :] < used[:, None]) & (rec0["status"] == 0)[:, None]
    assert np.array_equal(seq1[m], seq0[m])


def _against_oracle(gpu, got, want, rows):
    """rows: the ids (= rows of `got`) the oracle's `want` was computed for"""
    rec, nei, seq = (a[rows] for a in got)
    wrec, wnei, wseq = want
    ok = (rec["flags"] & gpu.OVLP_F_OVERFLOW) == 0    # (more than MAX_NEI neighbours: the caller runs those again, larger)
    floor = int((wrec["n_nei"] <= MAX_NEI).sum())     # the oracle alone: these rows fit the neighbour table
    print("rows compared %d of %d, floor %d" % (ok.sum(), len(ok), floor))
    assert ok.sum() >= floor, (ok.sum(), floor)
    for f in ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei"):
        assert np.array_equal(rec[f][ok], wrec[f][ok]), f
    for j in range(MAX_NEI):
        mj = ok & (wrec["n_nei"] > j)
        assert nei[mj, j].tobytes() == wnei[mj, j].tobytes(), j
    used = (wrec["len"] + np.maximum(wrec["ext_len"], 0)).astype(np.int64)
    m = (np.arange(seq.shape[1])[None, :] < used[:, None]) & (ok & (wrec["status"] == 0))[:, None]
    assert np.array_equal(seq[m], wseq[m])


class _Set:
    def __init__(self, gpu, reads, sample=None):
        self.bwt = gpu.build_bwt(reads)
        self.d = gpu.DevIndex.from_bwt(self.bwt)
        self.o = orcbind.OrcIndex(bwt=self.bwt)
        self.ids = np.arange(2 * len(reads), dtype=U64)
        self.rows = np.arange(len(self.ids)) if sample is None else np.sort(np.random.default_rng(sample).choice(len(self.ids), sample, replace=False))
        self.want = {}

    def oracle(self, mm):
        if mm not in self.want:
            self.want[mm] = self.o.overlap_batch(self.ids[self.rows], mm, L, MAX_NEI, 4, check_left=False)
        return self.want[mm]

    def close(self):
        self.d.close(); self.o.close()


def _phase_on_off(gpu, monkeypatch, s, mm, batch):
    """the sorted job in phase and free-running: equal byte for byte, and both the oracle's; returns the job in phase"""
    on = s.d.overlap_sorted(s.ids, mm, L, MAX_NEI, batch)
    monkeypatch.setenv("FMD_WALK_PHASE", "0")
    off = s.d.overlap_sorted(s.ids, mm, L, MAX_NEI, batch)
    monkeypatch.delenv("FMD_WALK_PHASE")
    _same(off, on)
    _against_oracle(gpu, on, s.oracle(mm), s.rows)
    _against_oracle(gpu, off, s.oracle(mm), s.rows)
    return on


@pytest.mark.parametrize("n_reads", [20, 33])
def test_one_generation_partly_filled(gpu, oracle_lib, monkeypatch, n_reads):
    """40 strands: lanes that find the queue drained stay idle while the others wait and walk; 66: one full generation and one of two lanes"""
    s = _Set(gpu, synth.reads(synth.DEFAULT_SEED + 3 * L + 30 + n_reads, n_reads, L, 30, 0.0))
    gens = _generations(_keys(s.o, s.ids), 0)
    assert [len(g) for g in gens] == ([40] if n_reads == 20 else [64, 2])
    got = _phase_on_off(gpu, monkeypatch, s, 50, 0)
    assert (got[0]["len"] == L).all()
    s.close()


@pytest.fixture(scope="module")
def set_b(gpu, oracle_lib):
    """6000 reads, 45-fold: the (b) set of test_gpu_walk_narrow32.py, with the oracle's records of all ids at -l32, made once"""
    s = _Set(gpu, synth.reads(synth.DEFAULT_SEED + 3 * L + 45, 6000, L, 45, 0.0))
    s.keys = _keys(s.o, s.ids)
    yield s
    s.close()


def test_read_set_b_has_keys_in_several_offsets(set_b):
    keys = set_b.keys
    assert (keys < KEY_NOMIN).all()
    mini, offs = keys >> np.uint64(5), keys & np.uint64(31)
    pairs = np.unique(np.stack([mini, offs], axis=1), axis=0)           # distinct (minimizer, offset)
    _, per_min = np.unique(pairs[:, 0], return_counts=True)
    assert (per_min >= 3).sum() > 100                                  # minimizers whose strands stand at three and more offsets
    for batch in (0, 1000):
        gens = _generations(keys, batch)
        assert len(gens) >= 12000 // 64 and max(int((g & np.uint64(31)).max() - (g & np.uint64(31)).min()) for g in gens) >= 12
    assert len(_generations(keys, 1000)[15]) == 1000 - 15 * 64         # a batch ends inside a generation: the next starts at sorted + b, keys + b


@pytest.mark.parametrize("batch", [0, 1000])
def test_several_generations_and_batches(gpu, monkeypatch, set_b, batch):
    got = _phase_on_off(gpu, monkeypatch, set_b, 32, batch)
    assert (got[0]["n_nei"] > 0).sum() > 3000 and (got[0]["len"] == L).all()


def test_more_generations_than_resident_waves(gpu, oracle_lib, monkeypatch):
    """a wave runs a second generation: state reset, the admission reopening, a close with fewer than 32 waiting once nobody walks"""
    import torch
    n = 150000
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 2 * n > 64 * 16 * cus, cus                                  # 16: the cap on resident waves per CU (FMD_WAVES_PER_CU)
    s = _Set(gpu, synth.reads(synth.DEFAULT_SEED + 3 * L + 30, n, L, 30, 0.0), sample=3000)
    got = _phase_on_off(gpu, monkeypatch, s, 50, 0)
    assert (got[0]["n_nei"] > 0).sum() > n // 2 and (got[0]["len"] == L).all()
    s.close()


def _ragged_with_n(reads):
    """the recipe of test_gpu_walk_narrow32.py's (d): a third of the reads cut to 40 .. 100 bases from either end, an N in one read of twelve -- and, for the
    two special keys, which that recipe does not reach: every 500th read cut to 20 .. 31 bases (shorter than the head), every 500th + 1 with an N in
    every 16-mer of its last 32 bases (positions len - 16 and len - 32)"""
    rng = np.random.default_rng(20261019)
    out = []
    for i, r in enumerate(reads):
        r = r.copy()
        u = rng.random()
        if u < 0.17:
            r = r[: rng.integers(40, 101)]
        elif u < 0.34:
            r = r[L - rng.integers(40, 101):]
        if rng.random() < 1 / 12:
            r[rng.integers(0, len(r))] = 5
        if i % 500 == 0:
            r = r[: 20 + (i // 500) % 12]
        elif i % 500 == 1:
            r[len(r) - 16] = 5; r[len(r) - 32] = 5
        out.append(r)
    return out


def test_ragged_lengths_ns_and_the_two_special_keys(gpu, oracle_lib, monkeypatch):
    n = 6000
    s = _Set(gpu, _ragged_with_n(synth.reads(synth.DEFAULT_SEED + 3 * L + 45, n, L, 45, 0.0)))
    keys = _keys(s.o, s.ids)
    assert (keys == KEY_NOMIN).sum() >= 12 and (keys == KEY_ENDED).sum() >= 24, ((keys == KEY_NOMIN).sum(), (keys == KEY_ENDED).sum())
    got = _phase_on_off(gpu, monkeypatch, s, 32, 0)
    ln = got[0]["len"]
    assert (ln < L).sum() > n // 2 and (ln < SPLIT).sum() >= 24 and (got[0]["n_nei"] > 0).sum() > n // 4
    # strands of one generation finish in different steps: generations that hold several lengths
    order = np.argsort(keys, kind="stable")
    assert sum(len(np.unique(ln[order[g:g + 64]])) > 3 for g in range(0, 2 * n, 64)) > 100
    s.close()


def test_a_generation_without_a_minimizer(gpu, oracle_lib, monkeypatch):
    """40 reads with an N in every 16-mer of the last 32 bases of either strand: only key 0xfffffffe, omax = 0, nobody waits"""
    reads = synth.reads(synth.DEFAULT_SEED + 3 * L + 5, 40, L, 30, 0.0)
    for p in (15, 31, L - 16, L - 32):
        reads[:, p] = 5
    s = _Set(gpu, reads)
    assert (_keys(s.o, s.ids) == KEY_NOMIN).all()
    got = _phase_on_off(gpu, monkeypatch, s, 50, 0)
    assert (got[0]["len"] == L).all()
    s.close()
