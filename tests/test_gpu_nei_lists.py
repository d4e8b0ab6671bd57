"""GPU: the two classifiers of overlap discovery -- the close of k_ovl_walk<WALK_TAIL2> and k_ovl_classify behind it (FMD_WALK_CLS=0) -- fill the SAME
work lists of get_nei, not merely lists that end in the same rows: one rule (fmd_ovl_list_of) and one layout of the lists (fmd_cls_list, fmd_kernel_common.h)
serve both, and what FMD_OVLP_STATS prints of a batch about the lists' CONTENTS -- strands to the unforked path, handed on, through the lane-per-strand kernel
at once, handed back, fix-ups, and the entries of each general list -- is the same either way.

The read set, 100-base reads: 6000 at 30-fold with 1 % substitutions (an error cuts a strand's overlaps short: the group-of-4 class, and forks that the fast
kernels hand on to the general lists), and 300 more, error-free, at 80-fold from one window of the same genome -- 375 bases: the oracle counts up to 49
candidates per strand there and more than 32, the slow list's, on 584 strands; spread over 2000 bases the 300 reads leave no strand with more than 27.
test_read_set_reaches_every_kind_of_list holds the read set to that without a GPU."""
import os
import re
import tempfile

import numpy as np
import pytest

import orcbind
from fermi_amd import synth

U64 = np.uint64
L, MM, MAX_NEI = 100, 40, 8
N_MAIN, N_DEEP, WINDOW = 6000, 300, 375


def _reads():
    seed = synth.DEFAULT_SEED + 1020
    main = synth.reads(seed, N_MAIN, L, 30, 0.01)
    gen = synth.genome(seed, N_MAIN, L, 30)
    w0 = len(gen) // 3
    r = np.arange(N_DEEP, dtype=U64)
    pos = w0 + (synth.rnd(seed, 41, r) % U64(WINDOW - L + 1)).astype(np.int64)
    deep = gen[pos[:, None] + np.arange(L)[None, :]]
    rc = (synth.rnd(seed, 42, r) >> U64(63)).astype(bool)
    deep = np.where(rc[:, None], (5 - deep)[:, ::-1], deep).astype(np.uint8)
    return np.concatenate([main, deep])


def _bwt_on_the_host(reads):
    """the BWT of read $ revcomp $ ... by sorting the suffixes (test_build_host.bwt_by_sorting, with the keys compared as byte strings)"""
    n, L1 = 2 * len(reads), L + 1
    text = np.zeros((n, 2 * L1), dtype=np.uint8)
    text[0::2, :L] = reads
    text[1::2, :L] = (5 - reads)[:, ::-1]
    keys = np.empty((n * L1, L1), dtype=np.uint8)
    for p in range(L1):
        keys[p::L1] = text[:, p:p + L1]
    sid, pos = np.repeat(np.arange(n), L1), np.tile(np.arange(L1), n)
    order = np.lexsort([sid, keys.view("S%d" % L1).ravel()])   # ('$' = 0 ends a byte string: a shorter suffix sorts first, equal ones by sequence)
    return np.where(pos[order] == 0, 0, text[sid[order], pos[order] - 1]).astype(np.uint8)


def test_read_set_reaches_every_kind_of_list(oracle_lib):
    """candidate counts by the oracle: strands for the group of 4, for the larger groups, and with more candidates than a group holds"""
    reads = _reads()
    o = orcbind.OrcIndex(bwt=_bwt_on_the_host(reads))
    ids = np.arange(0, 2 * len(reads), 3, dtype=U64)
    rec, _, _ = o.overlap_batch(ids, MM, L, MAX_NEI, 4, check_left=False)
    o.close()
    m = rec["n_ovlp"][rec["status"] == 0]
    assert ((m >= 1) & (m <= 4)).sum() > 100 and ((m > 4) & (m <= 32)).sum() > 1000 and (m > 32).sum() > 30, np.bincount(np.minimum(m, 40))


STATS = re.compile(r"part of (\d+) strands: (\d+) to the unforked path \((\d+) of them handed on\), (\d+) slots of the general group kernels' lists "
                   r"\(holes of the hand-over included\), (\d+) through the lane-per-strand kernel at once \+ (\d+) handed back to it, (\d+) fake forks fixed up")


def _stderr_of(fn):
    """what the library writes to file descriptor 2 while fn runs"""
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            res = fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return res, tmp.read().decode()


@pytest.fixture(scope="module")
def runs(gpu, oracle_lib):
    """one batch of all strands, twice: the lists by the walk's close, and by k_ovl_classify; and the oracle's rows"""
    reads = _reads()
    bwt = gpu.build_bwt(reads)
    d = gpu.DevIndex.from_bwt(bwt)
    ids = np.arange(2 * len(reads), dtype=U64)
    saved = {k: os.environ.get(k) for k in ("FMD_OVLP_STATS", "FMD_WALK_CLS")}
    try:
        os.environ["FMD_OVLP_STATS"] = "1"
        os.environ.pop("FMD_WALK_CLS", None)
        by_walk, msg_walk = _stderr_of(lambda: d.overlap_sorted(ids, MM, L, MAX_NEI, 0))
        os.environ["FMD_WALK_CLS"] = "0"
        by_kernel, msg_kernel = _stderr_of(lambda: d.overlap_sorted(ids, MM, L, MAX_NEI, 0))
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        d.close()
    o = orcbind.OrcIndex(bwt=bwt)
    by_oracle = o.overlap_batch(ids, MM, L, MAX_NEI, 4, check_left=False)
    o.close()
    return {"n": len(ids), "walk": by_walk, "kernel": by_kernel, "oracle": by_oracle, "msg_walk": msg_walk, "msg_kernel": msg_kernel}


ENTRIES = re.compile(r"of those slots (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) hold a strand")
FIGURES = ("strands", "to the unforked path", "handed on", "slots of the general lists", "through the lane-per-strand kernel at once", "handed back", "fake forks fixed up")
SLOTS = FIGURES.index("slots of the general lists")


@pytest.mark.gpu
def test_both_classifiers_fill_the_same_lists(runs):
    """Every figure of the stats line that says what the lists hold, and the entries of each general list.  The line's "slots of the general lists (holes of the
    hand-over included)" is no such figure and is not compared: a wave of a fast kernel reserves FMD_FAST_CHUNK (16) or FMD_LANE_CHUNK (64) slots of a general
    list at a time and leaves what it does not use of its last chunk as holes, so the slots depend on WHICH waves hand strands on -- 7117 .. 7197 from run to run
    on an MI355X with either classifier, and before the two shared their rule (profiles/nei_layout/stats_line.txt).  What is compared in its place is stronger:
    the entries that are no hole, list by list (the second line FMD_OVLP_STATS prints)."""
    sw, sk = STATS.findall(runs["msg_walk"]), STATS.findall(runs["msg_kernel"])
    ew, ek = ENTRIES.findall(runs["msg_walk"]), ENTRIES.findall(runs["msg_kernel"])
    assert len(sw) == 1 and len(sk) == 1 and len(ew) == 1 and len(ek) == 1, (runs["msg_walk"], runs["msg_kernel"])
    w, k = [int(v) for v in sw[0]], [int(v) for v in sk[0]]
    ew, ek = [int(v) for v in ew[0]], [int(v) for v in ek[0]]
    for name, a, b in zip(FIGURES, w, k):
        print("%-45s by the walk %6d   by k_ovl_classify %6d" % (name, a, b))
    print("entries of the general lists, by the walk %s   by k_ovl_classify %s" % (ew, ek))
    n, unforked, handed_on, slots, slow, handed_back, fixed = w
    assert n == runs["n"] and unforked > 0 and slots > 0 and slow > 0
    for i in range(len(FIGURES)):
        if i != SLOTS:
            assert w[i] == k[i], FIGURES[i]
    assert ew == ek
    # the group of 4 and larger groups are populated; nothing but holes separates slots from entries; every strand handed on is an entry
    assert ew[0] > 0 and sum(ew[1:]) > 0 and handed_on <= sum(ew) <= min(slots, k[SLOTS])


@pytest.mark.gpu
def test_both_classifiers_leave_the_same_rows_and_the_oracles(gpu, runs):
    """records, neighbours and sequences, byte for byte: whole records, the first n_nei neighbours, the len + ext_len bytes of a row (what lies beyond is
    unspecified, include/fmd_hip.h) -- between the two runs, and against the oracle on every strand that is not flagged"""
    rec, nei, seq = runs["walk"]
    assert runs["kernel"][0].tobytes() == rec.tobytes()
    ok = (rec["flags"] & gpu.OVLP_F_OVERFLOW) == 0
    assert ok.sum() > runs["n"] - runs["n"] // 20
    for f in ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei"):
        assert np.array_equal(rec[f][ok], runs["oracle"][0][f][ok]), f
    used = (rec["len"] + np.maximum(rec["ext_len"], 0)).astype(np.int64)
    in_row = (np.arange(seq.shape[1])[None, :] < used[:, None]) & (rec["status"] == 0)[:, None]
    for (_, onei, oseq), rows in ((runs["kernel"], np.ones(runs["n"], dtype=bool)), (runs["oracle"], ok)):
        for j in range(MAX_NEI):
            mj = rows & (rec["n_nei"] > j)
            assert onei[mj, j].tobytes() == nei[mj, j].tobytes(), j
        m = in_row & rows[:, None]
        assert np.array_equal(oseq[m], seq[m])
