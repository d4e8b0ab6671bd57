"""CPU: the brute-force harvest of tests/harvest_ref.py against what it restates -- the reference-made golden of `tiny` and the oracle's ec_collect on
every golden read set -- over the case list of tests/test_gpu_harvest.py, and the proof that this list reaches every branch the kernels have."""
import ctypes as C

import numpy as np
import pytest

import harvest_ref as hr
import orcbind


@pytest.fixture(scope="module")
def sets(oracle_lib, gold):
    """per read set the oracle's index and the brute force; dup32 has no FASTQ: its sequences are read back through the oracle"""
    out = {}
    for name in hr.NAMES:
        o = orcbind.OrcIndex(gold.path(name + ".fmd"))
        if name == "dup32":
            n_seq = int(o.mcnt[1])
            seqs, ln, _ = o.retrieve(np.arange(n_seq, dtype=np.uint64), stride=256)
            assert int(ln.max()) <= 256
            both = [seqs[x, :ln[x]] for x in range(n_seq)]
            for x in range(0, n_seq, 97):                                          # sequence 2 i + 1 is the reverse complement of sequence 2 i
                assert np.array_equal(both[x ^ 1], hr.revcomp(both[x]))
            fwd = both[0::2]
        else:
            fwd = hr.forward_as_indexed(name)
        out[name] = (o, hr.Harvest(fwd), {})
    yield out
    for o, _, _ in out.values():
        o.close()


def oracle_harvest(o, cache, w, min_occ):
    """orc_ec_collect over the non-empty buckets of the smallest suf_len that w allows -> (K ascending, best, val, cnt); the k-mer K does not depend on
    where it is cut into bucket and key"""
    sl = max(1, w - 15)
    if sl not in cache:
        top = o.traverse(sl)
        nz = np.nonzero(top["x"][:, 2])[0]
        cache[sl] = (nz, np.ascontiguousarray(top[nz]))
    nz, top = cache[sl]
    Ks, best, val, cnt = [], [], [], [0, 0]
    for i, b in enumerate(nz.tolist()):
        so = orcbind.SolidT(0, 0, None, None, (C.c_int64 * 2)(0, 0))
        o.L.orc_ec_collect(o.e, w, min_occ, sl, top[i:i + 1].ctypes.data, C.byref(so))
        cnt[0] += so.cnt[0]; cnt[1] += so.cnt[1]
        if so.n:
            k = np.zeros(so.n, dtype=np.uint32); v = np.zeros(so.n, dtype=np.uint8)
            C.memmove(k.ctypes.data, so.key, so.n * 4); C.memmove(v.ctypes.data, so.val, so.n)
            orcbind._libc.free(so.key); orcbind._libc.free(so.val)
            Ks.append((k.astype(np.uint64) >> np.uint64(2)) << np.uint64(2 * sl) | np.uint64(b)); best.append(k & 3); val.append(v)
    if not Ks:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8), cnt
    Ks, best, val = np.concatenate(Ks), np.concatenate(best), np.concatenate(val)
    order = np.argsort(Ks)
    return Ks[order], best[order], val[order], cnt


def kmers_of(a, suf_len):
    """(K, best, val) sorted by K from an Answer's (bucket, key, val)"""
    K = (a.key.astype(np.uint64) >> np.uint64(2)) << np.uint64(2 * suf_len) | a.bucket.astype(np.uint64)
    order = np.argsort(K)
    return K[order], a.key[order] & 3, a.val[order]


@pytest.mark.parametrize("w,mo", [(17, 3), (21, 3), (23, 2)])
def test_brute_force_equals_the_golden(sets, gold, w, mo):
    """tests/golden/tiny_solid.npz was written by the reference itself: sorted triples and cnt, at compute_SUF's suf_len"""
    v = gold.npz("tiny_solid.npz")
    tag = "w%d_o%d" % (w, mo)
    a = sets["tiny"][1].answer(w, mo, w - 15)
    o = np.lexsort([a.val, a.key, a.bucket])
    assert np.array_equal(a.bucket[o], v[tag + "_bucket"]) and np.array_equal(a.key[o], v[tag + "_key"]) and np.array_equal(a.val[o], v[tag + "_val"])
    assert a.cnt == [int(x) for x in v[tag + "_cnt"]]


@pytest.mark.parametrize("name", hr.NAMES)
def test_brute_force_equals_the_oracle(sets, name):
    o, h, cache = sets[name]
    for w, mo, sl in hr.CASES + [hr.EMPTY_CASE]:
        a = h.answer(w, mo, sl)
        K, best, val, cnt = oracle_harvest(o, cache, w, mo)
        gK, gbest, gval = kmers_of(a, sl)
        assert np.array_equal(gK, K) and np.array_equal(gbest, best) and np.array_equal(gval, val), (name, w, mo, sl)
        assert a.cnt == cnt and a.n == cnt[0], (name, w, mo, sl)
        assert (np.diff(a.bucket.astype(np.int64) << 32 | a.key.astype(np.int64)) > 0).all()
        if sl <= 8:                                                                # (orc_traverse holds all 4^suf_len buckets): the cut itself, as the oracle makes it
            B, Kk, V, _ = o.ec_range(w, mo, sl, 0, 1 << (2 * sl), 1)
            oo = np.lexsort([Kk, B])
            assert np.array_equal(B[oo], a.bucket) and np.array_equal(Kk[oo], a.key) and np.array_equal(V[oo], a.val), (name, w, mo, sl)
    assert h.answer(*hr.EMPTY_CASE).cnt == [0, 0]


def test_seed_masks_partition_the_harvest(sets):
    h = sets["special"][1]
    for w, mo, sl in ((5, 3, 2), (16, 1, 1)):
        whole = h.answer(w, mo, sl)
        parts = [h.answer(w, mo, sl, 1 << p) for p in range(4)]
        assert sum(p.n for p in parts) == whole.n and [sum(p.cnt[i] for p in parts) for i in (0, 1)] == whole.cnt
        for p in range(4):
            assert (parts[p].bucket & 3 == p).all() and parts[p].n > 0
        got = whole.in_parts([1, 2, 4, 8])
        assert all(np.array_equal(np.concatenate([getattr(q, f) for q in parts]), g) for f, g in zip(("bucket", "key", "val"), got))
        assert {c: sum(p.classes[c] for p in parts) for c in hr.CLASSES} == whole.classes


def test_level_counts(sets):
    h = sets["special"][1]
    lv = h.level_counts(16, 1, 1)
    assert lv[1] == 4 and (lv[1:] > 0).all() and lv[16] == len(h.table(16)[0])
    assert h.level_counts(16, 1, 1, 0x6)[1] == 2
    lv3 = h.level_counts(5, 3, 2)
    assert lv3[2] == h.level_counts(5, 1, 2)[2] and lv3[5] <= h.level_counts(5, 1, 2)[5]   # up to suf_len the threshold is 1
    uK, s = h.table(5)
    assert lv3[5] == int((s.sum(axis=1) >= 3).sum())


def test_case_list_reaches_every_class(sets):
    """nobody thins the list into blindness: over the cases of the GPU file every class has a member, and the two counts differ often"""
    total = {c: 0 for c in hr.CLASSES}
    differ = 0
    for name in hr.NAMES:
        for w, mo, sl in hr.CASES:
            a = sets[name][1].answer(w, mo, sl)
            for c in hr.CLASSES:
                total[c] += a.classes[c]
            differ += a.cnt[1] < a.cnt[0]
    print("classes over the case list:", total, "cases with cnt[1] < cnt[0]:", differ)
    for c in hr.CLASSES:
        assert total[c] > 0, c
    assert differ >= 4
