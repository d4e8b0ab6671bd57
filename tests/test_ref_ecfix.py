"""The CPU leg of bench.py's ec_fix line, pinned where the reference was compiled (oracle/_ref): the reference's own static ec_fix through
oracle/ref_ec_harness.c:refec_fix, its tables filled from the golden solid table of tiny.fmd, must print `fermi correct -t1`'s FASTQ; and bench.py's
numpy form of the marking rule (correct.c:247-252) must agree with it -- with refec_fix run here where oracle/_ref was built, and everywhere with
its output stored in tests/golden/tiny_refec_fix.npz (tests/golden/make_ref_ecfix.py).  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bench  # noqa: E402
from benchlegs import ecfix as ecfix_leg  # noqa: E402
import orcbind  # noqa: E402
from test_oracle_golden import _fastq_records  # noqa: E402


def _fixed_len(gold, L=100):
    recs = [r for r in _fastq_records(gold.text_gz("tiny.fq.gz"))]
    ids = [i for i, r in enumerate(recs) if len(r[1]) == L]
    nt6 = np.stack([bench.NT6_OF_ASCII[np.frombuffer(recs[i][1], dtype=np.uint8)] for i in ids])
    q = np.stack([np.frombuffer(recs[i][2], dtype=np.uint8) for i in ids])
    return ids, nt6, q


def _sorted_trip(v):
    o = np.argsort(v["w17_o3_bucket"], kind="stable")
    return (np.ascontiguousarray(v["w17_o3_bucket"][o], dtype=np.uint32), np.ascontiguousarray(v["w17_o3_key"][o], dtype=np.uint32), np.ascontiguousarray(v["w17_o3_val"][o], dtype=np.uint8))


def suf_len_of(w):
    return w - 15 if w > 15 else 1


def _trip_of(tabs, w):
    """the table of k-mer length w among `tabs` (tiny_solid.npz's, tiny_refec_fix_params.npz's), sorted by bucket as refec_fix wants it"""
    tag = [k[:-7] for k in tabs if k.startswith("w%d_o" % w) and k.endswith("_bucket")][0]
    o = np.argsort(tabs[tag + "_bucket"], kind="stable")
    return tuple(np.ascontiguousarray(tabs[tag + "_" + f][o], dtype=dt) for f, dt in (("bucket", np.uint32), ("key", np.uint32), ("val", np.uint8)))


def _kept_records(text):
    return {int(r[0].lstrip(b"@").split(b"_")[0]): (r[0].lstrip(b"@"), r[1], r[2]) for r in _fastq_records(text)}


@pytest.mark.parametrize("threads", [1, 3])
def test_refec_fix_prints_fermi_correct(gold, oracle_lib, threads, monkeypatch):
    if bench.ref_ec_lib() is None:
        pytest.skip("oracle/_ref/libref_ec.so not built here")
    monkeypatch.setattr(ecfix_leg, "usable_cpus", lambda: threads)
    ids, nt6, q = _fixed_len(gold)
    (txt, q2, info), _, _, lpr, kind, cores = bench.cpu_ecfix(17, 2, 5, _sorted_trip(gold.npz("tiny_solid.npz")), nt6, q)
    assert kind == "reference" and cores == threads and lpr > 20
    want = _kept_records(gold.text_gz("tiny.ec.fq.gz"))
    n_kept = 0
    for k, i in enumerate(ids):
        bad = info[k] >> 16 & 1
        assert (i in want) == (not bad), i                       # the filter of correct.c:412 (keep_bad = 0)
        if not bad:
            name, s, ql = want[i]
            assert name == b"%d_%d_%d" % (i, info[k] & 0xffff, info[k] >> 18) and s == txt[k].tobytes() and ql == q2[k].tobytes(), i
            n_kept += 1
    assert n_kept == len(want) and n_kept >= 2000   # (every record of the golden output has been compared)


def _marking_inputs(gold):
    """tiny.fq's reads of 100 bases and 400 more that the filter rejects"""
    ids, nt6, q = _fixed_len(gold)
    rng = np.random.default_rng(3)
    extra = nt6[:400].copy()                                      # reads the filter rejects: other genomes, reads with a third of their bases changed, Ns
    extra[:100] = rng.integers(1, 5, size=(100, nt6.shape[1]))
    for r in extra[100:300]:
        r[rng.choice(len(r), 35, replace=False)] = rng.integers(1, 5, size=35)
    extra[300:, ::17] = 5
    return np.concatenate([nt6, extra]), np.concatenate([q, q[:400]])


def test_marking_rule_in_numpy_equals_the_reference(gold, oracle_lib):
    """the oracle's ec_fix (nt6 bases, qualities and info BEFORE the marking: the contract of fmd_ecfix_dev) + bench.mark_corrected == refec_fix (after it)"""
    nt6, q = _marking_inputs(gold)
    v = gold.npz("tiny_solid.npz")
    want = gold.npz("tiny_refec_fix.npz")
    if bench.ref_ec_lib() is not None:
        (txt, q2, info), _, _, _, kind, _ = bench.cpu_ecfix(17, 2, 5, _sorted_trip(v), nt6, q)
        assert kind == "reference" and np.array_equal(txt, want["text"]) and np.array_equal(q2, want["qual"]) and np.array_equal(info, want["info"])
    s, qq, off, inf = orcbind.ec_fix(17, v["w17_o3_bucket"], v["w17_o3_key"], v["w17_o3_val"], list(nt6), list(q))
    m_txt, m_q, m_inf = bench.mark_corrected(nt6, s.reshape(nt6.shape), qq.reshape(nt6.shape), inf)
    assert np.array_equal(m_txt, want["text"]) and np.array_equal(m_q, want["qual"]) and np.array_equal(m_inf, want["info"])
    assert (m_txt >= ord("a")).sum() > 1000 and (m_inf >> 16 & 1).sum() > 100


# (k-mer length, step) beyond the w 17 / step 5 of tiny_refec_fix.npz: the other two golden tables, step 1 (no hop), 8 (the full mask of the kernel's
# batched hop) and 12 (beyond it), and the two ends of the k-mer lengths the table builder accepts below and at the reference's MAX_KMER
PARAM_CASES = [(21, 5), (23, 2), (17, 1), (17, 8), (17, 12), (11, 5), (27, 5)]


def _param_inputs(gold):
    """every fourth read of _marking_inputs: 500 reads of tiny.fq and 100 of those the filter rejects"""
    nt6, q = _marking_inputs(gold)
    return np.ascontiguousarray(nt6[::4]), np.ascontiguousarray(q[::4])


@pytest.mark.parametrize("w,step", PARAM_CASES)
def test_oracle_ecfix_at_other_k_and_step(gold, oracle_lib, w, step):
    """the oracle's ec_fix + bench.mark_corrected == the reference's ec_fix at other k-mer lengths and steps (tests/golden/make_ref_ecfix_params.py;
    the reference itself is run as well where oracle/_ref was built); the oracle's ec_collect gives the stored tables of w 11 and 27"""
    want = gold.npz("tiny_refec_fix_params.npz")
    tabs = gold.npz("tiny_solid.npz")
    tabs.update({k: a for k, a in want.items() if k.endswith(("_bucket", "_key", "_val"))})
    B, K, V = _trip_of(tabs, w)
    nt6, q = _param_inputs(gold)
    tag = "w%d_s%d_" % (w, step)
    if bench.ref_ec_lib() is not None:
        (txt, q2, info), _, _, _, kind, _ = bench.cpu_ecfix(w, suf_len_of(w), step, (B, K, V), nt6, q)
        assert kind == "reference" and np.array_equal(txt, want[tag + "text"]) and np.array_equal(q2, want[tag + "qual"]) and np.array_equal(info, want[tag + "info"])
    s, qq, off, inf = orcbind.ec_fix(w, B, K, V, list(nt6), list(q), step)
    m_txt, m_q, m_inf = bench.mark_corrected(nt6, s.reshape(nt6.shape), qq.reshape(nt6.shape), inf)
    assert np.array_equal(m_txt, want[tag + "text"]) and np.array_equal(m_q, want[tag + "qual"]) and np.array_equal(m_inf, want[tag + "info"])
    assert (m_txt >= ord("a")).sum() > 250 and (m_inf >> 16 & 1).sum() > 25      # (a quarter of the floors of the test above)
    if w in (11, 27):
        o = orcbind.OrcIndex(gold.path("tiny.fmd"))
        ob, ok, ov, _ = o.ec_range(w, 3, suf_len_of(w), 0, 1 << (2 * suf_len_of(w)), 2)
        o.close()
        srt = np.lexsort([ov, ok, ob])
        assert np.array_equal(ob[srt], B) and np.array_equal(ok[srt], K) and np.array_equal(ov[srt], V) and len(B) > 10000


def test_oracle_ecfix_statistics_form_changes_nothing(gold, oracle_lib):
    """orc_ecfix_batch_ex == orc_ecfix_batch on bases, qualities and info; its two numbers per read are what they say: 0 for a read that is never
    seeded, at least 2 entries of trace (the root and one choice) for every other read, a queue within the budget of correct.c:114 plus one expansion"""
    nt6, q = _marking_inputs(gold)
    v = gold.npz("tiny_solid.npz")
    nt6 = list(nt6) + [nt6[0][:17], nt6[1][:5]]
    q = list(q) + [q[0][:17], q[1][:5]]
    for step in (5, 0):
        a = orcbind.ec_fix(17, v["w17_o3_bucket"], v["w17_o3_key"], v["w17_o3_val"], nt6, q, step)
        b = orcbind.ec_fix(17, v["w17_o3_bucket"], v["w17_o3_key"], v["w17_o3_val"], nt6, q, step, stats=True)
        assert len(b) == 6 and all(np.array_equal(x, y) for x, y in zip(a, b[:4]))
        tmax, hmax = b[4], b[5]
        unseeded = a[3] == 0xffff
        assert unseeded[-2:].all() and unseeded.sum() < 500
        assert (tmax[unseeded] == 0).all() and (hmax[unseeded] == 0).all()
        assert (tmax[~unseeded] >= 2).all() and (hmax[~unseeded] >= 1).all() and hmax.max() <= 257 and tmax.max() >= 256   # (256: past the first allocation of the oracle's stack)
