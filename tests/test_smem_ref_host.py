"""CPU only: tests/smem_ref.py (the plain restatement of fm6_smem1_core and of the fm6_smem chain that test_gpu_smem_edges.py
measures k_smem with) against the oracle at every start of every case query, and the case list itself: every class of input the
kernel treats differently must be reached, asserted from the restatement's traces so that another seed cannot lose one silently.
The two starts the reference leaves undefined never go to the oracle (smem1_core would read a[0] of an empty vector): they are
listed by name in Cases.undefined and must return their marker."""
import numpy as np
import pytest

import orcbind
import smem_ref
from fermi_amd import synth

U64 = np.uint64
INDEXES = ["nested", "nested_non", "nested300"]


@pytest.fixture(scope="module")
def cs():
    return smem_ref.cases()


def test_bruteforce_ragged_bwt_equals_fermi_build(oracle_lib, gold):
    o = orcbind.OrcIndex(gold.path("tiny.fmd"))
    assert np.array_equal(smem_ref.bwt_by_sorting_ragged(gold.fastq_nt6("tiny.fq.gz")), o.decode_all())
    o.close()


def test_nested_indexes_have_the_stated_sizes(cs):
    assert len(cs.bwt("nested")) == 2 * (sum(k + 1 for k in range(1, 121)) + sum(k for k in range(2, 121)) + 50 * 31) == 32378
    assert cs.ref("nested").cnt[6] - cs.ref("nested").cnt[5] == 2 and cs.ref("nested_non").cnt[6] == cs.ref("nested_non").cnt[5]
    r3 = cs.ref("nested300")
    assert r3.cnt[6] - r3.cnt[5] == 2 and r3.n_seq == 2 * len(cs.reads["nested300"])


@pytest.mark.parametrize("index", INDEXES)
def test_smem1_equals_the_oracle_at_every_start(oracle_lib, cs, index):
    o = orcbind.OrcIndex(bwt=cs.bwt(index))
    seen_undefined, n = {}, 0
    for name, q in cs.queries[index].items():
        for sm in (0, 1):
            for x, (mem, ret, _) in enumerate(cs.single(index, name, sm)):
                if (index, name, x, sm) in cs.undefined or isinstance(ret, str):
                    seen_undefined[(index, name, x, sm)] = ret
                    assert len(mem) == 0
                    continue
                wmem, wret = o.smem1(q, x, sm)
                assert ret == wret and mem.tobytes() == wmem.tobytes(), (name, sm, x)
                n += 1
            mem, calls, und = cs.whole(index, name, sm)
            if und is None and len(q):
                assert mem.tobytes() == o.smem(q, sm).tobytes(), (name, sm)
    o.close()
    assert seen_undefined == {k: v for k, v in cs.undefined.items() if k[0] == index}
    print("%s: %d starts compared, %d undefined" % (index, n, len(seen_undefined)))


def ragged_tiny_queries():
    """the queries of test_gpu_parity.py::test_smem_vs_oracle_ragged"""
    rng = np.random.default_rng(7)
    reads = synth.reads(synth.DEFAULT_SEED, 2000, coverage=20, err=0.02)
    return [r[int(rng.integers(0, 50)):][:int(rng.integers(1, 100))] for r in reads[:600]]


def test_smem1_equals_the_oracle_on_ragged_queries_of_tiny(tiny_oracle):
    ix = smem_ref.RefIndex(tiny_oracle.decode_all())
    assert ix.cnt == [int(v) for v in tiny_oracle.cnt] and ix.n_seq == int(tiny_oracle.mcnt[1])
    qs = ragged_tiny_queries()[::3]
    assert len(qs) == 200 and min(len(q) for q in qs) == 1
    n = 0
    for q in qs:
        for sm in (0, 1):
            for x in range(len(q)):
                mem, ret, _ = smem_ref.smem1(ix, q, x, sm)
                wmem, wret = tiny_oracle.smem1(q, x, sm)
                assert ret == wret and mem.tobytes() == wmem.tobytes(), (q.tolist(), sm, x)
                n += 1
    assert n > 15000


@pytest.mark.parametrize("sm", [0, 1])
def test_chain_equals_the_golden_vectors(tiny_oracle, gold, sm):
    ix = smem_ref.RefIndex(tiny_oracle.decode_all())
    v = gold.npz("tiny_vectors.npz")
    off = v["smem%d_off" % sm]
    for i, q in enumerate(v["smem%d_reads" % sm]):
        mem, _, und = smem_ref.chain(ix, q, sm)
        assert und is None and np.array_equal(mem.view(U64).reshape(-1, 4), v["smem%d_mem" % sm][off[i]:off[i + 1]]), i


def test_full_rows_are_the_whole_sequences(cs):
    """FMD_SMEM_WIN_F_FULL's rule on query R: of its 120 SMEMs R[:k] the closed ones are all of them (every prefix is a read)"""
    mem, _, _ = cs.whole("nested", "R", 0)
    assert len(smem_ref.full_rows(cs.ref("nested"), mem)) == 120
    mem, _, _ = cs.whole("nested", "q2500", 0)
    assert 0 < len(smem_ref.full_rows(cs.ref("nested"), mem)) < len(mem)


def test_the_cases_reach_every_class(cs):
    calls = []   # (index, name, sm, x, len(q), mem, ret, trace) of every defined start
    for index, name in cs.names():
        for sm in (0, 1):
            q = cs.queries[index][name]
            calls += [(index, name, sm, x, len(q), m, r, t) for x, (m, r, t) in enumerate(cs.single(index, name, sm)) if not isinstance(r, str)]
    fwd_x0 = max(c[7]["fwd_len"] for c in calls if c[3] == 0)
    last_fed_by_curr = max(c[7]["last_prev"] for c in calls if c[7]["last_prev"] is not None and not c[7]["last_from_fwd"])
    last_fed_by_fwd = max(c[7]["last_prev"] for c in calls if c[7]["last_from_fwd"])
    rounds = max(c[7]["rounds"] for c in calls)
    skipped = max(c[7]["last_open_skipped"] for c in calls)
    per_read = {(ix, nm, sm): len(cs.whole(ix, nm, sm)[0]) for ix, nm in cs.names() for sm in (0, 1)}
    per_call = max(len(c[5]) for c in calls)
    print("forward list at x == 0: %d; last round fed by curr: %d, by the forward list: %d; backward rounds: %d; open entries skipped in a last round: %d; "
          "SMEMs per call: %d; per read: %s" % (fwd_x0, last_fed_by_curr, last_fed_by_fwd, rounds, skipped, per_call, sorted(per_read.values())[-4:]))
    assert fwd_x0 > 64 and last_fed_by_fwd > 64                                    # the first backward round is the last, over more than 64 entries
    assert last_fed_by_curr > 64                                                     # a curr list past the per-entry bits feeds an i == -1 round
    for sm in (0, 1):
        assert {c[7]["fwd_len"] & 1 for c in calls if c[2] == sm and c[7]["fwd_len"] > 2} == {0, 1}, sm   # the pending LDS slot at the start of the backward sweep
        assert any(c[7]["rounds"] >= 5 and c[7]["fwd_len"] > 64 for c in calls if c[2] == sm), sm
        assert any(c[7]["last_open_skipped"] > 0 and c[7]["last_prev"] > 64 for c in calls if c[2] == sm), sm
    assert rounds >= 5
    assert any(c[7]["fwd_len"] == 2 * c[4] for c in calls if c[3] == 0)              # a forward list of 2 len entries (capacity 2 len + 2)
    assert any(c[7]["fwd_len"] == 600 for c in calls if c[0] == "nested300")         # more than 2 * 256 + 2, fewer than 2 * 512 + 2
    assert any(x == len(cs.queries[ix][nm]) - 1 and x > 0 for ix, nm in cs.names() for sm in (0, 1) for x, _, _, _ in cs.whole(ix, nm, sm)[1])   # a chain call at the last base
    assert any(64 < v <= 256 for v in per_read.values()) and per_read[("nested", "q2500", 0)] > 256 and per_read[("nested", "q2500", 1)] > 1024
    assert per_read[("nested", "q2500", 0)] <= 1024 and per_read[("nested", "q2500", 1)] <= 4096   # `exact` grows 64 -> 256 -> 1024, and on to 4096 with -s
    assert set(cs.undefined.values()) == {smem_ref.UNDEF_NO_BASE, smem_ref.UNDEF_EMPTY_FWD}
    # the chains that an undefined start ends hold SMEMs found before it, and some hold none
    cut = {k: len(cs.whole(k[0], k[1], k[3])[0]) for k in cs.undefined}
    assert all(cs.whole(k[0], k[1], k[3])[2] == v for k, v in cs.undefined.items()) and min(cut.values()) == 0 and max(cut.values()) >= 20
