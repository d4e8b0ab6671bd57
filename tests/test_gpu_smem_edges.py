"""GPU: the edges of k_smem (fermi_amd/csrc/fmd_smem.hip) -- candidate lists past the 64 per-entry bits, windows with stop > start + 1,
every seq_off % 4, the two capacity flags (bit 31 of n_mem) on buffers of exactly the stated sizes, the two starts the reference leaves
undefined, and the callers that grow their capacities (`exact`, DevIndex.smem_chain).  Every comparison is exact.  The expected
values come from tests/smem_ref.py (a plain restatement, itself compared with the oracle by test_smem_ref_host.py, which also
asserts that the cases below reach each of those paths), or from the oracle where a test says so; never from the kernel."""
import os

import numpy as np
import pytest

import orcbind
import smem_ref
from smem_ref import INTV_DT
from test_gpu_locate import DevMem, GUARD

pytestmark = pytest.mark.gpu
U64 = np.uint64
FULL = 1                      # FMD_SMEM_WIN_F_FULL
OVER = 0x80000000
MAX_LEN = {"nested": 120, "nested_non": 120, "nested300": 300}   # the longest sequence of each index: R's sweep fills 2 len of 2 len + 2 entries
INDEXES = list(MAX_LEN)
ENVS = ({}, {"FMD_SMEM_REFILL": "64"}, {"FMD_SMEM_REFILL": "1"}, {"FMD_SMEM_PATIENCE": "2"})


@pytest.fixture(scope="module")
def cs():
    return smem_ref.cases()


@pytest.fixture(scope="module")
def dev(gpu, cs):
    """the three indexes, built on the GPU from the reads (reads of one base among them) and equal to the brute-force BWT"""
    out = {}
    for index in INDEXES:
        bwt = gpu.build_bwt(cs.reads[index])
        assert np.array_equal(bwt, cs.bwt(index)), index
        out[index] = gpu.DevIndex.from_bwt(bwt)
    yield out
    for d in out.values():
        d.close()


def place(seqs, residues=None):
    """the sequences in one buffer -> (flat, offsets); residues: seq_off % 4 of each (the gaps are filled with bases, not zeros)"""
    parts, offs, cur = [], [], 0
    for k, s in enumerate(seqs):
        if residues is not None:
            gap = (residues[k] - cur) % 4
            parts.append(np.full(gap, 1 + k % 4, dtype=np.uint8)); cur += gap
        offs.append(cur)
        parts.append(np.asarray(s, dtype=np.uint8)); cur += len(s)
    return np.concatenate(parts + [np.zeros(8, dtype=np.uint8)]), offs


def windows(rows):
    w = np.zeros(len(rows), dtype=[("seq_off", "<u8"), ("seq_len", "<u4"), ("start", "<u4"), ("stop", "<u4"), ("reserved", "<u4")])
    for k, r in enumerate(rows):
        w[k] = r
    return w


def win_batch(gpu, d, flat, wins, sm, max_len, max_mem):
    n = len(wins)
    mem = np.zeros((n, max_mem), dtype=INTV_DT); n_mem = np.full(n, 0x5A5A5A5A, dtype=np.uint32)
    gpu.check(gpu.lib().fmd_smem_win_batch(d.h, n, flat.ctypes.data, len(flat), wins.ctypes.data, sm, max_len, max_mem, mem.ctypes.data, n_mem.ctypes.data))
    return mem, n_mem


def read_batch(gpu, d, reads, sm, max_len, max_mem):
    flat, off = gpu.flatten_reads(reads)
    n = len(reads)
    mem = np.zeros((n, max_mem), dtype=INTV_DT); n_mem = np.full(n, 0x5A5A5A5A, dtype=np.uint32)
    gpu.check(gpu.lib().fmd_smem_batch(d.h, n, flat.ctypes.data, off.ctypes.data, sm, max_len, max_mem, mem.ctypes.data, n_mem.ctypes.data))
    return mem, n_mem


def check_rows(mem, n_mem, want, what):
    """row i holds exactly want[i] and its count says so (bit 31 clear)"""
    assert [int(v) for v in n_mem] == [len(w) for w in want], what
    for i, w in enumerate(want):
        assert mem[i, :len(w)].tobytes() == w.tobytes(), (what, i)


# ---- single calls -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", [0, 1])
@pytest.mark.parametrize("index", INDEXES)
def test_one_window_per_start(gpu, dev, cs, index, sm):
    """[x, x + 1) at every start x of every case query, plain and with FMD_SMEM_WIN_F_FULL, in one launch: n_mem and the rows equal
    smem1; an undefined start gives 0 SMEMs and no flag"""
    names = [nm for nm in cs.queries[index] if len(cs.queries[index][nm])]
    flat, offs = place([cs.queries[index][nm] for nm in names])
    rows, want = [], []
    for flag in (0, FULL):
        for nm, o in zip(names, offs):
            for x, (m, ret, _) in enumerate(cs.single(index, nm, sm)):
                rows.append((o, len(cs.queries[index][nm]), x, x + 1, flag))
                want.append(smem_ref.full_rows(cs.ref(index), m) if flag else m)
    if sm == 0 and index != "nested_non":
        assert any(len(w) > 64 for w in want)
    mem, n_mem = win_batch(gpu, dev[index], flat, windows(rows), sm, MAX_LEN[index], max(len(w) for w in want) + 1)
    check_rows(mem, n_mem, want, (index, sm))


# ---- chains inside a window ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", [0, 1])
@pytest.mark.parametrize("index", INDEXES)
def test_windows_walk_the_chain(gpu, dev, cs, index, sm):
    """windows [a, b) with b > a + 1: the concatenation of smem1 along x -> ret while x < b; [0, len) is what `exact -s` runs on a long
    query.  stop > seq_len is clamped, start >= stop and seq_len == 0 give nothing, an undefined start ends the window there."""
    names = list(cs.queries[index])
    flat, offs = place([cs.queries[index][nm] for nm in names])
    rows, want = [], []
    for nm, o in zip(names, offs):
        q = cs.queries[index][nm]
        L = len(q)
        for a, b in ((0, L), (0, L + 7), (L // 3, 2 * L // 3 + 2), (L // 2, L // 2), (L // 2 + 1, L // 2), (max(L - 1, 0), L + 5), (L, L + 1), (L + 3, L + 9), (1, min(L, 40))):
            rows.append((o, L, a, b, 0))
            want.append(cs.whole(index, nm, sm)[0] if (a, b) == (0, L) else smem_ref.chain(cs.ref(index), q, sm, a, b)[0])
    if index == "nested":
        assert any(r[1] == 0 for r in rows) and any(len(w) > 256 for w in want)
    mem, n_mem = win_batch(gpu, dev[index], flat, windows(rows), sm, MAX_LEN[index], max(len(w) for w in want) + 1)
    check_rows(mem, n_mem, want, (index, sm))
    # FULL over whole chains
    rows = [(o, len(cs.queries[index][nm]), 0, len(cs.queries[index][nm]), FULL) for nm, o in zip(names, offs)]
    want = [smem_ref.full_rows(cs.ref(index), cs.whole(index, nm, sm)[0]) for nm in names]
    mem, n_mem = win_batch(gpu, dev[index], flat, windows(rows), sm, MAX_LEN[index], max(len(w) for w in want) + 1)
    check_rows(mem, n_mem, want, (index, sm, "full"))


# ---- address residues ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", [0, 1])
def test_every_seq_off_residue(gpu, dev, cs, sm):
    """the kernel loads the read one aligned word per four bases, by absolute address: eight sequences at seq_off % 4 = 0, 1, 2, 3 (twice),
    windows on each in one launch, equal to the same sequences placed alone and to the restatement"""
    Q = cs.queries["nested"]
    seqs = [Q["R"], Q["last_base_start"], Q["mer_N"], Q["R_tail"], Q["junk_R"], Q["len1"], cs.mers[3], Q["R"][7:90]]
    flat, offs = place(seqs, residues=[0, 1, 2, 3, 3, 2, 1, 0])
    assert [o % 4 for o in offs] == [0, 1, 2, 3, 3, 2, 1, 0]
    spans = lambda L: ((0, L), (L // 2, L // 2 + 1), (L - 1, L), (1, L))
    rows = [(o, len(s), a, b, 0) for s, o in zip(seqs, offs) for a, b in spans(len(s))]
    want = [smem_ref.chain(cs.ref("nested"), s, sm, a, b)[0] for s in seqs for a, b in spans(len(s))]
    mm = max(len(w) for w in want) + 1
    mem, n_mem = win_batch(gpu, dev["nested"], flat, windows(rows), sm, 120, mm)
    check_rows(mem, n_mem, want, sm)
    k = 0
    for s in seqs:
        alone, _ = place([s])
        m1, n1 = win_batch(gpu, dev["nested"], alone, windows([(0, len(s), a, b, 0) for a, b in spans(len(s))]), sm, 120, mm)
        assert np.array_equal(n1, n_mem[k:k + 4]) and all(m1[j, :n1[j]].tobytes() == mem[k + j, :n1[j]].tobytes() for j in range(4))
        k += 4


# ---- whole reads --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", [0, 1])
@pytest.mark.parametrize("index", INDEXES)
def test_whole_reads_under_every_refill_policy(gpu, dev, cs, monkeypatch, index, sm):
    """fmd_smem_batch: the case queries as one ragged batch (an empty read among them), and each again as 66 reads of one length --
    the wave that waits for all its lanes -- under the refill settings of test_smem_lists_and_refill_policies.  A read that meets an
    undefined start reports the SMEMs found before it, flag clear, next to reads that are whole."""
    names = list(cs.queries[index])
    reads = [cs.queries[index][nm] for nm in names]
    want = [cs.whole(index, nm, sm)[0] for nm in names]
    mm = max(len(w) for w in want) + 1
    for env in ENVS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        mem, n_mem = read_batch(gpu, dev[index], reads, sm, max(len(r) for r in reads), mm)
        check_rows(mem, n_mem, want, (index, sm, env))
        for q, w in zip(reads, want):
            if len(q):
                mem, n_mem = read_batch(gpu, dev[index], [q] * 66, sm, len(q), len(w) + 1)
                check_rows(mem, n_mem, [w] * 66, (index, sm, env, len(q)))
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("sm", [0, 1])
def test_undefined_starts_end_the_read(gpu, dev, cs, sm):
    """the kernel's rule where the reference reads a[0] of an empty vector: the read stops, n_mem = the SMEMs found before the stop
    (the chain so far), bit 31 clear, and the reads around it are whole"""
    for index in ("nested_non", "nested300"):
        und = sorted({k[1] for k in cs.undefined if k[0] == index and k[3] == sm})
        if not und:   # (a forward sweep that pushes nothing needs self_match)
            assert (index, sm) == ("nested300", 0)
            continue
        whole = (cs.R if index == "nested_non" else cs.R3)[:40]
        w_whole, _, u = smem_ref.chain(cs.ref(index), whole, sm)
        assert u is None and len(und) >= 2 and all(cs.whole(index, nm, sm)[2] is not None for nm in und)
        reads = [whole] + [x for nm in und for x in (cs.queries[index][nm], whole)]
        want = [w_whole] + [x for nm in und for x in (cs.whole(index, nm, sm)[0], w_whole)]
        mem, n_mem = read_batch(gpu, dev[index], reads, sm, max(len(r) for r in reads), 700)
        assert not (n_mem >> 31).any()
        check_rows(mem, n_mem, want, (index, sm))


# ---- the capacity contract on buffers of exactly the stated sizes -------------------------------------------------------------------------
def smem_dev(gpu, d, pool, reads, sm, max_len, max_mem, wins=None, flat=None, guard=8):
    """one fmd_smem_dev (or fmd_smem_win_dev) call; mem, n_mem and the work area are exactly as large as stated, GUARD words behind
    each, and the rows are GUARD before the call -> (mem[n, max_mem], n_mem[n]); asserts the guards"""
    L = gpu.lib()
    n = len(wins) if wins is not None else len(reads)
    wb = L.fmd_smem_work_bytes(n, max_len)
    assert wb % 8 == 0
    rows = np.full(n * max_mem * 4 + guard, GUARD, dtype=U64)
    nm = np.full(n + 2 * guard, 0x5A5A5A5A, dtype=np.uint32)
    work = np.full(wb // 8 + guard, GUARD, dtype=U64)
    d_rows, d_nm, d_work = pool.put(rows), pool.put(nm), pool.put(work)
    if wins is not None:
        gpu.check(L.fmd_smem_win_dev(d.h, None, n, pool.put(flat), pool.put(wins), sm, max_len, max_mem, d_rows, d_nm, d_work, wb))
    else:
        flat, off = gpu.flatten_reads(reads)
        gpu.check(L.fmd_smem_dev(d.h, None, n, pool.put(flat), pool.put(off), sm, max_len, max_mem, d_rows, d_nm, d_work, wb))
    d.sync()
    pool.get(d_rows, rows); pool.get(d_nm, nm); pool.get(d_work, work)
    assert (rows[n * max_mem * 4:] == GUARD).all() and (nm[n:] == 0x5A5A5A5A).all() and (work[wb // 8:] == GUARD).all(), "a guard word was written"
    return rows[:n * max_mem * 4].view(INTV_DT).reshape(n, max_mem), nm[:n].copy()


@pytest.mark.parametrize("sm", [0, 1])
def test_max_mem_overflow(gpu, dev, cs, sm):
    """bit 31 exactly when a read has more SMEMs than max_mem; the low 31 bits are the true count either way; a row that fits equals the
    reference whatever its neighbours did; nothing is written past mem, n_mem or fmd_smem_work_bytes.  max_mem around the count of
    the read with the most SMEMs (q2500) and of a small one, and 1."""
    names = list(cs.queries["nested"])
    reads = [cs.queries["nested"][nm] for nm in names]
    want = [cs.whole("nested", nm, sm)[0] for nm in names]
    k_big, k_small = len(want[names.index("q2500")]), len(want[names.index("last_base_start")])
    assert k_big > 256 and 2 < k_small < 64
    pool = DevMem(gpu)
    try:
        for max_mem in (1, k_small - 1, k_small, k_small + 1, k_big - 1, k_big, k_big + 1):
            mem, n_mem = smem_dev(gpu, dev["nested"], pool, reads, sm, max(len(r) for r in reads), max_mem)
            assert [int(v) & 0x7fffffff for v in n_mem] == [len(w) for w in want], max_mem
            assert [int(v) >> 31 for v in n_mem] == [int(len(w) > max_mem) for w in want], max_mem
            for i, w in enumerate(want):
                if len(w) <= max_mem:
                    assert mem[i, :len(w)].tobytes() == w.tobytes(), (max_mem, names[i])
                    assert (mem[i, len(w):].view(U64) == GUARD).all(), (max_mem, names[i])
    finally:
        pool.free()


def test_max_len_overflow(gpu, dev, cs):
    """whole reads: a read longer than max_len gets exactly 0x80000000 and its row is not touched, the others are right.  Windows: the
    forward sweep over R fills 2 * 120 entries: with max_len = 100 (202 entries) bit 31 is set and nothing is written past the work
    area; with max_len = 120 the result equals the reference."""
    names = ["R_tail", "R", "last_base_start", "junk_R", "mer_N"]
    reads = [cs.queries["nested"][nm] for nm in names]
    want = [cs.whole("nested", nm, 0)[0] for nm in names]
    pool = DevMem(gpu)
    try:
        mem, n_mem = smem_dev(gpu, dev["nested"], pool, reads, 0, 120, 128)
        for i, nm in enumerate(names):
            if nm == "junk_R":   # 126 bases
                assert n_mem[i] == OVER and (mem[i].view(U64) == GUARD).all()
            else:
                assert n_mem[i] == len(want[i]) and mem[i, :n_mem[i]].tobytes() == want[i].tobytes(), nm
        R = cs.queries["nested"]["R"]
        flat, _ = place([R, cs.mers[5]])
        wins = windows([(0, 120, 0, 1, 0), (120, 30, 0, 30, 0), (0, 120, 60, 61, 0)])
        want = [cs.single("nested", "R", 0)[0][0], smem_ref.chain(cs.ref("nested"), cs.mers[5], 0)[0], cs.single("nested", "R", 0)[60][0]]
        mm = max(len(w) for w in want) + 1
        mem, n_mem = smem_dev(gpu, dev["nested"], pool, None, 0, 100, mm, wins=wins, flat=flat)
        assert n_mem[0] >> 31 == 1
        for i in (1, 2):   # (the sweep from x = 60 pushes 120 entries: it fits)
            assert n_mem[i] == len(want[i]) and mem[i, :n_mem[i]].tobytes() == want[i].tobytes(), i
        mem, n_mem = smem_dev(gpu, dev["nested"], pool, None, 0, 120, mm, wins=wins, flat=flat)
        check_rows(mem, n_mem, want, "max_len = 120")
    finally:
        pool.free()


# ---- the callers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", [0, 1])
@pytest.mark.parametrize("index", INDEXES)
def test_api_smem_chain_equals_the_oracle(gpu, dev, cs, oracle_lib, index, sm):
    """DevIndex.smem_chain == OrcIndex.smem on the case queries, for both self_match values (with self_match the chain's step is not the
    forward reach).  The queries with an undefined start, by name, cannot go to the oracle: with self_match the window stops there
    (the chain so far); without, smem_chain steps over a base the index lacks as `remap` and the long path of `exact` do."""
    o = orcbind.OrcIndex(bwt=cs.bwt(index))
    undefined = {k[1] for k in cs.undefined if k[0] == index and k[3] == sm}
    n = 0
    for nm, q in cs.queries[index].items():
        got = dev[index].smem_chain(q, max_len=MAX_LEN[index], self_match=sm)
        if nm in undefined:
            if sm:
                want = cs.whole(index, nm, sm)[0]
            else:
                parts, x = [np.zeros(0, dtype=INTV_DT)], 0
                while x < len(q):
                    m, ret, _ = cs.single(index, nm, sm)[x]
                    parts.append(m)
                    x = x + 1 if ret == smem_ref.UNDEF_NO_BASE else ret
                want = np.concatenate(parts)
        else:
            assert cs.whole(index, nm, sm)[2] is None
            want = o.smem(q, sm) if len(q) else np.zeros(0, dtype=INTV_DT)
            n += 1
        assert got.tobytes() == want.tobytes(), (index, nm, sm)
        full = dev[index].smem_chain(q, max_len=MAX_LEN[index], self_match=sm, full_only=True)
        assert full.tobytes() == smem_ref.full_rows(cs.ref(index), want).tobytes(), (index, nm, sm)
    o.close()
    assert n >= 1


@pytest.mark.parametrize("flag", [(), ("-s",)])
def test_exact_cli_grows_its_capacities(gpu, cs, oracle_lib, tmp_path, flag):
    """`fermi-amd exact [-s]` on an index of both nested read sets: the 2500-base query on the short path, where max_mem grows
    64 -> 256 -> 1024 (-> 4096 with -s), and a query of more than 4096 bases around the 300-base R on the long path, where the
    bound on the match grows 256 -> 512 (600 list entries against 514).  The bytes are the output rebuilt from oracle SMEMs."""
    import subprocess
    sm = int(bool(flag))
    bwt = gpu.build_bwt(cs.reads["nested"] + cs.reads["nested300"])
    ix = smem_ref.RefIndex(bwt)
    o = orcbind.OrcIndex(bwt=bwt)
    fmd, fa = str(tmp_path / "both.fmd"), str(tmp_path / "q.fa")
    o.dump(fmd)
    qs = [(b"q2500", cs.queries["nested"]["q2500"]), (b"long", cs.long_query), (b"r", cs.R)]
    assert len(cs.long_query) > 4096
    want = b""
    for name, q in qs:
        assert smem_ref.chain(ix, q, sm)[2] is None          # no undefined start: the oracle can be asked
        m = o.smem(q, sm)
        want += smem_ref.exact_record(name, len(q), m, ix.n_seq) + b"//\n"
        if name == b"q2500":
            assert (1024 < len(m) <= 4096) if sm else (256 < len(m) <= 1024)
    assert 514 < smem_ref.smem1(ix, cs.long_query, 2000, 0)[2]["fwd_len"] <= 1026
    with open(fa, "wb") as f:
        for name, q in qs:
            f.write(b">" + name + b"\n" + np.frombuffer(b"$ACGTN", dtype=np.uint8)[q].tobytes() + b"\n")
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fermi_amd", "bin", "fermi-amd")
    assert os.path.exists(exe), "fermi-amd is not built (make cli)"
    got = subprocess.run([exe, "exact"] + list(flag) + [fmd, fa], stdout=subprocess.PIPE, check=True).stdout
    o.close()
    assert got == want
