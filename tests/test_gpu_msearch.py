"""GPU: backward search over several FMD indexes at once (fmd_multi.hip, host/msearch_cmd.c) -- fmd_multi_bsearch_batch / _dev, api.multi_backward_search and
`fermi-amd msearch` against what the reference's fm_multi_backward_search recorded (tests/golden/msearch.npz), against the single search on the
merged file and on the one-shot build of the whole, with and without the prefix-table start, over ragged batches that refill lanes out of step."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
SETS = ["tiny_special", "tiny_special_repeat", "special_palin", "dup32_palin", "tiny_tiny", "tiny_empty_special"]


@pytest.fixture(scope="module")
def npz():
    d = dict(np.load(os.path.join(GOLD, "msearch.npz")))
    sets = json.loads(bytes(d["sets"]).decode())
    assert sorted(sets) == sorted(SETS)
    return d, sets


def _queries(d, name, keep=None):
    seqs, off = d[name + ".seqs"], d[name + ".off"].astype(np.int64)
    return [seqs[off[i]:off[i + 1]] for i in range(len(off) - 1) if keep is None or keep[i]]


def _recorded(d, name):
    return tuple(d[name + ".multi_" + f] for f in ("cnt", "beg", "end"))


def _same(got, want, what=None):
    for g, w, f in zip(got, want, ("cnt", "beg", "end")):
        assert np.array_equal(g, w), (what, f, np.flatnonzero(g != w)[:5])


def _open_parts(gpu, parts):
    return [gpu.DevIndex.open(os.path.join(GOLD, p + ".fmd"), empty_ok=(p == "sub.empty")) for p in parts]


def _close(ds):
    for x in ds:
        x.close()


@pytest.mark.parametrize("name", SETS)
def test_golden_parity(gpu, npz, name):
    """(1) the recorded results of the reference over the parts, which are also DevIndex.backward_search on the merged file"""
    d, sets = npz
    parts, merged = sets[name]
    qs = _queries(d, name)
    idx = _open_parts(gpu, parts)
    got = gpu.multi_backward_search(idx, qs)
    _same(got, _recorded(d, name), name)
    m = gpu.DevIndex.open(os.path.join(GOLD, merged + ".fmd"))
    _same(got, m.backward_search(qs), name + " vs merged file")
    _close(idx + [m])


def test_one_index_equals_the_single_search(gpu, npz):
    """(2) n_idx = 1 on `special` (reads with N): fmd_bsearch_batch, for every substring of its reads in the fixture"""
    d, sets = npz
    qs = []
    for name, (parts, _) in sets.items():
        if "special" in parts:
            qs += _queries(d, name, (d[name + ".src"] == parts.index("special")) & (d[name + ".kind"] == 0))
    assert len(qs) > 1000 and any((q == 5).any() for q in qs)
    s = gpu.DevIndex.open(os.path.join(GOLD, "special.fmd"))
    want = s.backward_search(qs)
    assert (want[0] > 0).all()
    _same(gpu.multi_backward_search([s], qs), want)
    s.close()


@pytest.fixture(scope="module")
def whole(gpu):
    """3 000 reads of 30-120 bp with Ns and duplicates, the one-shot index of all of them, queries, and the single search's answers"""
    from fermi_amd import synth
    rng = np.random.default_rng(11)
    gen = synth.genome(synth.DEFAULT_SEED + 5, 20000, 100, 10)
    reads = synth.ragged_reads(synth.DEFAULT_SEED + 77, 2700, gen, min_len=30, max_len=120, err=0.02)
    for r in reads[::9]:
        r[rng.integers(0, len(r), size=2)] = 5                                 # Ns
    reads += [reads[i].copy() for i in rng.integers(0, len(reads), size=300)]  # duplicates
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    assert len(reads) == 3000 and min(map(len, reads)) >= 30 and max(map(len, reads)) <= 120
    qs = []
    for _ in range(1500):
        r = reads[int(rng.integers(len(reads)))]
        ln = int(rng.integers(1, len(r) + 1)); at = int(rng.integers(0, len(r) - ln + 1))
        q = r[at:at + ln].copy()
        if rng.random() < 0.4:
            q[int(rng.integers(ln))] = int(rng.integers(1, 6))
        qs.append(q)
    qs += [rng.integers(1, 6, size=int(rng.integers(1, 11))).astype(np.uint8) for _ in range(500)]
    w = gpu.DevIndex.from_bwt(gpu.build_bwt(reads))
    want = w.backward_search(qs)
    assert 0.2 < (want[0] > 0).mean() < 0.9
    w.close()
    return reads, qs, want


@pytest.mark.parametrize("n_parts", [1, 2, 3, 5, 16])
def test_parts_against_the_whole(gpu, whole, n_parts):
    """(3) the reads cut into parts of very unequal size, in order -- one part a single read, one part empty (sub.empty.fmd) --, each part built:
    the multi search is the single search on the one-shot build of the whole (which test_gpu_merge pins to the merge of the parts)"""
    reads, qs, want = whole
    assert n_parts in (1, 2, 3, 5, gpu.FMD_MULTI_MAX)
    n = len(reads)
    if n_parts == 1:
        cuts, empty_at = [0, n], None
    elif n_parts == 2:
        cuts, empty_at = [0, 1, n], None
    else:                                             # a single read, the empty index, then sizes 1 : 2 : 4 : ..
        m = n_parts - 2
        sizes = np.array([1 << i for i in range(m)], dtype=np.float64)
        inner = 1 + np.floor(np.cumsum(sizes)[:-1] / sizes.sum() * (n - 1)).astype(int)
        cuts, empty_at = [0, 1] + inner.tolist() + [n], 1
        for i in range(1, len(cuts) - 1):             # (the smallest shares of 16 parts round to no read at all: at least one each)
            cuts[i] = max(cuts[i], cuts[i - 1] + 1)
    assert len(set(cuts)) == len(cuts) and cuts == sorted(cuts) and cuts[-1] == n
    idx = [gpu.DevIndex.from_bwt(gpu.build_bwt(reads[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]
    if empty_at is not None:
        idx.insert(empty_at, gpu.DevIndex.open(os.path.join(GOLD, "sub.empty.fmd"), empty_ok=True))
        assert idx[empty_at].n == 0 and not idx[empty_at].cnt.any()
    assert len(idx) == n_parts and sum(x.n for x in idx) == 2 * sum(len(r) + 1 for r in reads)
    _same(gpu.multi_backward_search(idx, qs), want, n_parts)
    _close(idx)


def test_lanes_and_refill(gpu, npz, gold):
    """(4) batches of 0, 1, 63, 64, 65 and 1 000 queries of lengths 0, 1, 2 and ragged 3..150, hits and early misses interleaved: a wave's lanes finish
    and refill out of step, the last wave is not full.  tiny + special against the merged file; the _dev form with its work area once more"""
    rng = np.random.default_rng(5)
    reads = gold.fastq_nt6("tiny.fq.gz") + gold.fastq_nt6("special.fq.gz")
    idx = _open_parts(gpu, ["tiny", "special"])
    m = gpu.DevIndex.open(os.path.join(GOLD, "merge.tiny_special.fmd"))

    def query(i):
        ln = [0, 1, 2][i % 7] if i % 7 < 3 else int(rng.integers(3, 151))
        r = reads[int(rng.integers(len(reads)))]
        if ln <= len(r) and i % 3:
            at = int(rng.integers(0, len(r) - ln + 1))
            q = r[at:at + ln].copy()
            if i % 5 == 0 and ln:
                q[int(rng.integers(ln))] = 5                                    # a miss some way in
            return q
        return rng.integers(1, 5, size=ln).astype(np.uint8)                     # a miss after a dozen bases
    for n in (0, 1, 63, 64, 65, 1000):
        qs = [query(i) for i in range(n)]
        got = gpu.multi_backward_search(idx, qs)
        want = m.backward_search(qs)
        _same(got, want, n)
        assert len(got[0]) == n
        if n == 1000:
            assert 0.2 < (want[0] > 0).mean() < 0.8 and min(map(len, qs)) == 0 and max(map(len, qs)) > 140
            _same(_search_dev(gpu, idx, qs), want, "_dev")
    _close(idx + [m])


def _search_dev(gpu, idx, qs):
    """fmd_multi_bsearch_dev on device copies, poisoned outputs, the work area it asks for"""
    L = gpu.lib()
    flat, off = gpu.flatten_reads(qs)
    n = len(off) - 1
    hs = (C.c_void_p * len(idx))(*[x.h for x in idx])
    wb = L.fmd_multi_bsearch_work_bytes(len(idx), n)
    assert wb > 0
    out = [np.full(n, 0x5555555555555555, np.uint64) for _ in range(3)]
    ptrs = []
    try:
        for b in (flat.nbytes, off.nbytes, n * 8, n * 8, n * 8, wb):
            p = C.c_void_p()
            gpu.check(L.fmd_dev_malloc(0, b, C.byref(p)))
            ptrs.append(p)
        d_seq, d_off, d_c, d_b, d_e, d_w = ptrs
        gpu.check(L.fmd_memcpy_h2d(d_seq, flat.ctypes.data, flat.nbytes, None))
        gpu.check(L.fmd_memcpy_h2d(d_off, off.ctypes.data, off.nbytes, None))
        for p, a in zip((d_c, d_b, d_e), out):
            gpu.check(L.fmd_memcpy_h2d(p, a.ctypes.data, a.nbytes, None))
        assert L.fmd_multi_bsearch_dev(len(idx), hs, None, n, d_seq, d_off, d_c, d_b, d_e, d_w, wb - 1) == gpu.FMD_E_ARG   # a work area too small
        gpu.check(L.fmd_multi_bsearch_dev(len(idx), hs, None, n, d_seq, d_off, d_c, d_b, d_e, d_w, wb))
        gpu.check(L.fmd_dev_sync(idx[0].h, None))
        for p, a in zip((d_c, d_b, d_e), out):
            gpu.check(L.fmd_memcpy_d2h(a.ctypes.data, p, a.nbytes, None))
    finally:
        for p in ptrs:
            L.fmd_dev_free(p)
    return tuple(out)


@pytest.mark.parametrize("name", SETS)
def test_table_start_changes_nothing(gpu, npz, name, monkeypatch):
    """(5) the parts opened with prefix tables of one depth (FMD_PTAB_DEPTH=4: the search starts four bases in where EVERY part holds those bases) and
    with the default depths (tiny 7, special 5, ..: no table start unless they agree); two-base blocks on one handle only.  Always the recorded results."""
    d, sets = npz
    parts, _ = sets[name]
    qs, want = _queries(d, name), _recorded(d, name)
    monkeypatch.setenv("FMD_PTAB_DEPTH", "4")
    idx = _open_parts(gpu, parts)
    monkeypatch.delenv("FMD_PTAB_DEPTH")
    _same(gpu.multi_backward_search(idx, qs), want, name + " depth 4")
    if name == "dup32_palin":
        # both tables are four deep here (8*10^6 and 5*10^4 symbols), and some query's last four bases are in one part's table and absent from the other's
        tails = [q[-4:] for q in qs if len(q) >= 4 and (q[-4:] <= 4).all()]
        hit = np.stack([x.backward_search(tails)[0] > 0 for x in idx])
        assert len(tails) > 1000 and (hit.any(0) & ~hit.all(0)).sum() > 50 and hit.all(0).sum() > 50
    assert idx[0].build_pairs()                                                # two-base blocks on the first handle only: not used, nothing changes
    _same(gpu.multi_backward_search(idx, qs), want, name + " pairs on one handle")
    _close(idx)
    idx = _open_parts(gpu, parts)                                              # default depths
    _same(gpu.multi_backward_search(idx, qs), want, name + " default depths")
    _close(idx)


def test_argument_errors(gpu):
    """(6) n_idx = 0, n_idx = FMD_MULTI_MAX + 1, a null handle: FMD_E_ARG; n = 0: nothing happens; the same handle FMD_MULTI_MAX times is legal"""
    L = gpu.lib()
    t = gpu.DevIndex.open(os.path.join(GOLD, "tiny.fmd"))
    q = [np.array([1, 2, 3, 4], np.uint8)]
    flat, off = gpu.flatten_reads(q)
    out = [np.full(1, 7, np.uint64) for _ in range(3)]
    args = (1, flat.ctypes.data, off.ctypes.data) + tuple(a.ctypes.data for a in out)
    many = (C.c_void_p * (gpu.FMD_MULTI_MAX + 1))(*[t.h] * (gpu.FMD_MULTI_MAX + 1))
    assert L.fmd_multi_bsearch_batch(0, many, *args) == gpu.FMD_E_ARG
    assert L.fmd_multi_bsearch_batch(gpu.FMD_MULTI_MAX + 1, many, *args) == gpu.FMD_E_ARG
    assert L.fmd_multi_bsearch_batch(2, (C.c_void_p * 2)(t.h, None), *args) == gpu.FMD_E_ARG
    assert [int(a[0]) for a in out] == [7, 7, 7]
    assert L.fmd_multi_bsearch_batch(1, many, 0, *args[1:]) == gpu.FMD_OK and [int(a[0]) for a in out] == [7, 7, 7]
    with pytest.raises(gpu.FmdError):
        gpu.multi_backward_search([], q)
    one = t.backward_search(q)
    got = gpu.multi_backward_search([t] * gpu.FMD_MULTI_MAX, q)
    assert int(one[0][0]) > 0 and int(got[0][0]) == gpu.FMD_MULTI_MAX * int(one[0][0]) and int(got[1][0]) == gpu.FMD_MULTI_MAX * int(one[1][0])
    t.close()


def test_an_empty_file_opens_only_on_request(gpu, npz):
    """sub.empty.fmd is refused as before by the plain open and with FMD_OPEN_NO_TABLES alone; with FMD_OPEN_EMPTY_OK it is a handle of no rows, with
    or without tables, and as the only part every query misses"""
    d, _ = npz
    L = gpu.lib()
    fn = os.path.join(GOLD, "sub.empty.fmd")
    h = C.c_void_p()
    assert L.fmd_dev_open_file(0, fn.encode(), C.byref(h)) == gpu.FMD_E_ARG
    assert L.fmd_dev_open_file_ex(0, fn.encode(), 1, C.byref(h)) == gpu.FMD_E_ARG
    with pytest.raises(gpu.FmdError):
        gpu.DevIndex.open(fn)
    qs = _queries(d, "tiny_empty_special")[:200]
    for flags in (gpu.FMD_OPEN_EMPTY_OK, gpu.FMD_OPEN_EMPTY_OK | 1):
        gpu.check(L.fmd_dev_open_file_ex(0, fn.encode(), flags, C.byref(h)))
        e = gpu.DevIndex(h)
        assert e.n == 0 and not e.cnt.any() and not e.mcnt.any()
        got = gpu.multi_backward_search([e], qs)
        assert all(len(g) == len(qs) and not g.any() for g in got)
        e.close()


def test_msearch_cli_takes_an_empty_file(gpu, npz, tmp_path):
    """`fermi-amd msearch` with sub.empty.fmd between tiny.fmd and special.fmd: the counts of tiny + special"""
    d, _ = npz
    qs = _queries(d, "tiny_empty_special")[:500]
    fa = tmp_path / "q.fa"
    with open(fa, "w") as f:
        for i, q in enumerate(qs):
            f.write(">q%d\n%s\n" % (i, "".join("$ACGTN"[c] for c in q)))
    p = subprocess.run([AMD, "msearch", str(fa)] + [os.path.join(GOLD, x + ".fmd") for x in ("tiny", "sub.empty", "special")], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    rows = [ln.split("\t") for ln in p.stdout.decode().splitlines()]
    cnt, beg, end = _recorded(d, "tiny_empty_special")
    assert len(rows) == len(qs) and (cnt[:500] > 0).any()
    for i, r in enumerate(rows):
        assert r[2:] == [str(int(cnt[i])), str(int(beg[i])), str(int(end[i]))], i


def test_msearch_cli(gpu, npz, tmp_path):
    """(7) `fermi-amd msearch` over tiny.rle.fmd (RLE\\6) and special.fmd (RLD\\2): name, length and the recorded count / beg / end of every query, in order"""
    d, _ = npz
    qs = _queries(d, "tiny_special")
    fa = tmp_path / "q.fa"
    with open(fa, "w") as f:
        for i, q in enumerate(qs):
            f.write(">q%d\n%s\n" % (i, "".join("$ACGTN"[c] for c in q)))
    p = subprocess.run([AMD, "msearch", str(fa), os.path.join(GOLD, "tiny.rle.fmd"), os.path.join(GOLD, "special.fmd")], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    rows = [ln.split("\t") for ln in p.stdout.decode().splitlines()]
    assert len(rows) == len(qs)
    cnt, beg, end = _recorded(d, "tiny_special")
    for i, r in enumerate(rows):
        assert r == ["q%d" % i, str(len(qs[i])), str(int(cnt[i])), str(int(beg[i])), str(int(end[i]))], i
    assert (cnt == 0).any() and rows[int(np.flatnonzero(cnt == 0)[0])][2:] == ["0", "0", "0"]
