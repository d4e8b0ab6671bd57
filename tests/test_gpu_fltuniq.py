"""GPU: `fermi-amd fltuniq` and the fmd_fltuniq_* entries (csrc/fmd_fltuniq.hip) -- the command against what the reference printed for
the same files (tests/golden/make_golden_readprep.py; the kept counts below are the reference's), the k-mer table and the verdicts
against a numpy restatement, batches cut anywhere, argument errors, and a mid-size paired set against the reference binary where
it is built."""
import ctypes as C
import gzip
import hashlib
import json
import math
import os
import re
import subprocess
import time

import numpy as np
import pytest

from fermi_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "fermi")
INFO = json.load(open(os.path.join(GOLD, "readprep.json")))["fltuniq"]
T_START = time.time()

# (input, -k or None for the k the file size gives) -> records `fermi fltuniq` keeps
KEPT = {
    ("tiny.fq.gz", None): 1209, ("tiny.fq.gz", 13): 1211, ("tiny.fq.gz", 11): 1211, ("tiny.fq.gz", 17): 1208, ("tiny.fq.gz", 18): 1207,
    ("tiny.ec.fq.gz", None): 1991, ("tiny.ec.fq.gz", 13): 1992, ("tiny.ec.fq.gz", 11): 1992,
    ("ctA.fq.gz", None): 1048, ("ctA.fq.gz", 13): 1048, ("ctA.fq.gz", 11): 1048,
    ("special.fq.gz", None): 152, ("special.fq.gz", 13): 155, ("special.fq.gz", 11): 160,
    ("pairs.fq.gz", None): 1367, ("pairs.fq.gz", 13): 1371, ("pairs.fq.gz", 11): 1377,
    ("pairs.cofq.fq.gz", 13): 1346,
    ("readprep.corner.fx", 5): 10, ("readprep.corner.fx", 3): 10, ("readprep.corner.fx", None): 10,
}
WITH_BYTES = ("special.fq.gz", "pairs.cofq.fq.gz", "readprep.corner.fx")


def _run(args, timeout=300, **kw):
    return subprocess.run([AMD] + args, capture_output=True, timeout=timeout, **kw)


def _ktag(k):
    return "kdef" if k is None else "k%d" % k


def _headers(out):
    ln, i, h = out.split(b"\n"), 0, []
    while i < len(ln) - 1:
        h.append(ln[i])
        i += 4 if ln[i][:1] == b"@" else 2
    return h


def _auto_k(size):
    return min(18, max(15, int(math.log(size) / math.log(4) + 1.499)))


@pytest.mark.parametrize("name,k", sorted(KEPT, key=lambda c: (c[0], c[1] or 0)))
def test_cli_writes_the_reference_bytes(gpu, name, k):
    p = _run(["fltuniq"] + ([] if k is None else ["-k%d" % k]) + [os.path.join(GOLD, name)])
    assert p.returncode == 0, p.stderr.decode()
    e = INFO["%s.%s" % (name, _ktag(k))]
    heads = _headers(p.stdout)
    assert len(heads) == KEPT[(name, k)] == e["kept"]
    assert hashlib.md5(p.stdout).hexdigest() == e["md5"]
    if name in WITH_BYTES:
        assert p.stdout == gzip.open(os.path.join(GOLD, "fltuniq.%s.%s.out.gz" % (name, _ktag(k)))).read()
    err = p.stderr.decode()
    assert "[M::main_fltuniq] building the hash table...\n" in err and "[M::main_fltuniq] filtering the reads...\n" in err
    assert ("[M::main_fltuniq] set the k-mer size as 15\n" in err) == (k is None)
    if name == "pairs.cofq.fq.gz":      # equal names are mates: every kept name twice, 25 reads went only because their mate failed
        assert all(heads.count(h) == 2 for h in set(heads))
        alone = _run(["fltuniq", "-k%d" % k, os.path.join(GOLD, "pairs.fq.gz")])
        assert len(_headers(alone.stdout)) - len(heads) == e["mate_only"] == 25


def test_corner_file_three_equal_names_and_a_two_line_record(gpu):
    p = _run(["fltuniq", "-k5", os.path.join(GOLD, "readprep.corner.fx")])
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode()
    assert "@a\n" not in out                                           # passes, holds an N, passes: nothing of the three is printed
    assert out.startswith(">b c d\nACGTACGTACGTAACCGGTT\n>c\n")         # two lines in, one line out, the comment after one space
    assert ">short\nACG\n>empty\n\n>e2 with a comment\n" in out and ">once" not in out
    assert "@q1 fastq comment\nacgtacgtacgtaacc\n+\nABCDEFGHIJKLMNOP\n" in out   # lower case counts as bases and is printed as it came


def test_pe2cofq_then_fltuniq(gpu, tmp_path):
    recs = gzip.open(os.path.join(GOLD, "pairs.fq.gz")).read().split(b"\n")
    for m in (b"/1", b"/2"):
        with open(str(tmp_path / ("m%s.fq" % m[1:].decode())), "wb") as f:
            for i in range(0, len(recs) - 1, 4):
                if recs[i].endswith(m):
                    f.write(b"\n".join(recs[i:i + 4]) + b"\n")
    cofq = _run(["pe2cofq", str(tmp_path / "m1.fq"), str(tmp_path / "m2.fq")])
    assert cofq.returncode == 0
    (tmp_path / "co.fq").write_bytes(cofq.stdout)
    p = _run(["fltuniq", "-k13", str(tmp_path / "co.fq")])
    assert p.returncode == 0 and p.stdout == gzip.open(os.path.join(GOLD, "fltuniq.pairs.cofq.fq.gz.k13.out.gz")).read()
    assert len(_headers(p.stdout)) == 1346


@pytest.mark.parametrize("name", ["tiny.fq.gz", "special.fq.gz"])
def test_default_k_comes_from_the_size_of_the_file_on_disk(gpu, tmp_path, name):
    gz = os.path.join(GOLD, name)
    plain = str(tmp_path / "plain.fq")
    with open(plain, "wb") as f:
        f.write(gzip.open(gz).read())
    outs = []
    for fn in (gz, plain):
        p = _run(["fltuniq", fn])
        assert p.returncode == 0, p.stderr.decode()
        m = re.search(r"\[M::main_fltuniq\] set the k-mer size as (\d+)\n", p.stderr.decode())
        assert m and int(m.group(1)) == _auto_k(os.path.getsize(fn))
        outs.append(p.stdout)
    assert outs[0] == outs[1]


def test_auto_k_formula(gpu):
    from fermi_amd import hostlib
    f = hostlib.lib().fmdh_fltuniq_auto_k
    f.restype = C.c_int; f.argtypes = [C.c_longlong]
    for size in (0, 1, 1000, 4 ** 13, int(4 ** 13.5), int(4 ** 13.502), int(4 ** 14.5), int(4 ** 14.502), 5 * 10 ** 8, 6 * 10 ** 8, int(4 ** 15.502),
                 int(4 ** 16.502), 10 ** 11, 10 ** 13):
        want = 15 if size < 1 else _auto_k(size)
        assert f(size) == want, size
    assert f(5 * 10 ** 8) == 15 and f(6 * 10 ** 8) == 16 and f(10 ** 13) == 18


# ---- the table and the verdicts without the reference
def _np_kmers(reads, k):
    """per read: (every base is A/C/G/T, the k-mers of its windows of k bases) -- seq.c:167-174"""
    w = np.int64(4) ** np.arange(k - 1, -1, -1, dtype=np.int64)
    out = []
    for r in reads:
        r = np.asarray(r, dtype=np.int64)
        ok = (r >= 1) & (r <= 4)
        if len(r) >= k:
            win = np.lib.stride_tricks.sliding_window_view(np.where(ok, r - 1, 0), k)
            okw = np.lib.stride_tricks.sliding_window_view(ok, k).all(axis=1)
            z = (win * w).sum(axis=1)[okw]
        else:
            z = np.zeros(0, np.int64)
        out.append((bool(ok.all()), z))
    return out


def _np_table(reads, k):
    km = _np_kmers(reads, k)
    u, cnt = np.unique(np.concatenate([z for _, z in km] + [np.zeros(0, np.int64)]), return_counts=True)
    tab = np.zeros(4 ** k // 32, dtype=np.uint64)
    state = np.where(cnt >= 2, 3, 1).astype(np.uint64) << ((u.astype(np.uint64) & np.uint64(31)) << np.uint64(1))
    np.bitwise_or.at(tab, u >> 5, state)
    twice = set(u[cnt >= 2].tolist())
    verdict = np.array([ok and all(int(x) in twice for x in z) for ok, z in km], dtype=bool)
    return tab, verdict


def _ragged(seed, n, n_frac=0.1):
    gen = synth.genome(synth.DEFAULT_SEED + seed, 4000, 100, 8)
    reads = synth.ragged_reads(synth.DEFAULT_SEED + seed + 1, n, gen, min_len=1, max_len=150, err=0.01, dup_frac=0.05)
    rng = np.random.default_rng(seed)
    reads = [np.array(r, dtype=np.uint8) for r in reads]
    for i in rng.choice(n, int(n * n_frac), replace=False):      # an N somewhere; a few codes that are no base at all
        reads[i][rng.integers(0, len(reads[i]))] = rng.choice([5, 5, 5, 0, 6, 200])
    reads[3] = np.zeros(0, np.uint8)                              # an empty read
    reads[7] = reads[8][:2].copy()                                # two bases: shorter than every k
    return reads


@pytest.mark.parametrize("k", [3, 5, 11, 16])
def test_table_and_verdicts_equal_numpy(gpu, k):
    reads = _ragged(100 + k, 1500)
    want, verdict = _np_table(reads, k)
    got = gpu.fltuniq_table(reads, k)
    assert got.dtype == np.uint64 and len(got) == 4 ** k // 32
    assert np.array_equal(got, want)
    if k <= 11:
        st = np.concatenate([(got >> np.uint64(2 * j)) & np.uint64(3) for j in range(32)])
        assert not (st == 2).any() and (st == 3).any() and (k < 11 or ((st == 1).any() and (st == 0).any()))
    ok = gpu.fltuniq_pass(reads, k)
    assert ok.dtype == bool and np.array_equal(ok, verdict)
    assert ok[3] and 0 < ok.sum() < len(ok)


def _dev(gpu, a):
    L = gpu.lib()
    p = C.c_void_p()
    gpu.check(L.fmd_dev_malloc(0, max(a.nbytes, 16), C.byref(p)))
    if a.nbytes:
        gpu.check(L.fmd_memcpy_h2d(p, a.ctypes.data, a.nbytes, None))
    return p


GUARD = 8      # 64-bit words on either side of the table, bytes on either side of the verdicts


@pytest.mark.parametrize("pieces", [1, 2, 7])
def test_count_in_pieces_gives_one_table_and_guards_stay(gpu, pieces):
    k = 11
    L = gpu.lib()
    reads = _ragged(55, 2000)
    want, verdict = _np_table(reads, k)
    flat, off = gpu.flatten_reads(reads)
    n, words = len(reads), 4 ** k // 32
    assert L.fmd_fltuniq_table_bytes(k) == words * 8
    host = np.full(words + 2 * GUARD, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    hpass = np.full(n + 2 * GUARD, 0x5A, dtype=np.uint8)
    d_seqs, d_off, d_tab, d_pass = _dev(gpu, flat), _dev(gpu, off), _dev(gpu, host), _dev(gpu, hpass)
    try:
        tab = C.c_void_p(d_tab.value + 8 * GUARD)
        gpu.check(L.fmd_memset_dev(tab, 0, words * 8, None))
        rng = np.random.default_rng(pieces)
        cuts = [0] + sorted(rng.choice(np.arange(1, n), pieces - 1, replace=False).tolist()) + [n]
        for a, b in zip(cuts[:-1], cuts[1:]):      # offsets stay absolute: a piece is a window into the offset array
            gpu.check(L.fmd_fltuniq_count_dev(0, None, k, d_seqs, C.c_void_p(d_off.value + 8 * a), b - a, tab))
        gpu.check(L.fmd_fltuniq_count_dev(0, None, k, d_seqs, d_off, 0, tab))                    # no reads: nothing happens
        gpu.check(L.fmd_fltuniq_test_dev(0, None, k, d_seqs, d_off, n, tab, C.c_void_p(d_pass.value + GUARD)))
        gpu.check(L.fmd_memcpy_d2h(host.ctypes.data, d_tab, host.nbytes, None))
        gpu.check(L.fmd_memcpy_d2h(hpass.ctypes.data, d_pass, hpass.nbytes, None))
    finally:
        for p in (d_seqs, d_off, d_tab, d_pass):
            L.fmd_dev_free(p)
    assert np.array_equal(host[GUARD:-GUARD], want)
    assert (host[:GUARD] == 0xA5A5A5A5A5A5A5A5).all() and (host[-GUARD:] == 0xA5A5A5A5A5A5A5A5).all()
    assert np.array_equal(hpass[GUARD:-GUARD].astype(bool), verdict) and set(hpass[GUARD:-GUARD].tolist()) <= {0, 1}
    assert (hpass[:GUARD] == 0x5A).all() and (hpass[-GUARD:] == 0x5A).all()


def test_argument_errors(gpu, tmp_path):
    L = gpu.lib()
    assert L.fmd_fltuniq_table_bytes(2) == 0 and L.fmd_fltuniq_table_bytes(40) == 0 and L.fmd_fltuniq_table_bytes(0) == 0
    assert L.fmd_fltuniq_table_bytes(3) == 16 and L.fmd_fltuniq_table_bytes(15) == 1 << 28 and L.fmd_fltuniq_table_bytes(18) == 1 << 34
    flat, off = gpu.flatten_reads([np.array([1, 2, 3, 4, 1], np.uint8)])
    ok = np.zeros(1, np.uint8)
    tab = np.zeros(2, np.uint64)
    for k in (2, 40, -1):
        assert L.fmd_fltuniq(0, k, flat.ctypes.data, off.ctypes.data, 1, ok.ctypes.data) == gpu.FMD_E_ARG
        assert L.fmd_fltuniq_table(0, k, flat.ctypes.data, off.ctypes.data, 1, tab.ctypes.data) == gpu.FMD_E_ARG
    assert L.fmd_fltuniq(0, 3, None, off.ctypes.data, 1, ok.ctypes.data) == gpu.FMD_E_ARG
    assert L.fmd_fltuniq(0, 3, flat.ctypes.data, None, 1, ok.ctypes.data) == gpu.FMD_E_ARG
    assert L.fmd_fltuniq(0, 3, flat.ctypes.data, off.ctypes.data, 1, None) == gpu.FMD_E_ARG
    assert L.fmd_fltuniq_table(0, 3, flat.ctypes.data, off.ctypes.data, 1, None) == gpu.FMD_E_ARG
    d = _dev(gpu, np.zeros(64, np.uint64))
    try:
        assert L.fmd_fltuniq_count_dev(0, None, 2, d, d, 1, d) == gpu.FMD_E_ARG
        assert L.fmd_fltuniq_count_dev(0, None, 40, d, d, 1, d) == gpu.FMD_E_ARG
        assert L.fmd_fltuniq_count_dev(0, None, 3, None, d, 1, d) == gpu.FMD_E_ARG
        assert L.fmd_fltuniq_count_dev(0, None, 3, d, None, 1, d) == gpu.FMD_E_ARG
        assert L.fmd_fltuniq_count_dev(0, None, 3, d, d, 1, None) == gpu.FMD_E_ARG
        assert L.fmd_fltuniq_test_dev(0, None, 2, d, d, 1, d, d) == gpu.FMD_E_ARG
        assert L.fmd_fltuniq_test_dev(0, None, 3, d, d, 1, None, d) == gpu.FMD_E_ARG
        assert L.fmd_fltuniq_test_dev(0, None, 3, d, d, 1, d, None) == gpu.FMD_E_ARG
    finally:
        L.fmd_dev_free(d)
    with pytest.raises(gpu.FmdError):
        gpu.fltuniq_pass([np.array([1, 2, 3], np.uint8)], 2)
    # the command
    p = _run(["fltuniq"])
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == "Usage: fermi-amd fltuniq [-k INT] [-g GPU] <in.fa>\n"
    missing = str(tmp_path / "none.fq")
    p = _run(["fltuniq", missing])
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == "[E::main_fltuniq] fail to open the input file\n"
    p = _run(["fltuniq", "-k", "13", missing])
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == "[E::main_fltuniq] fail to open file '%s'\n" % missing
    for k in ("2", "40"):
        p = _run(["fltuniq", "-k", k, os.path.join(GOLD, "special.fq.gz")])
        assert p.returncode == 1 and p.stdout == b"" and "[E::main_fltuniq] -k %s" % k in p.stderr.decode()
    p = _run(["fltuniq", "-g", "99", os.path.join(GOLD, "special.fq.gz")])
    assert p.returncode == 1 and p.stdout == b""


MID_READS = 200000


def test_mid_size_pairs_against_the_reference_binary(gpu, tmp_path):
    """2e5 reads of 100 bases with 0.5 % errors, mates under one name; `fltuniq` at the default k and at -k16: the reference's bytes."""
    if not os.path.exists(REF):
        pytest.skip("the reference binary is not built here (oracle/_ref/fermi)")
    rd = synth.reads(synth.DEFAULT_SEED + 41, MID_READS, 100, 30, err=0.005)
    tab = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    fq = str(tmp_path / "mid.fq")
    with open(fq, "wb") as f:
        qual = b"I" * 100
        f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i >> 1, tab[r].tobytes(), qual) for i, r in enumerate(rd)))
    for opt in ([], ["-k16"]):
        t0 = time.time()
        r = subprocess.run([REF, "fltuniq"] + opt + [fq], capture_output=True, timeout=600)
        t_ref = time.time() - t0
        t0 = time.time()
        p = _run(["fltuniq"] + opt + [fq], timeout=600)
        t_amd = time.time() - t0
        assert r.returncode == 0 and p.returncode == 0, p.stderr.decode()
        kept = len(_headers(p.stdout))
        print("fltuniq %s on %d reads: reference %.2f s, fermi-amd %.2f s; kept %d" % (" ".join(opt) or "(k = 15)", MID_READS, t_ref, t_amd, kept))
        assert hashlib.md5(p.stdout).hexdigest() == hashlib.md5(r.stdout).hexdigest()
        assert 0 < kept < MID_READS
        assert ("set the k-mer size as 15" in p.stderr.decode()) == (not opt)


def test_zz_duration_of_this_file(gpu):
    print("tests/test_gpu_fltuniq.py: %.1f s" % (time.time() - T_START))
