"""CPU: the host side of `esearch` -- the alignment of a pattern to its query (fmdh_esearch_cigar) against a plain Levenshtein table, the command's
argument checks, which come before the device is looked for; the header, the Python views and the library name the same entries."""
import os
import re
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
TINY = os.path.join(GOLD, "tiny.fmd")
QUERY = os.path.join(GOLD, "tiny.fq.gz")


def levenshtein(p, q):
    """the table in plain Python: unit costs, a base outside 1..4 equals none"""
    prev = list(range(len(q) + 1))
    for r in range(1, len(p) + 1):
        cur = [r] + [0] * len(q)
        for c in range(1, len(q) + 1):
            eq = p[r - 1] == q[c - 1] and 1 <= p[r - 1] <= 4
            cur[c] = min(prev[c - 1] + (not eq), prev[c] + 1, cur[c - 1] + 1)
        prev = cur
    return prev[len(q)]


def apply_cigar(cigar, q, p):
    """walks query and pattern along the operations; -> the operations that are not '=' (AssertionError unless the CIGAR aligns exactly these two strings)"""
    assert re.fullmatch(r"(\d+[=XID])*", cigar), cigar
    runs = [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", cigar)]
    assert all(n >= 1 for n, _ in runs) and all(a[1] != b[1] for a, b in zip(runs, runs[1:])), cigar      # run-length encoded: no empty run, no run cut in two
    i = j = cost = 0
    for n, op in runs:
        for _ in range(n):
            if op in "=X":
                assert i < len(q) and j < len(p)
                eq = q[i] == p[j] and 1 <= p[j] <= 4
                assert eq == (op == "="), (cigar, i, j)
                i, j = i + 1, j + 1
            elif op == "I":
                assert i < len(q)
                i += 1
            else:
                assert j < len(p)
                j += 1
            cost += op != "="
    assert i == len(q) and j == len(p), cigar
    return cost


def test_cigar_against_levenshtein():
    rng = np.random.default_rng(23)
    pairs = []
    for _ in range(150):                                                           # a string and a copy with a few edits of all three kinds
        q = rng.integers(1, 5, size=int(rng.integers(1, 60))).astype(np.uint8)
        p = q.tolist()
        for _ in range(int(rng.integers(0, 6))):
            at, kind = int(rng.integers(0, len(p) + 1)), int(rng.integers(3))
            if kind == 0 and at < len(p):
                p[at] = int(rng.integers(1, 5))
            elif kind == 1:
                p.insert(at, int(rng.integers(1, 5)))
            elif at < len(p) and len(p) > 1:
                del p[at]
        pairs.append((q, np.array(p, dtype=np.uint8)))
    for _ in range(60):                                                            # unrelated strings, length 1 among them: the band has to double
        pairs.append((rng.integers(1, 6, size=int(rng.integers(1, 40))).astype(np.uint8), rng.integers(1, 5, size=int(rng.integers(1, 40))).astype(np.uint8)))
    a = np.array([1, 2, 3, 4, 1, 1, 2], dtype=np.uint8)
    one = np.array([3], dtype=np.uint8)
    pairs += [(a, a[1:]), (a, a[:-1]), (a[1:], a), (a[:-1], a),                    # a pure insertion or deletion at either end
              (one, one), (one, np.array([2], dtype=np.uint8)), (one, a), (a, one), (np.array([5], dtype=np.uint8), np.array([1], dtype=np.uint8))]
    far = 0
    for q, p in pairs:
        cigar, ne = hostlib.esearch_cigar(q, p)
        want = levenshtein(p.tolist(), q.tolist())
        assert ne == want == apply_cigar(cigar, q.tolist(), p.tolist()), (q, p, cigar)
        far += want > 8
    assert far > 20
    assert hostlib.esearch_cigar(a, a) == ("7=", 0)
    assert hostlib.esearch_cigar(a, a[1:]) == ("1I6=", 1) and hostlib.esearch_cigar(a[1:], a) == ("1D6=", 1)
    assert hostlib.esearch_cigar(a, a[:-1]) == ("6=1I", 1) and hostlib.esearch_cigar(a[:-1], a) == ("6=1D", 1)
    # the tie-break: traced from the end, the diagonal first -- the gap of a run of equal bases comes out at the run's left end
    assert hostlib.esearch_cigar(np.array([2, 1, 1, 1, 3], dtype=np.uint8), np.array([2, 1, 1, 3], dtype=np.uint8)) == ("1=1I3=", 1)
    assert hostlib.esearch_cigar(np.array([5, 1], dtype=np.uint8), np.array([5, 1], dtype=np.uint8)) == ("1X1=", 1)      # an N equals nothing, itself included
    assert hostlib.esearch_cigar(np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8)) == ("", 0)


@pytest.mark.parametrize("args", [[], [TINY], ["-e", "5", TINY, QUERY], ["-e", "-1", TINY, QUERY], ["-m", "0", TINY, QUERY], ["-l", "-M", "0", TINY, QUERY], ["-b"],
                                  ["-d", "1", TINY, QUERY]])
def test_esearch_usage(args):
    """bad arguments (-d is asearch's option, not this command's): the usage, return 1, nothing on stdout -- whether or not there is a device"""
    p = subprocess.run([AMD, "esearch"] + args, capture_output=True, timeout=60)
    assert p.returncode == 1 and b"Usage:" in p.stderr and b"fermi-amd esearch" in p.stderr and p.stdout == b""
    assert b"unrecognized" not in p.stderr and b"no usable HIP device" not in p.stderr


def test_esearch_missing_file_before_the_device(tmp_path):
    fa = tmp_path / "q.fa"
    fa.write_text(">q\nACGT\n")
    for args, name in ((["-e", "2", str(tmp_path / "missing.fmd"), str(fa)], b"missing.fmd"), ([TINY, str(tmp_path / "missing.fa")], b"missing.fa"),
                       (["-l", "-r", str(tmp_path / "missing.rank"), TINY, str(fa)], b"missing.rank")):
        p = subprocess.run([AMD, "esearch"] + args, capture_output=True, timeout=60)
        assert p.returncode == 1 and name in p.stderr and b"no usable HIP device" not in p.stderr and p.stdout == b"", args
    assert b"esearch" in subprocess.run([AMD], capture_output=True, timeout=60).stderr


def test_views_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "fmd_hip.h")).read()
    assert "typedef struct { uint64_t beg, cnt; uint32_t query, n_edit, len, reserved; } fmd_esearch_hit_t;" in hdr
    assert "typedef struct { uint64_t n_hits, n_occ, n_skipped, n_truncated, n_unfinished, overflow, n_ext, widest_level; } fmd_esearch_stat_t;" in hdr
    assert api.ESEARCH_HIT_DT.itemsize == 32 and api.ESEARCH_HIT_DT.names == ("beg", "cnt", "query", "n_edit", "len", "reserved") and api.ESEARCH_HIT_DT == hostlib.ESEARCH_HIT_DT
    assert api.ESEARCH_HIT_DT.fields["query"][1] == 16 and api.ESEARCH_HIT_DT.fields["len"][1] == 24
    assert api.ESEARCH_STAT_DT.itemsize == 64 and api.ESEARCH_STAT_DT.names == ("n_hits", "n_occ", "n_skipped", "n_truncated", "n_unfinished", "overflow", "n_ext",
                                                                               "widest_level")
    assert "#define FMD_ESEARCH_MAX_EDIT %d\n" % api.ESEARCH_MAX_EDIT in hdr and api.ESEARCH_MAX_EDIT == 4
    assert "#define FMD_ESEARCH_MAX_LEN %du" % api.ESEARCH_MAX_LEN in hdr and api.ESEARCH_MAX_LEN == 16383
    assert "#define FMD_ESEARCH_MIN_CAP %du" % api.ESEARCH_MIN_CAP in hdr and api.ESEARCH_MIN_CAP == 4096
    assert "#define FMD_ESEARCH_MAX_CAP (1u << 28)" in hdr and api.ESEARCH_MAX_CAP == 1 << 28
    assert "#define FMD_ESEARCH_NO_PRUNE %du" % api.ESEARCH_NO_PRUNE in hdr and "#define FMD_ESEARCH_BEST %du" % api.ESEARCH_BEST in hdr
    L = api.lib()
    for s in ("fmd_esearch_work_bytes", "fmd_esearch_dev", "fmd_esearch_batch"):
        assert s in api.ABI_SYMBOLS and hasattr(L, s) and re.search(r"\b%s\(" % s, hdr)
    wb = L.fmd_esearch_work_bytes(100, api.ESEARCH_MIN_CAP)
    assert wb >= 2 * 32 * api.ESEARCH_MIN_CAP + 100 * 8 and wb % 16 == 0
    assert L.fmd_esearch_work_bytes(100, api.ESEARCH_MIN_CAP - 1) == 0 and L.fmd_esearch_work_bytes(100, api.ESEARCH_MAX_CAP + 1) == 0
    assert L.fmd_esearch_work_bytes(2 ** 32, api.ESEARCH_MIN_CAP) == 0
    assert L.fmd_esearch_work_bytes(10 ** 6, 1 << 20) - L.fmd_esearch_work_bytes(10 ** 6, 1 << 19) == 2 * 32 * (1 << 19)   # two frontiers of 32-byte entries
    assert hasattr(api.DevIndex, "edit_search") and hasattr(api.DevIndex, "edit_patterns")


def test_argument_errors_need_no_device():
    """what fmd_esearch_batch / _dev turn down before they touch the device"""
    L = api.lib()
    st = np.zeros(1, dtype=api.ESEARCH_STAT_DT)
    strata = np.zeros(16, dtype=np.uint64)
    flat, off = api.flatten_reads([np.array([1, 2, 3], dtype=np.uint8)])
    h = 1                                                                          # (never dereferenced: every call below fails on its arguments first)
    batch = lambda h=h, n=1, seqs=flat.ctypes.data, e=1, flags=0, cap=0, strata=strata.ctypes.data: L.fmd_esearch_batch(
        h, n, seqs, off.ctypes.data, e, 10, flags, cap, None, None, strata, st.ctypes.data)
    for max_edit in (-1, 5):
        assert batch(e=max_edit) == api.FMD_E_ARG
        assert L.fmd_esearch_dev(h, None, 1, 16, 16, None, max_edit, 10, 1, None, 0, 16, 16, 16, 1 << 20) == api.FMD_E_ARG
    assert batch(h=None) == api.FMD_E_ARG and batch(seqs=None) == api.FMD_E_ARG and batch(strata=None) == api.FMD_E_ARG
    assert batch(flags=4) == api.FMD_E_ARG                                         # an unknown flag
    assert batch(cap=api.ESEARCH_MIN_CAP - 1) == api.FMD_E_ARG and batch(cap=api.ESEARCH_MAX_CAP + 1) == api.FMD_E_ARG and batch(n=2 ** 32) == api.FMD_E_ARG
    assert L.fmd_esearch_dev(h, None, 1, None, 16, None, 1, 10, 1, None, 0, 16, 16, 16, 1 << 20) == api.FMD_E_ARG
    assert L.fmd_esearch_dev(h, None, 1, 16, 16, None, 1, 10, 1, None, 5, 16, 16, 16, 1 << 20) == api.FMD_E_ARG          # hit_cap without d_hits
    assert L.fmd_esearch_dev(h, None, 2 ** 32, 16, 16, None, 1, 10, 1, None, 0, 16, 16, 16, 1 << 20) == api.FMD_E_ARG
    assert L.fmd_esearch_dev(h, None, 0, None, None, None, 1, 10, 1, None, 0, None, None, None, 0) == api.FMD_OK         # n = 0 is a no-op
