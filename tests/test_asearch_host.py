"""CPU: the host side of `asearch` -- the command's argument checks, which come before the device is looked for, the pattern of a hit
(fmdh_asearch_pattern, api.approx_pattern); the header, the Python views and the library name the same entries."""
import os
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
TINY = os.path.join(GOLD, "tiny.fmd")
QUERY = os.path.join(GOLD, "tiny.fq.gz")


@pytest.mark.parametrize("args", [[], [TINY], ["-d", "5", TINY, QUERY], ["-d", "-1", TINY, QUERY], ["-m", "0", TINY, QUERY], ["-l", "-M", "0", TINY, QUERY], ["-b"]])
def test_asearch_usage(args):
    """bad arguments: the usage, return 1, nothing on stdout -- whether or not there is a device (before this command existed: `unrecognized command`)"""
    p = subprocess.run([AMD, "asearch"] + args, capture_output=True, timeout=60)
    assert p.returncode == 1 and b"Usage:" in p.stderr and b"fermi-amd asearch" in p.stderr and p.stdout == b""
    assert b"unrecognized" not in p.stderr and b"no usable HIP device" not in p.stderr


def test_asearch_missing_file_before_the_device(tmp_path):
    fa = tmp_path / "q.fa"
    fa.write_text(">q\nACGT\n")
    for args, name in ((["-d", "2", str(tmp_path / "missing.fmd"), str(fa)], b"missing.fmd"), ([TINY, str(tmp_path / "missing.fa")], b"missing.fa"),
                       (["-l", "-r", str(tmp_path / "missing.rank"), TINY, str(fa)], b"missing.rank")):
        p = subprocess.run([AMD, "asearch"] + args, capture_output=True, timeout=60)
        assert p.returncode == 1 and name in p.stderr and b"no usable HIP device" not in p.stderr and p.stdout == b"", args
    assert b"asearch" in subprocess.run([AMD], capture_output=True, timeout=60).stderr


def hit(n_sub, sub, query=0, beg=7, cnt=3):
    h = np.zeros(1, dtype=api.ASEARCH_HIT_DT)
    h[0] = (beg, cnt, query, n_sub, list(sub) + [0xFFFF] * (4 - len(sub)))
    return h[0]


def test_pattern_of_a_hit():
    q = np.array([1, 2, 3, 4, 5, 1, 1], dtype=np.uint8)                           # ACGTNAA
    assert hostlib.asearch_pattern(q, hit(0, [])).tolist() == q.tolist()
    h = hit(2, [4 << 2 | 2, 0 << 2 | 3])                                          # position 4 -> G, position 0 -> T, by descending position
    assert hostlib.asearch_pattern(q, h).tolist() == [4, 2, 3, 4, 3, 1, 1] == api.approx_pattern(q, h).tolist()
    h = hit(4, [6 << 2 | 1, 5 << 2 | 1, 1 << 2 | 0, 0 << 2 | 1])
    assert hostlib.asearch_pattern(q, h).tolist() == [2, 1, 3, 4, 5, 2, 2] == api.approx_pattern(q, h).tolist()
    for bad in (hit(1, [7 << 2]),                                                 # beyond the query
                hit(2, [0 << 2 | 1, 4 << 2 | 1]),                                 # ascending
                hit(2, [3 << 2 | 1, 3 << 2 | 2]),                                 # one position twice
                hit(1, [3 << 2 | 1, 2 << 2 | 1]),                                 # an entry beyond n_sub that is not 0xffff
                hit(2, [3 << 2 | 1]),                                             # an entry below n_sub that is
                hit(5, [])):
        with pytest.raises(ValueError):
            hostlib.asearch_pattern(q, bad)


def test_views_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "fmd_hip.h")).read()
    assert "typedef struct { uint64_t beg, cnt; uint32_t query, n_sub; uint16_t sub[4]; } fmd_asearch_hit_t;" in hdr
    assert "typedef struct { uint64_t n_hits, n_occ, n_skipped, n_truncated, n_unfinished, overflow, n_ext, widest_level; } fmd_asearch_stat_t;" in hdr
    assert api.ASEARCH_HIT_DT.itemsize == 32 and api.ASEARCH_HIT_DT.names == ("beg", "cnt", "query", "n_sub", "sub") and api.ASEARCH_HIT_DT == hostlib.ASEARCH_HIT_DT
    assert api.ASEARCH_HIT_DT.fields["sub"][1] == 24 and api.ASEARCH_HIT_DT.fields["query"][1] == 16
    assert api.ASEARCH_STAT_DT.itemsize == 64 and api.ASEARCH_STAT_DT.names == ("n_hits", "n_occ", "n_skipped", "n_truncated", "n_unfinished", "overflow", "n_ext",
                                                                               "widest_level")
    assert "#define FMD_ASEARCH_MAX_SUB %d\n" % api.ASEARCH_MAX_SUB in hdr and api.ASEARCH_MAX_SUB == 4
    assert "#define FMD_ASEARCH_MAX_LEN %du" % api.ASEARCH_MAX_LEN in hdr and api.ASEARCH_MAX_LEN == 16383
    assert "#define FMD_ASEARCH_MIN_CAP %du" % api.ASEARCH_MIN_CAP in hdr and api.ASEARCH_MIN_CAP == 4096
    assert "#define FMD_ASEARCH_MAX_CAP (1u << 28)" in hdr and api.ASEARCH_MAX_CAP == 1 << 28
    assert "#define FMD_ASEARCH_NO_PRUNE %du" % api.ASEARCH_NO_PRUNE in hdr and "#define FMD_ASEARCH_BEST %du" % api.ASEARCH_BEST in hdr
    L = api.lib()
    for s in ("fmd_asearch_work_bytes", "fmd_asearch_bound_dev", "fmd_asearch_dev", "fmd_asearch_batch"):
        assert s in api.ABI_SYMBOLS and hasattr(L, s)
    wb = L.fmd_asearch_work_bytes(100, api.ASEARCH_MIN_CAP)
    assert wb >= 2 * 32 * api.ASEARCH_MIN_CAP + 100 * 8 and wb % 16 == 0
    assert L.fmd_asearch_work_bytes(100, api.ASEARCH_MIN_CAP - 1) == 0 and L.fmd_asearch_work_bytes(100, api.ASEARCH_MAX_CAP + 1) == 0
    assert L.fmd_asearch_work_bytes(2 ** 32, api.ASEARCH_MIN_CAP) == 0
    assert L.fmd_asearch_work_bytes(10 ** 6, 1 << 20) - L.fmd_asearch_work_bytes(10 ** 6, 1 << 19) == 2 * 32 * (1 << 19)   # two frontiers of 32-byte entries


def test_argument_errors_need_no_device():
    """what fmd_asearch_batch / _dev turn down before they touch the device"""
    L = api.lib()
    st = np.zeros(1, dtype=api.ASEARCH_STAT_DT)
    strata = np.zeros(16, dtype=np.uint64)
    flat, off = api.flatten_reads([np.array([1, 2, 3], dtype=np.uint8)])
    h = 1                                                                          # (never dereferenced: every call below fails on its arguments first)
    for max_sub in (-1, 5):
        assert L.fmd_asearch_batch(h, 1, flat.ctypes.data, off.ctypes.data, max_sub, 10, 0, 0, None, None, strata.ctypes.data, st.ctypes.data) == api.FMD_E_ARG
        assert L.fmd_asearch_dev(h, None, 1, 16, 16, None, max_sub, 10, 1, None, 0, 16, 16, 16, 1 << 20) == api.FMD_E_ARG
    assert L.fmd_asearch_batch(None, 1, flat.ctypes.data, off.ctypes.data, 1, 10, 0, 0, None, None, strata.ctypes.data, st.ctypes.data) == api.FMD_E_ARG
    assert L.fmd_asearch_batch(h, 1, None, off.ctypes.data, 1, 10, 0, 0, None, None, strata.ctypes.data, st.ctypes.data) == api.FMD_E_ARG
    assert L.fmd_asearch_batch(h, 1, flat.ctypes.data, off.ctypes.data, 1, 10, 0, 0, None, None, None, st.ctypes.data) == api.FMD_E_ARG
    assert L.fmd_asearch_batch(h, 1, flat.ctypes.data, off.ctypes.data, 1, 10, 4, 0, None, None, strata.ctypes.data, st.ctypes.data) == api.FMD_E_ARG   # an unknown flag
    assert L.fmd_asearch_batch(h, 1, flat.ctypes.data, off.ctypes.data, 1, 10, 0, api.ASEARCH_MIN_CAP - 1, None, None, strata.ctypes.data, st.ctypes.data) == api.FMD_E_ARG
    assert L.fmd_asearch_batch(h, 1, flat.ctypes.data, off.ctypes.data, 1, 10, 0, api.ASEARCH_MAX_CAP + 1, None, None, strata.ctypes.data, st.ctypes.data) == api.FMD_E_ARG
    assert L.fmd_asearch_batch(h, 2 ** 32, flat.ctypes.data, off.ctypes.data, 1, 10, 0, 0, None, None, strata.ctypes.data, st.ctypes.data) == api.FMD_E_ARG
    assert L.fmd_asearch_dev(h, None, 1, None, 16, None, 1, 10, 1, None, 0, 16, 16, 16, 1 << 20) == api.FMD_E_ARG
    assert L.fmd_asearch_dev(h, None, 1, 16, 16, None, 1, 10, 1, None, 5, 16, 16, 16, 1 << 20) == api.FMD_E_ARG          # hit_cap without d_hits
    assert L.fmd_asearch_dev(h, None, 2 ** 32, 16, 16, None, 1, 10, 1, None, 0, 16, 16, 16, 1 << 20) == api.FMD_E_ARG
    assert L.fmd_asearch_bound_dev(h, None, 1, 16, 16, None) == api.FMD_E_ARG
    assert L.fmd_asearch_bound_dev(None, None, 0, None, None, None) == api.FMD_E_ARG
    assert L.fmd_asearch_dev(h, None, 0, None, None, None, 1, 10, 1, None, 0, None, None, None, 0) == api.FMD_OK         # n = 0 is a no-op
    assert L.fmd_asearch_bound_dev(h, None, 0, None, None, None) == api.FMD_OK
