"""CPU: the host side of `kcount` -- the command's argument checks, which come before the device is looked for, the text of a packed k-mer
(fmdh_kmer_text) and the histogram printer (fmdh_kcount_print_hist); the header, the Python views and the library name the same entries."""
import os
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
TINY = os.path.join(GOLD, "tiny.fmd")


@pytest.mark.parametrize("args", [[], ["-k", "0", TINY], ["-k", "33", TINY], ["-o", "0", TINY], ["-b", "1", TINY], ["-d"]])
def test_kcount_usage(args):
    """bad arguments: the usage, return 1, nothing on stdout -- whether or not there is a device (before this command existed: `unrecognized command`)"""
    p = subprocess.run([AMD, "kcount"] + args, capture_output=True, timeout=60)
    assert p.returncode == 1 and b"Usage:" in p.stderr and b"fermi-amd kcount" in p.stderr and p.stdout == b""
    assert b"unrecognized" not in p.stderr and b"no usable HIP device" not in p.stderr


def test_kcount_missing_file_before_the_device(tmp_path):
    p = subprocess.run([AMD, "kcount", "-k", "21", str(tmp_path / "missing.fmd")], capture_output=True, timeout=60)
    assert p.returncode == 1 and b"missing.fmd" in p.stderr and b"no usable HIP device" not in p.stderr and p.stdout == b""
    assert b"kcount" in subprocess.run([AMD], capture_output=True, timeout=60).stderr


def pack(s):
    v = 0
    for ch in s:
        v = v << 2 | "ACGT".index(ch)
    return v


def test_kmer_text():
    assert [hostlib.kmer_text(v, 1) for v in range(4)] == ["A", "C", "G", "T"]
    for s in ("A" * 31, "T" * 31, "A" * 32, "T" * 32, "ACGT" * 8, "TGCATTTACGGATCCAGTACGATCAAGT", "GATTACA", "C" + "A" * 31, "A" * 31 + "G"):
        assert hostlib.kmer_text(pack(s), len(s)) == s
    assert hostlib.kmer_text(2 ** 64 - 1, 32) == "T" * 32 and hostlib.kmer_text(0, 32) == "A" * 32
    assert hostlib.kmer_text(pack("ACGT"), 6) == "AAACGT"                         # the first base is the highest of the low 2k bits
    assert hostlib.kmer_text(2 ** 64 - 1, 3) == "TTT"                             # bits above 2k are not looked at
    for k in (0, 33, -1):
        with pytest.raises(ValueError):
            hostlib.kmer_text(0, k)


def test_hist_printer():
    h = np.zeros(10, dtype=np.uint64)
    assert hostlib.kcount_hist_text(h) == ""
    h[1], h[2], h[5], h[9] = 15448, 7, 2 ** 40, 3
    assert hostlib.kcount_hist_text(h) == "1\t15448\n2\t7\n5\t%d\n9\t3\n" % 2 ** 40   # empty bins skipped; the last bin is labelled n_bins - 1
    assert hostlib.kcount_hist_text(np.array([0, 4], dtype=np.uint64)) == "1\t4\n"


def test_views_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "fmd_hip.h")).read()
    assert "typedef struct { uint64_t n_kmers, n_total, n_ext, overflow, widest_level, n_parts, n_retries; } fmd_kcount_stat_t;" in hdr
    assert api.KCOUNT_STAT_DT.itemsize == 56 and api.KCOUNT_STAT_DT.names == ("n_kmers", "n_total", "n_ext", "overflow", "widest_level", "n_parts", "n_retries")
    assert "#define FMD_KCOUNT_MIN_CAP %du" % api.KCOUNT_MIN_CAP in hdr and api.KCOUNT_MIN_CAP <= 4096
    assert "#define FMD_KCOUNT_MAX_CAP (1u << 30)" in hdr and api.KCOUNT_MAX_CAP == 1 << 30
    L = api.lib()
    for s in ("fmd_kcount_work_bytes", "fmd_kcount_part_dev", "fmd_kcount"):
        assert s in api.ABI_SYMBOLS and hasattr(L, s)
    assert L.fmd_kcount_work_bytes(api.KCOUNT_MIN_CAP) >= 2 * 32 * api.KCOUNT_MIN_CAP and L.fmd_kcount_work_bytes(api.KCOUNT_MIN_CAP - 1) == 0
