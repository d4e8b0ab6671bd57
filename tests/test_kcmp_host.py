"""CPU: the host side of `kcmp` -- the command's argument checks, which come before the device is looked for, and the printer of the 2-D histogram
(fmdh_kcmp_print_hist); the header, the Python views and the library name the same entries."""
import os
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
A, B = os.path.join(GOLD, "ctA.fmd"), os.path.join(GOLD, "ctB.fmd")


@pytest.mark.parametrize("args", [[], [A], ["-k", "0", A, B], ["-k", "33", A, B], ["-a", "4", "-A", "3", A, B], ["-b", "1", "-B", "0", A, B], ["-n", "1", A, B],
                                  ["-n", "1025", A, B], ["-A", "many", A, B], ["-d"]])
def test_kcmp_usage(args):
    """bad arguments: the usage, return 1, nothing on stdout -- whether or not there is a device (before this command existed: `unrecognized command`)"""
    p = subprocess.run([AMD, "kcmp"] + args, capture_output=True, timeout=60)
    assert p.returncode == 1 and b"Usage:" in p.stderr and b"fermi-amd kcmp" in p.stderr and p.stdout == b""
    assert b"unrecognized" not in p.stderr and b"no usable HIP device" not in p.stderr


def test_kcmp_missing_file_before_the_device(tmp_path):
    p = subprocess.run([AMD, "kcmp", "-k", "21", A, str(tmp_path / "missing.fmd")], capture_output=True, timeout=60)
    assert p.returncode == 1 and b"missing.fmd" in p.stderr and b"no usable HIP device" not in p.stderr and p.stdout == b""
    p = subprocess.run([AMD, "kcmp", str(tmp_path / "absent.fmd"), B], capture_output=True, timeout=60)
    assert p.returncode == 1 and b"absent.fmd" in p.stderr and b"no usable HIP device" not in p.stderr and p.stdout == b""
    assert b"\n         kcmp " in subprocess.run([AMD], capture_output=True, timeout=60).stderr


def test_hist_printer():
    h = np.zeros((3, 3), dtype=np.uint64)
    assert hostlib.kcmp_hist_text(h) == ""
    h[0, 1], h[1, 0], h[1, 1], h[2, 2], h[2, 0] = 8878, 8882, 2 ** 40, 3, 7
    assert hostlib.kcmp_hist_text(h) == "0\t1\t8878\n1\t0\t8882\n1\t1\t%d\n2\t0\t7\n2\t2\t3\n" % 2 ** 40   # row-major, empty cells skipped; a label of 2 = n - 1
    assert hostlib.kcmp_hist_text(np.array([[0, 4], [0, 0]], dtype=np.uint64)) == "0\t1\t4\n"
    with pytest.raises(ValueError):
        hostlib.kcmp_hist_text(np.zeros((2, 3), dtype=np.uint64))


def test_views_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "fmd_hip.h")).read()
    assert "typedef struct { uint64_t n_kmers, n_total0, n_total1, n_only0, n_only1, n_shared, n_ext, overflow, widest_level, n_parts, n_retries; } fmd_kcmp_stat_t;" in hdr
    assert api.KCMP_STAT_DT.itemsize == 88
    assert api.KCMP_STAT_DT.names == ("n_kmers", "n_total0", "n_total1", "n_only0", "n_only1", "n_shared", "n_ext", "overflow", "widest_level", "n_parts", "n_retries")
    assert "typedef struct { uint64_t x0[2], size[2], kmer, reserved; } fmd_kcmp_node_t;" in hdr
    assert api.KCMP_NODE_DT.itemsize == 48 and api.KCMP_NODE_DT.names == ("x0", "size", "kmer", "reserved")
    assert [api.KCMP_NODE_DT.fields[f][1] for f in api.KCMP_NODE_DT.names] == [0, 16, 32, 40]
    assert "typedef struct { uint32_t min0, max0, min1, max1; } fmd_kcmp_sel_t;" in hdr
    assert api.KCMP_SEL_DT.itemsize == 16 and api.KCMP_SEL_DT.names == ("min0", "max0", "min1", "max1")
    assert "#define FMD_KCMP_MIN_CAP %du" % api.KCMP_MIN_CAP in hdr and "#define FMD_KCMP_MAX_CAP (1u << 30)" in hdr and api.KCMP_MAX_CAP == 1 << 30
    assert "#define FMD_KCMP_NO_MAX 0xffffffffu" in hdr and api.KCMP_NO_MAX == 0xFFFFFFFF
    L = api.lib()
    for s in ("fmd_kcmp_work_bytes", "fmd_kcmp_part_dev", "fmd_kcmp"):
        assert s in api.ABI_SYMBOLS and hasattr(L, s)
    assert L.fmd_kcmp_work_bytes(api.KCMP_MIN_CAP) >= 2 * 48 * api.KCMP_MIN_CAP
    assert L.fmd_kcmp_work_bytes(api.KCMP_MIN_CAP - 1) == 0 and L.fmd_kcmp_work_bytes(api.KCMP_MAX_CAP + 1) == 0
    assert hasattr(hostlib.lib(), "fmdh_kcmp_print_hist")
