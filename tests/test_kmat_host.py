"""CPU: the host side of `kmat` -- the command's argument checks, which come before the device is looked for, the parser of -s and the printers of the PT and
SM lines (fmdh_kmat_parse_sel, fmdh_kmat_print_pt, fmdh_kmat_print_sm); the header, the Python views and the library name the same entries."""
import os
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
A, B, D = (os.path.join(GOLD, n + ".fmd") for n in ("ctA", "ctB", "cnA"))


@pytest.mark.parametrize("args", [[], ["-d"], ["-k", "0", A, B], ["-k", "33", A, B], ["-p", "0", A, B], ["-p", "-2", A, B], ["-s", "3", A, B], ["-s", "4:3", A, B],
                                  ["-s", "0:,x:", A, B], ["-s", "1:,2:,3:", A, B], ["-s", "1:2:3", A, B], ["-s", ",", A, B], ["-s", "-1:", A, B], [A] * 9],
                         ids=lambda a: "_".join(os.path.basename(x) for x in a) or "none")
def test_kmat_usage(args):
    """bad arguments: the usage, return 1, nothing on stdout -- whether or not there is a device (before this command existed: `unrecognized command`)"""
    p = subprocess.run([AMD, "kmat"] + args, capture_output=True, timeout=60)
    assert p.returncode == 1 and b"Usage:" in p.stderr and b"fermi-amd kmat" in p.stderr and p.stdout == b""
    assert b"unrecognized" not in p.stderr and b"no usable HIP device" not in p.stderr


def test_kmat_missing_file_before_the_device(tmp_path):
    p = subprocess.run([AMD, "kmat", "-k", "21", A, B, str(tmp_path / "missing.fmd")], capture_output=True, timeout=60)
    assert p.returncode == 1 and b"missing.fmd" in p.stderr and b"no usable HIP device" not in p.stderr and b"Usage:" not in p.stderr and p.stdout == b""
    p = subprocess.run([AMD, "kmat", "-s", "3:,0:0", str(tmp_path / "absent.fmd"), B], capture_output=True, timeout=60)
    assert p.returncode == 1 and b"absent.fmd" in p.stderr and b"no usable HIP device" not in p.stderr and p.stdout == b""
    assert b"\n         kmat " in subprocess.run([AMD], capture_output=True, timeout=60).stderr


def test_sel_parser():
    assert hostlib.kmat_parse_sel(None, 3) == [(0, None)] * 3
    assert hostlib.kmat_parse_sel("3:,0:0,0:0", 3) == [(3, None), (0, 0), (0, 0)]
    assert hostlib.kmat_parse_sel(":", 1) == [(0, None)] and hostlib.kmat_parse_sel(":7", 2) == [(0, 7), (0, None)]   # missing trailing entries: `0:'
    assert hostlib.kmat_parse_sel("2:5,:,10:10", 8) == [(2, 5), (0, None), (10, 10)] + [(0, None)] * 5
    assert hostlib.kmat_parse_sel("0:4294967295,4294967294:99999999999", 2) == [(0, None), (4294967294, None)]        # 2^32 - 1 and more: no bound
    assert hostlib.kmat_parse_sel("1:,1:,1:,1:,1:,1:,1:,1:", 8) == [(1, None)] * 8
    for text, n in (("", 2), ("3", 2), ("4:3", 2), ("1:,2:,3:", 2), ("1:2:3", 2), (",", 2), ("1:,", 2), ("a:", 1), ("1: ", 1), ("-1:", 1), ("+1:", 1), (":", 0), (":", 9)):
        with pytest.raises(ValueError):
            hostlib.kmat_parse_sel(text, n)


def test_printers():
    h = np.zeros(8, dtype=np.uint64)
    assert hostlib.kmat_pt_text(h) == ""
    h[1], h[2], h[6], h[7] = 8878, 2 ** 40, 3, 7
    assert hostlib.kmat_pt_text(h) == "PT\t100\t8878\nPT\t010\t%d\nPT\t011\t3\nPT\t111\t7\n" % 2 ** 40   # ascending by pattern value, index 0 first, empty ones skipped
    assert hostlib.kmat_pt_text(np.array([5, 4], dtype=np.uint64)) == "PT\t0\t5\nPT\t1\t4\n"           # (pattern 0: possible with -p above 1)
    h = np.zeros(256, dtype=np.uint64); h[255] = 136; h[128] = 1
    assert hostlib.kmat_pt_text(h) == "PT\t00000001\t1\nPT\t11111111\t136\n"
    for bad in (np.zeros(3, dtype=np.uint64), np.zeros(1, dtype=np.uint64), np.zeros(512, dtype=np.uint64), np.zeros((2, 2), dtype=np.uint64)):
        with pytest.raises(ValueError):
            hostlib.kmat_pt_text(bad)
    assert hostlib.kmat_sm_text([5, 0, 2 ** 33], [17, 0, 2 ** 35]) == "SM\t0\t5\t17\nSM\t1\t0\t0\nSM\t2\t%d\t%d\n" % (2 ** 33, 2 ** 35)
    with pytest.raises(ValueError):
        hostlib.kmat_sm_text([1], [1, 2])


def test_views_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "fmd_hip.h")).read()
    assert "typedef struct { uint32_t min[8], max[8], present, reserved; } fmd_kmat_sel_t;" in hdr
    assert api.KMAT_SEL_DT.itemsize == 72 and api.KMAT_SEL_DT.names == ("min", "max", "present", "reserved")
    assert [api.KMAT_SEL_DT.fields[f][1] for f in api.KMAT_SEL_DT.names] == [0, 32, 64, 68]
    assert "typedef struct { uint64_t n_kmers, n_total[8], n_present[8], n_ext, overflow, widest_level, n_parts, n_retries; } fmd_kmat_stat_t;" in hdr
    assert api.KMAT_STAT_DT.itemsize == 176 and api.KMAT_STAT_DT.names == ("n_kmers", "n_total", "n_present", "n_ext", "overflow", "widest_level", "n_parts", "n_retries")
    assert [api.KMAT_STAT_DT.fields[f][1] for f in api.KMAT_STAT_DT.names] == [0, 8, 72, 136, 144, 152, 160, 168]
    assert "#define FMD_KMAT_MAX_IDX %d\n" % api.KMAT_MAX_IDX in hdr and api.KMAT_MAX_IDX == 8
    assert "#define FMD_KMAT_MIN_CAP %du" % api.KMAT_MIN_CAP in hdr and "#define FMD_KMAT_MAX_CAP (1u << 30)" in hdr and api.KMAT_MAX_CAP == 1 << 30
    assert "#define FMD_KMAT_NO_MAX 0xffffffffu" in hdr and api.KMAT_NO_MAX == 0xFFFFFFFF
    L = api.lib()
    for s in ("fmd_kmat_node_bytes", "fmd_kmat_work_bytes", "fmd_kmat_part_dev", "fmd_kmat"):
        assert s in api.ABI_SYMBOLS and hasattr(L, s) and s + "(" in hdr
    for n in range(1, 9):
        assert L.fmd_kmat_node_bytes(n) == 16 * (n + 1)
        assert L.fmd_kmat_work_bytes(n, api.KMAT_MIN_CAP) >= 2 * 16 * (n + 1) * api.KMAT_MIN_CAP and L.fmd_kmat_work_bytes(n, api.KMAT_MIN_CAP) % 16 == 0
        assert L.fmd_kmat_work_bytes(n, api.KMAT_MIN_CAP - 1) == 0 and L.fmd_kmat_work_bytes(n, api.KMAT_MAX_CAP + 1) == 0 and L.fmd_kmat_work_bytes(n, api.KMAT_MAX_CAP) > 0
    assert L.fmd_kmat_node_bytes(0) == 0 and L.fmd_kmat_node_bytes(9) == 0
    assert L.fmd_kmat_work_bytes(0, api.KMAT_MIN_CAP) == 0 and L.fmd_kmat_work_bytes(9, api.KMAT_MIN_CAP) == 0 and L.fmd_kmat_work_bytes(-1, api.KMAT_MIN_CAP) == 0
    assert L.fmd_kmat_work_bytes(3, 1 << 20) < L.fmd_kmat_work_bytes(8, 1 << 20)                         # the stride depends on the number of indexes
    for f in ("fmdh_kmat_parse_sel", "fmdh_kmat_print_pt", "fmdh_kmat_print_sm", "fmdh_main_kmat"):
        assert hasattr(hostlib.lib(), f)


def test_python_selection():
    s = api.kmat_sel(3, [(3, None), (0, 0)], present=2)
    assert s["min"][0].tolist() == [3, 0, 0, 0, 0, 0, 0, 0] and s["max"][0].tolist() == [api.KMAT_NO_MAX, 0] + [api.KMAT_NO_MAX] * 6 and int(s["present"][0]) == 2
    with pytest.raises(ValueError):
        api.kmat_sel(2, [(0, None)] * 3)
    assert callable(api.kmer_matrix_spectrum) and callable(api.kmer_matrix)
