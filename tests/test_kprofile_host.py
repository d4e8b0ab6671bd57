"""CPU: the host side of `kprofile` -- the command's argument checks, which come before the device is looked for; the header, the Python views and the
library name the same entries; and the three formatters (the KP line, the KS line, the quality line of -q) against their definitions restated in numpy."""
import os
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
TINY = os.path.join(GOLD, "tiny.fmd")
SPECIAL = os.path.join(GOLD, "special.fmd")


@pytest.fixture(scope="module")
def query(tmp_path_factory):
    p = tmp_path_factory.mktemp("kprofile") / "q.fa"
    p.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n>b\nacgtnACGT\n")
    return str(p)


@pytest.mark.parametrize("args", [[], ["-k", "21"], ["Q"], ["-k", "0", "Q", TINY], ["-k", str(api.KPROFILE_MAX_K + 1), "Q", TINY], ["-q", "Q", TINY, SPECIAL],
                                  ["-s", "-q", "Q", TINY]])
def test_kprofile_usage(query, args):
    """bad arguments: the usage, return 1, nothing on stdout -- whether or not there is a device (before this command existed: `unrecognized command`)"""
    p = subprocess.run([AMD, "kprofile"] + [query if a == "Q" else a for a in args], capture_output=True, timeout=60)
    assert p.returncode == 1 and b"Usage:" in p.stderr and b"fermi-amd kprofile" in p.stderr and p.stdout == b""
    assert b"unrecognized" not in p.stderr and b"no usable HIP device" not in p.stderr


def test_kprofile_missing_files_before_the_device(query, tmp_path):
    for args, name in (([query, str(tmp_path / "missing.fmd")], b"missing.fmd"), ([query, TINY, str(tmp_path / "missing2.fmd")], b"missing2.fmd"),
                       ([str(tmp_path / "missing.fa"), TINY], b"missing.fa")):
        p = subprocess.run([AMD, "kprofile", "-k", "21"] + args, capture_output=True, timeout=60)
        assert p.returncode == 1 and name in p.stderr and b"no usable HIP device" not in p.stderr and b"Usage:" not in p.stderr and p.stdout == b""
    assert b"kprofile" in subprocess.run([AMD], capture_output=True, timeout=60).stderr


def test_views_of_the_header():
    hdr = open(os.path.join(ROOT, "include", "fmd_hip.h")).read()
    assert "typedef struct { uint64_t n_windows, n_valid, n_hit, n_ext, n_table; } fmd_kprofile_stat_t;" in hdr
    assert api.KPROFILE_STAT_DT.itemsize == 40 and api.KPROFILE_STAT_DT.names == ("n_windows", "n_valid", "n_hit", "n_ext", "n_table")
    assert "#define FMD_KPROFILE_MAX_K %d\n" % api.KPROFILE_MAX_K in hdr and api.KPROFILE_MAX_K >= 255
    assert "#define FMD_KPROFILE_PLAIN  %du\n" % api.KPROFILE_PLAIN in hdr and api.KPROFILE_PLAIN == 1
    assert "#define FMD_KPROFILE_SHARED" not in hdr and not hasattr(api, "KPROFILE_SHARED")   # the shared path was measured, lost and left with its flag
    L = api.lib()
    for s in ("fmd_kprofile_dev", "fmd_kprofile_batch"):
        assert s in api.ABI_SYMBOLS and hasattr(L, s)


# ---- the formatters -----------------------------------------------------------------------------------------------------------------------------
def test_kp_line():
    assert hostlib.kprofile_kp_text(0, []) == "KP\t0\t*\n"
    assert hostlib.kprofile_kp_text(3, [7]) == "KP\t3\t7\n"
    c = np.array([0, 1, 2 ** 32 - 1, 25, 0, 0, 123456], dtype=np.uint32)           # a saturated count prints as 4294967295
    assert hostlib.kprofile_kp_text(1, c) == "KP\t1\t0,1,4294967295,25,0,0,123456\n"
    rng = np.random.default_rng(5)
    c = rng.integers(0, 2 ** 32, size=5000, dtype=np.uint64).astype(np.uint32)
    assert hostlib.kprofile_kp_text(12, c) == "KP\t12\t" + ",".join(str(int(v)) for v in c) + "\n"


def ks_want(idx, seq, k, counts):
    seq = np.asarray(seq, dtype=np.uint8)
    good = np.array([bool(((seq[j:j + k] >= 1) & (seq[j:j + k] <= 4)).all()) for j in range(max(0, len(seq) - k + 1))], dtype=bool)
    v = np.sort(np.asarray(counts, dtype=np.uint32)[good]) if len(good) else np.zeros(0, np.uint32)
    if len(v) == 0:
        return "KS\t%d\t0\t0\t*\t*\t*\t*\n" % idx
    return "KS\t%d\t%d\t%d\t%d\t%d\t%d\t%.3f\n" % (idx, len(v), int((v == 0).sum()), v[0], v[(len(v) - 1) // 2], v[-1], float(v.astype(np.float64).sum()) / len(v))


def test_ks_line():
    rng = np.random.default_rng(11)
    k = 5
    # no valid window: shorter than k, empty, every window with an N
    assert hostlib.kprofile_ks_text(0, [1, 2, 3], k, []) == "KS\t0\t0\t0\t*\t*\t*\t*\n"
    assert hostlib.kprofile_ks_text(2, [], k, []) == "KS\t2\t0\t0\t*\t*\t*\t*\n"
    assert hostlib.kprofile_ks_text(1, [1, 2, 5, 3, 4, 1, 5, 2], k, [9, 9, 9, 9]) == "KS\t1\t0\t0\t*\t*\t*\t*\n"
    # an even number of valid windows: the LOWER median
    assert hostlib.kprofile_ks_text(0, [1] * 8, k, [4, 1, 3, 2]) == "KS\t0\t4\t0\t1\t2\t4\t2.500\n"
    assert hostlib.kprofile_ks_text(0, [1] * 7, k, [4, 1, 3]) == "KS\t0\t3\t0\t1\t3\t4\t2.667\n"
    # all zeros; one window; a saturated count
    assert hostlib.kprofile_ks_text(4, [2] * 9, k, [0] * 5) == "KS\t4\t5\t5\t0\t0\t0\t0.000\n"
    assert hostlib.kprofile_ks_text(0, [1, 2, 3, 4, 1], k, [2 ** 32 - 1]) == "KS\t0\t1\t0\t4294967295\t4294967295\t4294967295\t4294967295.000\n"
    # windows with an N are left out whatever their count says (the kernel writes 0 there; the figures do not count them as zeros)
    seq = np.array([1, 2, 3, 4, 1, 5, 2, 3, 4, 1, 2, 3], dtype=np.uint8)
    cnt = np.array([6, 77, 77, 77, 77, 77, 3, 0], dtype=np.uint32)
    assert hostlib.kprofile_ks_text(0, seq, k, cnt) == "KS\t0\t3\t1\t0\t3\t6\t3.000\n" == ks_want(0, seq, k, cnt)
    for n, kk in ((200, 21), (201, 21), (64, 1), (40, 40), (300, 7)):
        seq = rng.integers(1, 5, size=n).astype(np.uint8)
        seq[rng.random(n) < 0.02] = 5
        cnt = rng.integers(0, 50, size=n - kk + 1).astype(np.uint32)
        assert hostlib.kprofile_ks_text(7, seq, kk, cnt) == ks_want(7, seq, kk, cnt)
    with pytest.raises(ValueError):
        hostlib.kprofile_ks_text(0, [1] * 8, k, [1, 2, 3])


def qual_want(length, k, counts):
    """brute force: for every base the largest count among the windows that cover it"""
    out = []
    for p in range(length):
        m = 0
        for j in range(max(0, p - k + 1), min(p, length - k) + 1):
            m = max(m, int(counts[j]))
        out.append(chr(33 + min(93, m)))
    return "".join(out)


def test_quality_line():
    k = 5
    assert hostlib.kprofile_qual_text(0, k, []) == ""
    assert hostlib.kprofile_qual_text(4, k, []) == "!!!!"                           # len < k: no window covers anything
    assert hostlib.kprofile_qual_text(5, k, [7]) == chr(40) * 5                     # len = k: the one window covers every base
    c = np.array([0, 3, 200, 1, 0, 0, 0, 0, 94], dtype=np.uint32)                   # len = 2k + 3; counts above 93 are capped
    got = hostlib.kprofile_qual_text(13, k, c)
    assert got == qual_want(13, k, c) == "!$~~~~~\"~~~~~"
    assert hostlib.kprofile_qual_text(3, 1, [2 ** 32 - 1, 93, 92]) == "~~}"
    rng = np.random.default_rng(3)
    for n, kk in ((2 * 21 + 3, 21), (300, 21), (300, 1), (120, 55), (64, 64), (500, 255)):
        c = rng.integers(0, 120, size=n - kk + 1).astype(np.uint32)
        c[rng.random(len(c)) < 0.5] = 0                                            # runs of zeros: bases no frequent window covers
        assert hostlib.kprofile_qual_text(n, kk, c) == qual_want(n, kk, c), (n, kk)
    with pytest.raises(ValueError):
        hostlib.kprofile_qual_text(10, k, [1, 2])
