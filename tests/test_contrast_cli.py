"""CPU: the contrast-assembly commands of `fermi-amd` that need no GPU -- the usage banner, and `bitand` (host/contrast_cmd.c) on the
.sub files the reference wrote (tests/golden/make_golden_contrast.py)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
K25 = os.path.join(GOLD, "contrast.k25o2.ctA-ctB.sub")
K55 = os.path.join(GOLD, "contrast.k55o3.ctA-ctB.sub")


def _run(args):
    if not os.path.exists(AMD):
        pytest.skip("fermi-amd is not built here")
    return subprocess.run([AMD] + args, capture_output=True, timeout=60)


def _bits(b):
    n = int(np.frombuffer(b[:8], np.uint64)[0])
    w = np.frombuffer(b[8:], np.uint64)
    assert len(w) == (n + 63) // 64
    return n, w


def test_usage_lists_contrast_sub_and_bitand():
    p = _run([])
    assert p.returncode == 1
    err = p.stderr.decode()
    assert "contrast   reads with k-mers the other index lacks (fermi contrast)" in err
    assert "sub        sub-index of selected reads (fermi sub)" in err
    assert "bitand     AND of bit arrays, no GPU needed (fermi bitand)" in err


def test_bitand_of_an_array_with_itself():
    p = _run(["bitand", K25, K25])
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout == open(K25, "rb").read()
    err = p.stderr.decode()
    assert err.count("[M::read_sub] loaded file `%s' containing 860 bits" % K25) == 2
    assert "[M::main_bitand] the output contains 860 bits" in err


def test_bitand_of_two_selections_is_numpys_and_the_references():
    p = _run(["bitand", K25, K55])
    assert p.returncode == 0, p.stderr.decode()
    (na, a), (nb, b) = _bits(open(K25, "rb").read()), _bits(open(K55, "rb").read())
    assert na == nb == 3000
    want = np.uint64(na).tobytes() + (a & b).tobytes()
    assert p.stdout == want
    assert p.stdout == open(os.path.join(GOLD, "contrast.and_k25_k55.ctA-ctB.sub"), "rb").read()
    n_out = int(np.unpackbits((a & b).view(np.uint8)).sum())
    assert "[M::main_bitand] the output contains %d bits" % n_out in p.stderr.decode()
    p3 = _run(["bitand", K25, K55, K25])                        # any number of arrays
    assert p3.returncode == 0 and p3.stdout == want


def test_bitand_errors_write_nothing(tmp_path):
    short = tmp_path / "short.sub"                              # another length
    short.write_bytes(np.uint64(128).tobytes() + np.zeros(2, np.uint64).tobytes())
    p = _run(["bitand", K25, str(short)])
    assert p.returncode == 1 and p.stdout == b"" and b"[E::main_bitand] unequal array length" in p.stderr
    for args in ([K25, str(tmp_path / "missing.sub")], [str(tmp_path / "missing.sub"), K25], [str(tmp_path / "m1.sub"), str(tmp_path / "m2.sub")]):
        p = _run(["bitand"] + args)
        assert p.returncode == 1 and p.stdout == b"" and b"[E::main_bitand]" in p.stderr, args
    cut = tmp_path / "cut.sub"                                  # fewer words than its length says
    cut.write_bytes(open(K25, "rb").read()[:200])
    p = _run(["bitand", K25, str(cut)])
    assert p.returncode == 1 and p.stdout == b""
    p = _run(["bitand", K25])
    assert p.returncode == 1 and b"Usage:" in p.stderr and p.stdout == b""
