"""CPU: the host side of `locate` -- fmdh_locate_hits (runs -> hits through seqsort's map) on hand-made runs, and the command's
argument checks, which come before the device is looked for."""
import os
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")


def runs_of(rows):
    r = np.zeros(len(rows), dtype=hostlib.LOCATE_RUN_DT)
    for i, (rank, n, off, query) in enumerate(rows):
        r[i] = (rank, n, off, query, 0)
    return r


def as_tuples(hits):
    return [(int(h["query"]), int(h["id"]), int(h["off"])) for h in hits]


def test_run_layouts_agree():
    """the two Python views of fmd_locate_run_t are the 24 bytes of include/fmd_hip.h; a hit is 16 bytes"""
    assert hostlib.LOCATE_RUN_DT == api.LOCATE_RUN_DT and api.LOCATE_RUN_DT.itemsize == 24
    assert api.LOCATE_STAT_DT.itemsize == 48 and hostlib.LOCATE_HIT_DT.itemsize == 16
    hdr = open(os.path.join(ROOT, "include", "fmd_hip.h")).read()
    assert "typedef struct { uint64_t rank; uint32_t n, off, query, reserved; } fmd_locate_run_t;" in hdr
    assert "typedef struct { uint64_t n_runs, n_rows, n_skipped, n_unfinished, overflow, n_ext; } fmd_locate_stat_t;" in hdr


def test_a_run_of_one():
    assert as_tuples(hostlib.locate_hits(runs_of([(5, 1, 7, 0)]), 8)) == [(0, 5, 7)]
    m = np.arange(8, dtype=np.uint64)[::-1] << np.uint64(2) | np.uint64(3)       # rank r -> id 7 - r, flags set
    assert as_tuples(hostlib.locate_hits(runs_of([(5, 1, 7, 0)]), 8, m)) == [(0, 2, 7)]
    assert len(hostlib.locate_hits(runs_of([]), 8)) == 0 and len(hostlib.locate_hits(runs_of([]), 0, m[:0])) == 0


def test_a_run_across_a_tie_group():
    """duplicate reads share a run: ranks 2..5 are one sequence four times over; the map scatters them over ids, the flags are dropped"""
    m = np.array([40, 41, 90 << 2 | 1, 12 << 2 | 1, 13 << 2 | 1, 88 << 2 | 1, 44, 45], dtype=np.uint64)
    m[[0, 1, 6, 7]] <<= np.uint64(2)
    got = as_tuples(hostlib.locate_hits(runs_of([(2, 4, 33, 0)]), 8, m))
    assert got == [(0, 12, 33), (0, 13, 33), (0, 88, 33), (0, 90, 33)]
    assert as_tuples(hostlib.locate_hits(runs_of([(2, 4, 33, 0)]), 8)) == [(0, 2, 33), (0, 3, 33), (0, 4, 33), (0, 5, 33)]


def test_two_queries_interleaved():
    """runs in no particular order, two queries mixed, one sequence hit twice by a query: sorted by (query, id, off)"""
    m = np.array([3, 0, 2, 1, 5, 4], dtype=np.uint64) << np.uint64(2)
    runs = runs_of([(4, 2, 9, 1), (0, 1, 30, 0), (1, 2, 2, 1), (0, 1, 4, 0), (3, 1, 0, 0), (1, 1, 1, 1)])
    want = sorted([(1, 5, 9), (1, 4, 9), (0, 3, 30), (1, 0, 2), (1, 2, 2), (0, 3, 4), (0, 1, 0), (1, 0, 1)])
    assert as_tuples(hostlib.locate_hits(runs, 6, m)) == want
    raw = sorted([(1, 4, 9), (1, 5, 9), (0, 0, 30), (1, 1, 2), (1, 2, 2), (0, 0, 4), (0, 3, 0), (1, 1, 1)])
    assert as_tuples(hostlib.locate_hits(runs, 6)) == raw


def test_a_rank_beyond_the_map_is_refused():
    """with the map exactly n_seq long and allocated on its own, a read past it would be a read out of bounds: it is an error instead"""
    m = np.arange(6, dtype=np.uint64) << np.uint64(2)
    for bad in ([(6, 1, 0, 0)], [(5, 2, 0, 0)], [(0, 1, 0, 0), (2, 5, 1, 0)], [(2 ** 63, 1, 0, 0)], [(0, 7, 0, 0)]):
        with pytest.raises(ValueError):
            hostlib.locate_hits(runs_of(bad), 6, m)
        with pytest.raises(ValueError):
            hostlib.locate_hits(runs_of(bad), 6)
    assert len(hostlib.locate_hits(runs_of([(5, 1, 0, 0), (0, 6, 1, 0)]), 6, m)) == 7
    with pytest.raises(ValueError):
        hostlib.locate_hits(runs_of([(0, 1, 0, 0)]), 6, m[:5])                 # a map shorter than the index


def test_locate_usage():
    """no arguments: the usage, return 1 (before this command existed: `unrecognized command`)"""
    for args in ([], [os.path.join(GOLD, "tiny.fmd")], ["-m", "5"], ["-m", "0", os.path.join(GOLD, "tiny.fmd"), os.path.join(GOLD, "tiny.fq.gz")]):
        p = subprocess.run([AMD, "locate"] + args, capture_output=True, timeout=60)
        assert p.returncode == 1 and b"Usage:" in p.stderr and b"fermi-amd locate" in p.stderr and b"unrecognized" not in p.stderr and p.stdout == b""
    p = subprocess.run([AMD], capture_output=True, timeout=60)
    assert b"locate" in p.stderr


def test_locate_unreadable_files_before_the_device(tmp_path):
    q, fmd = os.path.join(GOLD, "tiny.fq.gz"), os.path.join(GOLD, "tiny.fmd")
    for args, name in (([str(tmp_path / "missing.fmd"), q], b"missing.fmd"), ([fmd, str(tmp_path / "missing.fa")], b"missing.fa"),
                       (["-r", str(tmp_path / "missing.rank"), fmd, q], b"missing.rank")):
        p = subprocess.run([AMD, "locate"] + args, capture_output=True, timeout=60)
        assert p.returncode == 1 and name in p.stderr and b"no usable HIP device" not in p.stderr and p.stdout == b""
