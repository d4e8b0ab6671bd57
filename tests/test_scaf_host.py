"""CPU: the host side of `scaf` that needs no device (host/scaf_stat.c, scaf_core.c) against what the reference computed
(tests/golden/make_golden_scaf.py): the local alignment with coordinates, the incomplete beta function, the reader with rdist and A, and the
choice of links with its table replay, the P-values of the recorded gaps, and the command's usage text."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from fermi_amd import hostlib
from scaf_restate import NONE, restate

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
AMD = os.path.join(os.path.dirname(HERE), "fermi_amd", "bin", "fermi-amd")
META = json.load(open(os.path.join(GOLD, "scaf.json")))


def test_sw_align_coordinates():
    vec = json.load(open(os.path.join(GOLD, "scaf.sw.json")))
    lens = set(len(v["q"]) for v in vec)
    assert {1, 15, 16, 17, 340} <= lens and len(vec) > 100
    assert any(v["score"] == 0 for v in vec)                                                      # no alignment at all
    assert any(v["qb"] == 0 and v["te"] == len(v["t"]) - 1 and v["score"] >= 15 for v in vec)      # an end-to-end overlap
    bad = []
    for v in vec:
        got = hostlib.sw_align(v["q"].encode(), v["t"].encode())
        if got != (v["score"], v["te"], v["qe"], v["tb"], v["qb"]):
            bad.append((len(v["q"]), len(v["t"]), got, (v["score"], v["te"], v["qe"], v["tb"], v["qb"])))
    assert not bad, bad[:5]


def test_incomplete_beta():
    vec = json.load(open(os.path.join(GOLD, "scaf.stat.json")))["betai"]
    assert {v["a"] for v in vec} >= {0.5, 1.0, 25.0}                                              # 1, 2 and 50 degrees of freedom
    assert any(v["x"] < (v["a"] + 1) / (v["a"] + v["b"] + 2) for v in vec) and any(v["x"] >= (v["a"] + 1) / (v["a"] + v["b"] + 2) for v in vec)
    for v in vec:
        assert hostlib.scaf_betai(v["a"], v["b"], v["x"]).hex() == v["v"], v


def _mag(name):
    return os.path.join(GOLD, {"hand": "scaf.hand.mag", "hand2": "scaf.hand2.mag.gz"}.get(name, name + ".remapped.mag.gz"))


def _max_dist(name):
    return int(float(META[name]["avg"]) + 2. * float(META[name]["std"]) + .499)


def _unpatched(line):
    f = line.split("\t")
    if f[0] == "LK" and len(f) >= 9:
        f[8] = "-"
    return "\t".join(f)


@pytest.mark.parametrize("name", ["hand", "hand2", "scaf0", "scaf1", "scaf2"])
def test_choice_of_links_replays_the_reference_table(name):
    """The best two neighbours of every end, with the link stage restated in Python (tests/scaf_restate.py) and the choice made by
    fmdh_scaf_choose.  hand2 holds ends with 5, 13 and 26 neighbours of equal weight and ties at the ends behind them: its lines depend on the
    table's growth through 4, 8, 16, 32 and 64 buckets and on the bucket count carried from one end to the next.  No gap is patched on the
    host, so on the generated sets the patch field of a link is left out of the comparison; the hand-written ones have none."""
    got = hostlib.scaf_link_lines(_mag(name), restate, _max_dist(name), avg=META[name]["avg"], std=META[name]["std"])
    want = [l for l in META[name]["lines"] if not l.startswith("SW\t")]
    assert [_unpatched(l) for l in got] == [_unpatched(l) for l in want]
    if name.startswith("hand"):
        assert got == want
    if name == "hand2":
        ties = [l.split("\t") for l in got if l.startswith("LK") and len(l.split("\t")) >= 11 and l.split("\t")[7] == l.split("\t")[10]]
        assert len(ties) >= 6


@pytest.mark.parametrize("name", ["scaf0", "scaf1", "scaf2"])
def test_p_values_of_the_recorded_gaps(name):
    """The corrected mean (scaf.c:371-378) is a static function of the reference and cannot be recorded on its own.  It is pinned here through
    what it feeds: for every patched link of a fixture, the pair distances behind it (restated link stage), the gap length the reference
    found and the fixture's read length give fmdh_scaf_pvalue(n, sum, sum2, fmdh_scaf_correct_mean(2 max_len + l, avg, std)), and that must
    print the t of the reference's LK line."""
    avg, std, max_len = float(META[name]["avg"]), float(META[name]["std"]), META[name]["recipe"]["rlen"]
    lines, d = hostlib.scaf_link_lines(_mag(name), restate, _max_dist(name), details=True)
    kid, checked = {}, 0
    for l in lines:
        f = l.split("\t")
        kid[f[2]] = 2 * int(f[1].split(":")[0]) + int(f[1].split(":")[1])
    for l in META[name]["lines"]:
        f = l.split("\t")
        if f[0] != "LK" or len(f) < 9 or not f[8].startswith("1:"):
            continue
        p, q, gap = kid[f[2]], kid[f[6]], int(f[8].split(":")[1])
        if p > q:
            continue
        sel = (d["utig"] == (p >> 1)) & (d["own"] != NONE) & (d["mate"] != NONE) & ((d["mate"] >> 32) == q)
        dist = (d["own"][sel] & 0xffffffff).astype(int) + (d["mate"][sel] & 0xffffffff).astype(int) + gap
        t = hostlib.lib().fmdh_scaf_pvalue(len(dist), int(dist.sum()), int((dist * dist).sum()), hostlib.scaf_correct_mean(2 * max_len + gap, avg, std))
        assert "%.1e" % t == f[8].split(":")[2], l
        checked += 1
    assert checked >= 3


def test_reader_rdist_and_A():
    for name in ("scaf0", "scaf1", "scaf2", "hand", "hand2"):
        path = _mag(name)
        rdist, us = hostlib.scaf_unitigs(path)
        lk = [l.split("\t") for l in META[name]["lines"] if l.startswith("LK\t")]
        assert len(lk) == 2 * len(us) > 0 and rdist > 0
        for f in lk:
            u = us[int(f[1].split(":")[0])]
            side = int(f[1].split(":")[1])
            assert (str(u["k"][side]), str(u["len"]), str(u["nsr"]), "%.2f" % u["A"]) == (f[2], f[3], f[4], f[5]), f
    assert hostlib.scaf_unitigs(os.path.join(GOLD, "scaf.nour.mag"))[1] == []


def test_usage_without_arguments():
    p = subprocess.run([AMD, "scaf"], capture_output=True)
    assert p.returncode == 1 and p.stdout == b""
    err = p.stderr.decode()
    assert err.startswith("\nUsage:   fermi-amd scaf [options] <in.fmd> <in.remapped.mag> <avg> <std>\n\nOptions: -t INT")
    for opt, dflt in (("-m INT", "[5]"), ("-a FLOAT", "[20]"), ("-p FLOAT", "[1e-20]"), ("-P ", ""), ("-g INT", "[0]")):
        assert any(opt in l and dflt in l for l in err.split("\n")), opt
