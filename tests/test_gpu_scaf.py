"""GPU: `fermi-amd scaf` against what `fermi scaf -Pt1` printed for the same input (tests/golden/make_golden_scaf.py): the scaftig FASTA byte for
byte and the LK / CT / SW lines of stderr.  Each step that uses the GPU is a process of its own under its own `timeout`."""
import gzip
import hashlib
import json
import os
import re
import subprocess
import time

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "fermi")
META = json.load(open(os.path.join(GOLD, "scaf.json")))


def _run(args, seconds=120, **kw):
    return subprocess.run(["timeout", "-k", "10", str(seconds), AMD] + args, capture_output=True, **kw)


def _step(args, seconds=120, **kw):
    p = _run(args, seconds, **kw)
    assert p.returncode == 0, (args, p.returncode, p.stderr.decode(errors="replace")[-2000:])
    return p.stdout


def _gold(name):
    return gzip.open(os.path.join(GOLD, name)).read()


def _links(err):
    return [l for l in err.decode().split("\n") if l[:3] in ("LK\t", "CT\t", "SW\t")]


def _scaf(name, extra=(), mag=None):
    m = META[name]
    t0 = time.time()
    p = _run(["scaf", "-P"] + list(extra) + [os.path.join(GOLD, "pairs.fmd" if name.startswith("hand") else name + ".fmd"),
                                             mag or os.path.join(GOLD, {"hand": "scaf.hand.mag", "hand2": "scaf.hand2.mag.gz"}.get(name, name + ".remapped.mag.gz")), m["avg"], m["std"]])
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    return p.stdout, _links(p.stderr), time.time() - t0


@pytest.mark.parametrize("name", ["scaf0", "scaf1", "scaf2"])
def test_fixture(gpu, name):
    out, lines, wall = _scaf(name, ["-t1"])
    want = META[name]["lines"]
    first = next((i for i, (a, b) in enumerate(zip(lines, want)) if a != b), None)
    assert lines == want, (first, lines[first] if first is not None else len(lines), want[first] if first is not None else len(want))
    assert out == _gold(name + ".scaf.fa.gz") and out.count(b">") == META[name]["scaftigs"] < META[name]["unitigs"]
    if os.path.exists(REF):                              # both wall times, for the record; nothing is asserted on them
        t0 = time.time()
        subprocess.run([REF, "scaf", "-Pt1", os.path.join(GOLD, name + ".fmd"), os.path.join(GOLD, name + ".remapped.mag.gz"), META[name]["avg"], META[name]["std"]], capture_output=True)
        print("%s: fermi-amd scaf %.2f s, fermi scaf %.2f s" % (name, wall, time.time() - t0))


def test_threads_change_nothing_but_the_order_of_sw_lines(gpu):
    out, lines, _ = _scaf("scaf1", ["-t4"])
    assert out == _gold("scaf1.scaf.fa.gz") and sorted(lines) == sorted(META["scaf1"]["lines"])


def test_other_thresholds(gpu):
    m = META["scaf1"]
    out, lines, _ = _scaf("scaf1", ["-t1"] + m["alt_args"])
    assert lines == m["alt_lines"] and out == _gold("scaf1.scaf_m3_a10_p1e-5.fa.gz")
    assert lines != m["lines"]


def test_hand_written_mag_pins_the_order_of_equal_neighbours(gpu):
    out, lines, _ = _scaf("hand", ["-t1"])
    assert lines == META["hand"]["lines"] and out.decode() == META["hand"]["fa"]
    tie = [l.split("\t") for l in lines if l.startswith("LK\t0:1\t")][0]
    assert tie[7] == tie[10] and tie[6] != tie[9]


def test_table_growth_and_carried_bucket_count(gpu):
    """ends with 5, 13 and 26 neighbours of equal weight, and ties at the ends behind them (tests/golden/make_golden_scaf.py, build_hand2)"""
    out, lines, _ = _scaf("hand2", ["-t1"])
    assert lines == META["hand2"]["lines"] and hashlib.md5(out).hexdigest() == META["hand2"]["fa_md5"]


def test_no_ur_tag_gives_nothing(gpu):
    p = _run(["scaf", "-P", os.path.join(GOLD, "pairs.fmd"), os.path.join(GOLD, "scaf.nour.mag"), "300", "30"])
    assert p.returncode == 0 and p.stdout == b"" and _links(p.stderr) == []


def test_read_id_beyond_the_index(gpu, tmp_path):
    """The reference asserts (scaf.c:362); here a message and a non-zero exit.  The reads must be ones whose mates would be fetched: five
    pairs (min_supp) between two ends, one of them with an id the index does not hold."""
    text = open(os.path.join(GOLD, "scaf.hand.mag")).read().split("\n")
    recs = ["\n".join(text[i:i + 4]) + "\n" for i in range(0, len(text) - 1, 4)]
    big = 4000                                             # pairs.fmd holds 1400 reads
    ur = lambda rec, entries: re.sub(r"UR:Z:\S*", "UR:Z:" + "".join(entries), rec)
    a = ur(recs[0], ["%d,%d,%d;" % (r << 1, 800 + i, 860 + i) for i, r in enumerate([200, 202, 204, 206, big])])
    b = ur(recs[1], ["%d,%d,%d;" % ((r + 1) << 1 | 1, 20 + i, 80 + i) for i, r in enumerate([200, 202, 204, 206, big])])
    mag = tmp_path / "big.mag"
    mag.write_text(a + b)
    p = _run(["scaf", "-P", os.path.join(GOLD, "pairs.fmd"), str(mag), "300", "30"])
    assert p.returncode == 1 and b"is not in the index" in p.stderr and p.stdout == b""


def test_whole_chain_from_reads(gpu, tmp_path):
    """build -> seqrank -> unitig -r -> clean -> clean -CAOFo 30 -> remap -r -> scaf with fermi-amd alone, on the reads of one fixture;
    every stage is compared, so a failure names the first stage that differs."""
    fmd, rank, c2, rm = (str(tmp_path / n) for n in ("r.fmd", "r.rank", "c2.mag", "rm.mag"))
    _step(["build", "-fo", fmd, os.path.join(GOLD, "scaf0.reads.fa.gz")])
    assert open(fmd, "rb").read() == open(os.path.join(GOLD, "scaf0.fmd"), "rb").read(), "build"
    open(rank, "wb").write(_step(["seqrank", fmd]))
    md5 = META["scaf0"]["md5"]                               # of the reference's output of each stage
    mag = _step(["unitig", "-l35", "-r", rank, fmd])
    assert hashlib.md5(mag).hexdigest() == md5["unitig"], "unitig"
    c1 = _step(["clean", "-"], input=mag)
    assert hashlib.md5(c1).hexdigest() == md5["clean"], "clean"
    c2b = _step(["clean", "-CAOFo", "30", "-"], input=c1)
    assert hashlib.md5(c2b).hexdigest() == md5["clean2"], "clean -CAOFo 30"
    open(c2, "wb").write(c2b)
    p = _run(["remap", "-r", rank, fmd, c2])
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    assert p.stdout == _gold("scaf0.remapped.mag.gz"), "remap"
    assert ("avg = %s std = %s" % (META["scaf0"]["avg"], META["scaf0"]["std"])).encode() in p.stderr, "remap's insert size"
    open(rm, "wb").write(p.stdout)
    out, lines, _ = _scaf("scaf0", ["-t1"], mag=rm)
    assert lines == META["scaf0"]["lines"] and out == _gold("scaf0.scaf.fa.gz"), "scaf"
