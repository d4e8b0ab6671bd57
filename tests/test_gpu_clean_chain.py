"""GPU: the driver script's way to contigs with `fermi-amd` alone -- build, unitig, clean, clean -CAOFo 33 (run-fermi.pl:84-94) -- and
`example`, the caller of the in-memory API, with and without the cleaner; `seqrank`, the name that script uses for `seqsort`.  Every
expected byte was written by the reference (tests/golden/make_golden_clean.py, make_golden_api.py, make_golden.py).  Each step that
uses the GPU is a process of its own under its own `timeout`."""
import gzip
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")


def _step(args, seconds=120, **kw):
    p = subprocess.run(["timeout", "-k", "10", str(seconds), AMD] + args, capture_output=True, **kw)
    assert p.returncode == 0, (args, p.returncode, p.stderr.decode(errors="replace")[-2000:])
    return p.stdout


def _gold(name):
    return gzip.open(os.path.join(GOLD, name)).read()


def test_reads_to_contigs(gpu, tmp_path):
    fmd = str(tmp_path / "clean3.fmd")
    _step(["build", "-fo", fmd, os.path.join(GOLD, "clean3.fq.gz")])
    mag = _step(["unitig", "-l40", fmd])
    assert mag == _gold("clean3.mag.gz")
    p1 = _step(["clean", "-"], input=mag)
    assert p1 == _gold("clean3.clean.mag.gz")
    p2 = _step(["clean", "-CAOFo", "33", "-"], input=p1)
    assert p2 == _gold("clean3.clean_chain_CAOFo33.mag.gz") and 0 < p2.count(b"\n+\n") < 20 < p1.count(b"\n+\n") < mag.count(b"\n+\n")


@pytest.mark.parametrize("args,want", [(["-c", "-l", "40"], "clean3.example_c_l40.mag.gz"), (["-ce", "-k", "17", "-l", "40"], "clean3.example_ce_k17_l40.mag.gz")],
                         ids=["c_l40", "ce_k17_l40"])
def test_example_cleans_the_graph_of_the_api(gpu, args, want):
    got = _step(["example"] + args + [os.path.join(GOLD, "clean3.fq.gz")])
    assert got == _gold(want) and 0 < got.count(b"\n+\n") < 20


def test_example_without_the_cleaner(gpu):
    assert _step(["example", "-l", "20", os.path.join(GOLD, "special.fq.gz")]) == _gold("special.api_l20.mag.gz")
    assert _step(["example", "-eU", "-k", "17", os.path.join(GOLD, "tiny.fq.gz")]) == _gold("tiny.api_ec_k17.fq.gz")


def test_example_usage_and_arguments(gpu):
    p = subprocess.run(["timeout", "-k", "10", "60", AMD, "example"], capture_output=True)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == "Usage: fermi-amd example [-ceU] [-k ecKmer] [-l utgKmer] [-g GPU] <in.fq>\n"
    p = subprocess.run(["timeout", "-k", "10", "60", AMD, "example", "-g", "99", os.path.join(GOLD, "tiny.fq.gz")], capture_output=True)
    assert p.returncode == 1 and p.stdout == b"" and b"GPU 99" in p.stderr


def test_seqrank_is_seqsort(gpu):
    fmd = os.path.join(GOLD, "tiny.fmd")
    a, b = _step(["seqrank", fmd]), _step(["seqsort", fmd])
    assert a == b == open(os.path.join(GOLD, "tiny.rank"), "rb").read() and len(a) > 0
