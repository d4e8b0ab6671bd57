"""CPU: the read-preparation commands of `fermi-amd` that need no GPU -- `trimseq`, `pe2cofq`, `splitfa`, `cnt2qual` (host/readprep_cmd.c)
-- against what the reference printed for the same inputs (tests/golden/make_golden_readprep.py), the usage texts, and the
arguments `fltuniq` rejects before it looks for a device.  Every command runs with HIP_VISIBLE_DEVICES empty: no GPU is asked for."""
import gzip
import hashlib
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
INFO = json.load(open(os.path.join(GOLD, "readprep.json")))
TRIMQ = os.path.join(GOLD, "readprep.trimq.fq.gz")
CORNER = os.path.join(GOLD, "readprep.corner.fx")


def _run(args, **kw):
    if not os.path.exists(AMD):
        pytest.skip("fermi-amd is not built here")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    return subprocess.run([AMD] + args, capture_output=True, timeout=60, env=env, **kw)


def _gold(name):
    return gzip.open(os.path.join(GOLD, name)).read()


def _records(data):
    ln, i, out = data.split(b"\n"), 0, []
    while i < len(ln) - 1:
        step = 4 if ln[i][:1] == b"@" else 2
        out.append(ln[i:i + step])
        i += step
    return out


def test_usage_lists_the_five_commands():
    p = _run([])
    assert p.returncode == 1
    err = p.stderr.decode()
    for line in ("pe2cofq    interleave two mate files under one name, no GPU needed (fermi pe2cofq)",
                 "trimseq    trim / drop reads by quality, no GPU needed (fermi trimseq)",
                 "splitfa    deal read pairs to N files, no GPU needed (fermi splitfa)",
                 "cnt2qual   occurrence counts -> qualities, no GPU needed (fermi cnt2qual)",
                 "fltuniq    drop reads that hold a k-mer seen once, and their mates (fermi fltuniq)"):
        assert line in err


@pytest.mark.parametrize("cmd,usage", [
    ("trimseq", "Usage: fermi-amd trimseq [-N] [-q qual=3] [-l minLen=20] <in.fq>\n"),
    ("pe2cofq", "Usage: fermi-amd pe2cofq <in1.fq> <in2.fq>\n"),
    ("splitfa", "Usage: fermi-amd splitfa <in.fq> <out.prefix> [8]\n"),
    ("cnt2qual", "Usage: fermi-amd cnt2qual <in.fq> [17]\n"),
    ("fltuniq", "Usage: fermi-amd fltuniq [-k INT] [-g GPU] <in.fa>\n"),
])
def test_each_command_prints_its_usage_without_arguments(cmd, usage):
    p = _run([cmd])
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.decode() == usage


def test_trimseq_usage_shows_the_options_given():
    p = _run(["trimseq", "-q", "7", "-l", "33"])
    assert p.returncode == 1 and p.stderr.decode() == "Usage: fermi-amd trimseq [-N] [-q qual=7] [-l minLen=33] <in.fq>\n"


def test_fltuniq_rejects_its_arguments_before_it_needs_a_device(tmp_path):
    missing = str(tmp_path / "none.fq")
    p = _run(["fltuniq", missing])
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == "[E::main_fltuniq] fail to open the input file\n"
    p = _run(["fltuniq", "-k", "13", missing])
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == "[E::main_fltuniq] fail to open file '%s'\n" % missing
    p = _run(["fltuniq", "-k", "2", CORNER])
    assert p.returncode == 1 and p.stdout == b"" and "[E::main_fltuniq] -k 2" in p.stderr.decode()


@pytest.mark.parametrize("tag,opts", [("default", []), ("q10l30", ["-q", "10", "-l", "30"]), ("N", ["-N"])])
def test_trimseq_is_the_references(tag, opts):
    p = _run(["trimseq"] + opts + [TRIMQ])
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout == _gold("trimseq.%s.out.gz" % tag)
    # the fixture discriminates: some records shortened, some dropped, some dropped with their mate, some kept (counts by the reference)
    c = INFO["trimseq"][tag]
    src = dict((r[0], r[1]) for r in _records(gzip.open(TRIMQ).read()))
    recs = _records(p.stdout)
    assert len(recs) == c["kept"] > 0 and 400 - len(recs) == c["dropped"] > 0 and c["mate_dropped"] > 0
    assert sum(1 for r in recs if len(r[1]) < len(src[r[0]])) == c["shortened"] > 0


def test_trimseq_reads_stdin_and_plain_fasta():
    raw = gzip.open(TRIMQ).read()
    p = _run(["trimseq", "-"], input=raw)
    assert p.returncode == 0 and p.stdout == _gold("trimseq.default.out.gz")
    p = _run(["trimseq", CORNER])     # the record with an N goes, and both of its mates; the length bound holds only where there are qualities (seq.c:331-348)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode()
    assert out.startswith(">b c d\nACGTACGTACGTAACCGGTT\n>c\n") and "@a" not in out and ">short\nACG\n" in out


def test_pe2cofq_is_the_references():
    p = _run(["pe2cofq", os.path.join(GOLD, "readprep.pe_1.fq.gz"), os.path.join(GOLD, "readprep.pe_2.fq.gz")])
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout == _gold("pe2cofq.out.gz")
    recs = _records(p.stdout)
    assert len(recs) == 100                       # the shorter file ends the output
    assert all(recs[i][0] == recs[i + 1][0] and b"/" not in recs[i][0] for i in range(0, 100, 2))


def test_pe2cofq_of_the_split_pairs_is_the_cofq_fixture(tmp_path):
    recs = _records(gzip.open(os.path.join(GOLD, "pairs.fq.gz")).read())
    for m in (b"/1", b"/2"):
        (tmp_path / ("m%s.fq" % m[1:].decode())).write_bytes(b"".join(b"\n".join(r) + b"\n" for r in recs if r[0].endswith(m)))
    p = _run(["pe2cofq", str(tmp_path / "m1.fq"), str(tmp_path / "m2.fq")])
    assert p.returncode == 0 and p.stdout == _gold("pairs.cofq.fq.gz")


@pytest.mark.parametrize("name", ["readprep.trimq.fq.gz", "readprep.corner.fx"])
@pytest.mark.parametrize("q", [None, 2])
def test_cnt2qual_is_the_references(name, q):
    p = _run(["cnt2qual", os.path.join(GOLD, name)] + ([] if q is None else [str(q)]))
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout == _gold("cnt2qual.%s.q%d.out.gz" % (name, 17 if q is None else q))
    if name.endswith(".fx"):
        assert b"@b\tc d\n" in p.stdout           # a TAB before the comment, FASTA records under '@'
        assert (b"~~~~" in p.stdout) and (q is None or b"acegikmoqsuwy{}~" in p.stdout)   # saturation at '~'


def test_splitfa_three_files(tmp_path):
    p = _run(["splitfa", TRIMQ, str(tmp_path / "p3"), "3"])
    assert p.returncode == 0 and p.stdout == b"", p.stderr.decode()
    assert sorted(os.listdir(tmp_path)) == ["p3.%04d.fq.gz" % i for i in range(3)]
    n = 0
    for i in range(3):
        got = gzip.open(str(tmp_path / ("p3.%04d.fq.gz" % i))).read()
        assert got == open(os.path.join(GOLD, "splitfa.p3.%04d.fq" % i), "rb").read()
        n += len(_records(got))
    assert n == 400


def test_splitfa_default_eight_files_from_stdin(tmp_path):
    p = _run(["splitfa", "-", str(tmp_path / "p8")], input=open(os.path.join(GOLD, "special.fq.gz"), "rb").read())
    assert p.returncode == 0, p.stderr.decode()
    got = dict((fn, hashlib.md5(gzip.open(str(tmp_path / fn)).read()).hexdigest()) for fn in os.listdir(tmp_path))
    assert got == INFO["splitfa8"]
