"""GPU: `fermi-amd ropebwt` (host/ropebwt_cmd.c over fmd_build_bwt_strands) against what the reference's `ropebwt` printed for the same input
and options (tests/golden/make_golden_ropebwt.py: ropebwt.json lists them).  The text form is the reference's byte for byte; the -b form is
OUR run bytes (maximal runs split at 31), which decode to the reference's symbols and recode to the reference's RLD\\2 file."""
import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
INFO = json.load(open(os.path.join(GOLD, "ropebwt.json")))
IN = os.path.join(GOLD, "ropebwt.in.fa.gz")
NOEMPTY = os.path.join(GOLD, "ropebwt.noempty.fa.gz")


def _run(args, **kw):
    return subprocess.run([AMD] + args, capture_output=True, timeout=120, **kw)


def _gold(name):
    return gzip.open(os.path.join(GOLD, name)).read()


def _opts(opts, tmp_path):
    return [str(tmp_path / "bcr.tmp") if o == "TMP" else o for o in opts]


def _decode(rle):
    assert rle[:4] == b"RLE\6"
    b = np.frombuffer(rle, dtype=np.uint8)[4:]
    assert (b >> 3).min(initial=1) >= 1 and (b & 7).max(initial=0) <= 5
    return np.repeat(b & 7, b >> 3)


# the option sets of the issue, the empty strand set and the driver's line
@pytest.mark.parametrize("tag", sorted(INFO["cases"]))
def test_text_output_is_the_references(gpu, tmp_path, tag):
    e = INFO["cases"][tag]
    p = _run(["ropebwt"] + _opts(e["opts"], tmp_path) + [IN])
    assert p.stdout == _gold("ropebwt.%s.txt.gz" % tag), p.stderr.decode()
    assert len(p.stdout) == (e["symbols"] + 1 if e["rc"] == 0 else 0)
    if e["rc"] == 0:
        assert p.returncode == 0, p.stderr.decode()
    else:   # `-a bcr` without -N meets the record that has no bases: the reference is stopped by an assertion (return code 134) and prints nothing
        assert tag == "bcr" and e["rc"] == 134 and p.returncode == 1 and b"record `empty' has no bases" in p.stderr
    assert not (tmp_path / "bcr.tmp").exists()                    # no -f file is left behind
    assert (b"random base" in p.stderr) == (e["opts"][1] == "bcr" and not any("N" in o for o in e["opts"][2:]))


@pytest.mark.parametrize("tag", sorted(INFO["noempty"]))
def test_random_bases_for_N_are_the_references(gpu, tag):
    """without the record that has no bases `-a bcr` runs: every N became (lrand48() & 3) + 1 in read order, from the stream nobody seeds"""
    e = INFO["noempty"][tag]
    p = _run(["ropebwt"] + e["opts"] + [NOEMPTY])
    assert p.returncode == 0 and p.stdout == _gold("ropebwt.ne.%s.txt.gz" % tag), p.stderr.decode()
    if tag != "bpr":
        assert b"N" not in p.stdout
        assert p.stdout != _run(["ropebwt", "-a", "bpr"] + e["opts"][2:] + [NOEMPTY]).stdout     # (the Ns are there under bpr)


@pytest.mark.parametrize("tag", sorted(INFO["bin"]))
def test_binary_output_decodes_and_recodes_to_the_references(gpu, tmp_path, tag):
    e = INFO["bin"][tag]
    ours = tmp_path / "ours.rle.fmd"
    p = _run(["ropebwt"] + e["opts"] + ["-o", str(ours), IN])
    assert p.returncode == 0 and p.stdout == b"", p.stderr.decode()
    rle = ours.read_bytes()
    ref_rle = open(os.path.join(GOLD, "ropebwt.%s.rle.fmd" % tag), "rb").read()
    sym = _decode(rle)
    assert len(sym) == e["symbols"] and np.array_equal(sym, _decode(ref_rle))
    # our stream is canonical: neighbouring runs of one symbol only where the first is full
    b = np.frombuffer(rle, dtype=np.uint8)[4:]
    same = (b[1:] & 7) == (b[:-1] & 7)
    assert ((b[:-1] >> 3)[same] == 31).all() and len(b) <= len(ref_rle) - 4
    # the text form of the same options is the same symbols
    t = _run(["ropebwt"] + [o.replace("b", "") if o != "bcr" and o != "bpr" else o for o in e["opts"]] + [IN])
    assert t.returncode == 0 and t.stdout == bytes(b"$ACGTN"[s] for s in sym) + b"\n"
    # recode: the reference's RLD\2 file, from a path and from stdin
    want = open(os.path.join(GOLD, "ropebwt.%s.rld.fmd" % tag), "rb").read()
    r = _run(["recode", str(ours)])
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode()
    r = _run(["recode", os.path.join(GOLD, "ropebwt.%s.rle.fmd" % tag)])
    assert r.returncode == 0 and r.stdout == want
    # the file loads, and the device layout ranks every position right
    h = C.c_void_p()
    gpu.check(gpu.lib().fmd_dev_open_file(0, str(ours).encode(), C.byref(h)))
    d = gpu.DevIndex(h)
    try:
        bad, first = C.c_uint64(1), C.c_uint64()
        gpu.check(gpu.lib().fmd_dev_check_rank(d.h, C.byref(bad), C.byref(first)))
        assert bad.value == 0 and d.n == e["symbols"]
    finally:
        d.close()


def test_driver_pipeline_equals_build(gpu, gold, tmp_path):
    """`ropebwt -a bcr -bN x | recode -` is `build -fo` of the same N-free input, byte for byte -- and the reference's tiny.rle.fmd decodes to what
    ropebwt writes for tiny.fq.gz"""
    src = gold.path("tiny.fq.gz")
    fmd = tmp_path / "b.fmd"
    assert _run(["build", "-fo", str(fmd), src]).returncode == 0
    p = _run(["ropebwt", "-a", "bcr", "-v3", "-btNf", str(tmp_path / "bcr.tmp"), src])
    assert p.returncode == 0 and b"[M::main_ropebwt]" in p.stderr and not (tmp_path / "bcr.tmp").exists()
    r = _run(["recode", "-"], input=p.stdout)
    assert r.returncode == 0 and r.stdout == fmd.read_bytes() == open(gold.path("tiny.fmd"), "rb").read()
    assert np.array_equal(_decode(p.stdout), _decode(open(gold.path("tiny.rle.fmd"), "rb").read()))


def test_stdin_output_file_and_gzip_give_the_same_bytes(gpu, tmp_path):
    want = _gold("ropebwt.bcrN.txt.gz")
    plain = tmp_path / "in.fa"
    plain.write_bytes(gzip.open(IN).read())
    out = tmp_path / "o.txt"
    a = _run(["ropebwt", "-a", "bcr", "-N", "-"], input=plain.read_bytes())
    b = _run(["ropebwt", "-a", "bcr", "-N", "-"], input=open(IN, "rb").read())           # gzip through the pipe
    c = _run(["ropebwt", "-a", "bcr", "-N", "-o", str(out), str(plain)])
    assert a.returncode == b.returncode == c.returncode == 0
    assert a.stdout == b.stdout == out.read_bytes() == want and c.stdout == b""
    bo = tmp_path / "o.fmd"
    x = _run(["ropebwt", "-a", "bcr", "-bN", IN])
    y = _run(["ropebwt", "-a", "bcr", "-bN", "-o", str(bo), "-"], input=plain.read_bytes())
    assert x.returncode == y.returncode == 0 and x.stdout == bo.read_bytes() and x.stdout[:4] == b"RLE\6"


def test_text_comes_out_in_slices(gpu, tmp_path):
    """more symbols than two slices of the text writer (4 MiB each): 80 000 reads of 60 bp, 9.76 * 10^6 symbols, against fmd_build_bwt of the same reads"""
    from fermi_amd import synth
    reads = synth.reads(synth.DEFAULT_SEED + 5, 80000, 60, 20, 0.01)
    letters = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"".join(b">%d\n%s\n" % (i, row.tobytes()) for i, row in enumerate(letters[reads])))
    p = _run(["ropebwt", "-a", "bcr", "-NO", str(fa)])
    assert p.returncode == 0, p.stderr.decode()
    want = gpu.build_bwt(reads)
    assert len(p.stdout) == len(want) + 1 > 2 * (4 << 20) and p.stdout[-1:] == b"\n"
    assert np.array_equal(np.frombuffer(p.stdout, dtype=np.uint8)[:-1], letters[want])


def test_no_sequence_at_all(gpu, tmp_path):
    fa = tmp_path / "n.fa"
    fa.write_bytes(b">a\nNNNN\n>b\n")
    assert _run(["ropebwt", "-a", "bcr", "-N", str(fa)]).stdout == b"\n"
    p = _run(["ropebwt", "-a", "bcr", "-bN", str(fa)])
    assert p.returncode == 0 and p.stdout == b"RLE\6"
    assert _run(["ropebwt", str(tmp_path / "missing.fa")]).returncode == 1
