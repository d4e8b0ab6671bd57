"""CPU: what `fermi-amd ropebwt` (host/ropebwt_cmd.c) says before it looks for a device -- the reference's usage text and return code, its
two warnings word for word, the refusal of -T -- and `cg2cofq` (host/readprep_cmd.c) against what the reference printed for the same input
(tests/golden/make_golden_ropebwt.py).  Every command runs with HIP_VISIBLE_DEVICES empty: no GPU is asked for."""
import gzip
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
IN = os.path.join(GOLD, "ropebwt.in.fa.gz")

# ropebwt.c:78-92 with the defaults filled in (max_runs 512, max_nodes 64, bcr_verbose 2)
USAGE = """
Usage:   ropebwt [options] <in.fq.gz>

Options: -a STR     algorithm: bpr or bcr [bpr]
         -r INT     max number of runs in leaves (bpr only) [512]
         -n INT     max number children per internal node (bpr only) [64]
         -o FILE    output file [stdout]
         -f FILE    temporary sequence file name (bcr only) [null]
         -v INT     verbose level (bcr only) [2]
         -b         binary output (5+3 runs starting after 4 bytes)
         -t         enable threading (bcr only)
         -F         skip forward strand
         -R         skip reverse strand
         -N         cut at ambiguous bases
         -O         suppress end trimming when forward==reverse
         -T         print the tree stdout (bpr only)

"""
W_ALGO = "[W::main_ropebwt] available algorithms: bpr or bcr; default to bpr\n"
W_RANDOM = "Warning: With bcr, an ambiguous base will be converted to a random base\n"
NODEV = "[E::main] no usable HIP device (libfmdhip has no CPU fallback)\n"


def _run(args, **kw):
    assert os.path.exists(AMD), "fermi-amd is not built"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    return subprocess.run([AMD] + args, capture_output=True, timeout=60, env=env, **kw)


def test_usage_text_and_return_code_are_the_references():
    """the command is reached, and answers, where there is no device"""
    p = _run(["ropebwt"])
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == USAGE
    p = _run(["ropebwt", "-a", "bcr", "-v3", "-btNf", "x.tmp"])           # the driver's options, no input
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == USAGE.replace("[2]", "[3]")
    p = _run(["ropebwt", "-r", "100", "-n", "32"])
    assert p.stderr.decode() == USAGE.replace("[512]", "[100]").replace("[64]", "[32]")


def test_the_program_lists_both_commands():
    p = _run([])
    assert p.returncode == 1
    err = p.stderr.decode()
    assert "         ropebwt    " in err and "(fermi ropebwt)" in err and "         cg2cofq    " in err and "(fermi cg2cofq)" in err


def test_unknown_algorithm_warns_and_falls_back_to_bpr():
    p = _run(["ropebwt", "-a", "sais"])
    assert p.returncode == 1 and p.stderr.decode() == W_ALGO + USAGE
    p = _run(["ropebwt", "-a", "sais", IN])          # bpr: no word about random bases
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == W_ALGO + NODEV


def test_bcr_without_N_warns_about_random_bases():
    p = _run(["ropebwt", "-a", "bcr", IN])
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == W_RANDOM + NODEV
    for opts in (["-a", "bcr", "-N"], ["-a", "bpr"], []):
        p = _run(["ropebwt"] + opts + [IN])
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == NODEV, opts


def test_T_is_refused(tmp_path):
    out = tmp_path / "o.txt"
    p = _run(["ropebwt", "-T", "-o", str(out), IN])
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr.decode() == "[E::main_ropebwt] -T is not supported: the BWT is sorted on the GPU, there is no rope to print\n"
    assert not out.exists()
    assert _run(["ropebwt", "-T"]).stderr.decode() == USAGE         # no input: the usage first, as in the reference


def test_nothing_is_written_without_a_device(tmp_path):
    out, tmp = tmp_path / "o.fmd", tmp_path / "bcr.tmp"
    p = _run(["ropebwt", "-a", "bcr", "-v3", "-btNf", str(tmp), "-o", str(out), IN])
    assert p.returncode == 1 and p.stderr.decode() == NODEV
    assert not out.exists() and not tmp.exists()


def test_cg2cofq_writes_the_reference_bytes():
    want = gzip.open(os.path.join(GOLD, "cg2cofq.out.gz")).read()
    p = _run(["cg2cofq", os.path.join(GOLD, "cg2cofq.in.cgfq")])
    assert p.returncode == 0 and p.stderr == b"" and p.stdout == want
    assert want.count(b"@cg1\n") == 2 and b"comment" not in want and b"@cg4\nGGTT.ACAC\n+\nEFGH!IJKL\n" in want   # both arms under one name, the rest of the line kept
    p = _run(["cg2cofq", "-"], input=open(os.path.join(GOLD, "cg2cofq.in.cgfq"), "rb").read())
    assert p.returncode == 0 and p.stdout == want


def test_cg2cofq_usage_and_a_record_with_one_arm(tmp_path):
    p = _run(["cg2cofq"])
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == "Usage: fermi-amd cg2cofq <in.cgfq>\n"
    one = tmp_path / "one.fq"
    one.write_bytes(b"@a\nACGT\n+\nIIII\n>b\nACGT--\n")          # no second run of letters: the first record alone
    p = _run(["cg2cofq", str(one)])
    assert p.returncode == 0 and p.stdout == b"@a\nACGT\n+\nIIII\n>b\nACGT\n"
    assert _run(["cg2cofq", str(tmp_path / "none.fq")]).returncode == 1
