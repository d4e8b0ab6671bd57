#!/usr/bin/env python3
"""Fixtures of tests/test_ropebwt_cli.py and tests/test_gpu_ropebwt.py, written by the reference binary compiled in place
(oracle/_ref/fermi).  Only data: inputs, and what the reference prints for them.

Inputs
  ropebwt.in.fa.gz       64 reads of 20-40 bp: 50 drawn from both strands of a 240-bp sequence, and the corners -- one N inside, NN, an N
                         first, an N last, nothing but N, the even-length ACGTACGTACGTACGT that is its own reverse complement, a read whose
                         second piece becomes one only after a -N cut, a read twice, a record without bases, a byte >= 128, lower case
  ropebwt.noempty.fa.gz  the same without the record that has no bases
  cg2cofq.in.cgfq        hand-made: FASTQ and FASTA records whose sequence is two arms with other characters between them, one that starts with
                         such a character, one with a third arm, an empty one (all with a second run of letters where they have a first separator:
                         the reference's scan for it has no end, seq.c:238)
Outputs of the reference
  ropebwt.<tag>.txt.gz   the text form for every option set of CASES on ropebwt.in.fa.gz (ropebwt.json: tag -> options, return code)
  ropebwt.ne.<tag>.txt.gz   the same for NOEMPTY_CASES on ropebwt.noempty.fa.gz
  ropebwt.<tag>.rle.fmd, ropebwt.<tag>.rld.fmd   for BIN_CASES: `ropebwt -b`, and `recode` of it
  cg2cofq.out.gz
What the reference does with the record that has no bases, when -N does not drop it: its trim makes the length -1 (ropebwt.c:25-28);
`-a bpr` then inserts a '$' alone per strand (bprope6.c:218-224) and `-a bcr` is stopped by the assertion of bcr_append (bcr.c:361) --
return code 134 (SIGABRT), nothing on stdout.  That is recorded as it is (an empty text, "rc": 134), and the random-base rule of `-a bcr`
is recorded on ropebwt.noempty.fa.gz.
Asserted here, loudly:
  - bcr and bpr print the same text wherever -N is given or the input holds no N (the pieces of the -N cut);
  - the -N text is the BWT that `fermi build` of the same pieces holds (`chkbwt -p`);
  - -t and -f change nothing, and -f leaves no file.
Usage: python tests/golden/make_golden_ropebwt.py"""
import gzip, json, os, re, subprocess, sys, tempfile
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "fermi")

# tag -> options (text form, ropebwt.in.fa.gz); "TMP" stands for a temporary file name
CASES = {
    "bcrN": ["-a", "bcr", "-N"], "bprN": ["-a", "bpr", "-N"], "bcr": ["-a", "bcr"], "bpr": ["-a", "bpr"], "bprR": ["-a", "bpr", "-R"],
    "bcrNR": ["-a", "bcr", "-NR"], "bcrNF": ["-a", "bcr", "-NF"], "bprF": ["-a", "bpr", "-F"], "bcrNO": ["-a", "bcr", "-NO"],
    "bprO": ["-a", "bpr", "-O"], "bcrNtf": ["-a", "bcr", "-Nt", "-f", "TMP"],
    # beyond the list of the issue: the empty strand set, and the driver's own line in text form
    "bcrNFR": ["-a", "bcr", "-NFR"], "bprFR": ["-a", "bpr", "-FR"], "driver": ["-a", "bcr", "-v3", "-tNf", "TMP"],
}
NOEMPTY_CASES = {"bcr": ["-a", "bcr"], "bcrO": ["-a", "bcr", "-O"], "bcrR": ["-a", "bcr", "-R"], "bcrF": ["-a", "bcr", "-F"], "bpr": ["-a", "bpr"]}
BIN_CASES = {"bcrbN": ["-a", "bcr", "-bN"], "bprbR": ["-a", "bpr", "-bR"]}

CG = b"""@cg1 a comment that is dropped
ACGTACGTAC-----GGTTAACCGG
+
IIIIIIIIII!!!!!ABCDEFGHIJ
>cg2
acgtnacgt..TTGGCCAA
@cg3
--ACGT
+
!!IIII
@cg4
AACC.GGTT.ACAC
+
ABCD!EFGH!IJKL
>cg5
>cg6
ACGT7TGCA
"""


def gz_write(name, data):
    with gzip.GzipFile(os.path.join(HERE, name), "wb", 9, mtime=0) as f:
        f.write(data)


def run(args, stdin=None):
    return subprocess.run([REF] + args, capture_output=True, input=stdin)


def ropebwt(opts, path, tmp):
    tf = os.path.join(tmp, "bcr.tmp")
    p = run(["ropebwt"] + [tf if o == "TMP" else o for o in opts] + [path])
    assert not os.path.exists(tf), "the reference left its -f file behind"
    return p


def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def reads():
    rng = np.random.default_rng(20261018)
    genome = bytes(rng.choice(list(b"ACGT"), 240).astype(np.uint8))
    out = []
    for i in range(50):
        ln, at = int(rng.integers(20, 41)), 0
        at = int(rng.integers(0, len(genome) - ln + 1))
        s = genome[at:at + ln]
        out.append((b"r%02d" % i, revcomp(s) if rng.random() < 0.5 else s))
    g = lambda a, n: genome[a:a + n]
    out[7:7] = [(b"n_inside", g(3, 12) + b"N" + g(16, 14))]
    out[13:13] = [(b"nn", g(40, 9) + b"NN" + g(51, 17))]
    out[19:19] = [(b"n_first", b"N" + g(70, 24))]
    out[23:23] = [(b"n_last", g(90, 29) + b"N")]
    out[29:29] = [(b"all_n", b"N" * 22)]
    out[31:31] = [(b"palin", b"ACGTACGTACGTACGT" + b"")]
    out[37:37] = [(b"palin_after_cut", b"ACCGTAGGTACN" + b"AACGCGTT")]      # AACGCGTT is its own reverse complement, the whole read is not
    out[41:41] = [(b"dup", out[2][1]), (b"dup", out[2][1])]
    out[47:47] = [(b"empty", b"")]
    out[53:53] = [(b"high_byte", g(120, 10) + b"\xc3" + g(131, 12))]
    out[57:57] = [(b"lower", g(150, 26).lower())]
    out[59:59] = [(b"x_inside", g(180, 11) + b"X" + g(192, 11) + b"n" + g(204, 9))]
    assert 60 <= len(out) <= 70 and all(len(s) == 0 or 16 <= len(s) <= 40 for _, s in out)
    return out


def fasta(recs):
    return b"".join(b">" + n + b"\n" + s + (b"\n" if s else b"") for n, s in recs)


def pieces(recs):
    """what -N makes of the records: cut at everything that is not a base, empty pieces dropped"""
    out = []
    for _, s in recs:
        out += [p for p in re.split(rb"[^ACGT]", s.upper()) if p]
    return out


def main():
    assert os.path.exists(REF), "build oracle/_ref first (make ref)"
    info = {"cases": {}, "noempty": {}, "bin": {}}
    recs = reads()
    gz_write("ropebwt.in.fa.gz", fasta(recs))
    gz_write("ropebwt.noempty.fa.gz", fasta([r for r in recs if r[1]]))
    open(os.path.join(HERE, "cg2cofq.in.cgfq"), "wb").write(CG)
    src, src_ne = os.path.join(HERE, "ropebwt.in.fa.gz"), os.path.join(HERE, "ropebwt.noempty.fa.gz")
    text = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, opts in CASES.items():
            p = ropebwt(opts, src, tmp)
            rc = p.returncode if p.returncode >= 0 else 128 - p.returncode
            if tag == "bcr":     # the record without bases: bcr_append's assertion
                assert rc == 134 and p.stdout == b"" and b"bcr_append" in p.stderr, (rc, p.stderr)
            else:
                assert rc == 0 and p.stdout.endswith(b"\n") and set(p.stdout[:-1]) <= set(b"$ACGTN"), (tag, rc, p.stderr)
            text[tag] = p.stdout
            info["cases"][tag] = {"opts": opts, "rc": rc, "symbols": max(len(p.stdout) - 1, 0)}
            gz_write("ropebwt.%s.txt.gz" % tag, p.stdout)
            print("ropebwt %-8s rc %3d, %5d symbols" % (tag, rc, max(len(p.stdout) - 1, 0)))
        ne = {}
        for tag, opts in NOEMPTY_CASES.items():
            p = ropebwt(opts, src_ne, tmp)
            assert p.returncode == 0, (tag, p.stderr)
            ne[tag] = p.stdout
            info["noempty"][tag] = {"opts": opts, "rc": 0, "symbols": len(p.stdout) - 1}
            gz_write("ropebwt.ne.%s.txt.gz" % tag, p.stdout)
        for tag, opts in BIN_CASES.items():
            p = ropebwt(opts, src, tmp)
            assert p.returncode == 0 and p.stdout[:4] == b"RLE\6", (tag, p.stderr)
            rle = os.path.join(HERE, "ropebwt.%s.rle.fmd" % tag)
            open(rle, "wb").write(p.stdout)
            q = run(["recode", rle])
            assert q.returncode == 0 and q.stdout[:4] == b"RLD\2", q.stderr
            open(os.path.join(HERE, "ropebwt.%s.rld.fmd" % tag), "wb").write(q.stdout)
            dec = b"".join(bytes([b"$ACGTN"[b & 7]]) * (b >> 3) for b in p.stdout[4:]) + b"\n"
            info["bin"][tag] = {"opts": opts, "symbols": len(dec) - 1, "rle_bytes": len(p.stdout), "runs_at_31_or_split": sum(1 for b in p.stdout[4:] if b >> 3 == 31)}
            # the runs decode to the text of the same options
            t = ropebwt([o.replace("b", "") if o.startswith("-") and o != "-a" else o for o in opts], src, tmp)
            assert t.returncode == 0 and dec == t.stdout, tag
        # ---- what the issue assumes about the reference
        # 1. one BWT whatever the algorithm, wherever no N reaches it
        assert text["bcrN"] == text["bprN"], "bcr and bpr differ under -N"
        assert text["bcrNtf"] == text["bcrN"] == text["driver"], "-t / -f / -v change the BWT"
        for extra in (["-R"], ["-F"], ["-O"], ["-FR"]):
            a, b = ropebwt(["-a", "bcr", "-N"] + extra, src, tmp), ropebwt(["-a", "bpr", "-N"] + extra, src, tmp)
            assert a.returncode == 0 and a.stdout == b.stdout, ("bcr and bpr differ under -N", extra)
        assert text["bcrNR"] == ropebwt(["-a", "bpr", "-NR"], src, tmp).stdout and text["bcrNO"] == ropebwt(["-a", "bpr", "-NO"], src, tmp).stdout
        pc = pieces(recs)
        pfa = os.path.join(tmp, "pieces.fa")
        open(pfa, "wb").write(b"".join(b">p%d\n%s\n" % (i, s) for i, s in enumerate(pc)))
        for extra in ([], ["-R"], ["-F"], ["-O"]):      # no N in the input: -N or not, bcr or bpr
            outs = [ropebwt(["-a", a] + n + extra, pfa, tmp).stdout for a in ("bcr", "bpr") for n in ([], ["-N"])]
            assert all(o == outs[0] and len(o) > 1 for o in outs), ("bcr and bpr differ on an input without N", extra)
        assert ropebwt(["-a", "bcr"], pfa, tmp).stdout == text["bcrN"], "-N is not the same as indexing the pieces"
        # 2. the -N text is the BWT `fermi build` holds for the same pieces
        fmd = os.path.join(tmp, "pieces.fmd")
        for bopt, tag in ([], "bcrN"), (["-O"], "bcrNO"):
            b = run(["build", "-f"] + bopt + ["-o", fmd, pfa])
            assert b.returncode == 0, b.stderr
            c = run(["chkbwt", "-p", fmd])
            assert c.returncode == 0 and c.stdout == text[tag], "ropebwt -N and `fermi build` of the pieces hold different BWTs (%s)" % tag
        info["pieces"] = len(pc)
        # ---- cg2cofq
        p = run(["cg2cofq", os.path.join(HERE, "cg2cofq.in.cgfq")])
        assert p.returncode == 0 and p.stdout.count(b"\n") > 12, p.stderr
        gz_write("cg2cofq.out.gz", p.stdout)
    with open(os.path.join(HERE, "ropebwt.json"), "w") as f:
        json.dump(info, f, indent=1, sort_keys=True)
        f.write("\n")
    print("all assertions about the reference hold; %d pieces under -N" % len(pc))


if __name__ == "__main__":
    main()
