#!/usr/bin/env python3
"""Fixtures of tests/test_readprep_cli.py and tests/test_gpu_fltuniq.py, written by the reference binary compiled in place
(oracle/_ref/fermi).  Only data: inputs, and what the reference prints for them.

New inputs
  readprep.corner.fx     hand-written corners: three records named `a` whose middle one holds an N, a two-line FASTA record with
                         a comment, a record shorter than k, an empty sequence, a header with a comment, FASTQ and FASTA mixed,
                         lower-case bases
  pairs.cofq.fq.gz       pairs.fq.gz with the /1 /2 stripped (what `pe2cofq` makes of its two mate files): equal names = mates
  readprep.trimq.fq.gz   the first 400 records of pairs.fq.gz with random qualities: 20-40, a head of up to 24 and a tail of up
                         to 44 bases at quality 0-5 on about half of the records, an N in 5 % of them
  readprep.pe_1.fq.gz, readprep.pe_2.fq.gz   60 first mates, 50 second mates
Outputs of the reference
  fltuniq.<input>.<k>.out.gz for the small inputs; for every case the md5, the number of records kept and, for the paired input, how
  many went only because their mate failed, in readprep.json; trimseq.<opts>.out.gz (+ the four counts per option set, asserted
  non-zero here); pe2cofq.out.gz; cnt2qual.<input>.<q>.out.gz; splitfa.p3.000?.fq (decompressed: gzip bytes depend on the zlib
  at hand) and the md5 of the eight default files' contents.
Usage: python tests/golden/make_golden_readprep.py"""
import gzip, hashlib, json, os, subprocess, sys, tempfile
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "fermi")

CORNER = b"""@a
ACGTACGTACGTAACC
+
IIIIIIIIIIIIIIII
@a
ACGTNCGTACGTAACC
+
IIIIIIIIIIIIIIII
@a
ACGTACGTACGTAACC
+
IIIIIIIIIIIIIIII
>b c d
ACGTACGTAC
GTAACCGGTT
>c
ACGTACGTACGTAACCGGTT
>short
ACG
>empty
>e2 with a comment
ACGTACGTACGTAACC
@q1 fastq comment
acgtacgtacgtaacc
+
ABCDEFGHIJKLMNOP
>once
ACGTACGTACGTAACCTTTTT
>dup
ACGTACGTACGTAACC
>dup
ACGTACGTACGTAACC
@dup
ACGTACGTACGTAACC
+
~~~~~~~~~~~~~~~~
>tail x
ACGTACGTACGTAACC
"""

# (input, -k options) of `fltuniq`; None = the k the file size gives
FLTUNIQ = [("tiny.fq.gz", [None, 13, 11, 17, 18]), ("tiny.ec.fq.gz", [None, 13, 11]), ("ctA.fq.gz", [None, 13, 11]),
           ("special.fq.gz", [None, 13, 11]), ("pairs.fq.gz", [None, 13, 11]), ("pairs.cofq.fq.gz", [13]), ("readprep.corner.fx", [5, 3, None])]
KEEP_BYTES = {"special.fq.gz", "pairs.cofq.fq.gz", "readprep.corner.fx"}
TRIMSEQ = [("default", []), ("q10l30", ["-q", "10", "-l", "30"]), ("N", ["-N"])]


def ktag(k):
    return "kdef" if k is None else "k%d" % k


def records(data):
    """one-line records as the reference writes them (four lines after '@', two after '>') -> list of (header, seq, qual or None)"""
    ln, i, out = data.split(b"\n"), 0, []
    while i < len(ln) - 1:
        if ln[i][:1] == b"@":
            out.append((ln[i][1:], ln[i + 1], ln[i + 3]))
            i += 4
        else:
            assert ln[i][:1] == b">", ln[i]
            out.append((ln[i][1:], ln[i + 1], None))
            i += 2
    return out


def fastq(recs):
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in recs)


def gz_write(name, data):
    with gzip.GzipFile(os.path.join(HERE, name), "wb", 9, mtime=0) as f:
        f.write(data)


def ref(*args):
    return subprocess.run([REF] + list(args), check=True, capture_output=True).stdout


def main():
    info = {"fltuniq": {}, "trimseq": {}, "splitfa8": {}}
    pairs = records(gzip.open(os.path.join(HERE, "pairs.fq.gz")).read())
    # ---- inputs
    open(os.path.join(HERE, "readprep.corner.fx"), "wb").write(CORNER)
    gz_write("pairs.cofq.fq.gz", fastq([(n[:-2], s, q) for n, s, q in pairs]))
    rng = np.random.default_rng(20261016)
    trimq = []
    for n, s, q in pairs[:400]:
        ql = rng.integers(20, 41, len(s))
        if rng.random() < 0.5:
            h, t = int(rng.integers(0, 25)), int(rng.integers(0, 45))
            ql[:h] = rng.integers(0, 6, h)
            if t:
                ql[-t:] = rng.integers(0, 6, t)
        s = bytearray(s)
        if rng.random() < 0.05:
            s[int(rng.integers(0, len(s)))] = ord("N")
        trimq.append((n, bytes(s), bytes((ql + 33).astype(np.uint8))))
    gz_write("readprep.trimq.fq.gz", fastq(trimq))
    gz_write("readprep.pe_1.fq.gz", fastq([r for r in pairs if r[0].endswith(b"/1")][:60]))
    gz_write("readprep.pe_2.fq.gz", fastq([r for r in pairs if r[0].endswith(b"/2")][:50]))
    # ---- fltuniq
    for name, ks in FLTUNIQ:
        path = os.path.join(HERE, name)
        for k in ks:
            out = ref("fltuniq", *([] if k is None else ["-k%d" % k]), path)
            names = [r[0].split(b" ")[0] for r in records(out)]
            e = {"md5": hashlib.md5(out).hexdigest(), "kept": len(names)}
            if name == "pairs.cofq.fq.gz":     # how many fail on their own = records of the run on the unpaired names that are missing here
                alone = records(ref("fltuniq", "-k%d" % k, os.path.join(HERE, "pairs.fq.gz")))
                e["mate_only"] = len(alone) - len(names)
                assert all(names.count(n) == 2 for n in set(names)) and e["mate_only"] > 0
            info["fltuniq"]["%s.%s" % (name, ktag(k))] = e
            if name in KEEP_BYTES:
                gz_write("fltuniq.%s.%s.out.gz" % (name, ktag(k)), out)
            print("fltuniq %-22s %-5s kept %d" % (name, ktag(k), e["kept"]), e.get("mate_only", ""))
    # ---- trimseq: with the pairing, and on names that pair with nothing (what every record does on its own)
    with tempfile.TemporaryDirectory() as tmp:
        solo = os.path.join(tmp, "solo.fq")
        open(solo, "wb").write(fastq([(b"n%03d_" % i, s, q) for i, (n, s, q) in enumerate(trimq)]))
        src = dict((n, s) for n, s, q in trimq)
        for tag, opts in TRIMSEQ:
            out = ref("trimseq", *opts, os.path.join(HERE, "readprep.trimq.fq.gz"))
            recs = records(out)
            alone = records(ref("trimseq", *opts, solo))
            c = {"kept": len(recs), "shortened": sum(1 for n, s, q in recs if len(s) < len(src[n])), "dropped": len(trimq) - len(recs),
                 "mate_dropped": len(alone) - len(recs)}
            assert all(v > 0 for v in c.values()), (tag, c)
            info["trimseq"][tag] = c
            gz_write("trimseq.%s.out.gz" % tag, out)
            print("trimseq", tag, c)
        # ---- pe2cofq, cnt2qual, splitfa
        gz_write("pe2cofq.out.gz", ref("pe2cofq", os.path.join(HERE, "readprep.pe_1.fq.gz"), os.path.join(HERE, "readprep.pe_2.fq.gz")))
        for name in ("readprep.trimq.fq.gz", "readprep.corner.fx"):
            gz_write("cnt2qual.%s.q17.out.gz" % name, ref("cnt2qual", os.path.join(HERE, name)))
            gz_write("cnt2qual.%s.q2.out.gz" % name, ref("cnt2qual", os.path.join(HERE, name), "2"))
        ref("splitfa", os.path.join(HERE, "readprep.trimq.fq.gz"), os.path.join(tmp, "p3"), "3")
        for i in range(3):
            open(os.path.join(HERE, "splitfa.p3.%04d.fq" % i), "wb").write(gzip.open(os.path.join(tmp, "p3.%04d.fq.gz" % i)).read())
        ref("splitfa", os.path.join(HERE, "special.fq.gz"), os.path.join(tmp, "p8"))
        for fn in sorted(os.listdir(tmp)):
            if fn.startswith("p8."):
                info["splitfa8"][fn] = hashlib.md5(gzip.open(os.path.join(tmp, fn)).read()).hexdigest()
        assert len(info["splitfa8"]) == 8
    with open(os.path.join(HERE, "readprep.json"), "w") as f:
        json.dump(info, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
