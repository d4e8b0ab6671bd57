#!/usr/bin/env python3
"""Fixtures of tests/test_contrast_cli.py and tests/test_gpu_contrast.py, written by the reference binary compiled in place
(oracle/_ref/fermi): two RELATED samples -- reads of a small genome with repeats (ctA) and of a copy of it with six substitutions
and a 40-base deletion (ctB), with sequencing errors; the same without errors (cnA / cnB) -- as .fq.gz, .fmd (`fermi build`) and
.rank (`fermi seqsort`); the .sub files `fermi contrast` writes for them under several -k / -o; `fermi bitand` of two of those;
`fermi sub` and `sub -c` of ctA for two selections; the empty index `fermi sub` writes for an all-zero array.  Prints the selected
counts and the md5 of every index for the test files.
Usage: python tests/golden/make_golden_contrast.py"""
import gzip, hashlib, os, subprocess, sys, tempfile
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from fermi_amd import synth  # noqa: E402
REF = os.path.join(ROOT, "oracle", "_ref", "fermi")
OPTS = [(25, 2), (55, 3), (17, 1), (31, 5)]          # -k, -o for ctA / ctB
SUBS = [(25, 2), (55, 3)]                            # `fermi sub` / `sub -c` of ctA.fmd for these


def samples(err):
    g = synth.repeat_genome(synth.DEFAULT_SEED + 77, 6000, repeat_frac=0.05, min_len=100, max_len=300, max_copies=4)
    g2 = g.copy()
    for p in np.random.default_rng(5).choice(len(g), 6, replace=False):
        g2[p] = 1 + g2[p] % 4
    g2 = np.concatenate([g2[:3000], g2[3040:]])
    a = synth.ragged_reads(synth.DEFAULT_SEED + 1, 1500, g, min_len=70, max_len=120, err=err)
    b = synth.ragged_reads(synth.DEFAULT_SEED + 2, 1500, g2, min_len=70, max_len=120, err=err)
    return a, b


def build(name, reads, tmp):
    fq = os.path.join(tmp, name + ".fq")
    synth.to_fastq(reads, fq)
    with gzip.GzipFile(os.path.join(HERE, name + ".fq.gz"), "wb", 9, mtime=0) as f:
        f.write(open(fq, "rb").read())
    fmd = os.path.join(HERE, name + ".fmd")
    subprocess.run([REF, "build", "-fo", fmd, fq], check=True, stderr=subprocess.DEVNULL)
    with open(os.path.join(HERE, name + ".rank"), "wb") as f:
        f.write(subprocess.run([REF, "seqsort", fmd], check=True, capture_output=True).stdout)


def contrast(a, b, k, o, tag):
    fa, fb = os.path.join(HERE, "contrast.%s.%s-%s.sub" % (tag, a, b)), os.path.join(HERE, "contrast.%s.%s-%s.sub" % (tag, b, a))
    p = subprocess.run([REF, "contrast", "-k%d" % k, "-o%d" % o, "-t4", os.path.join(HERE, a + ".fmd"), os.path.join(HERE, a + ".rank"), fa,
                        os.path.join(HERE, b + ".fmd"), os.path.join(HERE, b + ".rank"), fb], check=True, capture_output=True)
    return [int(ln.split()[1]) for ln in p.stderr.decode().splitlines() if ln.startswith("[M::main_contrast]")]


def main():
    md5 = {}
    with tempfile.TemporaryDirectory() as tmp:
        for err, names in ((0.004, ("ctA", "ctB")), (0.0, ("cnA", "cnB"))):
            a, b = samples(err)
            build(names[0], a, tmp); build(names[1], b, tmp)
    for k, o in OPTS:
        print("ctA/ctB -k%d -o%d:" % (k, o), contrast("ctA", "ctB", k, o, "k%do%d" % (k, o)))
    print("cnA/cnB -k25 -o2:", contrast("cnA", "cnB", 25, 2, "k25o2"))
    x, y = (os.path.join(HERE, "contrast.k%do%d.ctA-ctB.sub" % ko) for ko in SUBS)
    with open(os.path.join(HERE, "contrast.and_k25_k55.ctA-ctB.sub"), "wb") as f:
        f.write(subprocess.run([REF, "bitand", x, y], check=True, capture_output=True).stdout)
    for k, o in SUBS:
        for flag in ("", "-c"):
            name = "sub%s.k%do%d.ctA" % ("c" if flag else "", k, o)
            cmd = [REF, "sub", "-t4"] + ([flag] if flag else []) + [os.path.join(HERE, "ctA.fmd"), os.path.join(HERE, "contrast.k%do%d.ctA-ctB.sub" % (k, o))]
            out = subprocess.run(cmd, check=True, capture_output=True).stdout
            open(os.path.join(HERE, name + ".fmd"), "wb").write(out)
            md5[name] = hashlib.md5(out).hexdigest()
    # an all-zero array for tiny.fmd (4000 sequences): the empty index; an all-ones one: `recode`
    with tempfile.TemporaryDirectory() as tmp:
        n = 4000
        zero, ones = os.path.join(tmp, "zero.sub"), os.path.join(tmp, "ones.sub")
        open(zero, "wb").write(np.uint64(n).tobytes() + np.zeros((n + 63) // 64, np.uint64).tobytes())
        w = np.full((n + 63) // 64, ~np.uint64(0), np.uint64)
        w[-1] = np.uint64((1 << (n % 64)) - 1) if n % 64 else w[-1]
        open(ones, "wb").write(np.uint64(n).tobytes() + w.tobytes())
        tiny = os.path.join(HERE, "tiny.rle.fmd")
        out = subprocess.run([REF, "sub", tiny, zero], check=True, capture_output=True).stdout
        open(os.path.join(HERE, "sub.empty.fmd"), "wb").write(out)
        md5["sub.empty"] = hashlib.md5(out).hexdigest()
        md5["tiny.rle all ones"] = hashlib.md5(subprocess.run([REF, "sub", tiny, ones], check=True, capture_output=True).stdout).hexdigest()
        md5["tiny.rle -c all zeros"] = hashlib.md5(subprocess.run([REF, "sub", "-c", tiny, zero], check=True, capture_output=True).stdout).hexdigest()
    for k, v in md5.items():
        print('    "%s": "%s",' % (k, v))


if __name__ == "__main__":
    sys.exit(main())
