#!/usr/bin/env python3
"""`make asan-scaf`, then this: build/scaf_asan (the host side of `scaf` with -fsanitize=address,undefined, a program of its own:
tools/scaf_main.c) over the fixtures of tests/golden/make_golden_scaf.py and over truncated and malformed MAGs.  On the fixtures its LK / CT
and SW lines and its FASTA must be the reference's, with the recorded gaps (tests/golden/scafN.ext.tsv) in the place of the local assemblies: the
joiner's insertions and overlaps, the shared gap strings, the P-values and the alignment fallback all run; everywhere the sanitizers must stay silent.
Host code only: run it where there is a C compiler, not on a GPU."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "build", "scaf_asan")
META = json.load(open(os.path.join(GOLD, "scaf.json")))
n_runs = 0


def run(args, rc=(0,)):
    global n_runs
    p = subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    err = p.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, (args, err[-3000:])
    assert p.returncode in rc, (args, p.returncode, err[-1000:])
    n_runs += 1
    return p.stdout, err


def unpatched(line):
    f = line.split("\t")
    if f[0] == "LK" and len(f) >= 9:
        f[8] = "-"
    return "\t".join(f)


with tempfile.TemporaryDirectory() as tmp:
    for name in ("scaf0", "scaf1", "scaf2", "hand", "hand2"):
        path = os.path.join(GOLD, {"hand": "scaf.hand.mag", "hand2": "scaf.hand2.mag.gz"}.get(name, name + ".remapped.mag.gz"))
        ext = os.path.join(GOLD, name + ".ext.tsv")
        out, err = run([path, META[name]["avg"], META[name]["std"], "20"] + ([ext] if os.path.exists(ext) else []))
        got = [l for l in err.split("\n") if l[:3] in ("LK\t", "CT\t", "SW\t")]
        assert got == META[name]["lines"], (name, [(a, b) for a, b in zip(got, META[name]["lines"]) if a != b][:3])
        if name.startswith("scaf"):
            assert out == gzip.open(os.path.join(GOLD, name + ".scaf.fa.gz")).read(), name
        elif name == "hand":
            assert out.decode() == META[name]["fa"]
        run([path, META[name]["avg"], META[name]["std"], "10"])
        run([path, "0", "0"]); run([path, "100000", "5"]); run([path, "-5", "-9"])
        data = gzip.open(path).read() if path.endswith(".gz") else open(path, "rb").read()
        for k, cut in enumerate((len(data) // 2, len(data) // 3 + 7, data.index(b"UR:Z:") + 9, data.index(b"UR:Z:") + 5, len(data) - 3)):
            p = os.path.join(tmp, "cut%d.mag" % k)
            open(p, "wb").write(data[:cut])
            run([p, META[name]["avg"], META[name]["std"]], rc=(0, 1))
    rec = "@%s\t%s\n%s\n+\n%s\n"
    bad = {
        "empty": b"",
        "no_ur": open(os.path.join(GOLD, "scaf.nour.mag"), "rb").read(),
        "ur_empty": (rec % ("1:2", "5\t3,20;\t.\tUR:Z:", "ACGTACGTAC", "5555555555")).encode(),
        "ur_garbage": (rec % ("1:2", "5\t3,20;\t.\tUR:Z:12,;;,,x", "ACGTACGTAC", "5555555555")).encode(),
        "ur_negative": (rec % ("1:2", "5\t3,20;\t.\tUR:Z:12,-5,-1;14,99999,100000;", "ACGTACGTAC", "5555555555")).encode(),
        "all_single_read": (rec % ("1:2", "5\t3,20;\t.\tUR:Z:12,0,5;", "ACGTACGTAC", '""""""""""')).encode(),
        "short_comment": (rec % ("1:2", "5 UR:Z:12,0,5;", "ACGTACGTAC", "5555555555")).encode(),
        "no_count": (rec % ("x", "UR:Z:12,0,5;13,2,8;", "ACGTNNNN", "55555555")).encode(),
        "no_overlaps": (rec % ("1:2", "50\t.\t.\tUR:Z:12,0,5;", "ACGTACGTAC", "5555555555")).encode() + (rec % ("3:4", "50\t.\t.\tUR:Z:13,0,5;", "ACGTACGTAC", "5555555555")).encode(),
        "fasta": b">1:2\t5\t3,4;\t.\tUR:Z:12,0,5;\nACGTACGT\n",
        "huge_ids": (rec % ("1:2", "5\t3,20;\t.\tUR:Z:18446744073709551615,0,5;9223372036854775807,1,4;", "ACGTACGTAC", "5555555555")).encode(),
    }
    for k, data in sorted(bad.items()):
        p = os.path.join(tmp, k + ".mag")
        open(p, "wb").write(data)
        run([p, "300", "20"], rc=(0, 1))
    for v in json.load(open(os.path.join(GOLD, "scaf.sw.json")))[::7]:
        out, _ = run(["--sw", v["q"], v["t"]])
        assert out.decode().split() == [str(v[k]) for k in ("score", "te", "qe", "tb", "qb")]
    for n, t in ((1, 0.0), (2, 3.5), (50, 1e3), (7, float("inf")), (3, float("nan"))):
        run(["--stat", str(n), str(t)])
print("%d runs, no sanitizer finding" % n_runs)
