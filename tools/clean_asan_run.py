#!/usr/bin/env python3
"""`make asan-mag`, then this: build/mag_asan (the graph module with -fsanitize=address,undefined, a program of its own) over every
fixture of tests/golden/make_golden_clean.py and over the malformed inputs of tests/test_clean.py.  The outputs must be the goldens, the
exit codes those of fermi-amd, and the sanitizers must stay silent.  Host code only: run it where there is a C compiler, not on a GPU."""
import gzip
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "build", "mag_asan")
sys.path.insert(0, GOLD)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_clean as mk  # noqa: E402
import test_clean as tc  # noqa: E402

n_runs = 0


def run(args, data, want=None, rc=0):
    global n_runs
    p = subprocess.run([EXE] + args + ["-"], input=data, capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    err = p.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, (args, err[-3000:])
    assert p.returncode in ((0, 1) if rc is None else (rc,)), (args, p.returncode, err[-1000:])
    assert want is None or p.stdout == want, args
    n_runs += 1
    return p.stdout


gz = lambda n: gzip.open(os.path.join(GOLD, n)).read()
mag = gz("clean3.mag.gz")
for tag, args in mk.RUNS:
    run(args, mag, gz("clean3.%s.mag.gz" % tag))
run(mk.CHAIN[1], gz("clean3.clean.mag.gz"), gz("clean3.%s.mag.gz" % mk.CHAIN[0]))
for name in mk.SMALL:
    for tag, args in mk.RUNS[:2]:
        run(args, gz(name + ".mag.gz"), gz("%s.%s.mag.gz" % (name, tag)))
for tag, args in mk.RUNS[:2]:
    run(args, gz("clean3.first100.fa.gz"), gz("clean3.first100.%s.mag.gz" % tag))
for args in ([], ["-C"], ["-CA"]):
    run(args, b"", b"")
for name, case in sorted(tc.HAND.items()):
    for args, want in case["out"].items():
        run(args.split(), case["mag"].encode(), want.encode())
for tag, args, data in tc._bad_inputs():
    run(args, data, b"", rc=1)
run(["-C"], mag[:len(mag) // 2], rc=None)   # cut in the middle of a sequence: an overlap longer than its vertex, an error or not, and no finding
run(["-CA", "-N1", "-n0"], mag)
run(["-C", "-l0", "-e0", "-i0", "-o0"], mag)
print("%d runs, no sanitizer finding" % n_runs)
