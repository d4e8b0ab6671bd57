#!/usr/bin/env python3
"""`fermi-amd clean -C` against `fermi clean -C` (oracle/_ref/fermi) on a graph larger than the fixtures: the generator of
tests/golden/make_golden_clean.py with a genome of 4 * 10^5 bases (240 000 reads), `fermi build` and `fermi unitig -l40 -t1` on the CPU.
Best of three of each, wall clock of the whole process, output to /dev/null; the two outputs must be the same bytes.
Usage: python tools/time_clean.py [genome_len] [workdir]"""
import hashlib
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_clean as mk  # noqa: E402

AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 400000
work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
mag = os.path.join(work, "big_%d.mag" % n)
if not os.path.exists(mag):
    open(mag, "wb").write(mk.unitig_of(mk.make_reads(random.Random(mk.SEED), genome_len=n), work))
print("%d unitigs, %.1f MB" % (open(mag, "rb").read().count(b"\n+\n"), os.path.getsize(mag) / 1e6))
env = dict(os.environ, HIP_VISIBLE_DEVICES="")
for args in (["-C"], []):
    best, md5 = {}, {}
    for rep in range(3):
        for name, exe in (("fermi", mk.REF), ("fermi-amd", AMD)):
            t = time.perf_counter()
            p = subprocess.run([exe, "clean"] + args + [mag], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env, check=True)
            dt = time.perf_counter() - t
            best[name] = min(best.get(name, 1e9), dt)
            md5[name] = hashlib.md5(p.stdout).hexdigest()
    assert md5["fermi"] == md5["fermi-amd"], md5
    print("clean %-3s fermi %.3f s   fermi-amd %.3f s   ratio %.2f   (same bytes, %s)" % (" ".join(args), best["fermi"], best["fermi-amd"], best["fermi-amd"] / best["fermi"], md5["fermi"][:8]))
