#!/usr/bin/env python3
"""Times `fermi-amd scaf` on a generated diploid paired-end set (the recipe of tests/golden/make_golden_scaf.py, a fixed seed): the reads go
through `fermi-amd` alone -- build, seqrank, unitig -r, clean, clean -CAOFo 30, remap -r -- and the remapped MAG is scaffolded with -t1 and
-t16; where the reference is compiled (oracle/_ref/fermi) it scaffolds the same MAG with -t1 and -t16 and the FASTAs are compared.  Prints
the four stage times of every run (read, rdist, paired, patched) and the wall time.
Usage: python tools/time_scaf.py [genome_len=2000000] [workdir]"""
import os
import random
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_scaf as mk  # noqa: E402

AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "fermi")


def run(cmd, stdin=None, out=None, limit=1100):
    t0 = time.time()
    with (open(out, "wb") if out else open(os.devnull, "wb")) as fo:
        p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, input=stdin, stdout=fo if out else subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode:
        sys.exit("%s: exit %d\n%s" % (" ".join(cmd[:3]), p.returncode, p.stderr.decode(errors="replace")[-2000:]))
    return p.stdout, p.stderr.decode(errors="replace"), time.time() - t0


def stages(err):
    out = []
    for key in ("read", "rdist", "paired", "patched"):
        m = re.search(r"\[M::[^\]]*\] %s[^\n]*? in ([0-9.]+) sec" % key, err)
        out.append("%s %s s" % (key, m.group(1) if m else "?"))
    return ", ".join(out)


def main():
    glen = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
    tmp = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="time_scaf.")
    os.makedirs(tmp, exist_ok=True)
    fa, fmd, rank, c2, rm = (os.path.join(tmp, n) for n in ("r.fa", "r.fmd", "r.rank", "c2.mag", "rm.mag"))
    t0 = time.time()
    reads = mk.make_reads(random.Random(20261018), glen=glen, snp=0.003, cov=30, rlen=80)
    with open(fa, "w") as f:
        f.write("".join(">r%d/%d\n%s\n" % (i >> 1, (i & 1) + 1, r) for i, r in enumerate(reads)))
    print("%d reads of a %d-base diploid genome generated in %.1f s" % (len(reads), glen, time.time() - t0), flush=True)
    run([AMD, "build", "-fo", fmd, fa])
    run([AMD, "seqrank", fmd], out=rank)
    mag = os.path.join(tmp, "u.mag")
    run([AMD, "unitig", "-l35", "-r", rank, fmd], out=mag)
    c1 = run([AMD, "clean", mag])[0]
    run([AMD, "clean", "-CAOFo", "30", "-"], stdin=c1, out=c2)
    _, err, _ = run([AMD, "remap", "-r", rank, fmd, c2], out=rm)
    m = re.search(r"avg = ([0-9.]+) std = ([0-9.]+)", err)
    avg, std = m.group(1), m.group(2)
    print("remapped MAG: %d unitigs, avg %s std %s" % (open(rm, "rb").read().count(b"\n+\n"), avg, std), flush=True)
    outs = {}
    for tool, exe in (("fermi-amd", AMD), ("fermi", REF)):
        if not os.path.exists(exe):
            print("%s: not built here" % tool)
            continue
        for t in ("1", "16"):
            o = os.path.join(tmp, "scaf.%s.t%s.fa" % (tool, t))
            _, err, wall = run([exe, "scaf", "-t" + t, fmd, rm, avg, std], out=o)
            outs[(tool, t)] = open(o, "rb").read()
            print("%s scaf -t%s: wall %.2f s; %s; %d scaftigs" % (tool, t, wall, stages(err), outs[(tool, t)].count(b">")), flush=True)
    first = next(iter(outs.values()))
    print("all FASTAs equal: %s" % all(sorted(v.split(b">")) == sorted(first.split(b">")) for v in outs.values()))
    print("byte-identical to the first: %s" % {"%s -t%s" % k: v == first for k, v in outs.items()})


if __name__ == "__main__":
    main()
