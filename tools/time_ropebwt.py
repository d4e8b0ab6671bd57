#!/usr/bin/env python3
"""Wall times of the driver script's index builder on one GPU (N reads x 100 bp of a genome at 30x with 1 % errors, written as FASTQ):
  `fermi-amd ropebwt -a bcr -bN reads.fq > x.rle.fmd`   the BWT of both strands on the GPU, out as RLE\\6 runs
  `fermi-amd build -fo x.fmd reads.fq`                  the same BWT, out as the RLD\\2 container
  `fermi-amd recode x.rle.fmd > y.fmd`                  what the driver's next step pays to load the first (same md5 as build's file, asserted)
  `oracle/_ref/fermi ropebwt -a bcr -btN reads.fq`      the reference where it is built (four threads by design; --no-ref skips it): its runs
                                                        decode to the same symbols (asserted through `recode`: same md5)
and with --strands also `-F` and `-R` alone.  Whole processes, start of the runtime included (FMD_TIMING prints it); one run each, so a
figure is a wall time of that run and not a distribution.
Usage: python tools/time_ropebwt.py [--reads 10000000] [--out profiles/ropebwt] [--dir DIR] [--no-ref] [--strands]"""
import argparse, hashlib, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fermi_amd import synth

AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "fermi")
SEED = synth.DEFAULT_SEED + 91


def write_fastq(n, path, chunk=1000000):
    tab = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    gen = synth.genome(SEED, n, 100, 30)
    with open(path, "wb") as f:
        for s in range(0, n, chunk):
            m = min(chunk, n - s)
            r = synth.reads(SEED, n, 100, 30, 0.01, start=s, count=m, gen=gen)
            rec = np.empty((m, 1 + 9 + 1 + 100 + 3 + 100 + 1), dtype=np.uint8)
            rec[:, 0] = ord("@")
            rec[:, 1] = ord("r")
            ids = np.arange(s, s + m)
            for j in range(8):
                rec[:, 9 - j] = 48 + (ids // 10 ** j) % 10
            rec[:, 10] = 10
            rec[:, 11:111] = tab[r]
            rec[:, 111:114] = np.frombuffer(b"\n+\n", dtype=np.uint8)
            rec[:, 114:214] = ord("I")
            rec[:, 214] = 10
            rec.tofile(f)


def run(cmd, stdout, env=None):
    t = time.time()
    p = subprocess.run(cmd, stdout=stdout, stderr=subprocess.PIPE, env=env)
    dt = time.time() - t
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return round(dt, 3), p.stderr.decode()


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def measure(n, d, with_ref, strands):
    env = dict(os.environ, FMD_TIMING="1")
    fq, rle, fmd, rec = (os.path.join(d, x) for x in ("reads.fq", "amd.rle.fmd", "amd.fmd", "amd.recode.fmd"))
    t = time.time(); write_fastq(n, fq); t_write = time.time() - t
    e = {"reads": n, "fastq_bytes": os.path.getsize(fq), "write_fastq_s": round(t_write, 1)}
    with open(rle, "wb") as f:
        e["ropebwt_bN_s"], err = run([AMD, "ropebwt", "-a", "bcr", "-v3", "-bN", fq], f, env)
    e["ropebwt_phases"] = [l.split("] ", 1)[1] for l in err.split("\n") if l.startswith("[M::main_ropebwt]")]
    e["rle_bytes"] = os.path.getsize(rle)
    e["build_s"], _ = run([AMD, "build", "-fo", fmd, fq], subprocess.DEVNULL, env)
    with open(rec, "wb") as f:
        e["recode_s"], _ = run([AMD, "recode", rle], f, env)
    e["fmd_md5"] = md5(fmd)
    assert md5(rec) == e["fmd_md5"], "recode of ropebwt's runs is not build's file"
    if strands:
        for opt in ("-F", "-R"):
            e["ropebwt_bN%s_s" % opt[1]], _ = run([AMD, "ropebwt", "-a", "bcr", "-bN", opt, fq], subprocess.DEVNULL, env)
    if with_ref:
        rrle = os.path.join(d, "ref.rle.fmd")
        with open(rrle, "wb") as f:
            e["ref_ropebwt_btN_s"], _ = run([REF, "ropebwt", "-a", "bcr", "-btN", fq], f)
        e["ref_rle_bytes"] = os.path.getsize(rrle)
        with open(rec, "wb") as f:
            run([AMD, "recode", rrle], f)
        assert md5(rec) == e["fmd_md5"], "the reference's runs decode to another BWT"
    print(json.dumps(e), flush=True)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--strands", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        e = measure(a.reads, d, not a.no_ref and os.path.exists(REF), a.strands)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "time_ropebwt.jsonl"), "a") as f:
            f.write(json.dumps(e) + "\n")


if __name__ == "__main__":
    main()
