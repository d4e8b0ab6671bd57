#!/usr/bin/env python3
"""End-to-end time of `fermi-amd merge` of two synthetic indexes (reads 0..N and N..2N of one 2N-read set, 100 bp, built on the GPU
and written as .fmd), its phases behind FMD_TIMING (load, walk, interleave, export, encode), the walk's rate against the random
64-byte gather ceiling of this GPU (fmd_probe_gather over a working set of the walked + other index), the walk without its atomics
(FMD_MERGE_TEST_HOOKS=1 FMD_MERGE_MARK=0: what the random atomic ORs into the bit array cost), with --pmc the counters of k_merge_walk
with and without them (rocprofv3 --pmc, runs of their own), and -- at each --ref-reads size per index, up to one the reference
finishes in a few minutes -- `oracle/_ref/fermi merge -t16` against `fermi-amd merge` on the same files (same bytes checked).
Usage: python tools/time_merge.py [--reads 25000000] [--ref-reads 2500000,10000000] [--out profiles/merge] [--rocprof] [--pmc]"""
import argparse, hashlib, json, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fermi_amd import api, hostlib, synth

AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "fermi")


def write_pair(n, d, seed):
    """two .fmd files of n reads each (the halves of one 2n-read set) -> paths, symbols of each"""
    import torch
    g = synth.genome_torch(seed, 2 * n, 100, 30)
    paths, syms = [], []
    for h in range(2):
        r = synth.reads_torch(seed, 2 * n, 100, 30, gen=g, start=h * n, count=n).cpu().numpy()
        idx = api.build_index_inplace(r)
        bwt = np.empty(idx.n, np.uint8)
        api.check(api.lib().fmd_dev_export_bwt(idx.h, 0, idx.n, bwt.ctypes.data))
        syms.append(idx.n)
        idx.close()
        p = os.path.join(d, "part%d_%d.fmd" % (h, n))
        assert hostlib.lib().fmdh_write_rld_from_bwt(bwt.ctypes.data, len(bwt), p.encode()) == 0
        paths.append(p)
        del r, bwt
    del g
    torch.cuda.empty_cache()
    return paths, syms


def run_merge(cmd, env=None):
    t = time.time()
    p = subprocess.run(cmd, capture_output=True, env=env)
    dt = time.time() - t
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return dt, p.stderr.decode()


def phases(err):
    m = re.search(r"walk ([\d.]+) s, interleave ([\d.]+) s, export ([\d.]+) s, encode ([\d.]+) s", err)
    ld = [float(x) for x in re.findall(r"load ([\d.]+) s", err)]
    return {"load_s": ld[-1] if ld else None, "walk_s": float(m.group(1)), "interleave_s": float(m.group(2)),
            "export_s": float(m.group(3)), "encode_s": float(m.group(4))}


def kernel_stats(db, out, n, syms):
    import sqlite3
    c = sqlite3.connect(db)
    rows = c.execute("select name, count(*), sum(end - start) from kernels group by name order by sum(end - start) desc limit 12").fetchall()
    tot = sum(r[2] for r in rows)
    with open(out, "w") as f:
        f.write("# rocprofv3 --kernel-trace --stats of `fermi-amd merge` of two %d-read indexes (%d + %d symbols), summarised from its database\n" % (n, syms[0], syms[1]))
        f.write("%-70s %6s %12s %7s\n" % ("kernel", "calls", "total_ms", "pct"))
        for name, k, dt in rows:
            f.write("%-70s %6d %12.3f %6.1f%%\n" % (name[:70], k, dt / 1e6, 100 * dt / tot))


PMC_PASSES = ["TCC_ATOMIC_sum TCC_EA0_ATOMIC_sum TCC_EA0_RDREQ_sum TCC_BUSY_avr", "TCC_EA0_ATOMIC_LEVEL_sum TA_BUSY_avr GRBM_GUI_ACTIVE"]


def pmc_walk(cmd, d, env, tag):
    """k_merge_walk's counters, one rocprofv3 --pmc run per pass (no tracing beside it) -> {counter: value}"""
    import csv, glob
    res = {}
    for j, cs in enumerate(PMC_PASSES):
        od = os.path.join(d, "pmc_%s_%d" % (tag, j))
        p = subprocess.run(["rocprofv3", "--pmc"] + cs.split() + ["--kernel-include-regex", "k_merge_walk", "--output-format", "csv", "-d", od, "-o", "walk", "--"] + cmd,
                           capture_output=True, env=env)
        if p.returncode != 0:
            res["error_pass_%d" % j] = p.stderr.decode()[-400:]
            continue
        for fn in glob.glob(os.path.join(od, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(fn)):
                if "k_merge_walk" in row.get("Kernel_Name", ""):
                    res[row["Counter_Name"]] = res.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    return res


def md5(p):
    h = hashlib.md5()
    with open(p, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=25_000_000)
    ap.add_argument("--ref-reads", default="2500000,10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--pmc", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    d = tempfile.mkdtemp(dir=a.tmp)
    res = {"reads_per_index": a.reads}
    try:
        env = dict(os.environ, FMD_TIMING="1")
        (p0, p1), syms = write_pair(a.reads, d, synth.DEFAULT_SEED + 21)
        res["symbols"] = syms
        out = os.path.join(d, "merged.fmd")
        dt, err = run_merge([AMD, "merge", "-t", "16", "-f", "-o", out, p0, p1], env)
        res["fermi_amd_merge_s"] = round(dt, 3)
        res["phases"] = phases(err)
        res["stderr"] = err.replace(d + os.sep, "").strip().splitlines()
        walked = min(syms)                              # the smaller index is walked: one step per symbol of it
        w = res["phases"]["walk_s"]
        res["walk_symbols_per_s"] = walked / w
        res["walk_requests_per_s"] = 2 * walked / w     # one 64-byte block of each index per step
        dt2, err2 = run_merge([AMD, "merge", "-t", "16", "-f", "-o", out, p0, p1], dict(env, FMD_MERGE_TEST_HOOKS="1", FMD_MERGE_MARK="0"))
        res["walk_s_without_atomics"] = phases(err2)["walk_s"]
        ms = api.probe_gather(sum(syms), 64, 200_000_000)
        res["probe_gather_64B_lines_per_s"] = 200_000_000 / (ms / 1e3)
        res["walk_requests_vs_probe"] = res["walk_requests_per_s"] / res["probe_gather_64B_lines_per_s"]
        if a.rocprof:   # the trace database stays in the scratch directory (tens of MB); its per-kernel summary goes to --out
            rp = os.path.join(d, "rocprof")
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", rp, "-o", "merge", "--", AMD, "merge", "-f", "-o", out, p0, p1],
                           check=True, capture_output=True)
            kernel_stats(os.path.join(rp, "merge_results.db"), os.path.join(a.out, "kernel_stats.txt"), a.reads, syms)
        if a.pmc:
            cmd = [AMD, "merge", "-f", "-o", out, p0, p1]
            res["pmc_walk"] = pmc_walk(cmd, d, dict(os.environ), "mark")
            res["pmc_walk_without_atomics"] = pmc_walk(cmd, d, dict(os.environ, FMD_MERGE_TEST_HOOKS="1", FMD_MERGE_MARK="0"), "nomark")
        os.remove(out)
        for p in (p0, p1):
            os.remove(p)
        res["reference"] = []
        for rn in [int(x) for x in a.ref_reads.split(",") if x] if os.path.exists(REF) else []:
            (q0, q1), s2 = write_pair(rn, d, synth.DEFAULT_SEED + 22)
            o1, o2 = os.path.join(d, "amd.fmd"), os.path.join(d, "ref.fmd")
            t_amd, err = run_merge([AMD, "merge", "-t", "16", "-f", "-o", o1, q0, q1], env)
            t_ref, _ = run_merge([REF, "merge", "-t", "16", "-f", "-o", o2, q0, q1])
            res["reference"].append({"reads_per_index": rn, "symbols": s2, "ref_merge_t16_s": round(t_ref, 3), "fermi_amd_merge_s": round(t_amd, 3),
                                     "fermi_amd_phases": phases(err), "speedup": round(t_ref / t_amd, 2), "same_bytes": md5(o1) == md5(o2)})
            for q in (q0, q1, o1, o2):
                os.remove(q)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    s = json.dumps(res, indent=1)
    print(s)
    with open(os.path.join(a.out, "time_merge.json"), "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
