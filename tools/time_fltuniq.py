#!/usr/bin/env python3
"""Times of `fltuniq` on one GPU (N paired reads x 100 bp of a genome at 30x with 1 % errors; mates share a name):
  kernels  in process, reads generated on the device: the count kernel on a zeroed table (all windows), the count kernel again on
           the finished table (every window that is not unique now skips its atomics: the price of the plain loads alone), the
           test kernel -- milliseconds and windows per second, for every --k;
  cli      the reads written as FASTQ, indexed (`fermi-amd build`), corrected (`fermi-amd correct`) -- the real input of the step --
           then `fermi-amd fltuniq` file to stdout (FMD_TIMING: the k chosen, both passes, the kernels' share) beside
           `oracle/_ref/fermi fltuniq` on the same file (one host thread by design), same md5; with --chain also
           `fltuniq | fermi-amd build` from both, same md5 of the index.
Counters: run the kernels mode under the profiler, tracing and counters in runs of their own, e.g.
  rocprofv3 --kernel-trace --stats -d OUT -o fu -- python tools/time_fltuniq.py kernels --reads 10000000 --k 15
  rocprofv3 --pmc TCC_REQ_sum TCC_EA0_ATOMIC_sum -d OUT -o fu -- python tools/time_fltuniq.py kernels --reads 10000000 --k 15
Usage: python tools/time_fltuniq.py kernels|cli [--reads 10000000] [--k 15 18] [--out profiles/fltuniq] [--dir DIR] [--no-ref] [--chain]"""
import argparse, ctypes as C, hashlib, json, os, re, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fermi_amd import api, synth

AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "fermi")
SEED = synth.DEFAULT_SEED + 90


def kernels(n, ks):
    import torch
    L = api.lib()
    rd = synth.reads_torch(SEED, n, 100, 30, err=0.01).contiguous()
    off = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * 100).contiguous()
    ok = torch.empty(n, dtype=torch.uint8, device="cuda")
    res = []
    for k in ks:
        words = L.fmd_fltuniq_table_bytes(k) // 8
        tab = torch.zeros(words, dtype=torch.int64, device="cuda")
        windows = n * (100 - k + 1)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            api.check(fn())
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        cnt = lambda: L.fmd_fltuniq_count_dev(0, st, k, rd.data_ptr(), off.data_ptr(), n, tab.data_ptr())
        tst = lambda: L.fmd_fltuniq_test_dev(0, st, k, rd.data_ptr(), off.data_ptr(), n, tab.data_ptr(), ok.data_ptr())
        ms_count = timed(cnt)
        ms_again = timed(cnt)          # nothing changes: a state depends on the multiset of k-mers... counted twice, every k-mer is now "seen twice"
        tab.zero_()
        timed(cnt)                     # (back to the table of ONE pass for the test)
        ms_test = min(timed(tst) for _ in range(3))
        e = {"mode": "kernels", "reads": n, "k": k, "table_gb": round(words * 8 / 1e9, 3), "windows": windows,
             "count_ms": round(ms_count, 3), "count_windows_per_s": round(windows / ms_count * 1e3, 0),
             "recount_ms": round(ms_again, 3), "test_ms": round(ms_test, 3), "test_windows_per_s": round(windows / ms_test * 1e3, 0),
             "kept_share": round(float(ok.sum().item()) / n, 4)}
        print(json.dumps(e), flush=True)
        res.append(e)
        del tab
        torch.cuda.empty_cache()
    return res


def write_fastq(n, path, chunk=1000000):
    """mates under one name (what pe2cofq writes): r<pair number>, fixed width"""
    import torch
    tab = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    gen = synth.genome_torch(SEED, n, 100, 30)
    with open(path, "wb") as f:
        for s in range(0, n, chunk):
            m = min(chunk, n - s)
            r = synth.reads_torch(SEED, n, 100, 30, err=0.01, start=s, count=m, gen=gen).cpu().numpy()
            rec = np.empty((m, 1 + 9 + 1 + 100 + 3 + 100 + 1), dtype=np.uint8)
            rec[:, 0] = ord("@")
            rec[:, 1] = ord("r")
            ids = (np.arange(s, s + m) >> 1)
            for j in range(8):
                rec[:, 9 - j] = 48 + (ids // 10 ** j) % 10
            rec[:, 10] = 10
            rec[:, 11:111] = tab[r]
            rec[:, 111:114] = np.frombuffer(b"\n+\n", dtype=np.uint8)
            rec[:, 114:214] = ord("I")
            rec[:, 214] = 10
            rec.tofile(f)
    del gen
    torch.cuda.empty_cache()


def run(cmd, stdout, env=None):
    t = time.time()
    p = subprocess.run(cmd, stdout=stdout, stderr=subprocess.PIPE, env=env)
    dt = time.time() - t
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return dt, p.stderr.decode()


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def cli(n, ks, d, with_ref, chain):
    env = dict(os.environ, FMD_TIMING="1")
    raw, fmd, ec = (os.path.join(d, x) for x in ("raw.fq", "raw.fmd", "ec.fq"))
    t = time.time(); write_fastq(n, raw); t_write = time.time() - t
    t_build, _ = run([AMD, "build", "-fo", fmd, raw], subprocess.DEVNULL)
    with open(ec, "wb") as f:
        t_correct, _ = run([AMD, "correct", "-t16", fmd, raw], f)
    os.remove(raw)
    res = []
    for k in ks:      # 0 = the k the file size gives
        opt = ["-k%d" % k] if k else []
        out = os.path.join(d, "amd.fq")
        with open(out, "wb") as f:
            dt, err = run([AMD, "fltuniq"] + opt + [ec], f, env)
        e = {"mode": "cli", "reads": n, "ec_bytes": os.path.getsize(ec), "k_option": k, "build_s": round(t_build, 2), "correct_s": round(t_correct, 2),
             "fltuniq_s": round(dt, 3), "md5": md5(out), "write_fastq_s": round(t_write, 1)}
        m = re.search(r"set the k-mer size as (\d+)", err)
        e["k"] = int(m.group(1)) if m else k
        m = re.search(r"(\d+) records, (\d+) bases; kept (\d+) records", err)
        if m:
            e["records"], e["bases"], e["kept"] = int(m.group(1)), int(m.group(2)), int(m.group(3))
        m = re.search(r"pass 1: ([\d.]+) s \(count kernels ([\d.]+) s\); pass 2: ([\d.]+) s \(test kernels ([\d.]+) s\)", err)
        if m:
            e["pass1_s"], e["count_kernels_s"], e["pass2_s"], e["test_kernels_s"] = (float(x) for x in m.groups())
        if chain:
            idx = os.path.join(d, "amd.fmd")
            e["build_of_kept_s"] = round(run([AMD, "build", "-fo", idx, out], subprocess.DEVNULL)[0], 2)
            e["index_md5"] = md5(idx)
        if with_ref:
            rout = os.path.join(d, "ref.fq")
            with open(rout, "wb") as f:
                e["ref_fltuniq_s"] = round(run([REF, "fltuniq"] + opt + [ec], f)[0], 2)
            e["ref_md5"] = md5(rout)
            assert e["ref_md5"] == e["md5"], "fltuniq: bytes differ from the reference"
            if chain:
                idx = os.path.join(d, "ref.fmd")
                run([AMD, "build", "-fo", idx, rout], subprocess.DEVNULL)
                e["ref_index_md5"] = md5(idx)
                assert e["ref_index_md5"] == e["index_md5"]
            os.remove(rout)
        print(json.dumps(e), flush=True)
        res.append(e)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "cli"])
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--k", type=int, nargs="*", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--chain", action="store_true")
    a = ap.parse_args()
    if a.mode == "kernels":
        res = kernels(a.reads, a.k or [15, 18])
    else:
        with tempfile.TemporaryDirectory(dir=a.dir) as d:
            res = cli(a.reads, a.k if a.k is not None else [0], d, not a.no_ref and os.path.exists(REF), a.chain)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "time_fltuniq.jsonl"), "a") as f:
            for e in res:
                f.write(json.dumps(e) + "\n")


if __name__ == "__main__":
    main()
