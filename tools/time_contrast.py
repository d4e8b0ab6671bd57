#!/usr/bin/env python3
"""Times of contrast assembly on two related synthetic samples (N reads x 100 bp each: a genome at 30x and a copy of it with one
substitution per 15 000 bases, 0.2 % errors; built on the GPU, written as .fmd, .rank by `fermi-amd seqsort`):
  - `fermi-amd contrast` and `fermi-amd sub`, file to file, with their phases (FMD_TIMING);
  - in process, kernels only: the mark walk of `sub` (walked symbols/s) beside fmd_merge_walk_dev of the same two indexes, the
    contrast walk (pair nodes/s, tip nodes/s) beside the k-mer harvest of the first index (extensions/s, KM_EXT);
  - at each --ref-reads size, `oracle/_ref/fermi contrast -t16` and `sub -t16` on the same files (same bytes checked).
Usage: python tools/time_contrast.py [--reads 20000000] [--ref-reads 200000] [--out profiles/contrast] [--rocprof]"""
import argparse, ctypes as C, hashlib, json, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fermi_amd import api, hostlib, synth

AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "fermi")


def write_pair(n, d, seed):
    """the two samples as .fmd + .rank -> paths"""
    import torch
    g = synth.genome_torch(seed, n, 100, 30)
    gh = g.cpu().numpy()
    pos = np.random.default_rng(seed & 0xffff).choice(len(gh), max(1, len(gh) // 15000), replace=False)
    gh[pos] = 1 + gh[pos] % 4
    gens = (g, torch.from_numpy(gh).to(g.device))
    fmd, rank = [], []
    for h in range(2):
        r = synth.reads_torch(seed + 1 + h, n, 100, 30, err=0.002, gen=gens[h]).cpu().numpy()
        idx = api.build_index_inplace(r)
        bwt = np.empty(idx.n, np.uint8)
        api.check(api.lib().fmd_dev_export_bwt(idx.h, 0, idx.n, bwt.ctypes.data))
        idx.close()
        p = os.path.join(d, "s%d_%d.fmd" % (h, n))
        assert hostlib.lib().fmdh_write_rld_from_bwt(bwt.ctypes.data, len(bwt), p.encode()) == 0
        del r, bwt
        q = p[:-4] + ".rank"
        with open(q, "wb") as f:
            subprocess.run([AMD, "seqsort", p], check=True, stdout=f, stderr=subprocess.DEVNULL)
        fmd.append(p); rank.append(q)
    del g, gens
    torch.cuda.empty_cache()
    return fmd, rank


def run(cmd, env=None, stdout=None):
    t = time.time()
    p = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=stdout if stdout else subprocess.DEVNULL, env=env)
    dt = time.time() - t
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return dt, p.stderr.decode()


def md5(p):
    h = hashlib.md5()
    with open(p, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def cli_pair(fmd, rank, d, env, tag, ref=False):
    """contrast then sub of the first sample -> times, selected counts, output paths"""
    exe, t = (REF, ["-t16"]) if ref else (AMD, [])
    subs = [os.path.join(d, "%s.%d.sub" % (tag, i)) for i in (0, 1)]
    out = os.path.join(d, tag + ".sub.fmd")
    dt, err = run([exe, "contrast"] + t + [fmd[0], rank[0], subs[0], fmd[1], rank[1], subs[1]], env)
    res = {"contrast_s": round(dt, 3), "selected": [int(x) for x in re.findall(r"\] (\d+) reads selected", err)]}
    m = re.search(r"load ([\d.]+) s, walk ([\d.]+) s", err)
    if m:
        res["contrast_phases"] = {"load_s": float(m.group(1)), "walk_s": float(m.group(2))}
    with open(out, "wb") as f:
        dt, err = run([exe, "sub"] + t + [fmd[0], subs[0]], env, stdout=f)
    res["sub_s"] = round(dt, 3)
    m = re.search(r"(\d+) of (\d+) symbols kept: load \+ mark ([\d.]+) s, select \+ export ([\d.]+) s, encode ([\d.]+) s", err)
    if m:
        res["sub_phases"] = {"kept": int(m.group(1)), "of": int(m.group(2)), "load_mark_s": float(m.group(3)), "select_export_s": float(m.group(4)), "encode_s": float(m.group(5))}
    return res, subs, out


def kernels_in_process(fmd, sub_path):
    """kernel times alone: mark walk, merge walk, contrast walk, harvest"""
    L = api.lib()
    a, b = api.DevIndex.open_bare(fmd[0]), api.DevIndex.open_bare(fmd[1])
    res = {}

    def dmalloc(nbytes):
        p = C.c_void_p()
        api.check(L.fmd_dev_malloc(0, max(int(nbytes), 16), C.byref(p)))
        return p

    def timed(f):
        api.check(L.fmd_dev_sync(a.h, None))
        t = time.time()
        api.check(f())
        api.check(L.fmd_dev_sync(a.h, None))
        return time.time() - t
    # mark walk
    raw = np.fromfile(sub_path, np.uint64)[1:]
    nw = (a.n + 63) // 64
    wb = L.fmd_sub_work_bytes(a.n)
    d_sub, d_bits, d_work = dmalloc(raw.nbytes), dmalloc(nw * 8 + 8), dmalloc(wb)
    api.check(L.fmd_memcpy_h2d(d_sub, raw.ctypes.data, raw.nbytes, None))
    best = None
    for _ in range(3):
        api.check(L.fmd_memset_dev(d_bits, 0, nw * 8 + 8, None))
        dt = timed(lambda: L.fmd_sub_mark_dev(a.h, None, d_sub, d_bits, d_work, wb, C.c_void_p(d_bits.value + nw * 8)))
        best = dt if best is None or dt < best else best
    n_set = np.zeros(1, np.uint64)
    api.check(L.fmd_memcpy_d2h(n_set.ctypes.data, C.c_void_p(d_bits.value + nw * 8), 8, None))
    res["mark_walk"] = {"s": best, "walked_symbols": int(n_set[0]), "symbols_per_s": int(n_set[0]) / best, "selected_sequences": int(np.unpackbits(raw.view(np.uint8)).sum())}
    for p in (d_sub, d_bits, d_work):
        L.fmd_dev_free(p)
    # the merge walk of the same two indexes (two gathers per step)
    n_tot = a.n + b.n
    wb = L.fmd_merge_work_bytes(n_tot)
    d_bits, d_work = dmalloc((n_tot + 63) // 64 * 8), dmalloc(wb)
    best = None
    for _ in range(3):
        api.check(L.fmd_memset_dev(d_bits, 0, (n_tot + 63) // 64 * 8, None))
        dt = timed(lambda: L.fmd_merge_walk_dev(a.h, b.h, None, d_bits, d_work, wb, None))
        best = dt if best is None or dt < best else best
    res["merge_walk"] = {"s": best, "walked_symbols": min(a.n, b.n), "symbols_per_s": min(a.n, b.n) / best}
    for p in (d_bits, d_work):
        L.fmd_dev_free(p)
    # contrast walk, capacity doubled until nothing overflows
    cap = 1 << 22
    while True:
        wb = L.fmd_contrast_work_bytes(cap)
        s0, s1, d_work, d_st = dmalloc((int(a.mcnt[1]) + 63) // 64 * 8 + 8), dmalloc((int(b.mcnt[1]) + 63) // 64 * 8 + 8), dmalloc(wb), dmalloc(32)
        api.check(L.fmd_memset_dev(s0, 0, (int(a.mcnt[1]) + 63) // 64 * 8 + 8, None)); api.check(L.fmd_memset_dev(s1, 0, (int(b.mcnt[1]) + 63) // 64 * 8 + 8, None))
        dt = timed(lambda: L.fmd_contrast_dev(a.h, b.h, None, 55, 3, 0xf, s0, s1, d_work, wb, cap, d_st))
        st = np.zeros(4, np.uint64)
        api.check(L.fmd_memcpy_d2h(st.ctypes.data, d_st, 32, None))
        for p in (s0, s1, d_work, d_st):
            L.fmd_dev_free(p)
        if st[1] == 0:
            break
        cap *= 2
    res["contrast_walk"] = {"s": dt, "cap": cap, "pair_nodes": int(st[0]), "tip_nodes": [int(st[2]), int(st[3])], "pair_nodes_per_s": int(st[0]) / dt,
                            "extensions_per_s": (2 * int(st[0]) + int(st[2]) + int(st[3])) / dt}
    # the harvest of the first index: w = 23, min_occ 3 (KM_EXT = word 68 of its work area)
    cap = 1 << 22
    while True:
        wb = L.fmd_kmer_work_bytes(cap)
        d_work, db, dk, dv, d_st = dmalloc(wb), dmalloc(cap * 4), dmalloc(cap * 4), dmalloc(cap), dmalloc(32)
        dt = timed(lambda: L.fmd_kmer_collect_dev(a.h, None, 23, 3, 8, d_work, wb, cap, db, dk, dv, d_st))
        st = np.zeros(4, np.uint64); ctr = np.zeros(72, np.uint64)
        api.check(L.fmd_memcpy_d2h(st.ctypes.data, d_st, 32, None)); api.check(L.fmd_memcpy_d2h(ctr.ctypes.data, d_work, 72 * 8, None))
        for p in (d_work, db, dk, dv, d_st):
            L.fmd_dev_free(p)
        if st[1] == 0:
            break
        cap *= 2
    res["harvest_w23"] = {"s": dt, "cap": cap, "extensions": int(ctr[68]), "extensions_per_s": int(ctr[68]) / dt}
    a.close(); b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--ref-reads", default="200000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrast"))
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--rocprof", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    d = tempfile.mkdtemp(dir=a.tmp)
    env = dict(os.environ, FMD_TIMING="1")
    res = {"runs": []}
    try:
        sizes = [(int(x), True) for x in a.ref_reads.split(",") if x] + ([(a.reads, False)] if a.reads else [])
        for n, with_ref in sizes:
            fmd, rank = write_pair(n, d, synth.DEFAULT_SEED + 41)
            r = {"reads_per_sample": n, "fmd_bytes": [os.path.getsize(p) for p in fmd]}
            r["fermi_amd"], subs, out = cli_pair(fmd, rank, d, env, "amd")
            if with_ref and os.path.exists(REF):
                r["reference_t16"], rsubs, rout = cli_pair(fmd, rank, d, None, "ref", ref=True)
                r["same_bytes"] = all(md5(x) == md5(y) for x, y in zip(subs + [out], rsubs + [rout]))
                for p in rsubs + [rout]:
                    os.remove(p)
            r["kernels"] = kernels_in_process(fmd, subs[0])
            if a.rocprof and not with_ref:
                rp = os.path.join(d, "rocprof")
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", rp, "-o", "sub", "--", AMD, "sub", fmd[0], subs[0]], check=True, capture_output=True)
                import sqlite3
                rows = sqlite3.connect(os.path.join(rp, "sub_results.db")).execute(
                    "select name, count(*), sum(end - start) from kernels group by name order by sum(end - start) desc limit 8").fetchall()
                with open(os.path.join(a.out, "kernel_stats_sub.txt"), "w") as f:
                    f.write("# rocprofv3 --kernel-trace --stats of `fermi-amd sub` at %d reads per sample\n" % n)
                    for name, k, dt in rows:
                        f.write("%-70s %6d %12.3f ms\n" % (name[:70], k, dt / 1e6))
            for p in fmd + rank + subs + [out]:
                os.remove(p)
            res["runs"].append(r)
            print(json.dumps(r, indent=1), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    with open(os.path.join(a.out, "time_contrast.json"), "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
