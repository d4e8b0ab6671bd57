#!/usr/bin/env python3
"""Time of kcount (fmd_kcount, fmd_kcount_part_dev) with the k-mer harvest of `correct` over the same index as the yardstick.  --reads 100 bp reads at
30x with --err substitutions are indexed on the GPU.  Per k:
  kcount      fmd_kcount, the host form: spectrum only (no sink), and with a sink that only counts what it is handed; allocation, the sort of the
              pairs and their copy to the host are inside the clock, as a caller sees them;
  part        fmd_kcount_part_dev from the four single-base roots on buffers made before the clock starts: the kernels alone, without and with a list;
  harvest     fmd_kmer_collect (host form, w = min(k, 27), the reference's suffix length, min_occ = 1 and 3), and fmd_kmer_collect_dev on buffers made
              before the clock starts, which also tells the extensions a pass does (the level counters of its work area).
Host clock around call + sync; one warm-up, then --repeats runs; median, and min .. max as the run-to-run spread.  Extensions / s = n_ext / median.
The device forms are the like-for-like pair: the host form of the harvest starts from a small capacity and pays for every pass that overflowed.
Writes time_kcount_<reads>.json (every run) and README.md (the table and the comparison; what stands under "## Notes" there is kept) into --out.
Usage: python tools/time_kcount.py [--reads 1000000] [--err 0.01] [-k 21 31] [--repeats 3] [--out profiles/kcount]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fermi_amd import api, synth

LEN = 100


def timed(fn, sync):
    t = time.perf_counter()
    r = fn()
    sync()
    return time.perf_counter() - t, r


def stats(v):
    runs, v = list(v), sorted(v)
    return {"median_s": v[len(v) // 2], "min_s": v[0], "max_s": v[-1], "runs_s": runs}


def repeat(fn, sync, n):
    fn(); sync()
    out = [timed(fn, sync) for _ in range(n)]
    return stats([t for t, _ in out]), out[-1][1]


def rate(n_ext, st):
    return {"n_ext": int(n_ext), "ext_per_s": n_ext / st["median_s"], "ext_per_s_min": n_ext / st["max_s"], "ext_per_s_max": n_ext / st["min_s"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--err", type=float, default=0.01)
    ap.add_argument("-k", type=int, nargs="+", default=[21, 31])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kcount"))
    a = ap.parse_args()
    assert all(2 <= k <= 32 for k in a.k) and a.repeats >= 3, "k = 2..32; at least three runs: the spread of the yardstick is part of the result"
    import torch
    assert api.device_count() > 0, "time_kcount.py needs a GPU: nothing here is measured without one"
    L = api.lib()
    N = a.reads
    reads = synth.reads_torch(synth.DEFAULT_SEED + 43, N, LEN, 30, err=a.err)
    d = api.build_index_inplace(reads.cpu().numpy())
    del reads
    torch.cuda.empty_cache()
    sync = lambda: api.check(L.fmd_dev_sync(d.h, None))
    res = {"reads": N, "read_len": LEN, "err": a.err, "symbols": d.n, "repeats": a.repeats, "k": {}}
    roots = np.zeros(4, dtype=api.INTV_DT)
    for i, c in enumerate((4, 3, 2, 1)):
        roots[i]["x"] = (d.cnt[c], d.cnt[5 - c], d.cnt[c + 1] - d.cnt[c]); roots[i]["info"] = c - 1
    d_roots = torch.from_numpy(roots.view(np.uint8)).to("cuda")
    for k in a.k:
        r = {}
        # ---- the host form, both modes
        st, (hist, s0) = repeat(lambda: d.kmer_spectrum(k, n_bins=10001), sync, a.repeats)
        r["kcount_spectrum"] = dict(st, stat=s0, **rate(s0["n_ext"], st))
        seen = [0, 0]

        def sink(ctx, n, kmer, count):
            seen[0] += n; seen[1] += 1
            return 0
        cb = api.KCOUNT_SINK(sink)
        h2, s2 = np.zeros(2, dtype=np.uint64), np.zeros(1, dtype=api.KCOUNT_STAT_DT)

        def listed():
            seen[0] = seen[1] = 0
            api.check(L.fmd_kcount(d.h, k, 1, 2, h2.ctypes.data, 0, C.cast(cb, C.c_void_p), None, s2.ctypes.data))
        st, _ = repeat(listed, sync, a.repeats)
        s1 = {f: int(s2[0][f]) for f in api.KCOUNT_STAT_DT.names}
        assert seen[0] == s1["n_kmers"] == s0["n_kmers"] == int(hist.sum()) and s1["n_total"] == s0["n_total"], "the two modes disagree"
        r["kcount_list"] = dict(st, stat=s1, slices=seen[1], **rate(s1["n_ext"], st))
        # ---- the kernels alone
        cap = d.n // 2 + (1 << 16)                     # (what the host form starts with)
        assert s0["n_retries"] == 0, "the host form needed more than that"
        wb = L.fmd_kcount_work_bytes(cap)
        work = torch.empty(wb, dtype=torch.uint8, device="cuda")
        d_hist = torch.zeros(10001, dtype=torch.int64, device="cuda")
        d_stat = torch.zeros(7, dtype=torch.int64, device="cuda")
        out_cap = s0["n_kmers"]
        d_kmer = torch.empty(out_cap, dtype=torch.int64, device="cuda"); d_count = torch.empty(out_cap, dtype=torch.int32, device="cuda")
        for name, lst in (("part_spectrum", False), ("part_list", True)):
            def part():
                d_hist.zero_()
                api.check(L.fmd_kcount_part_dev(d.h, None, k, 1, 1, 4, d_roots.data_ptr(), cap, 10001, d_hist.data_ptr(), d_kmer.data_ptr() if lst else None,
                                                d_count.data_ptr() if lst else None, out_cap, d_stat.data_ptr(), work.data_ptr(), wb))
            st, _ = repeat(part, sync, a.repeats)
            ps = dict(zip(api.KCOUNT_STAT_DT.names, d_stat.cpu().tolist()))
            assert ps["overflow"] == 0 and ps["n_kmers"] == s0["n_kmers"] and np.array_equal(d_hist.cpu().numpy().view(np.uint64), hist)
            r[name] = dict(st, cap=cap, **rate(ps["n_ext"], st))
        del work, d_kmer, d_count
        torch.cuda.empty_cache()
        # ---- the yardstick
        w = min(k, 27)
        suf = w - 15 if w > 15 else 1
        for min_occ in (1, 3):
            st, got = repeat(lambda: d.kmer_collect(w, min_occ, suf), sync, a.repeats)
            hcap = 1 << 24
            while True:
                hwb = L.fmd_kmer_work_bytes(hcap)
                hwork = torch.empty(hwb, dtype=torch.uint8, device="cuda")
                ob = torch.empty(hcap, dtype=torch.int32, device="cuda"); ok_ = torch.empty(hcap, dtype=torch.int32, device="cuda"); ov = torch.empty(hcap, dtype=torch.uint8, device="cuda")
                status = torch.zeros(4, dtype=torch.int64, device="cuda")
                dev = lambda: api.check(L.fmd_kmer_collect_dev(d.h, None, w, min_occ, suf, hwork.data_ptr(), hwb, hcap, ob.data_ptr(), ok_.data_ptr(), ov.data_ptr(), status.data_ptr()))
                dev(); sync()
                if int(status[1]) == 0:
                    break
                del hwork, ob, ok_, ov
                torch.cuda.empty_cache()
                hcap *= 2
            sd, _ = repeat(dev, sync, a.repeats)
            n_ext = int(hwork[: 72 * 8].cpu().numpy().view(np.uint64)[68])       # the harvest's extension counter (fmd_kmer.hip: KM_EXT)
            assert int(status[0]) == len(got[0])
            r["harvest_o%d" % min_occ] = dict(st, w=w, suf_len=suf, triples=len(got[0]), **rate(n_ext, st))
            r["harvest_dev_o%d" % min_occ] = dict(sd, w=w, cap=hcap, **rate(n_ext, sd))
            del hwork, ob, ok_, ov
            torch.cuda.empty_cache()
        res["k"][str(k)] = r
    d_n = d.n
    d.close()
    os.makedirs(a.out, exist_ok=True)
    s = json.dumps(res, indent=1)
    print(s)
    with open(os.path.join(a.out, "time_kcount_%d.json" % N), "w") as f:
        f.write(s + "\n")
    ms = lambda x: "%.1f ms (%.1f .. %.1f)" % (x["median_s"] * 1e3, x["min_s"] * 1e3, x["max_s"] * 1e3)
    readme = os.path.join(a.out, "README.md")
    notes = ""
    if os.path.exists(readme):                         # what was written by hand under "## Notes" stays
        old = open(readme).read()
        notes = old[old.index("## Notes"):] if "## Notes" in old else ""
    with open(readme, "w") as f:
        f.write("# profiles/kcount -- kcount against the k-mer harvest (`fmd_kcount.hip`, `fmd_kmer.hip`)\n\n")
        f.write("`python tools/time_kcount.py --reads %d --err %g -k %s` on an MI355X: %d reads of %d bp at 30x with %g substitutions per base, indexed on\n"
                "the GPU (%.3g symbols).  `kcount_*` = `fmd_kcount`, the host form (allocation, sort and copy inside the clock), spectrum only and with a sink that\n"
                "only counts; `part_*` = `fmd_kcount_part_dev` from the four roots on buffers made beforehand; `harvest_o*` = `fmd_kmer_collect`, the host form of the\n"
                "yardstick (w = min(k, 27), min_occ 1 and 3; it starts small and pays for every pass that overflowed), `harvest_dev_o*` = `fmd_kmer_collect_dev` on\n"
                "buffers made beforehand.  Host clock around call + sync, one warm-up, %d runs; min .. max is the run-to-run spread.  `time_kcount_%d.json` holds every run.\n\n"
                % (N, a.err, " ".join(map(str, a.k)), N, LEN, a.err, float(d_n), a.repeats, N))
        f.write("| k | leg | time (median, min .. max) | n_ext | extensions / s (at min .. max time) |\n|---|---|---|---|---|\n")
        for k, r in res["k"].items():
            for leg, x in r.items():
                f.write("| %s | %s | %s | %d | %.3g (%.3g .. %.3g) |\n" % (k, leg, ms(x), x["n_ext"], x["ext_per_s"], x["ext_per_s_max"], x["ext_per_s_min"]))
        f.write("\n")
        for k, r in res["k"].items():
            if int(k) > 27:
                continue
            for o in (1, 3):
                h, p = r["harvest_dev_o%d" % o], r["part_spectrum"]
                spread = h["ext_per_s_max"] - h["ext_per_s_min"]
                f.write("k = %s: the kernels of kcount (part_spectrum) do %.3g extensions / s, those of the harvest at min_occ %d %.3g with a spread of %.2g: kcount is %s.\n"
                        % (k, p["ext_per_s"], o, h["ext_per_s"], spread, "below it by more than that spread" if p["ext_per_s"] < h["ext_per_s"] - spread else "not below it by more than that spread"))
        f.write("\n" + notes)


if __name__ == "__main__":
    main()
