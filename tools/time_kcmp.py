#!/usr/bin/env python3
"""Time of kcmp (fmd_kcmp) with the only substitute there was as the yardstick, on the same handles in the same run.  Two related read sets: --reads
100 bp reads each at 30x with --err substitutions per base, the second from the genome of the first with --subs substitutions; both indexed on the GPU.
Per k:
  kcmp_spectrum      DevIndex.kmer_compare_spectrum, everything selected, 256 bins per axis: no list;
  kcmp_union_list    DevIndex.kmer_compare, everything selected: the union of both sets' k-mers with both counts;
  kcmp_aspec_list    DevIndex.kmer_compare with (3, inf, 0, 0): the k-mers at least 3 times in the first set and never in the second;
  two_kcount_union   the yardstick: DevIndex.kmer_counts of each index (fmd_kcount with a sink) and a merge-join of the two sorted lists on the host
                     (numpy: a stable sort of the two runs, run boundaries, two scatters) -> the same three columns; `+ hist` adds the 2-D histogram;
  two_kcount_lists   the two kmer_counts calls of that yardstick alone, without the join: what is left of it if the join were free;
  two_kcount_aspec   the yardstick of the selection: kmer_counts(min_occ = 3) of the first index, kmer_counts of the second, those of the first that the
                     second lacks (searchsorted).
Both sides copy every slice their sink is handed into numpy arrays and concatenate them; allocation, sort and copy to the host are inside the clock, as a
caller sees them.  The results are compared before anything is written.  For context: the contrast walk of the same two indexes (fmd_contrast_dev -k55
-o3, pair nodes / s; its time includes the tips).  Host clock around call + sync; one warm-up, then --repeats runs; median, and min .. max as the
run-to-run spread.  Writes time_kcmp_<reads>.json (every run) and README.md (the table; what stands under "## Notes" there is kept) into --out.
Usage: python tools/time_kcmp.py [--reads 1000000] [--err 0.01] [--subs 300] [-k 21 31] [--repeats 3] [--out profiles/kcmp]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fermi_amd import api, synth

LEN = 100
INF = api.KCMP_NO_MAX


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


def merge_join(ka, ca, kb, cb):
    """two ascending lists without repeats -> (their union ascending, the count in the first or 0, the count in the second or 0)"""
    cat = np.concatenate([ka, kb])
    order = np.argsort(cat, kind="stable")
    s = cat[order]
    first = np.ones(len(s), dtype=bool)
    first[1:] = s[1:] != s[:-1]
    slot = np.cumsum(first) - 1
    c0, c1 = np.zeros(int(first.sum()), dtype=np.uint32), np.zeros(int(first.sum()), dtype=np.uint32)
    from_a = order < len(ka)
    c0[slot[from_a]] = ca[order[from_a]]
    c1[slot[~from_a]] = cb[order[~from_a] - len(ka)]
    return s[first], c0, c1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--err", type=float, default=0.01)
    ap.add_argument("--subs", type=int, default=300)
    ap.add_argument("-k", type=int, nargs="+", default=[21, 31])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kcmp"))
    a = ap.parse_args()
    assert all(2 <= k <= 32 for k in a.k) and a.repeats >= 3, "k = 2..32; at least three runs: the spread of the yardstick is part of the result"
    import torch
    assert api.device_count() > 0, "time_kcmp.py needs a GPU: nothing here is measured without one"
    L = api.lib()
    N, seed = a.reads, synth.DEFAULT_SEED + 47
    gen = synth.genome_torch(seed, N, LEN, 30)
    gen2 = gen.clone()
    at = torch.from_numpy((synth.rnd(seed, 31, np.arange(a.subs, dtype=np.uint64)) % np.uint64(len(gen))).astype(np.int64)).to(gen.device)
    gen2[at] = (gen2[at] % 4 + 1).to(torch.uint8)     # A -> C -> G -> T -> A
    idx = []
    for s, g in ((seed, gen), (seed + 1, gen2)):
        reads = synth.reads_torch(s, N, LEN, 30, err=a.err, gen=g)
        idx.append(api.build_index_inplace(reads.cpu().numpy()))
        del reads
        torch.cuda.empty_cache()
    del gen, gen2
    d0, d1 = idx
    sync = lambda: api.check(L.fmd_dev_sync(d0.h, None))
    res = {"reads": N, "read_len": LEN, "err": a.err, "subs": a.subs, "symbols": [d0.n, d1.n], "repeats": a.repeats, "k": {}}
    for k in a.k:
        r = {}
        st, (hist, s0) = repeat(lambda: d0.kmer_compare_spectrum(d1, k, n_bins=256), sync, a.repeats)
        r["kcmp_spectrum"] = dict(st, stat=s0)
        st, (km, c0, c1, s1) = repeat(lambda: d0.kmer_compare(d1, k), sync, a.repeats)
        r["kcmp_union_list"] = dict(st, stat=s1)
        st, (km3, c03, c13, s3) = repeat(lambda: d0.kmer_compare(d1, k, sel=(3, INF, 0, 0)), sync, a.repeats)
        r["kcmp_aspec_list"] = dict(st, stat=s3)
        assert s0["n_retries"] == 0 and s1["n_kmers"] == s0["n_kmers"] == int(hist.sum()) == len(km), "the two modes disagree"

        def union():
            ka, ca, _ = d0.kmer_counts(k)
            kb, cb, _ = d1.kmer_counts(k)
            return merge_join(ka, ca, kb, cb)

        def union_hist():
            u, x0, x1 = union()
            cell = np.minimum(x0, 255).astype(np.int64) * 256 + np.minimum(x1, 255)
            return np.bincount(cell, minlength=65536).reshape(256, 256)

        def aspec():
            ka, ca, _ = d0.kmer_counts(k, min_occ=3)
            kb, cb, _ = d1.kmer_counts(k)
            j = np.minimum(np.searchsorted(kb, ka), len(kb) - 1)
            only = kb[j] != ka
            return ka[only], ca[only]
        st, _ = repeat(lambda: (d0.kmer_counts(k), d1.kmer_counts(k)) and None, sync, a.repeats)
        r["two_kcount_lists"] = dict(st, n=s0["n_only0"] + s0["n_only1"] + 2 * s0["n_shared"])
        st, (u, x0, x1) = repeat(union, sync, a.repeats)
        assert np.array_equal(u, km) and np.array_equal(x0, c0) and np.array_equal(x1, c1), "kcmp and the join of two kcount lists disagree"
        r["two_kcount_union"] = dict(st, n=len(u))
        st, h2 = repeat(union_hist, sync, a.repeats)
        assert np.array_equal(h2.astype(np.uint64), hist)
        r["two_kcount_union + hist"] = dict(st, n=len(u))
        st, (ua, xa) = repeat(aspec, sync, a.repeats)
        assert np.array_equal(ua, km3) and np.array_equal(xa, c03) and not c13.any()
        r["two_kcount_aspec"] = dict(st, n=len(ua))
        del km, c0, c1, u, x0, x1
        res["k"][str(k)] = r
    # the contrast walk of the same two indexes, for context: capacity doubled until nothing overflows
    dm = []

    def dmalloc(n):
        p = C.c_void_p()
        api.check(L.fmd_dev_malloc(0, n, C.byref(p)))
        dm.append(p)
        return p
    cap = 1 << 22
    while True:
        wb = L.fmd_contrast_work_bytes(cap)
        nb0, nb1 = (int(d0.mcnt[1]) + 63) // 64 * 8 + 8, (int(d1.mcnt[1]) + 63) // 64 * 8 + 8
        b0, b1, d_work, d_st = dmalloc(nb0), dmalloc(nb1), dmalloc(wb), dmalloc(32)
        api.check(L.fmd_memset_dev(b0, 0, nb0, None)); api.check(L.fmd_memset_dev(b1, 0, nb1, None))
        sync()
        dt, _ = timed(lambda: api.check(L.fmd_contrast_dev(d0.h, d1.h, None, 55, 3, 0xf, b0, b1, d_work, wb, cap, d_st)), sync)
        cs = np.zeros(4, np.uint64)
        api.check(L.fmd_memcpy_d2h(cs.ctypes.data, d_st, 32, None))
        while dm:
            L.fmd_dev_free(dm.pop())
        if cs[1] == 0:
            break
        cap *= 2
    res["contrast_walk"] = {"s": dt, "cap": cap, "pair_nodes": int(cs[0]), "pair_nodes_per_s": int(cs[0]) / dt}
    d0.close(); d1.close()
    os.makedirs(a.out, exist_ok=True)
    s = json.dumps(res, indent=1)
    print(s)
    with open(os.path.join(a.out, "time_kcmp_%d.json" % N), "w") as f:
        f.write(s + "\n")
    ms = lambda x: "%.1f ms (%.1f .. %.1f)" % (x["median_s"] * 1e3, x["min_s"] * 1e3, x["max_s"] * 1e3)
    readme = os.path.join(a.out, "README.md")
    notes = ""
    if os.path.exists(readme):                         # what was written by hand under "## Notes" stays
        old = open(readme).read()
        notes = old[old.index("## Notes"):] if "## Notes" in old else ""
    with open(readme, "w") as f:
        f.write("# profiles/kcmp -- kcmp against two kcount lists joined on the host (`fmd_kcmp.hip`, `fmd_kcount.hip`)\n\n")
        f.write("`python tools/time_kcmp.py --reads %d --err %g --subs %d -k %s` on an MI355X: two sets of %d reads of %d bp at 30x with %g substitutions per base,\n"
                "the second from the first's genome with %d substitutions, indexed on the GPU (%.3g and %.3g symbols).  `kcmp_*` = `fmd_kcmp` through\n"
                "`DevIndex.kmer_compare_spectrum` / `kmer_compare`; `two_kcount_*` = the yardstick, `DevIndex.kmer_counts` of each index and a numpy merge-join\n"
                "on the host (see the tool's head).  Host clock around call + sync, one warm-up, %d runs; min .. max is the run-to-run spread.\n"
                "`time_kcmp_%d.json` holds every run.\n\n" % (N, a.err, a.subs, " ".join(map(str, a.k)), N, LEN, a.err, a.subs, float(res["symbols"][0]), float(res["symbols"][1]), a.repeats, N))
        f.write("| k | leg | time (median, min .. max) | k-mers | pair-side extensions / s |\n|---|---|---|---|---|\n")
        for k, r in res["k"].items():
            for leg, x in r.items():
                n = x["stat"]["n_kmers"] if "stat" in x else x["n"]
                f.write("| %s | %s | %s | %d | %s |\n" % (k, leg, ms(x), n, "%.3g" % (x["stat"]["n_ext"] / x["median_s"]) if "stat" in x else "-"))
        f.write("\n")
        for k, r in res["k"].items():
            for mine, yard in (("kcmp_spectrum", "two_kcount_union + hist"), ("kcmp_union_list", "two_kcount_union"), ("kcmp_union_list", "two_kcount_lists"),
                                ("kcmp_aspec_list", "two_kcount_aspec")):
                m, y = r[mine], r[yard]
                verdict = "faster beyond the spread" if m["max_s"] < y["min_s"] else ("**slower beyond the spread**" if m["min_s"] > y["max_s"] else "within the spread")
                f.write("k = %s: %s %.1f ms against %s %.1f ms (%.1f .. %.1f): %s, %.2fx.\n" % (k, mine, m["median_s"] * 1e3, yard, y["median_s"] * 1e3, y["min_s"] * 1e3,
                                                                                             y["max_s"] * 1e3, verdict, y["median_s"] / m["median_s"]))
        c = res["contrast_walk"]
        f.write("\nFor context, the contrast walk (`k_ct_level` and the tips, -k55 -o3) of the same two indexes: %.3g pair nodes in %.1f ms, %.3g pair nodes / s.\n"
                % (c["pair_nodes"], c["s"] * 1e3, c["pair_nodes_per_s"]))
        f.write("\n" + notes)


if __name__ == "__main__":
    main()
