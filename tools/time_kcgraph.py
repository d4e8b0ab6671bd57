#!/usr/bin/env python3
"""Time of kcgraph (fmd_kcarcs, fmd_kcunitig) against its substitutes, on the data tools/time_kmat.py uses: four related read sets, --reads 100 bp reads each at
30x with --err substitutions per base, sets 1..3 from the genome of set 0 with --subs substitutions each, all indexed on the GPU.  N = the first N sets; N = 8
is the four sets twice (every handle given twice: eight sides are walked, four distinct indexes are read).  Per k, min_occ and N, on the same handles in one run:
  kcarcs      fmd_kcarcs with a sink that only counts what it is handed (allocation, sort and the copy to the host inside the clock);
  karcs_sum   the floor the joint pass aims at: N plain fmd_karcs calls with counting sinks, no join -- the same 2 N extensions per node;
  karcs_join  the only substitute there is: N fmd_karcs lists to sinks that keep them, joined on the host in numpy -> the same k-mers, arc bytes and union
              bytes, and the counts of every colour that holds the node (a plain list has no count below min_occ);
  compact     link resolution, doubling and the per-unitig sums on the GPU: ms_links + ms_label of fmd_kcunitig's stat (host clock, each ended by a wait);
  walk        fmdh_kcgraph_compact_host (C, one thread) on the same arrays, sums included;
  kcunitig    fmd_kcunitig whole, as a caller sees it.
and for N = 1: kcarcs against fmd_karcs and kcunitig against fmd_kunitig themselves.
Host clock; the first call of every leg is discarded (the second call on the handles is the first that counts), then --repeats runs: median, min .. max as the
run-to-run spread.  The answers are compared before anything is written.  Writes time_kcgraph_<reads>.json and README.md (what stands under "## Notes" there is
kept) into --out.
Usage: python tools/time_kcgraph.py [--reads 1000000] [--err 0.01] [--subs 300] [-k 21 31] [-o 1 3] [-n 2 3 4 8] [--repeats 5] [--out profiles/kcgraph]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fermi_amd import api, hostlib, synth

LEN = 100


def stats(v):
    runs, v = list(v), sorted(v)
    return {"median_s": v[len(v) // 2], "min_s": v[0], "max_s": v[-1], "runs_s": runs}


def repeat(fn, n, value=None):
    """fn once unclocked, then n clocked runs; value(result) replaces the host clock where the call measures itself"""
    fn()
    out = []
    for _ in range(n):
        t = time.perf_counter()
        r = fn()
        out.append(value(r) if value else time.perf_counter() - t)
    return stats(out), r


def join(lists):
    """N ascending lists (kmers, counts, arcs) -> (their union ascending, counts[n, N], arcs[n, N], uarcs), 0 where a list lacks the k-mer"""
    km = np.unique(np.concatenate([x[0] for x in lists]))
    counts, arcs = np.zeros((len(km), len(lists)), np.uint32, order="F"), np.zeros((len(km), len(lists)), np.uint8, order="F")
    for i, (k, c, a) in enumerate(lists):
        at = np.searchsorted(km, k)
        counts[at, i] = c; arcs[at, i] = a
    return km, counts, arcs, np.bitwise_or.reduce(arcs, axis=1)


def verdict(m, y):
    return "faster beyond the spread" if m["max_s"] < y["min_s"] else ("**slower beyond the spread**" if m["min_s"] > y["max_s"] else "within the spread")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--err", type=float, default=0.01)
    ap.add_argument("--subs", type=int, default=300)
    ap.add_argument("-k", type=int, nargs="+", default=[21, 31])
    ap.add_argument("-o", type=int, nargs="+", default=[1, 3])
    ap.add_argument("-n", type=int, nargs="+", default=[2, 3, 4, 8])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kcgraph"))
    a = ap.parse_args()
    assert all(3 <= k <= 31 and k & 1 for k in a.k) and all(1 <= n <= 8 for n in a.n) and a.repeats >= 5, "k odd, 3..31; N 1..8; the median of at least 5"
    import torch
    assert api.device_count() > 0, "time_kcgraph.py needs a GPU: nothing here is measured without one"
    L, H = api.lib(), hostlib.lib()
    N, seed = a.reads, synth.DEFAULT_SEED + 53
    gen = synth.genome_torch(seed, N, LEN, 30)
    four = []
    for s in range(4):
        g = gen.clone()
        if s:
            at = torch.from_numpy((synth.rnd(seed, 31 + s, np.arange(a.subs, dtype=np.uint64)) % np.uint64(len(gen))).astype(np.int64)).to(gen.device)
            g[at] = (g[at] % 4 + 1).to(torch.uint8)   # A -> C -> G -> T -> A
        reads = synth.reads_torch(seed + s, N, LEN, 30, err=a.err, gen=g)
        four.append(api.build_index_inplace(reads.cpu().numpy()))
        del reads, g
        torch.cuda.empty_cache()
    del gen
    os.makedirs(a.out, exist_ok=True)
    res = {"reads": N, "read_len": LEN, "err": a.err, "subs": a.subs, "symbols": [d.n for d in four], "repeats": a.repeats, "points": {}}
    seen = [0]

    def sink_c(ctx, n, kmer, count, arcs, uarcs):
        seen[0] += n
        return 0

    def sink_p(ctx, n, kmer, count, arcs):
        seen[0] += n
        return 0
    cbc, cbp = api.KCARCS_SINK(sink_c), api.KARCS_SINK(sink_p)
    for k in a.k:
        for mo in a.o:
            for n in [1] + list(a.n):
                d = [four[i % 4] for i in range(n)]
                hs = api._handles(d)
                r = {}
                st = api.KCGraphStatC()
                pst = np.zeros(1, dtype=api.KGRAPH_STAT_DT)

                def kcarcs():
                    seen[0] = 0
                    api.check(L.fmd_kcarcs(n, hs, k, mo, 0, C.cast(cbc, C.c_void_p), None, C.byref(st)))
                r["kcarcs"], _ = repeat(kcarcs, a.repeats)
                n_nodes = int(st.g.n_nodes)
                assert seen[0] == n_nodes

                def karcs_sum():
                    for x in d:
                        api.check(L.fmd_karcs(x.h, k, mo, 0, C.cast(cbp, C.c_void_p), None, pst.ctypes.data))
                r["karcs_sum"], _ = repeat(karcs_sum, a.repeats)
                gk, gc, ga, gu = api.kmer_joint_arcs(d, k, mo)
                if n > 1:
                    r["karcs_join"], (jk, jc, ja, ju) = repeat(lambda: join([x.kmer_arcs(k, mo) for x in d]), a.repeats)
                    assert np.array_equal(jk, gk) and np.array_equal(ja, ga) and np.array_equal(ju, gu) and np.array_equal(jc, np.where(gc >= mo, gc, 0)), \
                        "fmd_kcarcs and the join of the fmd_karcs lists disagree"
                    del jk, jc, ja, ju
                pt = np.zeros(len(gk), np.uint8)
                for i in range(n):
                    pt |= ((gc[:, i] >= mo).astype(np.uint8) << i).astype(np.uint8)
                g = api.KCUnitigC()

                def whole():
                    api.check(L.fmd_kcunitig(n, hs, k, mo, 0, 0, C.byref(g)))
                    s = api._kcgraph_stat(g.stat, n)
                    for _, field, _ in api.KCUnitigs.NODE + api.KCUnitigs.UNITIG:
                        L.fmd_host_free(getattr(g, field))
                    return s
                r["compact"], s = repeat(whole, a.repeats, value=lambda s: (s["ms_links"] + s["ms_label"]) * 1e-3)
                r["kcunitig"], s = repeat(whole, a.repeats)
                r["stat"] = s
                hg = api.KCUnitigC()

                def walk():
                    assert H.fmdh_kcgraph_compact_host(k, n, len(gk), gk.ctypes.data, gc.ctypes.data, gu.ctypes.data, pt.ctypes.data, 0, C.addressof(hg)) == 0
                    nu = int(hg.n_unitigs)
                    H.fmdh_kcgraph_free(C.addressof(hg))
                    return nu
                r["walk"], nu = repeat(walk, a.repeats)
                assert nu == s["n_unitigs"], "the device's labelling and the host walk disagree"
                if n == 1:
                    pg = api.KUnitigC()

                    def plain():
                        api.check(L.fmd_kunitig(d[0].h, k, mo, 0, C.byref(pg)))
                        for _, field, _ in api.KUnitigs.NODE + api.KUnitigs.UNITIG:
                            L.fmd_host_free(getattr(pg, field))
                        return int(pg.n_unitigs)
                    r["kunitig"], pu = repeat(plain, a.repeats)
                    assert pu == s["n_unitigs"]
                res["points"]["k%d_o%d_n%d" % (k, mo, n)] = r
                with open(os.path.join(a.out, "time_kcgraph_%d.json" % N), "w") as f:   # (every point as soon as it is there)
                    f.write(json.dumps(res, indent=1) + "\n")
                print("[time_kcgraph] k = %d, min_occ = %d, N = %d: %d nodes, kcarcs %.1f ms, sum %.1f ms%s" % (
                    k, mo, n, n_nodes, r["kcarcs"]["median_s"] * 1e3, r["karcs_sum"]["median_s"] * 1e3,
                    ", join %.1f ms" % (r["karcs_join"]["median_s"] * 1e3) if n > 1 else ""), file=sys.stderr, flush=True)
                del gk, gc, ga, gu, pt
    for x in four:
        x.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "time_kcgraph_%d.json" % N), "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    ms = lambda x: "%.1f ms (%.1f .. %.1f)" % (x["median_s"] * 1e3, x["min_s"] * 1e3, x["max_s"] * 1e3)
    readme = os.path.join(a.out, "README.md")
    notes = ""
    if os.path.exists(readme):                         # what was written by hand under "## Notes" stays
        old = open(readme).read()
        notes = old[old.index("## Notes"):] if "## Notes" in old else ""
    with open(readme, "w") as f:
        f.write("# profiles/kcgraph -- kcgraph against N plain kgraph runs, joined on the host or not (`fmd_kcgraph.hip`, `kcgraph_cmd.c`)\n\n")
        f.write("`python tools/time_kcgraph.py --reads %d --err %g --subs %d` on an MI355X: four sets of %d reads of %d bp at 30x with %g substitutions per base, sets\n"
                "1..3 from the genome of set 0 with %d substitutions each, indexed on the GPU (%s symbols).  N = the first N sets; N = 8 = the four sets twice.\n"
                "`kcarcs` = `fmd_kcarcs` with a counting sink; `karcs_sum` = N `fmd_karcs` calls with counting sinks; `karcs_join` = N `fmd_karcs` lists kept and\n"
                "joined in numpy; `compact` = `ms_links + ms_label` of `fmd_kcunitig`; `walk` = `fmdh_kcgraph_compact_host`, C, one thread; `kcunitig` whole.  Host\n"
                "clock, the first call of a leg discarded, %d runs: median (min .. max).  `time_kcgraph_%d.json` holds every run.\n\n"
                % (N, a.err, a.subs, N, LEN, a.err, a.subs, ", ".join("%.3g" % float(v) for v in res["symbols"]), a.repeats, N))
        f.write("| k | min_occ | N | nodes | unitigs | kcarcs | karcs_sum | kcarcs / sum | karcs_join | join / kcarcs | compact | walk | kcunitig |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for key, r in res["points"].items():
            k, mo, n = (int(x[1:]) for x in key.split("_"))
            j = r.get("karcs_join")
            f.write("| %d | %d | %d | %d | %d | %s | %s | %.2f | %s | %s | %s | %s | %s |\n" % (
                k, mo, n, r["stat"]["n_nodes"], r["stat"]["n_unitigs"], ms(r["kcarcs"]), ms(r["karcs_sum"]), r["kcarcs"]["median_s"] / r["karcs_sum"]["median_s"],
                ms(j) if j else "-", "%.2f" % (j["median_s"] / r["kcarcs"]["median_s"]) if j else "-", ms(r["compact"]), ms(r["walk"]), ms(r["kcunitig"])))
        f.write("\n")
        for key, r in res["points"].items():
            k, mo, n = (int(x[1:]) for x in key.split("_"))
            if n == 1:
                f.write("k = %d, min_occ = %d, N = 1: kcarcs against fmd_karcs %s; kcunitig %s against fmd_kunitig %s: %s.\n" % (
                    k, mo, verdict(r["kcarcs"], r["karcs_sum"]), ms(r["kcunitig"]), ms(r["kunitig"]), verdict(r["kcunitig"], r["kunitig"])))
            else:
                f.write("k = %d, min_occ = %d, N = %d: kcarcs against the join %s, against the sum of the plain calls %s; compact against the walk %s.\n" % (
                    k, mo, n, verdict(r["kcarcs"], r["karcs_join"]), verdict(r["kcarcs"], r["karcs_sum"]), verdict(r["compact"], r["walk"])))
        f.write("\n" + notes)
    print(open(readme).read())


if __name__ == "__main__":
    main()
