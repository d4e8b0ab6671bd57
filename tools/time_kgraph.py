#!/usr/bin/env python3
"""Time of kgraph (fmd_karcs, fmd_kunitig) on the index tools/time_kcount.py uses: --reads 100 bp reads at 30x with --err substitutions, indexed on the GPU.
Per k (21, 31) and min_occ (1, 3), one handle in one run:
  arcs        fmd_karcs, the host form, with a sink that only counts what it is handed (allocation, sort and the copy to the host inside the clock);
  join        its only substitute: two fmd_kcount lists (k and k + 1) to sinks that keep them, and the join of the two in numpy -> the same arc bytes;
  compact     the GPU link resolution and doubling: ms_links + ms_label of fmd_kunitig's stat (host clock, each ended by a wait for the device);
  walk        fmdh_kgraph_compact_host (C, one thread) on the same k-mers and arcs;
  kunitig     fmd_kunitig whole, as a caller sees it (arcs + compact + the copy of nine arrays);
  kcount      fmd_kcount alone at k with a counting sink, for context.
Host clock; the first call of every leg is discarded, then --repeats runs: median, min .. max as the run-to-run spread.  A path WINS when it is faster than its
yardstick by more than the sum of the two spreads at every measured point.  Writes time_kgraph_<reads>.json and README.md (what stands under "## Notes"
there is kept) into --out.
Usage: python tools/time_kgraph.py [--reads 1000000] [--err 0.01] [-k 21 31] [-o 1 3] [--repeats 5] [--out profiles/kgraph]"""
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


def np_revcomp(w, m):
    out = np.zeros_like(w)
    for i in range(m):
        out |= (np.uint64(3) - (w >> np.uint64(2 * i) & np.uint64(3))) << np.uint64(2 * (m - 1 - i))
    return out


def join(km, k1, k):
    """the arc bytes of the ascending k-mers km from the (k+1)-mers k1: each in both orientations is a right arc of its first k bases"""
    arcs = np.zeros(len(km), dtype=np.float64)
    rc1 = np_revcomp(k1, k + 1)
    for q in (k1, rc1[rc1 != k1]):                    # (one that is its own reverse complement is one arc bit, not two)
        x, c = q >> np.uint64(2), (q & np.uint64(3)).astype(np.int64)
        r = np_revcomp(x, k)
        fw = x < r
        node = np.searchsorted(km, np.where(fw, x, r))
        arcs += np.bincount(node, weights=np.where(fw, 1 << c, 16 << (3 - c)), minlength=len(km))   # every (node, bit) once: the sum is the OR
    return arcs.astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--err", type=float, default=0.01)
    ap.add_argument("-k", type=int, nargs="+", default=[21, 31])
    ap.add_argument("-o", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kgraph"))
    a = ap.parse_args()
    assert all(3 <= k <= 31 and k & 1 for k in a.k) and a.repeats >= 3, "k odd, 3..31; at least three runs: the spread of the yardstick is part of the result"
    import torch
    assert api.device_count() > 0, "time_kgraph.py needs a GPU: nothing here is measured without one"
    L, H = api.lib(), hostlib.lib()
    N = a.reads
    reads = synth.reads_torch(synth.DEFAULT_SEED + 43, N, LEN, 30, err=a.err)
    d = api.build_index_inplace(reads.cpu().numpy())
    del reads
    torch.cuda.empty_cache()
    res = {"reads": N, "read_len": LEN, "err": a.err, "symbols": d.n, "repeats": a.repeats, "points": {}}
    for k in a.k:
        for mo in a.o:
            r = {}
            seen = [0]

            def count_sink3(ctx, n, kmer, count, arcs):
                seen[0] += n
                return 0
            cb3 = api.KARCS_SINK(count_sink3)
            stat = np.zeros(1, dtype=api.KGRAPH_STAT_DT)

            def arcs_only():
                seen[0] = 0
                api.check(L.fmd_karcs(d.h, k, mo, 0, C.cast(cb3, C.c_void_p), None, stat.ctypes.data))
            r["arcs"], _ = repeat(arcs_only, a.repeats)
            n_nodes = int(stat[0]["n_nodes"])
            assert seen[0] == n_nodes
            print("k=%d o=%d arcs %.1f ms, %d nodes" % (k, mo, r["arcs"]["median_s"] * 1e3, n_nodes), flush=True)

            def joined():
                km, _, _ = d.kmer_counts(k, mo)
                k1, _, _ = d.kmer_counts(k + 1, mo)
                return km, join(km, k1, k)
            r["join"], (km, ja) = repeat(joined, a.repeats)
            print("k=%d o=%d join %.1f ms" % (k, mo, r["join"]["median_s"] * 1e3), flush=True)
            gk, gc, ga = d.kmer_arcs(k, mo)
            assert np.array_equal(gk, km) and np.array_equal(ga, ja), "fmd_karcs and the join disagree"

            g = api.KUnitigC()

            def whole():
                api.check(L.fmd_kunitig(d.h, k, mo, 0, C.byref(g)))
                s = {f: getattr(g.stat, f) for f in api.KGRAPH_STAT_DT.names}
                for _, field, _ in api.KUnitigs.NODE + api.KUnitigs.UNITIG:
                    L.fmd_host_free(getattr(g, field))
                return s
            r["compact"], s = repeat(whole, a.repeats, value=lambda s: (s["ms_links"] + s["ms_label"]) * 1e-3)
            r["kunitig"], s = repeat(whole, a.repeats)
            r["stat"] = s
            print("k=%d o=%d compact %.1f ms, kunitig %.1f ms, %d unitigs, %d rounds" % (k, mo, r["compact"]["median_s"] * 1e3, r["kunitig"]["median_s"] * 1e3,
                                                                                         s["n_unitigs"], s["n_rounds"]), flush=True)
            hg = api.KUnitigC()

            def walk():
                assert H.fmdh_kgraph_compact_host(k, len(gk), gk.ctypes.data, ga.ctypes.data, C.addressof(hg)) == 0
                nu = int(hg.n_unitigs)
                H.fmdh_kgraph_free(C.addressof(hg))
                return nu
            r["walk"], nu = repeat(walk, a.repeats)
            assert nu == s["n_unitigs"], "the device's labelling and the host walk disagree"
            print("k=%d o=%d walk %.1f ms" % (k, mo, r["walk"]["median_s"] * 1e3), flush=True)
            seen2 = [0]

            def count_sink2(ctx, n, kmer, count):
                seen2[0] += n
                return 0
            cb2 = api.KCOUNT_SINK(count_sink2)
            h2, s2 = np.zeros(2, dtype=np.uint64), np.zeros(1, dtype=api.KCOUNT_STAT_DT)
            r["kcount"], _ = repeat(lambda: api.check(L.fmd_kcount(d.h, k, mo, 2, h2.ctypes.data, 0, C.cast(cb2, C.c_void_p), None, s2.ctypes.data)), a.repeats)
            for fast, slow in (("arcs", "join"), ("compact", "walk")):
                f, y = r[fast], r[slow]
                r[fast + "_wins"] = bool(y["median_s"] - f["median_s"] > (f["max_s"] - f["min_s"]) + (y["max_s"] - y["min_s"]))
            res["points"]["k%d_o%d" % (k, mo)] = r
    d_n = d.n
    d.close()
    os.makedirs(a.out, exist_ok=True)
    s = json.dumps(res, indent=1)
    with open(os.path.join(a.out, "time_kgraph_%d.json" % N), "w") as f:
        f.write(s + "\n")
    ms = lambda x: "%.1f ms (%.1f .. %.1f)" % (x["median_s"] * 1e3, x["min_s"] * 1e3, x["max_s"] * 1e3)
    notes = ""
    if os.path.exists(os.path.join(a.out, "README.md")):   # what was written by hand under "## Notes" stays
        old = open(os.path.join(a.out, "README.md")).read()
        notes = "\n" + old[old.index("## Notes"):] if "## Notes" in old else ""
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("# profiles/kgraph -- kgraph against its substitutes (`fmd_kgraph.hip`, `kgraph_cmd.c`)\n\n")
        f.write("`python tools/time_kgraph.py --reads %d --err %g` on an MI355X: %d reads of %d bp at 30x with %g substitutions per base, indexed on the GPU (%.3g\n"
                "symbols), one handle in one run.  `arcs` = `fmd_karcs` with a counting sink; `join` = two `fmd_kcount` lists (k, k + 1) kept and joined in numpy;\n"
                "`compact` = link resolution + doubling on the GPU (`ms_links + ms_label`); `walk` = `fmdh_kgraph_compact_host`, C, one thread, on the same arcs;\n"
                "`kunitig` = `fmd_kunitig` whole; `kcount` = `fmd_kcount` alone at k with a counting sink.  Host clock, the first call discarded, %d runs: median\n"
                "(min .. max).  A path wins when it is faster than its yardstick by more than the sum of the two spreads.  `time_kgraph_%d.json` holds every run.\n\n"
                % (N, a.err, N, LEN, a.err, float(d_n), a.repeats, N))
        f.write("| k | min_occ | nodes | unitigs | rounds | arcs | join | arcs wins | compact | walk | compact wins | kunitig | kcount |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for k in a.k:
            for mo in a.o:
                r = res["points"]["k%d_o%d" % (k, mo)]
                f.write("| %d | %d | %d | %d | %d | %s | %s | %s | %s | %s | %s | %s | %s |\n" % (
                    k, mo, r["stat"]["n_nodes"], r["stat"]["n_unitigs"], r["stat"]["n_rounds"], ms(r["arcs"]), ms(r["join"]), "yes" if r["arcs_wins"] else "no",
                    ms(r["compact"]), ms(r["walk"]), "yes" if r["compact_wins"] else "no", ms(r["kunitig"]), ms(r["kcount"])))
        f.write(notes)
    print(open(os.path.join(a.out, "README.md")).read())


if __name__ == "__main__":
    main()
