#!/usr/bin/env python3
"""Time of kbubble's stage (fmd_kcbubble) against its yardstick, the plain one-thread host walk: two read sets of --reads 100 bp reads each at 30x with --err
substitutions per base, the second from the genome of the first with --subs substitutions and --indels insertions / deletions of 1 to 4 bases, both indexed on
the GPU.  Per k and min_occ, on the same two handles in one run:
  (a) bubble      ms_bubble of fmd_kcbubble: the flag kernel, the scan, the emit kernel and the copy of the records (host clock, ended by a wait), against
      host_walk   fmdh_kcbubble_host (C, ONE thread, a binary search per step, no labels) over the arrays fmd_kcunitig returned;
  (b) kcbubble    fmd_kcbubble whole, as a caller sees it, against
      unitig+walk fmd_kcunitig whole and then the host walk over what it returned: what a caller had to do without the stage;
  (c) links       ms_links of the same fmd_kcbubble calls -- the same ports and the same binary searches -- and bubble as a share of it.
Host clock; the first call of every leg is discarded, then --repeats runs: median, min .. max as the run-to-run spread.  The records of the device and of the
host walk are compared before anything is written.  Writes time_kbubble_<reads>.json and README.md (what stands under "## Notes" there is kept) into --out.
Usage: python tools/time_kbubble.py [--reads 1000000] [--err 0.01] [--subs 300] [--indels 100] [-k 21 31] [-o 2 3] [--repeats 5] [--out profiles/kbubble]"""
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


def verdict(m, y):
    """m against the yardstick y: faster only when the gap is more than the sum of the two run-to-run ranges"""
    spread = (m["max_s"] - m["min_s"]) + (y["max_s"] - y["min_s"])
    if y["median_s"] - m["median_s"] > spread:
        return "faster beyond the spread"
    return "**slower beyond the spread**" if m["median_s"] - y["median_s"] > spread else "**within the spread**"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--err", type=float, default=0.01)
    ap.add_argument("--subs", type=int, default=300)
    ap.add_argument("--indels", type=int, default=100)
    ap.add_argument("-k", type=int, nargs="+", default=[21, 31])
    ap.add_argument("-o", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kbubble"))
    a = ap.parse_args()
    assert all(3 <= k <= 31 and k & 1 for k in a.k) and a.repeats >= 5, "k odd, 3..31; the median of at least 5"
    import torch
    assert api.device_count() > 0, "time_kbubble.py needs a GPU: nothing here is measured without one"
    L, H = api.lib(), hostlib.lib()
    N, seed = a.reads, synth.DEFAULT_SEED + 59
    gen = synth.genome_torch(seed, N, LEN, 30)
    g = gen.cpu().numpy().copy()
    at = (synth.rnd(seed, 31, np.arange(a.subs, dtype=np.uint64)) % np.uint64(len(g))).astype(np.int64)
    g[at] = g[at] % 4 + 1                              # A -> C -> G -> T -> A
    at = np.sort((synth.rnd(seed, 37, np.arange(a.indels, dtype=np.uint64)) % np.uint64(len(g) - 8)).astype(np.int64))[::-1]
    for x, p in enumerate(at):                         # from the right end on, so that the places to the left stay: deletions and insertions in turn
        m = 1 + int(synth.rnd(seed, 41, np.array([x], dtype=np.uint64))[0] % np.uint64(4))
        if x % 2:
            g = np.delete(g, np.arange(p, p + m))
        else:
            g = np.insert(g, p, (1 + synth.rnd(seed, 43 + x, np.arange(m, dtype=np.uint64)) % np.uint64(4)).astype(np.uint8))
    two = []
    for s, gs in enumerate((gen, torch.from_numpy(g).to(gen.device))):
        reads = synth.reads_torch(seed + s, N, LEN, 30, err=a.err, gen=gs)
        two.append(api.build_index_inplace(reads.cpu().numpy()))
        del reads
        torch.cuda.empty_cache()
    del gen, g
    hs = api._handles(two)
    os.makedirs(a.out, exist_ok=True)
    res = {"reads": N, "read_len": LEN, "err": a.err, "subs": a.subs, "indels": a.indels, "symbols": [d.n for d in two], "repeats": a.repeats, "points": {}}
    out_json = os.path.join(a.out, "time_kbubble_%d.json" % N)
    for k in a.k:
        for mo in a.o:
            r = {}
            o = api.KCBubbleC()

            def whole():
                api.check(L.fmd_kcbubble(2, hs, k, mo, 0, 0, C.byref(o)))
                s = api._kcgraph_stat(o.g.stat, 2)
                s.update(ms_bubble=float(o.ms_bubble), n_forks=int(o.n_forks), n_bubbles=int(o.n_bubbles))
                api._kcunitig_free(o.g)
                L.fmd_host_free(o.bubble)
                return s
            whole()                                      # (the first call is discarded; the same runs give the three figures)
            runs = []
            for _ in range(a.repeats):
                t = time.perf_counter()
                s = whole()
                runs.append((time.perf_counter() - t, s["ms_bubble"] * 1e-3, s["ms_links"] * 1e-3))
            r["kcbubble"], r["bubble"], r["links"] = (stats([x[j] for x in runs]) for j in range(3))
            r["stat"] = s
            g, b = api.kmer_joint_bubbles(two, k, mo)
            c = g.as_c()
            nf, nb, ptr = C.c_uint64(), C.c_uint64(), C.c_void_p()

            def walk():
                assert H.fmdh_kcbubble_host(k, C.addressof(c), 0, C.byref(nf), C.byref(nb), C.byref(ptr)) == 0
                n = int(nb.value)
                L.fmd_host_free(ptr)
                return n
            r["host_walk"], n_host = repeat(walk, a.repeats)
            n_forks, hb = hostlib.kcbubble_host(g)
            assert n_host == len(b) and n_forks == g.n_forks == s["n_forks"] and np.array_equal(hb, b), "the device's bubbles and the host walk disagree"
            u = api.KCUnitigC()

            def unitig_walk():
                api.check(L.fmd_kcunitig(2, hs, k, mo, 0, 0, C.byref(u)))
                assert H.fmdh_kcbubble_host(k, C.addressof(u), 0, C.byref(nf), C.byref(nb), C.byref(ptr)) == 0
                L.fmd_host_free(ptr)
                api._kcunitig_free(u)
            r["unitig+walk"], _ = repeat(unitig_walk, a.repeats)
            kinds = [ln.split("\t", 3)[2] for ln in hostlib.kbubble_text(g, b).splitlines()]
            r["kinds"] = {t: kinds.count(t) for t in ("SNP", "MNP", "INDEL", "COMPLEX")}
            res["points"]["k%d_o%d" % (k, mo)] = r
            with open(out_json, "w") as f:              # (every point as soon as it is there)
                f.write(json.dumps(res, indent=1) + "\n")
            print("[time_kbubble] k = %d, min_occ = %d: %d nodes, %d forks, %d bubbles, stage %.2f ms, host walk %.2f ms" % (
                k, mo, s["n_nodes"], s["n_forks"], s["n_bubbles"], r["bubble"]["median_s"] * 1e3, r["host_walk"]["median_s"] * 1e3), file=sys.stderr, flush=True)
            del g, b, hb, c
    for x in two:
        x.close()
    ms = lambda x: "%.2f ms (%.2f .. %.2f)" % (x["median_s"] * 1e3, x["min_s"] * 1e3, x["max_s"] * 1e3)
    readme = os.path.join(a.out, "README.md")
    notes = ""
    if os.path.exists(readme):                         # what was written by hand under "## Notes" stays
        old = open(readme).read()
        notes = old[old.index("## Notes"):] if "## Notes" in old else ""
    with open(readme, "w") as f:
        f.write("# profiles/kbubble -- kbubble's stage against the one-thread host walk (`fmd_kbubble.hip`, `kbubble_cmd.c`)\n\n")
        f.write("`python tools/time_kbubble.py --reads %d --err %g --subs %d --indels %d` on an MI355X: two sets of %d reads of %d bp at 30x with %g substitutions per\n"
                "base, the second from the genome of the first with %d substitutions and %d insertions / deletions of 1 to 4 bases, indexed on the GPU (%s symbols).\n"
                "`bubble` = `ms_bubble` of `fmd_kcbubble`; `host walk` = `fmdh_kcbubble_host`, C, ONE thread, a binary search per step, over the arrays `fmd_kcunitig`\n"
                "returned; `kcbubble` = `fmd_kcbubble` whole; `unitig + walk` = `fmd_kcunitig` whole, then the host walk; `links` = `ms_links` of the same calls (the\n"
                "same ports, the same searches).  Host clock, the first call of a leg discarded, %d runs: median (min .. max).  `time_kbubble_%d.json` holds every run.\n\n"
                % (N, a.err, a.subs, a.indels, N, LEN, a.err, a.subs, a.indels, ", ".join("%.3g" % float(v) for v in res["symbols"]), a.repeats, N))
        f.write("| k | min_occ | nodes | forks | bubbles (SNP / MNP / INDEL / COMPLEX) | bubble | host walk | walk / bubble | kcbubble | unitig + walk | links | bubble / links |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for key, r in res["points"].items():
            k, mo = (int(x[1:]) for x in key.split("_"))
            f.write("| %d | %d | %d | %d | %d (%s) | %s | %s | %.1f | %s | %s | %s | %.2f |\n" % (
                k, mo, r["stat"]["n_nodes"], r["stat"]["n_forks"], r["stat"]["n_bubbles"], " / ".join("%d" % r["kinds"][t] for t in ("SNP", "MNP", "INDEL", "COMPLEX")),
                ms(r["bubble"]), ms(r["host_walk"]), r["host_walk"]["median_s"] / r["bubble"]["median_s"], ms(r["kcbubble"]), ms(r["unitig+walk"]), ms(r["links"]),
                r["bubble"]["median_s"] / r["links"]["median_s"]))
        f.write("\n")
        for key, r in res["points"].items():
            k, mo = (int(x[1:]) for x in key.split("_"))
            f.write("k = %d, min_occ = %d: the stage against the host walk %s; fmd_kcbubble whole against fmd_kcunitig and the host walk %s.\n" % (
                k, mo, verdict(r["bubble"], r["host_walk"]), verdict(r["kcbubble"], r["unitig+walk"])))
        f.write("\n" + notes)
    print(open(readme).read())


if __name__ == "__main__":
    main()
