#!/usr/bin/env python3
"""Time of kmat (fmd_kmat) with its substitutes as the yardsticks, on the same handles in the same run.  Four related read sets: --reads 100 bp reads each at
30x with --err substitutions per base, sets 1..3 from the genome of set 0 with --subs substitutions each (at places of their own); all indexed on the GPU.
Per k and per N = 2, 3, 4 (the first N sets):
  kmat_spectrum      api.kmer_matrix_spectrum, everything selected: the 2^N pattern cells and the sums, no list;
  kmat_list          api.kmer_matrix, everything selected: the union of the sets' k-mers with N counts each;
  kmat_trio_list     api.kmer_matrix with (3, inf), (0, 0), ..: the k-mers at least 3 times in the first set and never in any other;
  kcount_join        yardstick (a), the only general substitute: DevIndex.kmer_counts of each index (fmd_kcount with a sink) and an N-way join of the
                     sorted lists on the host (numpy: a stable sort of the N runs, run boundaries, N scatters) -> the same columns;
  kcount_lists       the N kmer_counts calls of that yardstick alone, without the join: what is left of it if the join were free;
  kcount_trio        yardstick (a) of the selection: kmer_counts(min_occ = 3) of the first index, kmer_counts of the others, those the others lack;
  kcmp_*             yardstick (b), N = 2 only: fmd_kcmp itself (kmer_compare_spectrum with 2 bins per axis, kmer_compare, kmer_compare with (3, inf, 0, 0));
  merge_kcmp_trio    yardstick (c), N >= 3: fmd_dev_merge of the other indexes (no tables), then kmer_compare with (3, inf, 0, 0); the merge is inside the clock.
Every side copies every slice its sink is handed into numpy arrays and concatenates them; allocation, sort and copy to the host are inside the clock, as a
caller sees them.  The answers are compared before anything is written.  Host clock around call + sync; one warm-up, then --repeats runs (the second and later
calls on the handles); median, and min .. max as the run-to-run spread.  Writes time_kmat_<reads>.json (every run) and README.md (the table; what stands
under "## Notes" there is kept) into --out.
Usage: python tools/time_kmat.py [--reads 1000000] [--err 0.01] [--subs 300] [-k 21 31] [--repeats 3] [--out profiles/kmat]"""
import argparse, json, os, sys, time
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


def join(lists):
    """N ascending lists (kmers, counts) without repeats -> (their union ascending, counts[n, N], 0 where a list lacks the k-mer)"""
    cat = np.concatenate([k for k, _ in lists])
    src = np.repeat(np.arange(len(lists)), [len(k) for k, _ in lists])
    order = np.argsort(cat, kind="stable")
    s = cat[order]
    first = np.ones(len(s), dtype=bool)
    first[1:] = s[1:] != s[:-1]
    slot = np.cumsum(first) - 1
    out = np.zeros((int(first.sum()), len(lists)), dtype=np.uint32)
    vals = np.concatenate([c for _, c in lists])[order]
    out[slot, src[order]] = vals
    return s[first], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--err", type=float, default=0.01)
    ap.add_argument("--subs", type=int, default=300)
    ap.add_argument("-k", type=int, nargs="+", default=[21, 31])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmat"))
    a = ap.parse_args()
    assert all(2 <= k <= 32 for k in a.k) and a.repeats >= 3, "k = 2..32; at least three runs: the spread of the yardsticks is part of the result"
    import torch
    assert api.device_count() > 0, "time_kmat.py needs a GPU: nothing here is measured without one"
    L = api.lib()
    N, seed = a.reads, synth.DEFAULT_SEED + 53
    gen = synth.genome_torch(seed, N, LEN, 30)
    idx = []
    for s in range(4):
        g = gen.clone()
        if s:
            at = torch.from_numpy((synth.rnd(seed, 31 + s, np.arange(a.subs, dtype=np.uint64)) % np.uint64(len(gen))).astype(np.int64)).to(gen.device)
            g[at] = (g[at] % 4 + 1).to(torch.uint8)   # A -> C -> G -> T -> A
        reads = synth.reads_torch(seed + s, N, LEN, 30, err=a.err, gen=g)
        idx.append(api.build_index_inplace(reads.cpu().numpy()))
        del reads, g
        torch.cuda.empty_cache()
    del gen
    sync = lambda: api.check(L.fmd_dev_sync(idx[0].h, None))
    res = {"reads": N, "read_len": LEN, "err": a.err, "subs": a.subs, "symbols": [d.n for d in idx], "repeats": a.repeats, "k": {}}
    for k in a.k:
        res["k"][str(k)] = {}
        for n in (2, 3, 4):
            d = idx[:n]
            trio = [(3, None)] + [(0, 0)] * (n - 1)
            r = {}
            st, (hist, s0) = repeat(lambda: api.kmer_matrix_spectrum(d, k), sync, a.repeats)
            r["kmat_spectrum"] = dict(st, stat=s0)
            st, (km, c, s1) = repeat(lambda: api.kmer_matrix(d, k), sync, a.repeats)
            r["kmat_list"] = dict(st, stat=s1)
            st, (km3, c3, s3) = repeat(lambda: api.kmer_matrix(d, k, sel=trio), sync, a.repeats)
            r["kmat_trio_list"] = dict(st, stat=s3)
            assert s0["n_retries"] == 0 and s1["n_kmers"] == s0["n_kmers"] == int(hist.sum()) == len(km), "the two modes disagree"

            def trio_by_kcount():
                ka, ca, _ = d[0].kmer_counts(k, min_occ=3)
                for o in d[1:]:
                    kb, _, _ = o.kmer_counts(k)
                    only = kb[np.minimum(np.searchsorted(kb, ka), len(kb) - 1)] != ka
                    ka, ca = ka[only], ca[only]
                return ka, ca
            st, _ = repeat(lambda: [x.kmer_counts(k) for x in d] and None, sync, a.repeats)
            r["kcount_lists"] = dict(st, n=int(c.astype(bool).sum()))
            st, (u, x) = repeat(lambda: join([x.kmer_counts(k)[:2] for x in d]), sync, a.repeats)
            assert np.array_equal(u, km) and np.array_equal(x, c), "kmat and the join of the kcount lists disagree"
            pat = (x.astype(bool).astype(np.int64) << np.arange(n)).sum(axis=1)
            assert np.array_equal(np.bincount(pat, minlength=1 << n).astype(np.uint64), hist), "the spectrum and the join disagree"
            r["kcount_join"] = dict(st, n=len(u))
            del u, x, pat
            st, (ua, xa) = repeat(trio_by_kcount, sync, a.repeats)
            assert np.array_equal(ua, km3) and np.array_equal(xa, c3[:, 0]) and not c3[:, 1:].any(), "kmat and the kcount lists disagree on the selection"
            r["kcount_trio"] = dict(st, n=len(ua))
            if n == 2:
                st, (h2, t0) = repeat(lambda: d[0].kmer_compare_spectrum(d[1], k, n_bins=2), sync, a.repeats)
                assert [int(h2[1, 0]), int(h2[0, 1]), int(h2[1, 1])] == [int(v) for v in hist[1:]], "kmat and kcmp disagree on the spectrum"
                r["kcmp_spectrum"] = dict(st, stat=t0)
                st, (kk, k0, k1, t1) = repeat(lambda: d[0].kmer_compare(d[1], k), sync, a.repeats)
                assert np.array_equal(kk, km) and np.array_equal(k0, c[:, 0]) and np.array_equal(k1, c[:, 1]), "kmat and kcmp disagree on the list"
                r["kcmp_list"] = dict(st, stat=t1)
                del kk, k0, k1
                st, (kk, k0, k1, t3) = repeat(lambda: d[0].kmer_compare(d[1], k, sel=(3, INF, 0, 0)), sync, a.repeats)
                assert np.array_equal(kk, km3) and np.array_equal(k0, c3[:, 0])
                r["kcmp_trio_list"] = dict(st, stat=t3)
            else:
                def merged_trio():
                    m = d[1]
                    for o in d[2:]:
                        m2 = m.merge(o, tables=False)
                        if m is not d[1]:
                            m.close()
                        m = m2
                    out = d[0].kmer_compare(m, k, sel=(3, INF, 0, 0))
                    m.close()
                    return out
                st, (kk, k0, k1, t3) = repeat(merged_trio, sync, a.repeats)
                assert np.array_equal(kk, km3) and np.array_equal(k0, c3[:, 0]), "kmat and kcmp on the merged others disagree"
                r["merge_kcmp_trio"] = dict(st, stat=t3)
            del km, c, km3, c3
            res["k"][str(k)][str(n)] = r
            print("[time_kmat] k = %d, N = %d: done" % (k, n), file=sys.stderr, flush=True)
    for d in idx:
        d.close()
    os.makedirs(a.out, exist_ok=True)
    s = json.dumps(res, indent=1)
    print(s)
    with open(os.path.join(a.out, "time_kmat_%d.json" % N), "w") as f:
        f.write(s + "\n")
    ms = lambda x: "%.1f ms (%.1f .. %.1f)" % (x["median_s"] * 1e3, x["min_s"] * 1e3, x["max_s"] * 1e3)
    readme = os.path.join(a.out, "README.md")
    notes = ""
    if os.path.exists(readme):                         # what was written by hand under "## Notes" stays
        old = open(readme).read()
        notes = old[old.index("## Notes"):] if "## Notes" in old else ""
    with open(readme, "w") as f:
        f.write("# profiles/kmat -- kmat against kcount lists joined on the host, kcmp, and merge + kcmp (`fmd_kmat.hip`)\n\n")
        f.write("`python tools/time_kmat.py --reads %d --err %g --subs %d -k %s` on an MI355X: four sets of %d reads of %d bp at 30x with %g substitutions per base,\n"
                "sets 1..3 from the genome of set 0 with %d substitutions each, indexed on the GPU (%s symbols).  N = the first N sets.  `kmat_*` = `fmd_kmat`\n"
                "through `api.kmer_matrix_spectrum` / `kmer_matrix`; the other legs are the yardsticks (see the tool's head).  Host clock around call + sync, one\n"
                "warm-up, %d runs; min .. max is the run-to-run spread.  `time_kmat_%d.json` holds every run.\n\n"
                % (N, a.err, a.subs, " ".join(map(str, a.k)), N, LEN, a.err, a.subs, ", ".join("%.3g" % float(v) for v in res["symbols"]), a.repeats, N))
        f.write("| k | N | leg | time (median, min .. max) | k-mers | extensions / s |\n|---|---|---|---|---|---|\n")
        for k, by_n in res["k"].items():
            for n, r in by_n.items():
                for leg, x in r.items():
                    cnt = x["stat"]["n_kmers"] if "stat" in x else x["n"]
                    f.write("| %s | %s | %s | %s | %d | %s |\n" % (k, n, leg, ms(x), cnt, "%.3g" % (x["stat"]["n_ext"] / x["median_s"]) if "stat" in x else "-"))
        f.write("\n")
        for k, by_n in res["k"].items():
            for n, r in by_n.items():
                pairs = [("kmat_list", "kcount_join"), ("kmat_list", "kcount_lists"), ("kmat_trio_list", "kcount_trio")]
                pairs += [("kmat_spectrum", "kcmp_spectrum"), ("kmat_list", "kcmp_list"), ("kmat_trio_list", "kcmp_trio_list")] if n == "2" else [("kmat_trio_list", "merge_kcmp_trio")]
                for mine, yard in pairs:
                    m, y = r[mine], r[yard]
                    verdict = "faster beyond the spread" if m["max_s"] < y["min_s"] else ("**slower beyond the spread**" if m["min_s"] > y["max_s"] else "within the spread")
                    f.write("k = %s, N = %s: %s %.1f ms against %s %.1f ms (%.1f .. %.1f): %s, %.2fx.\n" % (k, n, mine, m["median_s"] * 1e3, yard, y["median_s"] * 1e3,
                                                                                                       y["min_s"] * 1e3, y["max_s"] * 1e3, verdict, y["median_s"] / m["median_s"]))
        f.write("\n" + notes)


if __name__ == "__main__":
    main()
