#!/usr/bin/env python3
"""Time of kprofile (fmd_kprofile_dev) on its paths, with the only substitute there was as the yardstick: the N-free windows of the same queries,
materialised on the device as separate reads, through fmd_bsearch_dev on the same handle in the same run (materialisation and upload not charged).
--reads 100 bp reads at 30x with --err substitutions are indexed on the GPU, the way tools/time_kcount.py builds its index.  Query sets:
  a  the first --queries of the indexed reads;   b  as many error-free reads of the same genome;   c  the genome itself in pieces of 10 kb.
Per (set, k) and path -- plain (FMD_KPROFILE_PLAIN) and the library's choice (flags = 0); any further path goes into PATHS -- fmd_kprofile_dev on buffers made
before the clock starts: host clock around call + sync, the first call discarded, then --repeats runs; median, min .. max as the run-to-run spread,
windows / s, n_ext.  Every path's counts are compared with the plain path's, and the yardstick's cnt with them (a window that is its own reverse
complement: halved).  Writes time_kprofile_<reads>.json (every run) and README.md (the table, the comparison and the rule of choice it gives; what
stands under "## Notes" there is kept) into --out.
Usage: python tools/time_kprofile.py [--reads 1000000] [--err 0.01] [--queries 200000] [-k 21 31 55] [--repeats 5] [--out profiles/kprofile]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fermi_amd import api, synth

LEN = 100
# (the shared path -- FMD_KPROFILE_SHARED with groups of 4 and of 8 -- stood here when profiles/kprofile was measured; it lost everywhere and left the library)
PATHS = (("plain", api.KPROFILE_PLAIN), ("default", 0))


def stats(v):
    runs, v = list(v), sorted(v)
    return {"median_s": v[len(v) // 2], "min_s": v[0], "max_s": v[-1], "runs_s": runs}


def repeat(fn, sync, n):
    fn(); sync()                                       # the first call on the handle is discarded
    out = []
    for _ in range(n):
        t = time.perf_counter()
        fn(); sync()
        out.append(time.perf_counter() - t)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--err", type=float, default=0.01)
    ap.add_argument("--queries", type=int, default=200_000)
    ap.add_argument("-k", type=int, nargs="+", default=[21, 31, 55])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kprofile"))
    a = ap.parse_args()
    assert all(1 <= k <= min(LEN, api.KPROFILE_MAX_K) for k in a.k) and a.repeats >= 5, "k within a read; at least five runs: the spreads decide the rule of choice"
    import torch
    assert api.device_count() > 0, "time_kprofile.py needs a GPU: nothing here is measured without one"
    L = api.lib()
    N, Q = a.reads, min(a.queries, a.reads)
    seed = synth.DEFAULT_SEED + 43
    gen = synth.genome_torch(seed, N, LEN, 30)
    reads = synth.reads_torch(seed, N, LEN, 30, err=a.err, gen=gen)
    d = api.build_index_inplace(reads.cpu().numpy())
    sets = {"a": reads[:Q].reshape(-1).clone(), "b": synth.reads_torch(seed + 1, Q, LEN, 30, err=0.0, gen=gen).reshape(-1), "c": gen.clone()}
    lens = {"a": [LEN] * Q, "b": [LEN] * Q, "c": [min(10000, len(gen) - s) for s in range(0, len(gen), 10000)]}
    del reads
    torch.cuda.empty_cache()
    sync = lambda: api.check(L.fmd_dev_sync(d.h, None))
    res = {"reads": N, "read_len": LEN, "err": a.err, "symbols": d.n, "repeats": a.repeats, "sets": {}}
    ar = torch.arange
    for name, flat in sets.items():
        n = len(lens[name])
        off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        off[1:] = torch.cumsum(torch.tensor(lens[name], dtype=torch.int64, device="cuda"), 0)
        seqs = torch.zeros(int(off[-1]) + 16, dtype=torch.uint8, device="cuda")
        seqs[:int(off[-1])] = flat
        res["sets"][name] = {"sequences": n, "bases": int(off[-1]), "k": {}}
        for k in a.k:
            nw = torch.clamp(off[1:] - off[:-1] - k + 1, min=0)
            woff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            woff[1:] = torch.cumsum(nw, 0)
            W = int(woff[-1])
            count = torch.zeros(W, dtype=torch.int32, device="cuda")
            stat = torch.zeros(5, dtype=torch.int64, device="cuda")
            r, ref = {"windows": W}, None
            for pname, flags in PATHS:
                def run():
                    stat.zero_()
                    api.check(L.fmd_kprofile_dev(d.h, None, n, seqs.data_ptr(), off.data_ptr(), woff.data_ptr(), k, flags, count.data_ptr(), stat.data_ptr()))
                st = repeat(run, sync, a.repeats)
                s = dict(zip(api.KPROFILE_STAT_DT.names, stat.cpu().tolist()))
                if ref is None:
                    ref = count.clone()
                assert torch.equal(count, ref) and s["n_windows"] == W, "the paths disagree"
                r[pname] = dict(st, stat=s, n_ext=s["n_ext"], windows_per_s=W / st["median_s"], windows_per_s_min=W / st["max_s"], windows_per_s_max=W / st["min_s"])
            # ---- the yardstick: every N-free window a read of its own, made here and not charged
            first = torch.repeat_interleave(off[:-1] - woff[:-1], nw) + ar(W, dtype=torch.int64, device="cuda")   # where window g begins
            step = 1 << 22
            good = torch.empty(W, dtype=torch.bool, device="cuda"); pal = torch.empty(W, dtype=torch.bool, device="cuda")
            for s0 in range(0, W, step):
                m = seqs[first[s0:s0 + step, None] + ar(k, device="cuda")[None, :]]
                good[s0:s0 + step] = ((m >= 1) & (m <= 4)).all(1)
                pal[s0:s0 + step] = (m == (5 - m).flip(1)).all(1)
            keep = torch.nonzero(good).reshape(-1)
            Wv = len(keep)
            y_seqs = torch.zeros(Wv * k + 16, dtype=torch.uint8, device="cuda")
            for s0 in range(0, Wv, step):
                y_seqs[s0 * k:min(s0 + step, Wv) * k] = seqs[first[keep[s0:s0 + step], None] + ar(k, device="cuda")[None, :]].reshape(-1)
            y_off = ar(Wv + 1, dtype=torch.int64, device="cuda") * k
            y_cnt = torch.zeros(Wv, dtype=torch.int64, device="cuda"); y_beg = torch.zeros_like(y_cnt); y_end = torch.zeros_like(y_cnt)
            yard = lambda: api.check(L.fmd_bsearch_dev(d.h, None, Wv, y_seqs.data_ptr(), y_off.data_ptr(), y_cnt.data_ptr(), y_beg.data_ptr(), y_end.data_ptr()))
            st = repeat(yard, sync, a.repeats)
            want = torch.where(pal[keep], y_cnt >> 1, y_cnt).clamp(max=2 ** 32 - 1)
            assert torch.equal(want, ref[keep].to(torch.int64) & 0xFFFFFFFF) and not bool(ref[~good].any()), "the yardstick and the profile disagree"
            r["bsearch_windows"] = dict(st, windows=Wv, bytes=Wv * k, windows_per_s=Wv / st["median_s"], windows_per_s_min=Wv / st["max_s"], windows_per_s_max=Wv / st["min_s"])
            res["sets"][name]["k"][str(k)] = r
            del first, good, pal, keep, y_seqs, y_off, y_cnt, y_beg, y_end, count
            torch.cuda.empty_cache()
    d_n = d.n
    d.close()
    os.makedirs(a.out, exist_ok=True)
    s = json.dumps(res, indent=1)
    with open(os.path.join(a.out, "time_kprofile_%d.json" % N), "w") as f:
        f.write(s + "\n")
    ms = lambda x: "%.2f ms (%.2f .. %.2f)" % (x["median_s"] * 1e3, x["min_s"] * 1e3, x["max_s"] * 1e3)
    spread = lambda x: x["max_s"] - x["min_s"]
    readme = os.path.join(a.out, "README.md")
    notes = ""
    if os.path.exists(readme):                         # what was written by hand under "## Notes" stays
        old = open(readme).read()
        notes = old[old.index("## Notes"):] if "## Notes" in old else ""
    lines = []
    lines.append("# profiles/kprofile -- kprofile on its paths against backward search of the materialised windows (`fmd_kprofile.hip`, `k_bsearch`)\n\n")
    lines.append("`python tools/time_kprofile.py --reads %d --err %g --queries %d -k %s --repeats %d` on an MI355X: %d reads of %d bp at 30x with %g substitutions per\n"
                 "base, indexed on the GPU (%.3g symbols).  Sets: a = %d of the indexed reads, b = %d error-free reads of the same genome, c = the genome in pieces of\n"
                 "10 kb.  %s = `fmd_kprofile_dev` with flags %s, on\n"
                 "buffers made beforehand; `bsearch_windows` = `fmd_bsearch_dev` over the N-free windows as separate reads (k times the bytes; made and uploaded outside\n"
                 "the clock).  Host clock around call + sync, the first call discarded, %d runs; min .. max is the run-to-run spread.  `time_kprofile_%d.json` holds every run.\n\n"
                 % (N, a.err, Q, " ".join(map(str, a.k)), a.repeats, N, LEN, a.err, float(d_n), Q, Q, " / ".join("`%s`" % p for p, _ in PATHS), " / ".join(str(f) for _, f in PATHS), a.repeats, N))
    lines.append("| set | k | leg | time (median, min .. max) | windows | windows / s (at max .. min time) | n_ext | n_ext / window |\n|---|---|---|---|---|---|---|---|\n")
    verdicts = []
    for name, sv in res["sets"].items():
        for k, r in sv["k"].items():
            for leg in [p for p, _ in PATHS] + ["bsearch_windows"]:
                x = r[leg]
                w = x.get("windows", r["windows"])
                lines.append("| %s | %s | %s | %s | %d | %.3g (%.3g .. %.3g) | %s | %s |\n" % (name, k, leg, ms(x), w, x["windows_per_s"], x["windows_per_s_min"], x["windows_per_s_max"],
                             x.get("n_ext", "-"), ("%.2f" % (x["n_ext"] / w)) if "n_ext" in x else "-"))
            p, y = r["plain"], r["bsearch_windows"]
            for g in [p_ for p_, _ in PATHS if p_ not in ("plain", "default")]:
                s_ = r[g]
                gain = p["median_s"] - s_["median_s"]
                verdicts.append("set %s, k = %s: %s takes %.2f x the time of plain (%s against %s); it is %s.\n"
                                % (name, k, g, s_["median_s"] / p["median_s"], ms(s_), ms(p),
                                   "faster by more than the sum of the two spreads (%.2f ms)" % ((spread(p) + spread(s_)) * 1e3) if gain > spread(p) + spread(s_) else
                                   "NOT faster by more than the sum of the two spreads (%.2f ms)" % ((spread(p) + spread(s_)) * 1e3)))
            dflt = r["default"]
            verdicts.append("set %s, k = %s: the default path takes %.2f x the time of the yardstick (%s against %s, the yardstick's own spread %.2f ms): it %s.\n"
                            % (name, k, dflt["median_s"] / y["median_s"], ms(dflt), ms(y), spread(y) * 1e3,
                               "beats it by more than the two spreads" if y["median_s"] - dflt["median_s"] > spread(y) + spread(dflt) else "does NOT beat it by more than the two spreads"))
    lines.append("\n" + "".join(verdicts) + "\n" + notes)
    with open(readme, "w") as f:
        f.write("".join(lines))
    print("".join(lines))


if __name__ == "__main__":
    main()
