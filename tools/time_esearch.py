#!/usr/bin/env python3
"""Time of esearch (fmd_asearch_bound_dev + fmd_esearch_dev).  There is no substitute to beat -- the edit neighbours of a query cannot be enumerated the way
the Hamming neighbours were for asearch --, so nothing here is a threshold: the figures are the time, the backward extensions and the widest level, with asearch
at the SAME budget on the same queries, the same handle and the same run as context (it answers a smaller question: substitutions only).
--reads 100 bp reads at 30x with 1 % substitutions are indexed on the GPU, once; the queries are pieces of --len bases (default 25, 40, 100) of OTHER reads of the
same genome, with errors of their own; --max-edit budgets (default 1, 2), --queries queries at budget 1 and a twentieth of them at budget 2 and above (the widest level of
a 25-mer at two edits takes 1.7 x 10^3 slots per query: more queries than that do not fit FMD_ESEARCH_MAX_CAP in one call).  Legs per
(length, budget):
  esearch             the bound, level 0 and len + budget - 1 levels, hits listed (max_hits = --max-hits)
  esearch_pair_pruned / esearch_no_prune   the pruned / unpruned pair, with the bound and without, on the first --pair-queries queries (unpruned, every node within
                      the budget of ANY string is walked for a dozen levels: the frontier of all the queries at once does not fit)
  esearch_count_only  with the bound, no hit listed
  asearch             fmd_asearch_bound_dev + fmd_asearch_dev at max_sub = budget, hits listed
Everything is on the device before the clock starts; a timing is the host clock around enqueue + fmd_dev_sync.  One warm-up round, then --repeats rounds that
alternate the legs; the median of each, and min / max as the run-to-run spread.  Checked: the esearch legs give the same strata; per query and budget
esearch finds at least the hits of asearch.
Usage: python tools/time_esearch.py [--reads 1000000] [--queries 1000000] [--len 25,40,100] [--max-edit 1,2] [--repeats 7] [--out profiles/esearch]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fermi_amd import api, synth

LEN = 100
STAT = ("n_hits", "n_occ", "n_skipped", "n_truncated", "n_unfinished", "overflow", "n_ext", "widest_level")


def timed(fn, sync):
    t = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t


def stats(v):
    runs, v = list(v), sorted(v)
    return {"median_s": v[len(v) // 2], "min_s": v[0], "max_s": v[-1], "runs_s": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--len", default="25,40,100")
    ap.add_argument("--max-edit", default="1,2")
    ap.add_argument("--max-hits", type=int, default=1000)
    ap.add_argument("--pair-queries", type=int, default=20_000)
    ap.add_argument("--cap", type=int, default=1 << 27)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esearch"))
    a = ap.parse_args()
    lens, budgets = [int(x) for x in a.len.split(",")], [int(x) for x in a.max_edit.split(",")]
    assert all(1 <= k <= LEN for k in lens) and all(0 <= e <= api.ESEARCH_MAX_EDIT for e in budgets) and a.repeats >= 5, "at least five runs: the spread is part of the result"
    import torch
    assert api.device_count() > 0, "time_esearch.py needs a GPU: nothing here is measured without one"
    L = api.lib()
    N = a.reads
    gen = synth.genome_torch(synth.DEFAULT_SEED + 51, N, LEN, 30)
    reads = synth.reads_torch(synth.DEFAULT_SEED + 51, N, LEN, 30, err=0.01, gen=gen)
    d = api.build_index_inplace(reads.cpu().numpy())
    del reads
    sync = lambda: api.check(L.fmd_dev_sync(d.h, None))
    other = synth.reads_torch(synth.DEFAULT_SEED + 52, a.queries, LEN, 30, err=0.01, gen=gen)   # another sample of the same genome
    del gen
    work = torch.zeros(max(L.fmd_esearch_work_bytes(a.queries, a.cap), L.fmd_asearch_work_bytes(a.queries, a.cap)), dtype=torch.uint8, device="cuda")
    assert work.numel() > 0, "--cap is outside FMD_ESEARCH_MIN_CAP .. FMD_ESEARCH_MAX_CAP"
    hits = torch.zeros(a.queries * 64 * 4, dtype=torch.int64, device="cuda")       # the legs run one after the other: one work area, one hit array
    os.makedirs(a.out, exist_ok=True)
    ok = True
    for K in lens:
        g = torch.Generator(device="cpu"); g.manual_seed(7)
        at = torch.randint(0, LEN - K + 1, (a.queries,), generator=g).to("cuda")
        qs_all = torch.gather(other, 1, at[:, None] + torch.arange(K, device="cuda")[None, :]).contiguous()
        for D in budgets:
            Q = a.queries if D <= 1 else max(1, a.queries // 20)
            flat = torch.zeros(Q * K + 64, dtype=torch.uint8, device="cuda"); flat[:Q * K] = qs_all[:Q].reshape(-1)
            off = torch.arange(Q + 1, dtype=torch.int64, device="cuda") * K
            lb = torch.zeros(Q * K + 64, dtype=torch.uint8, device="cuda")
            hit_cap = Q * 64

            P = min(Q, a.pair_queries)

            def leg(entry, n, levels, prune, listed):
                work_bytes = (L.fmd_esearch_work_bytes if entry is L.fmd_esearch_dev else L.fmd_asearch_work_bytes)(n, a.cap)
                strata = torch.zeros(n * (D + 1) * 2, dtype=torch.int64, device="cuda")
                stat = torch.zeros(8, dtype=torch.int64, device="cuda")

                def run():
                    if prune:
                        api.check(L.fmd_asearch_bound_dev(d.h, None, n, flat.data_ptr(), off.data_ptr(), lb.data_ptr()))
                    api.check(entry(d.h, None, n, flat.data_ptr(), off.data_ptr(), lb.data_ptr() if prune else None, D, a.max_hits, levels,
                                    hits.data_ptr() if listed else None, hit_cap if listed else 0, strata.data_ptr(), stat.data_ptr(), work.data_ptr(), work_bytes))
                return run, strata, stat

            legs, keep = {}, {}
            for name, entry, n, levels, prune, listed in (("esearch", L.fmd_esearch_dev, Q, K + D - 1, True, True),
                                                          ("esearch_count_only", L.fmd_esearch_dev, Q, K + D - 1, True, False),
                                                          ("esearch_pair_pruned", L.fmd_esearch_dev, P, K + D - 1, True, True),
                                                          ("esearch_no_prune", L.fmd_esearch_dev, P, K + D - 1, False, True),
                                                          ("asearch", L.fmd_asearch_dev, Q, K - 1, True, True)):
                legs[name], *keep[name] = leg(entry, n, levels, prune, listed)
            torch.cuda.synchronize()
            for f in legs.values():
                f(); sync()
            times = {k: [] for k in legs}
            for _ in range(a.repeats):
                for k, f in legs.items():
                    times[k].append(timed(f, sync))
            st = {k: dict(zip(STAT, keep[k][1].cpu().tolist())) for k in keep}
            e, s = keep["esearch"][0].view(Q, D + 1, 2), keep["asearch"][0].view(Q, D + 1, 2)
            same = bool(torch.equal(keep["esearch_no_prune"][0], keep["esearch_pair_pruned"][0])) and bool(torch.equal(keep["esearch_count_only"][0], keep["esearch"][0]))
            same = same and bool(torch.equal(keep["esearch_pair_pruned"][0], keep["esearch"][0][:P * (D + 1) * 2]))
            covers = bool((e[:, :, 0].cumsum(1) >= s[:, :, 0].cumsum(1)).all())     # a pattern within j substitutions is within j edits
            clean = all(v["overflow"] == 0 and v["n_unfinished"] == 0 for v in st.values())
            res = {"reads": N, "read_len": LEN, "err": 0.01, "symbols": d.n, "queries": Q, "pair_queries": P, "query_len": K, "max_edit": D, "max_hits": a.max_hits, "cap": a.cap,
                   "repeats": a.repeats, "esearch_legs_agree": same, "esearch_covers_asearch": covers, "no_overflow": clean, "stat": st}
            for k in legs:
                res[k] = stats(times[k])
                res[k]["extensions"] = st[k]["n_ext"]
                res[k]["extensions_per_s"] = st[k]["n_ext"] / res[k]["median_s"]
                res[k]["widest_level"] = st[k]["widest_level"]
            res["esearch_over_asearch"] = res["esearch"]["median_s"] / res["asearch"]["median_s"]
            res["no_prune_over_pruned"] = res["esearch_no_prune"]["median_s"] / res["esearch_pair_pruned"]["median_s"]
            text = json.dumps(res, indent=1)
            print(text, flush=True)
            with open(os.path.join(a.out, "time_esearch_%d_q%d_len%d_e%d.json" % (N, Q, K, D)), "w") as f:
                f.write(text + "\n")
            ok = ok and same and covers and clean
            del flat, off, lb, legs, keep
    d.close()
    assert ok, "the esearch legs disagree, asearch found more, or a leg overflowed: see the files"


if __name__ == "__main__":
    main()
