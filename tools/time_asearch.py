#!/usr/bin/env python3
"""Time of asearch (fmd_asearch_bound_dev + fmd_asearch_dev) against the only substitute there was: the Hamming neighbours of every query enumerated and sent
through the exact search (fmd_bsearch_dev); at max_sub = 0 the exact search of the queries themselves.  --reads 100 bp reads at 30x with 1 % substitutions are
indexed on the GPU; the queries are --queries pieces of --len bases (25, 40, 100) of OTHER reads of the same genome, with errors of their own.
  asearch    the bound, level 0 and len - 1 levels, hits listed (max_hits = --max-hits), with pruning and without; count-only as well;
  yardstick  the queries with at most max_sub bases changed -- 1 + 3 L at one substitution, 1 + 3 L + 9 L (L - 1) / 2 at two -- built ON THE DEVICE before the
             clock starts (the enumeration itself, which a caller would do on the host, is not charged) and searched in one fmd_bsearch_dev call.  The
             neighbours of 10^6 queries at max_sub = 2 are 2.8 x 10^9 strings for 25-mers and 4.5 x 10^10 (4.5 TB) for 100-base reads: the yardstick takes the first queries whose
             neighbours stay below --yardstick-strings, and asearch is timed on THOSE queries too -- the comparison is between the two on the same queries,
             the same handle and the same run; asearch on all the queries is reported beside it.
Everything is on the device before the clock starts; a timing is the host clock around enqueue + fmd_dev_sync.  One warm-up round, then --repeats rounds that
alternate the legs; the median of each, and min / max as the run-to-run spread.  The two answers are compared: per query the number of neighbours found and the
sum of their counts against the strata.  Reported: ms, backward extensions (asearch: n_ext; yardstick: the bases of the strings it was given, an upper bound --
a search stops at its first miss) and extensions per second.
Usage: python tools/time_asearch.py [--reads 1000000] [--queries 1000000] [--len 25] [--max-sub 1] [--repeats 7] [--out profiles/asearch]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
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


def neighbours(torch, q, d):
    """[M, L] queries -> [M * K, L]: every query, then each with one base changed, then (d = 2) each with two"""
    M, L = q.shape
    out = [q[:, None, :]]
    if d >= 1:
        one = q[:, None, None, :].repeat(1, L, 3, 1)                               # [M, pos, alt, L]
        p = torch.arange(L, device=q.device)
        alt = 1 + (q[:, :, None].long() - 1 + 1 + torch.arange(3, device=q.device)[None, None, :]) % 4   # the three other bases
        one[:, p, :, p] = alt.permute(1, 0, 2).to(torch.uint8)
        out.append(one.reshape(M, 3 * L, L))
    if d >= 2:
        i, j = torch.triu_indices(L, L, 1, device=q.device)
        P = i.numel()
        two = q[:, None, None, :].repeat(1, P, 9, 1)                               # [M, pair, alt x alt, L]
        a = torch.arange(9, device=q.device)
        ai = 1 + (q[:, i, None].long() - 1 + 1 + (a // 3)[None, None, :]) % 4
        aj = 1 + (q[:, j, None].long() - 1 + 1 + (a % 3)[None, None, :]) % 4
        k = torch.arange(P, device=q.device)
        two[:, k, :, i] = ai.permute(1, 0, 2).to(torch.uint8)
        two[:, k, :, j] = aj.permute(1, 0, 2).to(torch.uint8)
        out.append(two.reshape(M, 9 * P, L))
    return torch.cat(out, dim=1).reshape(-1, L).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=25)
    ap.add_argument("--max-sub", type=int, default=1)
    ap.add_argument("--max-hits", type=int, default=1000)
    ap.add_argument("--yardstick-strings", type=int, default=100_000_000)
    ap.add_argument("--cap", type=int, default=1 << 24)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asearch"))
    a = ap.parse_args()
    assert 1 <= a.len <= LEN and 0 <= a.max_sub <= 2 and a.repeats >= 5, "at least five runs: the spread of the yardstick is part of the result"
    import torch
    assert api.device_count() > 0, "time_asearch.py needs a GPU: nothing here is measured without one"
    L = api.lib()
    N, Q, K, D = a.reads, a.queries, a.len, a.max_sub
    gen = synth.genome_torch(synth.DEFAULT_SEED + 51, N, LEN, 30)
    reads = synth.reads_torch(synth.DEFAULT_SEED + 51, N, LEN, 30, err=0.01, gen=gen)
    d = api.build_index_inplace(reads.cpu().numpy())
    del reads
    sync = lambda: api.check(L.fmd_dev_sync(d.h, None))
    other = synth.reads_torch(synth.DEFAULT_SEED + 52, Q, LEN, 30, err=0.01, gen=gen)   # another sample of the same genome
    g = torch.Generator(device="cpu"); g.manual_seed(7)
    at = torch.randint(0, LEN - K + 1, (Q,), generator=g).to("cuda")
    qs = torch.gather(other, 1, at[:, None] + torch.arange(K, device="cuda")[None, :]).contiguous()
    del other, gen
    per = 1 + (3 * K if D >= 1 else 0) + (9 * K * (K - 1) // 2 if D >= 2 else 0)      # neighbours of one query
    M = max(1, min(Q, a.yardstick_strings // per))                                   # the queries both sides are compared on

    def batch(q):
        n = q.shape[0]
        flat = torch.zeros(n * K + 64, dtype=torch.uint8, device="cuda"); flat[:n * K] = q.reshape(-1)
        return n, flat, torch.arange(n + 1, dtype=torch.int64, device="cuda") * K

    work = torch.zeros(L.fmd_asearch_work_bytes(Q, a.cap), dtype=torch.uint8, device="cuda")   # the legs run one after the other: one work area, one hit array
    hits = torch.zeros(Q * 64 * 4, dtype=torch.int64, device="cuda")
    assert work.numel() > 0, "--cap is outside FMD_ASEARCH_MIN_CAP .. FMD_ASEARCH_MAX_CAP"

    def asearch_leg(q, prune, listed):
        n, flat, off = batch(q)
        lb = torch.zeros(n * K + 64, dtype=torch.uint8, device="cuda")
        wb = L.fmd_asearch_work_bytes(n, a.cap)
        hit_cap = n * 64 if listed else 0
        strata = torch.zeros(n * (D + 1) * 2, dtype=torch.int64, device="cuda")
        stat = torch.zeros(8, dtype=torch.int64, device="cuda")

        def run():
            if prune:
                api.check(L.fmd_asearch_bound_dev(d.h, None, n, flat.data_ptr(), off.data_ptr(), lb.data_ptr()))
            api.check(L.fmd_asearch_dev(d.h, None, n, flat.data_ptr(), off.data_ptr(), lb.data_ptr() if prune else None, D, a.max_hits, K - 1,
                                        hits.data_ptr() if listed else None, hit_cap, strata.data_ptr(), stat.data_ptr(), work.data_ptr(), wb))
        return run, strata, stat, (flat, off, lb)

    legs, keep = {}, {}
    for name, q, prune, listed in (("asearch", qs[:M], True, True), ("asearch_no_prune", qs[:M], False, True), ("asearch_count_only", qs[:M], True, False),
                                   ("asearch_all_queries", qs, True, True)):
        legs[name], *keep[name] = asearch_leg(q, prune, listed)
    nb = neighbours(torch, qs[:M], D)
    n_nb, nb_flat, nb_off = batch(nb)
    del nb
    cnt, beg, end = (torch.zeros(n_nb, dtype=torch.int64, device="cuda") for _ in range(3))
    legs["yardstick"] = lambda: api.check(L.fmd_bsearch_dev(d.h, None, n_nb, nb_flat.data_ptr(), nb_off.data_ptr(), cnt.data_ptr(), beg.data_ptr(), end.data_ptr()))
    torch.cuda.synchronize()
    for f in legs.values():
        f(); sync()
    times = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, f in legs.items():
            times[k].append(timed(f, sync))
    st = {k: dict(zip(STAT, keep[k][1].cpu().tolist())) for k in keep}
    # the two answers, per query: patterns found and the sum of their counts (distinct neighbours are distinct patterns)
    c = cnt.view(M, per)
    strata = keep["asearch"][0].view(M, D + 1, 2)
    same = bool(torch.equal((c > 0).sum(1), strata[:, :, 0].sum(1))) and bool(torch.equal(c.sum(1), strata[:, :, 1].sum(1)))
    same = same and bool(torch.equal(keep["asearch_no_prune"][0], keep["asearch"][0])) and bool(torch.equal(keep["asearch_count_only"][0], keep["asearch"][0]))
    res = {"reads": N, "read_len": LEN, "err": 0.01, "symbols": d.n, "queries": Q, "query_len": K, "max_sub": D, "max_hits": a.max_hits, "cap": a.cap,
           "compared_queries": M, "neighbours_per_query": per, "yardstick_strings": n_nb, "repeats": a.repeats,
           "asearch_equals_yardstick": same, "stat": st}
    for k in legs:
        res[k] = stats(times[k])
        ext = st[k]["n_ext"] if k in st else n_nb * K
        res[k]["extensions"] = ext
        res[k]["extensions_per_s"] = ext / res[k]["median_s"]
    res["yardstick"]["extensions_are_an_upper_bound"] = True
    res["yardstick_spread_s"] = res["yardstick"]["max_s"] - res["yardstick"]["min_s"]
    res["yardstick_over_asearch"] = res["yardstick"]["median_s"] / res["asearch"]["median_s"]
    res["asearch_beats_yardstick_by_more_than_its_spread"] = bool(res["yardstick"]["min_s"] - res["asearch"]["max_s"] > res["yardstick_spread_s"])
    d.close()
    os.makedirs(a.out, exist_ok=True)
    s = json.dumps(res, indent=1)
    print(s)
    with open(os.path.join(a.out, "time_asearch_%d_q%d_len%d_d%d.json" % (N, Q, K, D)), "w") as f:
        f.write(s + "\n")
    assert same and all(v["overflow"] == 0 and v["n_unfinished"] == 0 for v in st.values()), "asearch and the enumerated neighbours disagree, or a leg overflowed"


if __name__ == "__main__":
    main()
