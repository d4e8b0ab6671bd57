#!/usr/bin/env python3
"""Time of locate (fmd_locate_dev) against the row-by-row walk it replaces.  --reads 100 bp reads at 30x are indexed on the GPU; one --k-mer is drawn from
every read and searched (fmd_bsearch_dev); its SA interval is what both sides get:
  locate     fmd_locate_dev over the N intervals, 100 - k + 1 levels (every row of a k-mer has ended by then): the rows of an interval walk together;
  yardstick  fmd_retrieve_dev over the same rows expanded one by one, stride 1 (it writes one base, the length and the rank per row): one LF-walk per row.
             It is the yardstick only -- no public substitute for locate: it has no notion of a query, a limit or a run.
Everything is on the device before the clock starts; a timing is the host clock around enqueue + fmd_dev_sync.  One warm-up round, then --repeats rounds that
alternate the two; the median of each, and min / max as the run-to-run spread.  The two answers are compared as multisets of (rank, offset).  Also reported:
the backward extensions locate did (n_ext) and the rank requests of the yardstick (one per base + one for the sentinel, per row).
Usage: python tools/time_locate.py [--reads 1000000] [--k 25] [--repeats 7] [--out profiles/locate]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fermi_amd import api, synth

LEN = 100


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
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate"))
    a = ap.parse_args()
    assert 1 <= a.k <= LEN and a.repeats >= 5, "at least five runs: the spread of the yardstick is part of the result"
    import torch
    assert api.device_count() > 0, "time_locate.py needs a GPU: nothing here is measured without one"
    L = api.lib()
    N, K = a.reads, a.k
    reads = synth.reads_torch(synth.DEFAULT_SEED + 41, N, LEN, 30)                   # uint8 [N, LEN] on the device
    d = api.build_index_inplace(reads.cpu().numpy())
    sync = lambda: api.check(L.fmd_dev_sync(d.h, None))
    g = torch.Generator(device="cpu"); g.manual_seed(7)
    at = torch.randint(0, LEN - K + 1, (N,), generator=g).to("cuda")
    kmers = torch.gather(reads, 1, at[:, None] + torch.arange(K, device="cuda")[None, :]).contiguous()
    del reads
    flat = torch.zeros(N * K + 64, dtype=torch.uint8, device="cuda"); flat[:N * K] = kmers.reshape(-1)
    off = torch.arange(N + 1, dtype=torch.int64, device="cuda") * K
    cnt, beg, end = (torch.zeros(N, dtype=torch.int64, device="cuda") for _ in range(3))
    api.check(L.fmd_bsearch_dev(d.h, None, N, flat.data_ptr(), off.data_ptr(), cnt.data_ptr(), beg.data_ptr(), end.data_ptr()))
    sync()
    assert int((cnt > 0).sum()) == N, "a k-mer of a read was not found"
    total = int(cnt.sum())
    first = torch.cumsum(cnt, 0) - cnt
    rows = (torch.repeat_interleave(beg - first, cnt) + torch.arange(total, dtype=torch.int64, device="cuda")).contiguous()
    levels = LEN - K + 1
    wb = L.fmd_locate_work_bytes(N, total)
    work = torch.zeros(wb, dtype=torch.uint8, device="cuda")
    runs = torch.zeros(total * 3, dtype=torch.int64, device="cuda")                  # fmd_locate_run_t: 24 bytes
    stat = torch.zeros(6, dtype=torch.int64, device="cuda")
    r_seq = torch.zeros(total, dtype=torch.uint8, device="cuda")
    r_len = torch.zeros(total, dtype=torch.int32, device="cuda")
    r_rank = torch.zeros(total, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def locate():
        api.check(L.fmd_locate_dev(d.h, None, N, beg.data_ptr(), cnt.data_ptr(), 0xffffffff, levels, runs.data_ptr(), total, stat.data_ptr(), work.data_ptr(), wb))

    def yardstick():
        api.check(L.fmd_retrieve_dev(d.h, None, total, rows.data_ptr(), r_seq.data_ptr(), 1, r_len.data_ptr(), r_rank.data_ptr()))

    legs = {"locate": locate, "yardstick": yardstick}
    for f in legs.values():
        f(); sync()
    times = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, f in legs.items():
            times[k].append(timed(f, sync))
    st = dict(zip(("n_runs", "n_rows", "n_skipped", "n_unfinished", "overflow", "n_ext"), stat.cpu().tolist()))
    # the two answers: (rank, offset) of every row
    rr = runs.view(-1, 3)[:st["n_runs"]]
    r_n, r_off = rr[:, 1] & 0xffffffff, (rr[:, 1] >> 32) & 0xffffffff
    start = torch.cumsum(r_n, 0) - r_n
    e_rank = torch.repeat_interleave(rr[:, 0] - start, r_n) + torch.arange(int(r_n.sum()), dtype=torch.int64, device="cuda")
    mine = torch.sort(e_rank * 256 + torch.repeat_interleave(r_off, r_n)).values
    theirs = torch.sort(r_rank * 256 + r_len.to(torch.int64)).values
    same = mine.shape == theirs.shape and bool(torch.equal(mine, theirs))
    res = {"reads": N, "read_len": LEN, "k": K, "symbols": d.n, "intervals": N, "rows": total, "rows_per_interval": total / N, "levels": levels, "repeats": a.repeats,
           "locate": stats(times["locate"]), "yardstick": stats(times["yardstick"]), "locate_stat": st,
           "locate_extensions": st["n_ext"], "yardstick_rank_requests": int(r_len.to(torch.int64).sum()) + total,
           "locate_equals_yardstick": same}
    res["yardstick_spread_s"] = res["yardstick"]["max_s"] - res["yardstick"]["min_s"]
    res["yardstick_over_locate"] = res["yardstick"]["median_s"] / res["locate"]["median_s"]
    res["locate_beats_yardstick_by_more_than_its_spread"] = bool(res["yardstick"]["min_s"] - res["locate"]["max_s"] > res["yardstick_spread_s"])
    d.close()
    assert same and st["overflow"] == 0 and st["n_unfinished"] == 0 and st["n_rows"] == total, "locate and the row-by-row walk disagree"
    os.makedirs(a.out, exist_ok=True)
    s = json.dumps(res, indent=1)
    print(s)
    with open(os.path.join(a.out, "time_locate_%d_k%d.json" % (N, K)), "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
