#!/usr/bin/env python3
"""Time of the multi-index backward search (fmd_multi_bsearch_dev) against the single search it can be put beside.  One set of --reads 100 bp reads is
cut into --parts equal parts in read order, each part indexed on the GPU.  Three things are timed, every read searched whole:
  multi      fmd_multi_bsearch_dev of ALL reads over the P parts: reads x P index walks (a read is found in its own part; in the others it vanishes
             after a dozen bases and the walk goes on along the insertion point, one rank per base);
  yardstick  the sum of P fmd_bsearch_dev runs, part j over its OWN reads (full-length walks): reads x 1 index walks.  Per index walk -- the figure
             to compare -- multi / P stands against it (`*_ns_per_walk`);
  merged     the merge of the parts into one index (DevIndex.merge, left to right) and one fmd_bsearch_dev of all reads on it.
Everything is on the device before the clock starts; a timing is the host clock around enqueue + fmd_dev_sync.  One warm-up round, then --repeats rounds
that alternate the three; the median, and min / max as the run-to-run spread.  The results of multi and merged are compared (cnt, beg, end).
With --lines the rank blocks each part's handle was asked for by one multi search of --line-reads reads (libfmdhip_count.so), beside those of the yardstick.
Usage: python tools/time_msearch.py [--reads 4000000] [--parts 4] [--repeats 7] [--lines] [--out profiles/msearch]"""
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


def line_counts(L, handles):
    out = []
    for h in handles:
        buf, cnt = (C.c_uint64 * 3)(), C.c_int(0)
        api.check(L.fmd_dev_line_count3(h, buf, 1, C.byref(cnt)))
        assert cnt.value, "the counting build does not count"
        out.append([int(buf[0]), int(buf[1])])
    return out


def count_pass(parts, bounds, d_reads, d_off, outs, n_reads):
    """rank blocks (and table lines) per handle through the instrumented build: one multi search of the first n_reads reads, then part 0 alone over them"""
    Lc = api.count_lib()
    if Lc is None:
        return None
    hs = []
    for p in parts:                                   # the same BWTs under the counting library
        bwt = np.empty(p.n, np.uint8)
        api.check(api.lib().fmd_dev_export_bwt(p.h, 0, p.n, bwt.ctypes.data))
        h = C.c_void_p()
        api.check(Lc.fmd_dev_open_bwt(0, bwt.ctypes.data, len(bwt), C.byref(h)))
        hs.append(h)
        del bwt
    arr = (C.c_void_p * len(hs))(*[h.value for h in hs])
    wb = Lc.fmd_multi_bsearch_work_bytes(len(hs), n_reads)
    d_w = C.c_void_p()
    api.check(Lc.fmd_dev_malloc(0, wb, C.byref(d_w)))
    line_counts(Lc, hs)                               # reset
    api.check(Lc.fmd_multi_bsearch_dev(len(hs), arr, None, n_reads, d_reads, d_off, outs[0], outs[1], outs[2], d_w, wb))
    api.check(Lc.fmd_dev_sync(hs[0], None))
    res = {"reads": n_reads, "multi_lines_per_handle": line_counts(Lc, hs)}
    api.check(Lc.fmd_bsearch_dev(hs[0], None, n_reads, d_reads, d_off, outs[0], outs[1], outs[2]))
    api.check(Lc.fmd_dev_sync(hs[0], None))
    res["single_lines_part0_own_reads"] = line_counts(Lc, hs)[0]
    res["note"] = "[rank blocks, table lines]; the first %d reads are part 0's own: handle 0 walks them whole in both searches, the other handles follow insertion points" % n_reads
    Lc.fmd_dev_free(d_w)
    for h in hs:
        Lc.fmd_dev_close(h)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--parts", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--lines", action="store_true")
    ap.add_argument("--line-reads", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msearch"))
    a = ap.parse_args()
    assert 1 <= a.parts <= api.FMD_MULTI_MAX and a.reads >= a.parts
    import torch
    assert api.device_count() > 0, "time_msearch.py needs a GPU: nothing here is measured without one"
    L = api.lib()
    N, P = a.reads, a.parts
    gen = synth.genome_torch(synth.DEFAULT_SEED + 31, N, LEN, 30)
    reads = synth.reads_torch(synth.DEFAULT_SEED + 31, N, LEN, 30, gen=gen)           # uint8 [N, LEN] on the device
    del gen
    bounds = [N * j // P for j in range(P + 1)]
    parts = [api.build_index_inplace(reads[bounds[j]:bounds[j + 1]].cpu().numpy()) for j in range(P)]
    pad = torch.zeros(N * LEN + 64, dtype=torch.uint8, device="cuda")
    pad[:N * LEN] = reads.reshape(-1)
    del reads
    off = torch.arange(N + 1, dtype=torch.int64, device="cuda") * LEN
    out_m = [torch.zeros(N, dtype=torch.int64, device="cuda") for _ in range(3)]
    out_s = [torch.zeros(N, dtype=torch.int64, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    hs = (C.c_void_p * P)(*[p.h.value for p in parts])
    wb = L.fmd_multi_bsearch_work_bytes(P, N)
    work = torch.zeros(wb, dtype=torch.uint8, device="cuda")
    sync = lambda: api.check(L.fmd_dev_sync(parts[0].h, None))
    pm, ps = [t.data_ptr() for t in out_m], [t.data_ptr() for t in out_s]

    def multi():
        api.check(L.fmd_multi_bsearch_dev(P, hs, None, N, pad.data_ptr(), off.data_ptr(), pm[0], pm[1], pm[2], work.data_ptr(), wb))

    def yardstick():
        for j in range(P):                              # part j over its own reads: the offsets are absolute, the arrays start at read bounds[j]
            b, m = bounds[j], bounds[j + 1] - bounds[j]
            api.check(L.fmd_bsearch_dev(parts[j].h, None, m, pad.data_ptr(), off.data_ptr() + 8 * b, ps[0] + 8 * b, ps[1] + 8 * b, ps[2] + 8 * b))

    t0 = time.perf_counter()
    merged = parts[0]
    for j in range(1, P):
        nxt = merged.merge(parts[j])
        if merged is not parts[0]:
            merged.close()
        merged = nxt
    sync()
    merge_s = time.perf_counter() - t0

    def single_merged():
        api.check(L.fmd_bsearch_dev(merged.h, None, N, pad.data_ptr(), off.data_ptr(), ps[0], ps[1], ps[2]))

    yardstick(); sync()
    own_found = int((out_s[0] > 0).sum().item())
    legs = {"multi": multi, "yardstick": yardstick, "merged": single_merged}
    for f in legs.values():                             # warm-up: every shape the timed rounds use
        f(); sync()
    times = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, f in legs.items():
            times[k].append(timed(f, sync))
    multi(); single_merged(); sync()
    same = all(bool(torch.equal(x, y)) for x, y in zip(out_m, out_s))
    res = {"reads": N, "read_len": LEN, "parts": P, "symbols_per_part": [p.n for p in parts], "repeats": a.repeats,
           "multi": stats(times["multi"]), "yardstick": stats(times["yardstick"]), "merged_search": stats(times["merged"]), "merge_s": merge_s,
           "index_walks": {"multi": N * P, "yardstick": N, "merged": N},
           "multi_equals_merged_search": same, "own_reads_found_by_yardstick": own_found}
    res["multi_ns_per_walk"] = 1e9 * res["multi"]["median_s"] / (N * P)
    res["yardstick_ns_per_walk"] = 1e9 * res["yardstick"]["median_s"] / N
    res["yardstick_spread_s"] = res["yardstick"]["max_s"] - res["yardstick"]["min_s"]
    res["merged_total_s"] = merge_s + res["merged_search"]["median_s"]
    if a.lines:
        res["lines"] = count_pass(parts, bounds, pad.data_ptr(), off.data_ptr(), pm, min(a.line_reads, bounds[1]))
    if merged is not parts[0]:
        merged.close()
    for p in parts:
        p.close()
    assert same, "the multi search and the search on the merged index disagree"
    os.makedirs(a.out, exist_ok=True)
    s = json.dumps(res, indent=1)
    print(s)
    with open(os.path.join(a.out, "time_msearch_%d_x%d.json" % (N, P)), "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
