#!/usr/bin/env python3
"""tools/ab_overlap.py's A/B on reads of ragged lengths: every read of the synthetic 30-fold set cut to lo .. hi bases (uniform), one index, and for every
setting given as ENV=VAL[,ENV=VAL...] the HIP-event time of `steps` passes of the sorted overlap job over all strands and whether records, neighbours
and sequences are the first setting's.  In phase (k_ovl_walk<WALK_TAIL2>) a generation lasts as long as its longest strand: this is what that costs.
Usage: python tools/ab_overlap_ragged.py [n_reads=10000000] [lo=70] [hi=100] [steps=3] -- SETTING [SETTING...]     ('-' = defaults)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from fermi_amd import api, synth, workload
import bench

args = sys.argv[1:]
cut = args.index("--") if "--" in args else len(args)
pos, settings = args[:cut], args[cut + 1:] or ["-"]
n_reads = int(pos[0]) if len(pos) > 0 else 10_000_000
lo = int(pos[1]) if len(pos) > 1 else 70
hi = int(pos[2]) if len(pos) > 2 else 100
steps = int(pos[3]) if len(pos) > 3 else 3
L = hi
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
full = synth.reads_torch(synth.DEFAULT_SEED, n_reads, L, 30, 0.0, dev)
ln = lo + torch.from_numpy((synth.rnd(synth.DEFAULT_SEED, 7, torch.arange(n_reads).numpy()) % (hi - lo + 1)).astype("int64")).to(dev)
rd = workload.ReadsOnDevice.__new__(workload.ReadsOnDevice)
rd.n, rd.L, rd.total = n_reads, L, int(ln.sum().item())
rd.flat = torch.zeros(rd.total + 64, dtype=torch.uint8, device=dev)
rd.flat[: rd.total] = full[torch.arange(L, device=dev)[None, :] < ln[:, None]]      # the first ln bases of every read, in read order
rd.off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(ln, 0)])
del full
import ctypes as C
d_bwt, n_sym = C.c_void_p(), C.c_uint64()
api.check(api.lib().fmd_build_bwt_dev(0, None, rd.n, rd.flat.data_ptr(), rd.off.data_ptr(), rd.total, rd.L, 0, C.byref(d_bwt), C.byref(n_sym)))   # (0: lengths differ)
n_sym = n_sym.value
del rd
index = api.DevIndex.from_bwt_dev(d_bwt, n_sym, 0)
api.lib().fmd_dev_free(d_bwt)
torch.cuda.empty_cache()
print("index: %d reads of %d .. %d bases, %d symbols" % (n_reads, lo, hi, n_sym), flush=True)
job = bench.OverlapJob(torch, api, index, dev, 2 * n_reads, 0, 1, L, 50)


def wsum(t):
    """position-weighted wrap-around sum of a byte tensor (multiple of 8 bytes) on the device"""
    v = t.reshape(-1).view(torch.int64)
    return int((v * (torch.arange(v.numel(), device=dev, dtype=torch.int64) % 1000003 + 1)).sum().item())


def digest():
    """tools/ab_overlap.py's: all records, the neighbours up to n_nei, the rows up to len + ext_len"""
    g = job.rec.view(torch.int32).view(job.n, 16)   # fmd_ovlp_rec_t: len = word 8, ext_len = 12, n_nei = 13
    n_nei = g[:, 13].clamp(0, job.max_nei)
    nei = job.nei.view(torch.int64).view(job.n, job.max_nei, 4)
    a, b = wsum(job.rec), 0
    for o in range(0, job.n, 1 << 22):   # in pieces: the masks are as large as the arrays
        e = min(job.n, o + (1 << 22))
        keep = torch.arange(job.max_nei, device=dev)[None, :] < n_nei[o:e, None]
        b += wsum((nei[o:e] * keep[:, :, None]).contiguous().view(torch.uint8))
        used = (g[o:e, 8] + g[o:e, 12].clamp(min=0)).clamp(0, job.stride)
        seq = job.seq.view(job.n, job.stride)[o:e]
        b += wsum((seq * (torch.arange(job.stride, device=dev)[None, :] < used[:, None])).contiguous())
    return "%016x.%016x" % (a & (2**64 - 1), b & (2**64 - 1))


first = None
for s in settings:
    saved = {}
    if s != "-":
        for kv in s.split(","):
            k, v = kv.split("=", 1)
            saved[k] = os.environ.get(k)
            os.environ[k] = v
    job.rec.zero_(); job.nei.zero_(); job.seq.zero_()
    job.compute()
    torch.cuda.synchronize()
    dg = digest()
    first = first or dg
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(job.stream)
    for _ in range(steps):
        job.compute()
    e1.record(job.stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    print("%-40s %8.1f ms per pass = %.3e strands/s   %s" % (s, ms, job.n / ms * 1e3, ("same bytes" if dg == first else "DIFFERENT") + "  digest " + dg), flush=True)
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
index.close()
