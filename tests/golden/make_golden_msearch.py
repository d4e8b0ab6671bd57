#!/usr/bin/env python3
"""Fixture of the multi-index backward search (tests/test_msearch_golden.py, tests/test_gpu_msearch.py): queries over sets of golden .fmd
files, what the reference's fm_multi_backward_search (exact.c:25-57) returns over the parts, what its fm_backward_search (exact.c:7-23)
returns on each part and on the file `fermi merge` wrote of them (tests/golden/merge.*.fmd).  Made where the reference is compiled in place
(oracle/_ref/libfermi_ref.so), called through ctypes; only data is recorded.

Queries of a set, from a fixed seed: substrings of the parts' reads (read back with fm_retrieve), the same with one base changed to a random
symbol of 1..5, random strings of 1..10 symbols of 1..5.  A miss is recorded as cnt = beg = end = 0 (the reference leaves beg / end as they
were).  The script asserts what the CPU test asserts again from the file.
Usage: python tests/golden/make_golden_msearch.py   ->  tests/golden/msearch.npz"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFDIR = os.path.join(ROOT, "oracle", "_ref")
# set -> (parts, the merged file)
SETS = {
    "tiny_special": (["tiny", "special"], "merge.tiny_special"),
    "tiny_special_repeat": (["tiny", "special", "repeat"], "merge.tiny_special_repeat"),
    "special_palin": (["special", "palin"], "merge.special_palin"),
    "dup32_palin": (["dup32", "palin"], "merge.dup32_palin"),
    "tiny_tiny": (["tiny", "tiny"], "merge.tiny_tiny"),
    "tiny_empty_special": (["tiny", "sub.empty", "special"], "merge.tiny_special"),
}
N_EACH = 1400          # queries of each of the three kinds per set
SEED = 20261019


class KString(C.Structure):
    _fields_ = [("l", C.c_uint32), ("m", C.c_uint32), ("s", C.c_void_p)]     # kstring_t (kstring.h:39-42)


def ref_lib():
    lib = C.CDLL(os.path.join(REFDIR, "libfermi_ref.so"))
    lib.rld_restore.restype = C.c_void_p; lib.rld_restore.argtypes = [C.c_char_p]
    lib.fm_backward_search.restype = C.c_uint64
    lib.fm_backward_search.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.fm_multi_backward_search.restype = C.c_uint64
    lib.fm_multi_backward_search.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.fm_retrieve.restype = C.c_int64; lib.fm_retrieve.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(KString)]
    return lib


def single(lib, e, q):
    b, t = C.c_uint64(0), C.c_uint64(0)
    n = lib.fm_backward_search(e, len(q), q.ctypes.data, C.byref(b), C.byref(t))
    return (n, b.value, t.value) if n else (0, 0, 0)


def multi(lib, es, q):
    arr = (C.c_void_p * len(es))(*es)
    b, t = C.c_uint64(0), C.c_uint64(0)
    n = lib.fm_multi_backward_search(len(es), arr, len(q), q.ctypes.data, C.byref(b), C.byref(t))
    return (n, b.value, t.value) if n else (0, 0, 0)


def reads_of(lib, e):
    """every sequence of the index (both strands of every read), in read order"""
    n_seq = single(lib, e, np.zeros(1, np.uint8))[0]          # the rows below '$'
    out = []
    for x in range(n_seq):
        s = KString(0, 0, None)
        lib.fm_retrieve(e, x, C.byref(s))
        out.append(np.frombuffer(C.string_at(s.s, s.l), dtype=np.uint8)[::-1].copy())     # (fm_retrieve emits the sequence backwards)
    return out


def queries(rng, part_reads):
    qs, kind, src = [], [], []
    pool = [(p, r) for p, rs in enumerate(part_reads) for r in rs if len(r)]
    for k in (0, 1):
        for _ in range(N_EACH):
            p, r = pool[int(rng.integers(len(pool)))]
            ln = int(rng.integers(1, len(r) + 1))
            at = int(rng.integers(0, len(r) - ln + 1))
            q = r[at:at + ln].copy()
            if k == 1:
                q[int(rng.integers(ln))] = int(rng.integers(1, 6))
            qs.append(q); kind.append(k); src.append(p)
    for _ in range(N_EACH):
        qs.append(rng.integers(1, 6, size=int(rng.integers(1, 11))).astype(np.uint8)); kind.append(2); src.append(-1)
    order = rng.permutation(len(qs))                          # hits and misses interleaved
    return [qs[i] for i in order], np.array(kind, np.int8)[order], np.array(src, np.int8)[order]


def check_set(name, parts, d):
    """what tests/test_msearch_golden.py asserts from the file"""
    m = np.stack([d[name + ".multi_cnt"], d[name + ".multi_beg"], d[name + ".multi_end"]])
    s = np.stack([d[name + ".single_cnt"], d[name + ".single_beg"], d[name + ".single_end"]])
    assert np.array_equal(m, s), name
    if len(set(parts)) > 1:
        hit = d[name + ".part_cnt"] > 0
        partial, miss = hit.any(0) & ~hit.all(0), ~hit.any(0)
        assert partial.mean() >= 0.2 and miss.mean() >= 0.2, (name, partial.mean(), miss.mean())
        return partial.mean(), miss.mean()
    return None


def main():
    lib = ref_lib()
    idx, reads = {}, {}
    out = {"sets": np.frombuffer(json.dumps(SETS).encode(), dtype=np.uint8)}
    for si, (name, (parts, merged)) in enumerate(SETS.items()):
        for p in set(parts) | {merged}:
            if p not in idx:
                idx[p] = lib.rld_restore(os.path.join(HERE, p + ".fmd").encode())
                assert idx[p], p
        for p in parts:
            if p not in reads:
                reads[p] = reads_of(lib, idx[p])
        rng = np.random.default_rng(SEED + si)
        qs, kind, src = queries(rng, [reads[p] for p in parts])
        es = [idx[p] for p in parts]
        mres = np.array([multi(lib, es, q) for q in qs], dtype=np.uint64)
        sres = np.array([single(lib, idx[merged], q) for q in qs], dtype=np.uint64)
        pcnt = np.array([[single(lib, e, q)[0] for q in qs] for e in es], dtype=np.uint64)
        off = np.zeros(len(qs) + 1, np.uint64)
        np.cumsum([len(q) for q in qs], out=off[1:])
        out[name + ".seqs"] = np.concatenate(qs); out[name + ".off"] = off
        out[name + ".kind"] = kind; out[name + ".src"] = src; out[name + ".part_cnt"] = pcnt
        for j, f in enumerate(("cnt", "beg", "end")):
            out[name + ".multi_" + f] = mres[:, j].copy(); out[name + ".single_" + f] = sres[:, j].copy()
        print(name, len(qs), "queries; partial hits, misses:", check_set(name, parts, out))
    fn = os.path.join(HERE, "msearch.npz")
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    sys.exit(main())
