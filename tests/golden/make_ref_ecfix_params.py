#!/usr/bin/env python3
"""tiny_refec_fix_params.npz: the reference's own static ec_fix (oracle/ref_ec_harness.c:refec_fix, oracle/_ref/libref_ec.so from
`make -C oracle ref`) at the k-mer lengths and steps that tiny_refec_fix.npz (w 17, step 5) does not hold, on every fourth read of
tests/test_ref_ecfix.py::_marking_inputs (600 reads, 100 of them reads the filter rejects), after the marking of correct.c:247-252:
text, qual and info per case of test_ref_ecfix.PARAM_CASES.  The tables of w 21 / 23 / 17 are tiny_solid.npz's; those of w 11 and
w 27 come from the reference's ec_collect on tiny.fmd (refec_collect, min_occ 3, suf_len = w - 15 for w > 15 and 1 otherwise) and
are stored here as well.  tests/test_ref_ecfix.py::test_oracle_ecfix_at_other_k_and_step compares the oracle with it.
Usage: python tests/golden/make_ref_ecfix_params.py"""
import ctypes as C
import gzip
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_ref_ecfix as t  # noqa: E402


class Gold:
    @staticmethod
    def text_gz(name):
        with gzip.open(os.path.join(HERE, name), "rb") as f:
            return f.read()

    @staticmethod
    def npz(name):
        return dict(np.load(os.path.join(HERE, name)))


Lec = t.bench.ref_ec_lib()
assert Lec is not None, "oracle/_ref/libref_ec.so is not built: make -C oracle ref"
Lec.refec_collect.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                              C.POINTER(C.c_uint64), C.c_void_p]
Lec.refec_free.argtypes = [C.c_void_p]
kv = {}
for w in (11, 27):
    b, k, v, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    cnt = (C.c_int64 * 2)()
    assert Lec.refec_collect(os.path.join(HERE, "tiny.fmd").encode(), w, 3, t.suf_len_of(w), C.byref(b), C.byref(k), C.byref(v), C.byref(n), cnt) == 0
    m = n.value
    B = np.frombuffer(C.string_at(b, m * 4), dtype=np.uint32); K = np.frombuffer(C.string_at(k, m * 4), dtype=np.uint32)
    V = np.frombuffer(C.string_at(v, m), dtype=np.uint8)
    for p in (b, k, v):
        Lec.refec_free(p)
    o = np.lexsort([V, K, B])
    kv["w%d_o3_bucket" % w], kv["w%d_o3_key" % w], kv["w%d_o3_val" % w] = B[o], K[o], V[o]
tabs = dict(Gold.npz("tiny_solid.npz"))
tabs.update(kv)
nt6, q = t._param_inputs(Gold)
for w, step in t.PARAM_CASES:
    (txt, q2, info), _, _, _, kind, _ = t.bench.cpu_ecfix(w, t.suf_len_of(w), step, t._trip_of(tabs, w), nt6, q)
    assert kind == "reference"
    tag = "w%d_s%d_" % (w, step)
    kv[tag + "text"], kv[tag + "qual"], kv[tag + "info"] = txt, q2, info
out = os.path.join(HERE, "tiny_refec_fix_params.npz")
np.savez_compressed(out, **kv)
mp = os.path.join(HERE, "MANIFEST.json")
man = json.load(open(mp))
man["files"]["tiny_refec_fix_params.npz"] = {"md5": hashlib.md5(open(out, "rb").read()).hexdigest(), "bytes": os.path.getsize(out)}
json.dump(man, open(mp, "w"), indent=1, sort_keys=True)
print(out, nt6.shape, os.path.getsize(out))
