#!/usr/bin/env python3
"""tiny_refec_fix.npz: the reference's own static ec_fix (oracle/ref_ec_harness.c:refec_fix, oracle/_ref/libref_ec.so from `make -C oracle ref`)
on the reads of tests/test_ref_ecfix.py::test_marking_rule_in_numpy_equals_the_reference, after the marking of correct.c:247-252: text, qual,
info.  That test compares the oracle's ec_fix + bench.mark_corrected with it where oracle/_ref was not built.
Usage: python tests/golden/make_ref_ecfix.py"""
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


assert t.bench.ref_ec_lib() is not None, "oracle/_ref/libref_ec.so is not built: make -C oracle ref"
nt6, q = t._marking_inputs(Gold)
(txt, q2, info), _, _, _, kind, _ = t.bench.cpu_ecfix(17, 2, 5, t._sorted_trip(Gold.npz("tiny_solid.npz")), nt6, q)
assert kind == "reference"
out = os.path.join(HERE, "tiny_refec_fix.npz")
np.savez_compressed(out, text=txt, qual=q2, info=info)
mp = os.path.join(HERE, "MANIFEST.json")
man = json.load(open(mp))
man["files"]["tiny_refec_fix.npz"] = {"md5": hashlib.md5(open(out, "rb").read()).hexdigest(), "bytes": os.path.getsize(out)}
json.dump(man, open(mp, "w"), indent=1, sort_keys=True)
print(out, txt.shape, os.path.getsize(out))
