#!/usr/bin/env python3
"""Merged indexes written by the reference: `fermi merge` of golden .fmd files (tiny+special, special+palin and palin+special --
both walk directions of the GPU merge --, tiny+tiny, the RLE\\6 tiny.rle.fmd+special, dup32+palin, tiny+special+repeat) and
`fermi build -i tiny.fmd special.fq.gz` (which writes what `fermi merge tiny.fmd special.fmd` writes).  Made HERE with the reference
binary compiled in place; prints the md5 of every file for tests/test_gpu_merge.py.
Usage: python tests/golden/make_golden_merge.py"""
import hashlib, os, subprocess, sys
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "fermi")
MERGES = {
    "tiny_special": ["tiny", "special"], "special_palin": ["special", "palin"], "palin_special": ["palin", "special"],
    "tiny_tiny": ["tiny", "tiny"], "tinyrle_special": ["tiny.rle", "special"], "dup32_palin": ["dup32", "palin"],
    "tiny_special_repeat": ["tiny", "special", "repeat"],
}


def main():
    out = {}
    for name, parts in MERGES.items():
        fn = os.path.join(HERE, "merge.%s.fmd" % name)
        if os.path.exists(fn): os.remove(fn)
        subprocess.run([REF, "merge", "-o", fn] + [os.path.join(HERE, p + ".fmd") for p in parts], check=True, stderr=subprocess.DEVNULL)
        out[name] = hashlib.md5(open(fn, "rb").read()).hexdigest()
    b = subprocess.run([REF, "build", "-i", os.path.join(HERE, "tiny.fmd"), os.path.join(HERE, "special.fq.gz")], check=True, capture_output=True).stdout
    out["build_i_tiny_special"] = hashlib.md5(b).hexdigest()
    r = subprocess.run([REF, "recode", os.path.join(HERE, "tiny.rle.fmd")], check=True, capture_output=True).stdout
    out["recode_tiny_rle"] = hashlib.md5(r).hexdigest()
    for k, v in out.items(): print('    "%s": "%s",' % (k, v))


if __name__ == "__main__":
    sys.exit(main())
