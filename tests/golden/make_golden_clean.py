#!/usr/bin/env python3
"""Fixtures of `fermi clean` and `fermi example -c`, made where the reference is compiled in place (oracle/_ref/fermi,
oracle/_ref/libfermi_ref.so).  Everything an output here holds was written by the reference; nothing is typed in by hand.

  clean3.fq.gz                  4800 reads of 100 bases, 60x over THREE haplotypes of an 8000-base genome that holds a 300-base
                                repeat and an 84-base tandem repeat (a 7-mer x 12).  Haplotype 2 differs from 1 by a SNP, a deletion
                                (1-3) or an insertion (1-4) every 150-600 bases; haplotype 3 has, at every second of these sites, a
                                third allele and a second SNP 12 bases on.  0.4 % substitutions.  With two haplotypes only, no vertex
                                is ever off the two best paths of a bubble (bubble.c:160); without the tandem repeat no arm is shorter
                                than its two overlaps (bubble.c:215-224).
  clean3.mag.gz                 fermi unitig -l40 -t1 of fermi build of these reads
  clean3.<tag>.mag.gz           fermi clean <options> of it, one per entry of RUNS (chain: -CAOFo 33 over the output of plain clean)
  clean3.example_*.mag.gz       fermi example -c -l 40 / -ce -k 17 -l 40 of the reads
  clean3.first100.fa.gz         the first 100 records of clean3.mag as FASTA records (no qualities), and their two outputs
  <name>.clean[_C].mag.gz       the existing small graphs through clean and clean -C
  clean.hand.json.gz            graphs of 2-6 vertices written by build_hand() below, and what the reference makes of each
  clean.sw.json                 sequence pairs and the score ksw_align gives them with xtra = 0 (the call of bubble.c:233)
  clean.manifest.json           md5 of every file above
Usage: python tests/golden/make_golden_clean.py"""
import ctypes as C
import gzip
import hashlib
import json
import os
import random
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REFDIR = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref")
REF = os.path.join(REFDIR, "fermi")
SEED = 20261018
RUNS = [("clean", []), ("clean_C", ["-C"]), ("clean_C_N2_n1", ["-C", "-N2", "-n1"]), ("clean_CS", ["-CS"]), ("clean_CA", ["-CA"]),
        ("clean_C_d09_R09", ["-C", "-d0.9", "-R0.9"]), ("clean_C_l150_e2_i2", ["-C", "-l150", "-e2", "-i2"]),
        ("clean_C_w5_r03_o40", ["-C", "-w5", "-r0.3", "-o40"]), ("clean_C_i1", ["-C", "-i1"]), ("clean_O", ["-O"])]
CHAIN = ("clean_chain_CAOFo33", ["-CAOFo", "33"])
SMALL = ["circle", "palin", "repeat", "special", "tiny", "gen_rule_20k"]
HAND_RUNS = [[], ["-C"], ["-CA"]]
written = {}


def put_gz(name, data):
    with open(os.path.join(HERE, name), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(data)
    written[name] = hashlib.md5(data).hexdigest()


def put_json(name, obj):
    data = json.dumps(obj, separators=(",", ":"), sort_keys=True).encode() + b"\n"
    if name.endswith(".gz"):
        return put_gz(name, data)
    open(os.path.join(HERE, name), "wb").write(data)
    written[name] = hashlib.md5(data).hexdigest()


def ref(args, data=None):
    p = subprocess.run([REF] + args, input=data, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    assert p.returncode == 0, (args, p.returncode)     # a graph the reference stumbles over is a wrong graph
    return p.stdout


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def other(rng, *bases):
    return rng.choice([b for b in "ACGT" if b not in bases])


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def make_reads(rng, genome_len=8000, n_reads=None, cov=60, read_len=100):
    g = list(rand_seq(rng, genome_len))
    mid = genome_len // 2
    g[mid:mid + 300] = g[genome_len // 8:genome_len // 8 + 300]               # a 300-base repeat
    for at in range(3000, genome_len - 200, 8000):                            # a tandem repeat every 8000 bases
        g[at:at + 84] = list(rand_seq(rng, 7) * 12)
    h1 = "".join(g)
    sites, pos = [], rng.randint(150, 600)
    while pos < genome_len - 150:
        sites.append(pos)
        pos += rng.randint(150, 600)
    h2, h3 = list(h1), list(h1)
    for n, pos in reversed(list(enumerate(sites))):                           # right to left: the positions to the left stay valid
        kind = rng.choice(("snp", "del", "ins"))
        if kind == "snp":
            h2[pos] = other(rng, h1[pos])
        elif kind == "del":
            del h2[pos:pos + rng.randint(1, 3)]
        else:
            h2[pos:pos] = list(rand_seq(rng, rng.randint(1, 4)))
        if n % 2 == 0:
            h3[pos] = other(rng, h1[pos], h2[pos] if kind == "snp" else h1[pos])
            h3[pos + 12] = other(rng, h1[pos + 12])
    haps = [h1, "".join(h2), "".join(h3)]
    n_reads = n_reads or genome_len * cov // read_len
    out = []
    for i in range(n_reads):
        h = haps[rng.randrange(3)]
        at = rng.randrange(len(h) - read_len + 1)
        r = list(h[at:at + read_len])
        for j in range(read_len):
            if rng.random() < 0.004:
                r[j] = other(rng, r[j])
        r = "".join(r)
        if rng.random() < 0.5:
            r = revcomp(r)
        out.append("@r%d\n%s\n+\n%s\n" % (i, r, "I" * read_len))
    return "".join(out).encode()


def unitig_of(fq_bytes, tmp, min_match=40):
    fq, fmd = os.path.join(tmp, "r.fq"), os.path.join(tmp, "r.fmd")
    open(fq, "wb").write(fq_bytes)
    ref(["build", "-fo", fmd, fq])
    return ref(["unitig", "-l%d" % min_match, "-t1", fmd])


# ---- graphs written by hand: vertices (name, bases, reads, coverage letter), arcs (vertex, side, vertex, side, overlap) ----
def mag_text(vs, arcs, missing=()):
    ids = dict((v[0], (100 + 10 * i, 101 + 10 * i)) for i, v in enumerate(vs))
    nei = dict((v[0], ([], [])) for v in vs)
    for a, sa, b, sb, ov in arcs:
        nei[a][sa].append("%d,%d;" % (ids[b][sb], ov))
        nei[b][sb].append("%d,%d;" % (ids[a][sa], ov))
    for a, sa, tid, ov in missing:
        nei[a][sa].append("%d,%d;" % (tid, ov))
    out = []
    for name, seq, nsr, cov in vs:
        out.append("@%d:%d\t%d\t%s\t%s\n%s\n+\n%s\n" % (ids[name][0], ids[name][1], nsr, "".join(nei[name][0]) or ".", "".join(nei[name][1]) or ".", seq, cov * len(seq)))
    return "".join(out)


def build_hand(rng):
    L, R = 0, 1
    S, E, S2, E2 = (rand_seq(rng, 400) for _ in range(4))
    mid = rand_seq(rng, 50)
    snp = mid[:25] + other(rng, mid[25]) + mid[26:]
    arm = lambda m: S[-50:] + m + E[:50]
    g = {}
    g["tip"] = mag_text([("a", S, 12, "5"), ("b", E, 12, "5"), ("c", S2, 12, "5"), ("t", E[-50:] + rand_seq(rng, 30), 2, "#")],
                        [("a", R, "b", L, 50), ("b", R, "c", L, 50), ("b", R, "t", L, 50)])
    for tag, n2, c2 in (("bubble_weak_arm", 2, "#"), ("bubble_equal_arms", 6, "5")):
        g[tag] = mag_text([("s", S, 12, "5"), ("x", arm(mid), 6, "5"), ("y", arm(snp), n2, c2), ("e", E, 12, "5")],
                          [("s", R, "x", L, 50), ("s", R, "y", L, 50), ("x", R, "e", L, 50), ("y", R, "e", L, 50)])
    g["arm_shorter_than_overlaps"] = mag_text([("s", S, 12, "5"), ("x", arm(mid), 6, "5"), ("y", S[-50:][:40] + E[:50][10:], 3, "'"), ("e", E, 12, "5")],
                                              [("s", R, "x", L, 50), ("s", R, "y", L, 50), ("x", R, "e", L, 50), ("y", R, "e", L, 50)])
    g["flip_on_merge"] = mag_text([("a", S, 8, "5"), ("b", revcomp(S[-50:] + E), 8, "5"), ("c", S2, 8, "5")],
                                  [("a", R, "b", R, 50), ("b", L, "c", L, 60)])
    m = S[-85:] + E[:85][70:]                                                   # 100 bases, overlaps of 85 on either side: the neighbours overlap by 70
    g["low_count_internal"] = mag_text([("a1", S, 10, "5"), ("a2", S2[:-85] + S[-85:], 10, "5"), ("m", m, 2, "#"), ("b1", E, 10, "5"), ("b2", E[:85] + E2[85:], 10, "5")],
                                       [("a1", R, "m", L, 85), ("a2", R, "m", L, 85), ("m", R, "b1", L, 85), ("m", R, "b2", L, 85)])
    g["neighbour_missing"] = mag_text([("a", S, 8, "5"), ("b", S[-50:] + E, 8, "5")], [("a", R, "b", L, 50)], missing=[("a", R, 999, 60), ("b", R, 998, 45)])
    return g


def sw_pairs(rng):
    lib = C.CDLL(os.path.join(REFDIR, "libfermi_ref.so"))

    class Kswr(C.Structure):
        _fields_ = [(n, C.c_int) for n in ("score", "te", "qe", "score2", "te2", "tb", "qb")]
    lib.ksw_align.restype = Kswr
    lib.ksw_align.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    mat = bytes((5 if i == j else 256 - 4) for i in range(4) for j in range(4))
    code = lambda s: bytes("ACGT".index(c) for c in s)

    def mutate(s, n):
        s = list(s)
        for _ in range(n):
            at, kind = rng.randrange(len(s)), rng.randrange(3)
            if kind == 0:
                s[at] = other(rng, s[at])
            elif kind == 1 and len(s) > 1:
                del s[at:at + rng.randint(1, 3)]
            else:
                s[at:at] = list(rand_seq(rng, rng.randint(1, 3)))
        return "".join(s) or "A"
    pairs = [("A", "A"), ("A", "C"), ("AC", "AC"), ("AC", "CA"), ("A", "ACGT"), ("AAAAAAAA", "CCCCCCCC")]
    base = rand_seq(rng, 60)
    pairs += [(base, base), (base, base[:30] + base[31:]), (base, base[:30] + "G" + base[30:]), (base, base[:20] + base[25:])]
    for _ in range(150):
        a = rand_seq(rng, rng.randint(1, 300))
        pairs.append((a, mutate(a, rng.randint(0, 8)) if rng.random() < 0.8 else rand_seq(rng, rng.randint(1, 300))))
    out = [{"a": a, "b": b, "score": lib.ksw_align(len(a), code(a), len(b), code(b), 4, mat, 5, 2, 0, None).score} for a, b in pairs]
    for n in (6553, 6554, 7000):                                                # where the 16-bit lanes saturate: a sequence against itself ("b" left out)
        s = rand_seq(rng, n)
        out.append({"a": s, "score": lib.ksw_align(n, code(s), n, code(s), 4, mat, 5, 2, 0, None).score})
    return out


def main():
    rng = random.Random(SEED)
    with tempfile.TemporaryDirectory() as tmp:
        fq = make_reads(rng)
        put_gz("clean3.fq.gz", fq)
        mag = unitig_of(fq, tmp)
        put_gz("clean3.mag.gz", mag)
        src = os.path.join(tmp, "clean3.mag")
        open(src, "wb").write(mag)
        counts = {"unitig": mag.count(b"\n+\n")}
        outs = {}
        for tag, args in RUNS:
            outs[tag] = ref(["clean"] + args + [src])
            put_gz("clean3.%s.mag.gz" % tag, outs[tag])
            counts[tag] = outs[tag].count(b"\n+\n")
        chain = ref(["clean"] + CHAIN[1] + ["-"], outs["clean"])
        put_gz("clean3.%s.mag.gz" % CHAIN[0], chain)
        counts[CHAIN[0]] = chain.count(b"\n+\n")
        assert len(set(hashlib.md5(o).hexdigest() for o in list(outs.values()) + [chain, mag])) == len(outs) + 2, "two option sets gave the same graph"
        fqp = os.path.join(tmp, "r.fq")
        put_gz("clean3.example_c_l40.mag.gz", ref(["example", "-c", "-l", "40", fqp]))
        put_gz("clean3.example_ce_k17_l40.mag.gz", ref(["example", "-ce", "-k", "17", "-l", "40", fqp]))
        # FASTA records: no quality line
        recs = mag.split(b"\n")[:400]
        fa = b"".join(b">" + recs[i][1:] + b"\n" + recs[i + 1] + b"\n" for i in range(0, 400, 4))
        put_gz("clean3.first100.fa.gz", fa)
        fap = os.path.join(tmp, "f.fa")
        open(fap, "wb").write(fa)
        for tag, args in RUNS[:2]:
            put_gz("clean3.first100.%s.mag.gz" % tag, ref(["clean"] + args + [fap]))
        empty = os.path.join(tmp, "empty.mag")
        open(empty, "wb").close()
        assert ref(["clean", empty]) == b"" and ref(["clean", "-C", empty]) == b""
        for name in SMALL:
            for tag, args in RUNS[:2]:
                put_gz("%s.%s.mag.gz" % (name, tag), ref(["clean"] + args + [os.path.join(HERE, name + ".mag.gz")]))
        hand = {}
        for name, text in sorted(build_hand(rng).items()):
            p = os.path.join(tmp, "h.mag")
            open(p, "w").write(text)
            hand[name] = {"mag": text, "out": dict((" ".join(a), ref(["clean"] + a + [p]).decode("ascii")) for a in HAND_RUNS)}
        put_json("clean.hand.json.gz", hand)
        put_json("clean.sw.json", sw_pairs(rng))
    put_json("clean.manifest.json", {"seed": SEED, "unitigs": counts, "md5": dict(sorted(written.items()))})
    for k, v in counts.items():
        print("%-24s %5d unitigs" % (k, v))
    print("%d files, %d bytes" % (len(written), sum(os.path.getsize(os.path.join(HERE, n)) for n in written)))


if __name__ == "__main__":
    main()
