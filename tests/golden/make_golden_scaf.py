#!/usr/bin/env python3
"""Fixtures of `fermi scaf`, made where the reference is compiled in place (oracle/_ref/fermi, oracle/_ref/libfermi_ref.so).  Every expected
byte was written by the reference; the read sets are generated here and (but for one) not kept.

  scafN.fmd                   fermi build of a generated paired-end set (interleaved mates, forward/reverse, inserts N(300, 20))
  scafN.remapped.mag.gz       fermi remap -t1 -r rank over clean | clean -CAOFo 30 of unitig -l35 -r rank
  scafN.scaf.fa.gz            stdout of fermi scaf -Pt1 <fmd> <remapped> <avg> <std>
  scaf.json                   per fixture: avg, std (remap's log), the LK|CT|SW lines of scaf -Pt1, what each fixture holds; for one
                              fixture also stdout and lines of scaf -Pt1 -m 3 -a 10 -p 1e-5
  scaf0.reads.fa.gz           the reads of the first fixture (for the test that runs the whole chain)
  scaf.hand.mag               a remapped MAG written by hand over pairs.fmd (build_hand below) and, in scaf.json, what the reference prints for it
  scafN.ext.tsv               the gap of every patched link as the reference left it (from its LK lines; the inserted bases cut out of its FASTA):
                              first line the longest mate, then lower end, upper end, patched, l, t, bases -- what `make asan-scaf` replays
  scaf.hand2.mag.gz           a second hand-written MAG: ends with 5, 13 and 26 neighbours of EQUAL weight, and ties at ends that come after them, so
                              the LK lines depend on the small table's growth (4 -> 8 -> 16 -> 32 -> 64 buckets) and on the bucket count it carries over
  scaf.nour.mag               records without a UR:Z: tag
  scaf.sw.json                sequence pairs and what ksw_align(..., KSW_XSTART, ...) returns for them (the call of scaf.c:504)
  scaf.stat.json              kf_betai (scaf.c:308-335) at recorded arguments, as hex doubles (the corrected mean, scaf.c:371-378, is static there:
                              it is pinned through the P-values of the LK lines)
The set must hold, between its fixtures, at least one of each event listed in NEED; seeds are tried until it does.
Usage: python tests/golden/make_golden_scaf.py"""
import ctypes as C
import gzip
import json
import os
import random
import re
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REFDIR = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref")
REF = os.path.join(REFDIR, "fermi")
NEED = ("filled_gap", "overlap_join", "sw_line", "ct_line", "second_neighbour", "scaftig_of_3", "low_A")
RECIPES = [dict(glen=14000, snp=0.0, cov=30, rlen=70), dict(glen=20000, snp=0.003, cov=30, rlen=80), dict(glen=14000, snp=0.01, cov=40, rlen=70)]
ALT = ["-m", "3", "-a", "10", "-p", "1e-5"]


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def make_reads(rng, glen, snp, cov, rlen):
    g = [rng.choice("ACGT") for _ in range(glen)]
    for _ in range(4):                                                          # four copied segments of 90-260 bases
        n, a, b = rng.randint(90, 260), rng.randrange(glen - 300), rng.randrange(glen - 300)
        g[b:b + n] = g[a:a + n]
    h1 = "".join(g)
    h2 = "".join(rng.choice([c for c in "ACGT" if c != b]) if rng.random() < snp else b for b in h1)
    thin = [(rng.randrange(500, glen - 500), rng.randint(20, 60)) for _ in range(5)]   # windows where 90 % of the reads are dropped
    out, n_pairs = [], glen * cov // (2 * rlen)
    while len(out) < 2 * n_pairs:
        ins = max(2 * rlen, int(rng.gauss(300, 20)))
        at = rng.randrange(glen - ins)
        h = h1 if rng.random() < 0.5 else h2
        a, b = h[at:at + rlen], revcomp(h[at + ins - rlen:at + ins])
        if any(at < w + n and w < at + rlen or at + ins - rlen < w + n and w < at + ins for w, n in thin) and rng.random() < 0.9:
            continue
        if rng.random() < 0.5:
            a, b = b, a
        out += [a, b]
    return out


def run(args, stdin=None):
    p = subprocess.run([REF] + args, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (args, p.returncode, p.stderr[-300:])
    return p.stdout, p.stderr.decode()


def links(err):
    return [l for l in err.split("\n") if l[:3] in ("LK\t", "CT\t", "SW\t")]


def events(fa, lk):
    ev = set()
    for l in lk:
        f = l.split("\t")
        if f[0] == "SW":
            ev.add("sw_line")
        elif f[0] == "CT":
            ev.add("ct_line")
        else:
            if float(f[5]) < 20:
                ev.add("low_A")
            if len(f) >= 9:
                patched, ln, _ = f[8].split(":")
                if patched == "1":
                    ev.add("filled_gap" if int(ln) > 0 else "overlap_join")
            if len(f) >= 11:
                ev.add("second_neighbour")
    for l in fa.decode().split("\n"):
        if l.startswith(">") and int(l.split("\t")[1]) >= 3:
            ev.add("scaftig_of_3")
    return ev


def pipeline(reads, tmp):
    fa, fmd, rank = (os.path.join(tmp, n) for n in ("r.fa", "r.fmd", "r.rank"))
    open(fa, "w").write("".join(">r%d/%d\n%s\n" % (i >> 1, (i & 1) + 1, r) for i, r in enumerate(reads)))
    run(["build", "-fo", fmd, fa])
    open(rank, "wb").write(run(["seqrank", fmd])[0])
    mag = run(["unitig", "-l35", "-t1", "-r", rank, fmd])[0]
    c2 = run(["clean", "-CAOFo", "30", "-"], run(["clean", "-"], mag)[0])[0]
    cp = os.path.join(tmp, "c.mag")
    open(cp, "wb").write(c2)
    rm, err = run(["remap", "-t1", "-r", rank, fmd, cp])
    m = re.search(r"avg = ([0-9.]+) std = ([0-9.]+)", err)
    rp = os.path.join(tmp, "rm.mag")
    open(rp, "wb").write(rm)
    avg, std = m.group(1), m.group(2)
    out, err = run(["scaf", "-Pt1", fmd, rp, avg, std])
    alt, aerr = run(["scaf", "-Pt1"] + ALT + [fmd, rp, avg, std])
    import hashlib
    md5 = dict(unitig=hashlib.md5(mag).hexdigest(), clean=hashlib.md5(run(["clean", "-"], mag)[0]).hexdigest(), clean2=hashlib.md5(c2).hexdigest())
    return dict(md5=md5, fmd=open(fmd, "rb").read(), remapped=rm, avg=avg, std=std, fa=out, lk=links(err), alt_fa=out if alt == out else alt, alt_lk=links(aerr),
                n_utig=rm.count(b"\n+\n"), n_scaf=out.count(b">"))


def put_gz(name, data):
    with open(os.path.join(HERE, name), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="", compresslevel=9) as f:
        f.write(data)


# ---- the remapped MAG written by hand over pairs.fmd (1400 reads: read ids 0 .. 1399, mates 2i and 2i + 1) ----
def build_hand(rng):
    L = 1000
    seq = lambda: "".join(rng.choice("ACGT") for _ in range(L))
    fwd = lambda r, at: "%d,%d,%d;" % (r << 1, at, at + 60)                     # strand 0: towards the right end, distance L - at
    rev = lambda r, at: "%d,%d,%d;" % (r << 1 | 1, at, at + 60)                 # strand 1: towards the left end, distance at + 60
    ur = {k: [] for k in "ABCDE"}
    # A's right end sees B and C with TWO pairs each and the same sum of distances (the tie); D through three pairs
    for i, (pa, pb) in enumerate([(700, 100), (760, 160)]):
        ur["A"].append(fwd(2 * i, pa)); ur["B"].append(rev(2 * i + 1, pb))
    for i, (pa, pc) in enumerate([(720, 120), (740, 140)]):
        ur["A"].append(fwd(20 + 2 * i, pa)); ur["C"].append(rev(21 + 2 * i, pc))
    for i in range(3):
        ur["B"].append(fwd(40 + 2 * i, 800 + 10 * i)); ur["D"].append(rev(41 + 2 * i, 50 + 10 * i))
    ur["A"] += [fwd(60, 750), fwd(60, 770)]; ur["B"].append(rev(61, 90))        # a read listed twice, and its mate
    ur["A"].append(fwd(64, 730)); ur["C"] += [rev(65, 100), rev(65, 110), rev(65, 130)]   # a read listed three times, and its mate
    ur["D"] += [fwd(80, 600), rev(81, 300)]                                     # both mates on one unitig
    ur["C"].append(fwd(90, 100)); ur["D"].append(rev(91, 200))                  # beyond max_dist on C's side
    ur["E"] += [fwd(100, 900)]; ur["A"].append(rev(101, 20))                    # E has a low A: excluded
    recs = []
    for i, k in enumerate("ABCDE"):
        nsr = 100 if k != "E" else 140
        recs.append("@%d:%d\t%d\t%d,40;\t%d,35;\tUR:Z:%s\n%s\n+\n%s\n" % (1000 + 10 * i, 1001 + 10 * i, nsr, 5000 + i, 6000 + i, "".join(ur[k]), seq(), "5" * L))
    recs.insert(2, "@77:78\t9\t.\t.\n%s\n+\n%s\n" % (seq()[:80], "5" * 80))   # no UR tag: skipped
    return "".join(recs)


def build_hand2(rng):
    """hubs whose right end sees n neighbours through ONE pair each, all with the same sum of distances; behind each hub a unitig whose right end sees two
    equal neighbours: its table has the bucket count the hub left (8 after five keys, 16 after thirteen; 26 keys end at 64, which is thrown away)"""
    L, pair, recs, ident = 400, [0], [], [2000]
    seq = lambda: "".join(rng.choice("ACGT") for _ in range(L))

    def unitig(ur):
        ident[0] += 10
        recs.append("@%d:%d\t100\t%d,40;\t%d,35;\tUR:Z:%s\n%s\n+\n%s\n" % (ident[0], ident[0] + 1, 7000 + len(recs), 8000 + len(recs), "".join(ur), seq(), "5" * L))
        return len(recs) - 1

    def star(n):
        own, others = [], []
        for _ in range(n):
            p = pair[0]; pair[0] += 1
            own.append("%d,%d,%d;" % ((2 * p) << 1, L - 100, L - 40))                  # forward, 100 from the right end
            others.append(["%d,%d,%d;" % ((2 * p + 1) << 1 | 1, 20, 80)])              # its mate, reverse, 80 from the left end of a unitig of its own
        return own, others
    for n in (5, 2, 13, 2, 26, 3):
        own, others = star(n)
        at = unitig(own)
        recs[at:at] = []                                                               # (the hub first, then its neighbours: ends are visited in file order)
        for o in others:
            unitig(o)
    return "".join(recs)


def trimmed_unitigs(mag):
    """the unitigs scaf keeps (a UR:Z: tag), single-read ends cut off, as it numbers them"""
    out, lines = [], mag.decode().split("\n")
    for i in range(0, len(lines) - 1, 4):
        if "UR:Z:" not in lines[i]:
            continue
        q, sq = lines[i + 3], lines[i + 1]
        b = len(q) - len(q.lstrip('"')); e = len(q.rstrip('"'))
        out.append(sq[b:e] if b < e else sq)
    return out


def gaps(mag, fa, lk):
    """per patched link (lower end first): patched, l, t as the LK line prints them, and the bases between the two unitigs in the FASTA"""
    us = trimmed_unitigs(mag)
    tigs = [l for l in fa.decode().split("\n") if l and not l.startswith(">")]
    tigs += [revcomp(t) for t in tigs]
    kid = {}
    rows = [l.split("\t") for l in lk if l.startswith("LK\t")]
    for f in rows:
        kid[f[2]] = 2 * int(f[1].split(":")[0]) + int(f[1].split(":")[1])
    out = []
    for f in rows:
        if len(f) < 9 or f[8].split(":")[0] != "1":
            continue
        p, q = kid[f[2]], kid[f[6]]
        if p > q:
            continue
        _, l, t = f[8].split(":")
        l, s = int(l), "."
        if l > 0:
            left = us[p >> 1] if p & 1 else revcomp(us[p >> 1])
            right = us[q >> 1] if not q & 1 else revcomp(us[q >> 1])
            for tig in tigs:
                at = tig.find(left[-60:])
                while at >= 0 and s == ".":
                    cut = at + len(left[-60:])
                    if tig[cut + l:cut + l + 40] == right[:40]:
                        s = tig[cut:cut + l]
                    at = tig.find(left[-60:], at + 1)
        out.append("%d\t%d\t1\t%d\t%s\t%s" % (p, q, l, t, s))
    return out


def sw_vectors(rng):
    lib = C.CDLL(os.path.join(REFDIR, "libfermi_ref.so"))

    class Kswr(C.Structure):
        _fields_ = [(n, C.c_int) for n in ("score", "te", "qe", "score2", "te2", "tb", "qb")]
    lib.ksw_align.restype = Kswr
    lib.ksw_align.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    mat = bytes((1 if i == j else 256 - 3) for i in range(5) for j in range(5))
    code = lambda s: bytes("$ACGT".index(c) for c in s)                         # nt6 codes 1..4, as scaf.c hands them over
    rs = lambda n: "".join(rng.choice("ACGT") for _ in range(n))

    def sub(s, at):
        return s[:at] + rng.choice([c for c in "ACGT" if c != s[at]]) + s[at + 1:]
    pairs = []
    for n in (1, 15, 16, 17, 340):
        a = rs(n)
        pairs += [(a, a), (a, rs(n))]
        if n >= 15:
            pairs += [(a, sub(a, 2)), (a, sub(a, n - 3)), (sub(a, 1), sub(a, n - 2))]
    for ov in (15, 16, 17, 20, 40, 69):                                         # q starts with what t ends in: the overlap of two unitig ends
        t, q = rs(340), rs(340)
        q = t[-ov:] + q[ov:]
        pairs += [(q, t), (sub(q, 2), t), (sub(q, ov - 3), t), (q[:ov] + q, t), (q, t[:-ov] + t[-ov:-ov // 2] + rs(rng.randint(1, 3)) + t[-ov // 2:])]
    pairs += [("AAAA", "CCCC"), ("ACGT" * 10, "TTTT" * 10), ("A" * 30, "A" * 30), ("AC" * 20, "CA" * 20)]
    for _ in range(60):
        a = rs(rng.randint(1, 340))
        b = list(a)
        for _ in range(rng.randint(0, 6)):
            at = rng.randrange(len(b) + 1)
            b[at:at + rng.randint(0, 2)] = rs(rng.randint(0, 2))
        pairs.append((a, "".join(b) or "A"))
    out = []
    for q, t in pairs:
        r = lib.ksw_align(len(q), code(q), len(t), code(t), 5, mat, 5, 2, 0x80000, None)
        out.append(dict(q=q, t=t, score=r.score, te=r.te, qe=r.qe, tb=r.tb, qb=r.qb))
    return out


def stat_vectors(rng):
    lib = C.CDLL(os.path.join(REFDIR, "libfermi_ref.so"))
    lib.kf_betai.restype = C.c_double
    lib.kf_betai.argtypes = [C.c_double] * 3
    beta = []
    for n in (1, 2, 3, 7, 20, 50):
        for t in (0.0, 0.01, 0.3, 1.0, 2.5, 7.0, 40.0, 1e3):
            x = n / (n + t * t)
            beta.append(dict(a=.5 * n, b=.5, x=x, v=lib.kf_betai(.5 * n, .5, x).hex()))      # both branches: x below and above (a + 1) / (a + b + 2)
    return dict(betai=beta)


def main():
    meta, have, seed = {}, set(), 20261018
    with tempfile.TemporaryDirectory() as tmp:
        for i, rec in enumerate(RECIPES):
            want = {0: {"filled_gap", "scaftig_of_3"}, 1: {"ct_line", "overlap_join"}, 2: {"sw_line"}}[i]
            for attempt in range(400):
                seed += 1
                rng = random.Random(seed)
                reads = make_reads(rng, **rec)
                r = pipeline(reads, tmp)
                ev = events(r["fa"], r["lk"])
                if want <= ev and (i < 2 or set(NEED) <= have | ev):
                    break
            else:
                raise SystemExit("no seed gave %s for fixture %d" % (sorted(want), i))
            have |= ev
            name = "scaf%d" % i
            open(os.path.join(HERE, name + ".fmd"), "wb").write(r["fmd"])
            put_gz(name + ".remapped.mag.gz", r["remapped"])
            put_gz(name + ".scaf.fa.gz", r["fa"])
            meta[name] = dict(seed=seed, recipe=rec, avg=r["avg"], std=r["std"], lines=r["lk"], events=sorted(ev), unitigs=r["n_utig"], scaftigs=r["n_scaf"])
            meta[name]["md5"] = r["md5"]
            open(os.path.join(HERE, name + ".ext.tsv"), "w").write("max_len\t%d\n" % rec["rlen"] + "".join(g + "\n" for g in gaps(r["remapped"], r["fa"], r["lk"])))
            if i == 1:
                put_gz(name + ".scaf_m3_a10_p1e-5.fa.gz", r["alt_fa"])
                meta[name]["alt_args"], meta[name]["alt_lines"] = ALT, r["alt_lk"]
            if i == 0:
                put_gz(name + ".reads.fa.gz", "".join(">r%d/%d\n%s\n" % (j >> 1, (j & 1) + 1, s) for j, s in enumerate(reads)).encode())
            print(name, "seed", seed, r["n_utig"], "->", r["n_scaf"], sorted(ev))
        assert set(NEED) <= have, sorted(set(NEED) - have)
        rng = random.Random(20261018)
        hand = build_hand(rng)
        open(os.path.join(HERE, "scaf.hand.mag"), "w").write(hand)
        out, err = run(["scaf", "-Pt1", os.path.join(HERE, "pairs.fmd"), os.path.join(HERE, "scaf.hand.mag"), "300", "30"])
        meta["hand"] = dict(avg="300", std="30", lines=links(err), fa=out.decode())
        lk = [l.split("\t") for l in links(err) if l.startswith("LK")]
        assert any(len(f) >= 11 and f[7].split(":")[0] == f[10].split(":")[0] and f[7] == f[10] for f in lk), "the hand-written MAG holds no tie"
        put_gz("scaf.hand2.mag.gz", build_hand2(rng).encode())
        out, err = run(["scaf", "-Pt1", os.path.join(HERE, "pairs.fmd"), os.path.join(HERE, "scaf.hand2.mag.gz"), "300", "30"])
        meta["hand2"] = dict(avg="300", std="30", lines=links(err), fa_md5=__import__("hashlib").md5(out).hexdigest())
        assert sum(1 for l in links(err) if len(l.split("\t")) >= 11 and l.split("\t")[7] == l.split("\t")[10]) >= 6, "hand2 holds too few ties"
        nour = "".join(r for r in re.findall(r"@[^\n]*\n[^\n]*\n\+\n[^\n]*\n", hand)).replace("\tUR:Z:", "\tXX:Z:")
        open(os.path.join(HERE, "scaf.nour.mag"), "w").write(nour)
        out, err = run(["scaf", "-Pt1", os.path.join(HERE, "pairs.fmd"), os.path.join(HERE, "scaf.nour.mag"), "300", "30"])
        assert out == b"" and not links(err)
        json.dump(sw_vectors(rng), open(os.path.join(HERE, "scaf.sw.json"), "w"), separators=(",", ":"))
        json.dump(stat_vectors(rng), open(os.path.join(HERE, "scaf.stat.json"), "w"), separators=(",", ":"))
    json.dump(meta, open(os.path.join(HERE, "scaf.json"), "w"), indent=0, sort_keys=True)
    for fn in sorted(os.listdir(HERE)):
        if fn.startswith("scaf"):
            print("%8d %s" % (os.path.getsize(os.path.join(HERE, fn)), fn))


if __name__ == "__main__":
    main()
