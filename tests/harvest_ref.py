"""The k-mer harvest of `correct` (fmd_kmer_collect*, fermi_amd/csrc/fmd_kmer.hip) by definition, over the reads themselves: numpy integers and
IEEE doubles, no index and no oracle.

Every sequence as indexed and its reverse complement (N stays N) is cut into its N-free w-windows.  A window is the number K with its rightmost base
in bits 0-1 (base - 1, two bits each); the symbol to its left is 0 at the start of a sequence, 1..4 for a base, 5 for N.  Per distinct K that gives
s[0..5] and sz = sum(s) -- what one backward extension of K's interval returns -- and correct.c:56-75 turns them into (bucket, key, val) and cnt[].
The trie's pruning needs no restating: counts only fall along a path, so depth w is reached exactly when sz >= min_occ, and mx >= min_occ asks more."""
import gzip
import os

import numpy as np

from fermi_amd import hostlib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (w, min_occ, suf_len): w at both limits, w - suf_len at 15 and at 1, suf_len at 16 (the last whose bucket fits 32 bits), levels at or below suf_len
# (threshold 1) and beyond it (threshold min_occ)
CASES = [(2, 1, 1), (3, 2, 1), (5, 3, 2), (8, 1, 7), (11, 3, 1), (15, 2, 1), (16, 1, 1), (16, 3, 15), (17, 1, 2), (17, 3, 16), (27, 1, 12), (27, 2, 16)]
NAMES = ["tiny", "special", "palin", "repeat", "dup32"]
EMPTY_CASE = (17, 1 << 30, 2)       # a min_occ above every count
# over kept k-mers: interval wider than 63 at depth w (the two-rank branch of km_extend_back), ratio above 31 before the cap, rest == 0, rest > 7
# (the 3-bit field saturates), two bases tie for the maximum (the lowest wins), a sequence starts here, an N to the left, a ratio below 31 ending in .5
CLASSES = ("wide", "capped", "rest0", "rest_gt7", "tie", "s0", "s5", "half")


def fastq_reads(name):
    tab = np.full(256, 5, dtype=np.uint8)
    for ch, v in zip(b"ACGTacgt", [1, 2, 3, 4, 1, 2, 3, 4]):
        tab[ch] = v
    with gzip.open(os.path.join(GOLD, name + ".fq.gz"), "rb") as f:
        lines = f.read().split(b"\n")
    return [tab[np.frombuffer(lines[i], dtype=np.uint8)] for i in range(1, len(lines) - 1, 4)]


def forward_as_indexed(name):
    """the reads of the golden FASTQ; an even-length read that is its own reverse complement loses its last base, as `build` trims it"""
    out = []
    for r in fastq_reads(name):
        r = np.ascontiguousarray(r, dtype=np.uint8)
        out.append(r[:hostlib.trim_palindrome(r)])
    return out


def revcomp(s):
    out = s[::-1].copy()
    m = (out >= 1) & (out <= 4)
    out[m] = 5 - out[m]
    return out


class Answer:
    """bucket, key, val sorted by (bucket, key); cnt = [kept, informative]; classes = members of each of CLASSES among the kept"""

    def __init__(self, bucket, key, val, cnt, classes):
        self.bucket, self.key, self.val, self.cnt, self.classes, self.n = bucket, key, val, cnt, classes, len(bucket)

    def in_parts(self, masks):
        """the triples as the host forms return them: one sorted run per mask (k-mers whose last base, bits 0-1 of the bucket, is in it), concatenated"""
        runs = [((m >> (self.bucket & 3).astype(np.int64)) & 1) == 1 for m in masks]
        return tuple(np.concatenate([a[r] for r in runs]) for a in (self.bucket, self.key, self.val))


class Harvest:
    """brute force for one read set; per w the table of left symbols is computed once"""

    def __init__(self, seqs):
        zero = np.zeros(1, dtype=np.uint8)
        mult = {}
        for r in seqs:                                                             # a sequence that occurs m times is cut once, and counts m times
            r = np.ascontiguousarray(r, dtype=np.uint8).tobytes()
            mult[r] = mult.get(r, 0) + 1
        parts, wt = [zero], [np.zeros(1, dtype=np.int64)]
        for r, m in mult.items():
            r = np.frombuffer(r, dtype=np.uint8)
            parts += [r, zero, revcomp(r), zero]
            wt.append(np.full(2 * len(r) + 2, m, dtype=np.int64))
        self.text = np.concatenate(parts)                                          # 0 = no sequence here: ends every window, and is the left symbol 0
        self.mult = np.concatenate(wt)                                             # per position of the text, how often its sequence occurs
        self.by_w, self.by_d = {}, {}

    def windows(self, d):
        """(K, left symbol, multiplicity) of every N-free d-window of both strands, in no order"""
        t = self.text
        n = len(t) - d + 1
        if n <= 0:
            return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        base = ((t.astype(np.int64) - 1) & 3).astype(np.uint64)
        bad = np.concatenate([[0], np.cumsum((t < 1) | (t > 4))])
        good = (bad[d:] - bad[:-d]) == 0
        K = np.zeros(n, dtype=np.uint64)
        for j in range(d):
            K = (K << np.uint64(2)) | base[j:j + n]
        left = np.zeros(n, dtype=np.int64)
        left[1:] = t[:n - 1]                                                       # (window 0 starts on the leading 0 and is never good)
        return K[good], left[good], self.mult[:n][good]

    @staticmethod
    def summed(index, mult, size):
        """out[i] = sum of mult over index == i, in integers (a double holds these sums exactly: they are below 2^53)"""
        return np.rint(np.bincount(index, weights=mult.astype(np.float64), minlength=size)).astype(np.int64)

    def table(self, w):
        """distinct K ascending, s[:, 0..5]"""
        if w not in self.by_w:
            K, left, m = self.windows(w)
            uK, inv = np.unique(K, return_inverse=True)
            self.by_w[w] = (uK, self.summed(inv.astype(np.int64).ravel() * 6 + left, m, 6 * len(uK)).reshape(len(uK), 6))
        return self.by_w[w]

    def answer(self, w, min_occ, suf_len, seed_mask=0xf):
        uK, s = self.table(w)
        sz = s.sum(axis=1)
        b = s[:, 1:5]
        best = b.argmax(axis=1).astype(np.uint64)                                  # the first maximum: the lowest base wins a tie
        mx = b.max(axis=1) if len(uK) else np.zeros(0, dtype=np.int64)
        keep = (mx >= min_occ) & (((seed_mask >> (uK & np.uint64(3)).astype(np.int64)) & 1) == 1)
        rest = sz - mx - s[:, 0] - s[:, 5]
        raw = np.where(rest == 0, mx.astype(np.float64), mx.astype(np.float64) / np.maximum(rest, 1).astype(np.float64))
        r = np.minimum(raw, 31.0)
        val = (np.floor(r + .499).astype(np.int64) << 3 | np.minimum(rest, 7)).astype(np.uint8)
        inf = keep & (rest <= 7) & (r >= float(min_occ))
        bucket = (uK & np.uint64((1 << (2 * suf_len)) - 1))
        key = ((uK >> np.uint64(2 * suf_len)) << np.uint64(2)) | best
        assert int(bucket.max(initial=0)) < 1 << 32 and int(key.max(initial=0)) < 1 << 32
        classes = {
            "wide": sz > 63, "capped": raw > 31.0, "rest0": rest == 0, "rest_gt7": rest > 7, "tie": (b == mx[:, None]).sum(axis=1) >= 2,
            "s0": s[:, 0] > 0, "s5": s[:, 5] > 0,
            "half": (rest > 0) & ((2 * mx) % np.maximum(rest, 1) == 0) & (mx % np.maximum(rest, 1) != 0) & (mx < 31 * rest),
        }
        classes = {c: int((m & keep).sum()) for c, m in classes.items()}
        bucket, key, val = bucket[keep].astype(np.uint32), key[keep].astype(np.uint32), val[keep]
        o = np.lexsort([key, bucket])
        return Answer(bucket[o], key[o], val[o], [int(keep.sum()), int(inf.sum())], classes)

    def level_counts(self, w, min_occ, suf_len, seed_mask=0xf):
        """out[d], d = 1..w: the distinct d-mers the trie holds at depth d -- those with at least 1 occurrence up to depth suf_len, min_occ beyond"""
        out = np.zeros(w + 1, dtype=np.int64)
        for d in range(1, w + 1):
            if d not in self.by_d:
                K, _, m = self.windows(d)
                u, inv = np.unique(K, return_inverse=True)
                self.by_d[d] = (u, self.summed(inv.astype(np.int64).ravel(), m, len(u)))
            u, c = self.by_d[d]
            sel = ((seed_mask >> (u & np.uint64(3)).astype(np.int64)) & 1) == 1
            out[d] = int((sel & (c >= (1 if d <= suf_len else min_occ))).sum())
        return out
