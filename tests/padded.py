"""Helper (no tests): a small real read set S sitting beyond 2^32 positions.  M filler reads A^Lf are put IN FRONT of S (read $ revcomp $ ...: the filler's
strands are A^Lf and T^Lf, ids 0 .. 2M-1; the strands of S get the ids 2M ..), and the BWT of filler + S is written down from the BWT of S alone:

  sentinel rows   the 2M rows `$` of the filler come before those of S (sentinels sort by sequence id); their BWT symbols alternate A, T.
  A^k $, k=1..Lf  M equal rows each.  They sort at the LOWER BOUND of A^k $ among the suffixes of S -- the number of suffixes of S smaller than A^k $,
                  defined whether A^k occurs in S or not -- and, being of smaller ids, before a suffix of S that equals them.  That bound follows from
                  the BWT of S by the backward-search recurrence  lo_0 = 0,  lo_k = C[A] + occ(A, lo_{k-1}):  a suffix is smaller than A Q exactly when it
                  starts with `$`, or with A and goes on smaller than Q.  lo_k does not fall with k, and where lo_k = lo_{k+1} the rows of A^k $ come first.
                  Their BWT symbol is A for k < Lf and `$` for k = Lf (the whole strand).
  T^k $           the same with T.  Every A^k $ is smaller than every T^k $.
  rows of S       keep their order: row p of S moves up by M for every group of M filler rows inserted at or before p.

So the new string is S cut at 2 + 2 Lf places (`Padding.ins`, sorted, 0 twice for the 2M sentinels) with M equal symbols put in at each.  A row number of
S -> its row number in the padded string is `map_pos`.  The fields of an overlap record that count SEQUENCES before a row (fm_retrieve's rank, the two
ends of the interval of `$read$`, x[0] of a neighbour: the number of BWT symbols `$` before the row) move by M for each of the two groups of whole
filler strands (the rows A^Lf $ and T^Lf $) at or before them: `map_rank`."""
import numpy as np

U64 = np.uint64
I64 = np.int64
A, T = 1, 4


class Padding:
    """where the filler's rows go into the BWT of S (from that BWT alone), and what it does to positions, ranks and ids"""

    def __init__(self, bwt_S, M, Lf):
        bwt = np.ascontiguousarray(bwt_S, dtype=np.uint8)
        self.M, self.Lf, self.n_S = int(M), int(Lf), len(bwt)
        cnt = np.bincount(bwt, minlength=6).astype(I64)
        acc = np.concatenate([[0], np.cumsum(cnt)])                      # acc[c] = symbols smaller than c
        pts = {}
        for c in (A, T):
            occ = np.concatenate([[0], np.cumsum(bwt == c, dtype=I64)])  # occ[i] = symbols c among rows [0, i)
            lo, p = 0, []
            for _ in range(self.Lf):
                lo = int(acc[c] + occ[lo])
                p.append(lo)
            pts[c] = p
        # the groups of M equal rows in the order they appear: (row of S they are inserted before, BWT symbol); the sentinels' 2M rows are two groups
        self.sym = np.array([0, 0] + [A] * (self.Lf - 1) + [0] + [T] * (self.Lf - 1) + [0], dtype=np.uint8)
        self.ins = np.array([0, 0] + pts[A] + pts[T], dtype=I64)
        assert (np.diff(self.ins) >= 0).all()
        occ0 = np.concatenate([[0], np.cumsum(bwt == 0, dtype=I64)])
        self.rank_A, self.rank_T = int(occ0[pts[A][-1]]), int(occ0[pts[T][-1]])   # sequences of S sorted before A^Lf, before T^Lf
        self.n = self.n_S + 2 * self.M * (self.Lf + 1)
        self.id_shift = 2 * self.M
        self.n_seq = int(cnt[0]) + 2 * self.M

    def map_pos(self, p):
        """row p of the BWT of S (0 .. n_S) -> its row in the padded BWT"""
        p = np.asarray(p).astype(I64)
        return (p + self.M * np.searchsorted(self.ins, p, side="right")).astype(U64)

    def map_rank(self, r):
        """a sequence's rank among the sorted sequences of S -> among those of filler + S"""
        r = np.asarray(r).astype(I64)
        return (r + self.M * ((r >= self.rank_A).astype(I64) + (r >= self.rank_T))).astype(U64)

    def occ_filler(self, p):
        """[len(p), 6]: the filler's rows of each symbol before row p of S in the padded BWT (half of the sentinels' rows hold A, half T)"""
        ev = np.array([A, T] + [A] * (self.Lf - 1) + [0] + [T] * (self.Lf - 1) + [0])
        cum = np.zeros((len(ev) + 1, 6), dtype=I64)
        cum[1:] = np.cumsum(ev[:, None] == np.arange(6)[None, :], axis=0)
        return self.M * cum[np.searchsorted(self.ins, np.asarray(p).astype(I64), side="right")]

    def longest_fill(self):
        """the longest stretch of equal filler symbols that no row of S interrupts (a run of the BWT at least that long)"""
        best = cur = 0
        last = -1
        for seg in self.segments():
            if seg[0] == "fill" and seg[1] is not None and seg[1] == last:
                cur += seg[2]
            else:
                cur, last = (seg[2], seg[1]) if seg[0] == "fill" and seg[1] is not None else (0, -1)
            best = max(best, cur)
        return best

    def segments(self):
        """the padded string as pieces in order: ("fill", symbol or None for the alternating sentinels, count) and ("S", from, to)"""
        out = [("fill", None, 2 * self.M)]
        at = 0
        for p, s in zip(self.ins[2:], self.sym[2:]):
            if p > at:
                out.append(("S", at, int(p)))
                at = int(p)
            out.append(("fill", int(s), self.M))
        if at < self.n_S:
            out.append(("S", at, self.n_S))
        return out

    def counts(self):
        """symbols of each kind in the padded string (index $ A C G T N)"""
        return {"n": self.n, "sentinels": self.n_seq, "M": self.M, "Lf": self.Lf, "rows of S": self.n_S, "first row of S": int(self.map_pos(0)),
                "last row of S": int(self.map_pos(self.n_S - 1))}


def padded_bwt_host(bwt_S, M, Lf):
    """numpy, for small M: (the BWT of filler + S, Padding)"""
    bwt = np.ascontiguousarray(bwt_S, dtype=np.uint8)
    pad = Padding(bwt, M, Lf)
    parts = []
    for seg in pad.segments():
        if seg[0] == "S":
            parts.append(bwt[seg[1]:seg[2]])
        elif seg[1] is None:
            parts.append(np.tile(np.array([A, T], dtype=np.uint8), seg[2] // 2))
        else:
            parts.append(np.full(seg[2], seg[1], dtype=np.uint8))
    out = np.concatenate(parts)
    assert len(out) == pad.n
    return out, pad


def padded_bwt_device(bwt_S, M, Lf, dev):
    """torch, for large M: (the BWT of filler + S as a uint8 tensor in HBM, Padding).  Segment-wise fills into one allocation: no second copy of the
    big string on the device and none on the host."""
    import torch
    bwt = np.ascontiguousarray(bwt_S, dtype=np.uint8)
    pad = Padding(bwt, M, Lf)
    src = torch.from_numpy(bwt).to(dev)
    out = torch.empty(pad.n, dtype=torch.uint8, device=dev)
    at = 0
    for seg in pad.segments():
        if seg[0] == "S":
            m = seg[2] - seg[1]
            out[at:at + m] = src[seg[1]:seg[2]]
        elif seg[1] is None:
            m = seg[2]
            out[at:at + m].view(torch.int16).fill_(A | T << 8)        # (little-endian: A first)
        else:
            m = seg[2]
            out[at:at + m].fill_(seg[1])
        at += m
    assert at == pad.n
    return out, pad


def strands_bwt_by_sorting(strands):
    """the BWT of strand $ strand $ ... by sorting every suffix up to its `$` (sequences of any lengths; equal suffixes by sequence id): the definition"""
    n, L1 = len(strands), max(len(s) for s in strands) + 1
    text = np.zeros((n, 2 * L1), dtype=np.uint8)
    lens = np.array([len(s) for s in strands], dtype=I64)
    for i, s in enumerate(strands):
        text[i, :len(s)] = s
    keys = np.empty((n * L1, L1), dtype=np.uint8)
    for p in range(L1):
        keys[p::L1] = text[:, p:p + L1]
    sid, pos = np.repeat(np.arange(n), L1), np.tile(np.arange(L1), n)
    real = pos <= lens[sid]                                              # the suffixes that exist: up to the strand's own `$`
    keys, sid, pos = keys[real], sid[real], pos[real]
    order = np.lexsort([sid, np.ascontiguousarray(keys).view("S%d" % L1).ravel()])
    return np.where(pos[order] == 0, 0, text[sid[order], pos[order] - 1]).astype(np.uint8)


def strands_of(reads):
    """read, revcomp, read, revcomp, ... (nt6 codes, A/C/G/T only)"""
    out = []
    for r in reads:
        r = np.asarray(r, dtype=np.uint8)
        out += [r, (5 - r)[::-1]]
    return out


def filler_strands(M, Lf):
    return strands_of([np.full(Lf, A, dtype=np.uint8)] * M)


def ragged_reads():
    """a small ragged set for the tie rule and the interleaving: 300 reads of 30-fold cover with 1 % errors cut to 20 .. 60 bases, and reads that END in
    A^k and in T^k, that ARE A^k / T^k (equal to a filler suffix: the filler goes first), and that hold runs A^k inside, k = 1 .. 9"""
    from fermi_amd import synth
    rng = np.random.default_rng(20261020)
    base = synth.reads(synth.DEFAULT_SEED + 77, 300, 60, 30, 0.01)
    reads = [r[: rng.integers(20, 61)].copy() for r in base]
    for k in range(1, 10):
        body = rng.integers(1, 5, 25).astype(np.uint8)
        body[-1] = 2                                                     # (so that the run that follows is exactly k long)
        for c in (A, T):
            run = np.full(k, c, dtype=np.uint8)
            reads += [np.concatenate([body, run]), run.copy(), np.concatenate([body[:9], run, body[9:]]), np.concatenate([run, body])]
    return reads
