"""A plain restatement of fm6_smem1_core (smem.c:13-80) and of the fm6_smem chain (smem.c:397-410) over a decoded BWT, and the
case list that the host test (test_smem_ref_host.py) and the GPU test (test_gpu_smem_edges.py) of k_smem share.

Ranks come from prefix counts (np.cumsum of the six one-hot planes of the BWT): nothing here is shared with the kernel or with the
oracle's rank code.  The two starts that the reference leaves undefined -- a first base the index lacks, and a forward sweep that
pushes nothing -- return a marker instead of reading an empty list."""
import functools

import numpy as np

INTV_DT = np.dtype([("x", "<u8", 3), ("info", "<u8")])
UNDEF_NO_BASE = "undefined: the index lacks q[x]"
UNDEF_EMPTY_FWD = "undefined: the forward sweep pushed nothing"
ORDER = (0, 4, 3, 2, 1, 5)   # running-sum order of the other strand's coordinate ($, T, G, C, A, N)


def comp6(c):
    return 5 - c if 1 <= c <= 4 else c


def revcomp(s):
    s = np.asarray(s, dtype=np.uint8)[::-1]
    return np.where((s >= 1) & (s <= 4), 5 - s, s).astype(np.uint8)


def bwt_by_sorting_ragged(reads):
    """The BWT of read $ revcomp $ ... by sorting every suffix; the sentinels are ordered by sequence id (read i is 2i, its reverse
    complement 2i + 1).  Reads of any length >= 1."""
    keys = []
    sid = 0
    for r in reads:
        for s in (np.asarray(r, dtype=np.uint8), revcomp(r)):
            b = s.tobytes()
            tail = b"\x00" + sid.to_bytes(4, "big")
            keys.extend((b[p:] + tail, b[p - 1] if p else 0) for p in range(len(b) + 1))
            sid += 1
    keys.sort()
    return np.array([k[1] for k in keys], dtype=np.uint8)


class RefIndex:
    """cnt, the number of sequences and occ[k][c] = how many c in bwt[0:k]"""

    def __init__(self, bwt):
        bwt = np.asarray(bwt, dtype=np.uint8)
        self.n = len(bwt)
        self.occ = np.zeros((self.n + 1, 6), dtype=np.int64)
        for c in range(6):
            np.cumsum(bwt == c, out=self.occ[1:, c])
        tot = self.occ[self.n].tolist()
        self.cnt = [sum(tot[:c]) for c in range(7)]
        self.n_seq = tot[0]

    def set_intv(self, c):
        return (self.cnt[c], self.cnt[comp6(c)], self.cnt[c + 1] - self.cnt[c])

    def extend(self, ik, back):
        """fm6_extend (exact.c:72-88) of one interval (x0, x1, size): the six children, without info"""
        d = 1 if back else 0
        o = 1 - d
        tk = self.occ[ik[o]].tolist()
        tl = self.occ[ik[o] + ik[2]].tolist()
        ok = [[0, 0, tl[c] - tk[c]] for c in range(6)]
        for c in range(6):
            ok[c][o] = self.cnt[c] + tk[c]
        acc = ik[d]
        for c in ORDER:
            ok[c][d] = acc
            acc += ok[c][2]
        return [tuple(v) for v in ok]

    def extend_back_many(self, prev, c):
        """backward fm6_extend of every interval of a list (rows x0, x1, size, info): child c of each, and the size of each '$' child"""
        tk = self.occ[prev[:, 0]]
        s = self.occ[prev[:, 0] + prev[:, 2]] - tk
        before = np.zeros(len(prev), dtype=np.int64)
        for b in ORDER:
            if b == c:
                break
            before += s[:, b]
        return np.stack([self.cnt[c] + tk[:, c], prev[:, 1] + before, s[:, c], prev[:, 3]], axis=1), s[:, 0]


def _rows(mem):
    out = np.zeros(len(mem), dtype=INTV_DT)
    for k, (x0, x1, sz, info) in enumerate(mem):
        out[k]["x"] = (x0, x1, sz)
        out[k]["info"] = info
    return out


def smem1(ix, q, x, self_match):
    """fm6_smem1_core -> (mem, ret, trace).  mem: INTV_DT rows in the reference's order; ret: the next start, or one of the two
    UNDEF_* markers (mem is then empty).  trace: fwd_len = entries the forward sweep pushed; max_curr = the longest curr list of
    a backward round; last_prev = len(prev) in the i == -1 round (None: not reached); last_from_fwd = that prev is the forward list;
    rounds = backward rounds; last_open_skipped = entries 1..63 of the i == -1 round that are not sentinel-closed and
    come when curr is non-empty (they can neither be reported nor matter: the kernel skips them)."""
    q = [int(v) for v in q]
    L = len(q)
    sm = bool(self_match)
    trace = {"fwd_len": 0, "max_curr": 0, "last_prev": None, "last_from_fwd": False, "rounds": 0, "last_open_skipped": 0}
    ik = ix.set_intv(q[x])
    if ik[2] == 0:
        return _rows([]), UNDEF_NO_BASE, trace
    ik = ik + (x + 1,)
    curr = []
    i = x + 1
    while i < L:   # forward sweep
        c = comp6(q[i])
        ok = ix.extend(ik, 0)
        if ok[c][2] != ik[2]:
            if ik[2] != ok[0][2]:
                curr.append(ik)
            if not sm and ok[0][2]:
                curr.append(ok[0] + (i,))
        if (ok[c][2] < 2) if sm else (ok[c][2] == 0):
            break
        ik = ok[c] + (i + 1,)
        i += 1
    if i == L:
        curr.append(ik)
        if not sm:
            ok = ix.extend(ik, 0)
            if ok[0][2]:
                curr.append(ok[0] + (L,))
    trace["fwd_len"] = len(curr)
    if not curr:
        return _rows([]), UNDEF_EMPTY_FWD, trace
    curr.reverse()
    ret = curr[0][3]
    prev = np.array(curr, dtype=np.int64)
    mem = []
    i = x - 1
    while i >= -1:   # backward sweep over the whole list
        c = 0 if i < 0 else q[i]
        trace["rounds"] += 1
        if i == -1:
            trace["last_prev"] = len(prev)
            trace["last_from_fwd"] = x == 0
        child, s0 = ix.extend_back_many(prev, c)
        sc = child[:, 2]
        closed = prev[:, 1] < ix.n_seq
        fl_match = (s0 != 0) & closed
        cont = sc > 1 if sm else sc != 0
        if i != -1 and cont.all() and not fl_match.any() and (closed[1:] | (sc[1:] != sc[:-1])).all():
            # no interval ends in this round and no open child has the size of the child before it: the loop below would report
            # nothing and keep every child (by induction over j).  A long list of a nested index spends most of its rounds here.
            keep = range(len(prev))
        else:
            keep = []
            sc_l, cont_l, fl_l, closed_l = sc.tolist(), cont.tolist(), fl_match.tolist(), closed.tolist()
            for j in range(len(prev)):
                if i == -1 and 0 < j < 64 and keep and not closed_l[j]:
                    trace["last_open_skipped"] += 1
                if not cont_l[j] or fl_l[j] or i == -1:
                    if not keep or fl_l[j]:
                        if fl_l[j] or not mem or i + 1 < (mem[-1][3] >> 32 & 0x3fffffff):
                            p = prev[j].tolist()
                            mem.append((p[0], p[1], p[2], p[3] | (int(s0[j]) != 0) << 63 | (i + 1) << 32))
                if cont_l[j] and (closed_l[j] or not keep or sc_l[j] != sc_l[keep[-1]]):
                    keep.append(j)
        trace["max_curr"] = max(trace["max_curr"], len(keep))
        if len(keep) == 0:
            break
        prev = child[list(keep)] if not isinstance(keep, range) else child
        i -= 1
    mem.reverse()
    return _rows(mem), ret, trace


def chain(ix, q, self_match, start=0, stop=None):
    """fm6_smem from `start` while x < stop -> (mem, calls, undefined).  calls: (x, ret, n, trace) of every defined call;
    undefined: None, or the marker of the start that ended the walk (mem then holds the SMEMs found before it)."""
    L = len(q)
    stop = L if stop is None else min(stop, L)
    out, calls = [_rows([])], []
    x = start
    if L > 0 and x < stop:
        while True:
            mem, ret, tr = smem1(ix, q, x, self_match)
            if isinstance(ret, str):
                return np.concatenate(out), calls, ret
            out.append(mem)
            calls.append((x, ret, len(mem), tr))
            x = ret
            if x >= stop:
                break
    return np.concatenate(out), calls, None


def full_rows(ix, mem):
    """what FMD_SMEM_WIN_F_FULL keeps: the rows closed by a sentinel on both sides, in order"""
    return mem[(mem["info"] >> np.uint64(63) != 0) & (mem["x"][:, 1] < ix.n_seq)]


def exact_record(name, length, mem, n_seq):
    """what `fermi exact` prints for one query (cmd.c:320-327, smem.c:412-418), without the closing "//" line"""
    out = [b"SQ\t%s\t%d\t%d" % (name, length, len(mem))]
    for r in mem:
        info = int(r["info"])
        out.append(b"EM\t%d\t%d\t%d\t%s%s" % (info >> 32 & 0x3fffffff, info & 0x3fffffff, min(int(r["x"][2]), 0xffffffff),
                                                b"OT"[info >> 63:(info >> 63) + 1], b"OT"[int(r["x"][1]) < n_seq:][:1]))
    return b"\n".join(out) + b"\n"


# ---- the cases -------------------------------------------------------------------------------------------------------------------
SEED = 20261
A, C_, G, T, N = 1, 2, 3, 4, 5


class Cases:
    """Three indexes and their queries.
    nested:     R = 120 random bases; reads R[:k] (k = 1..120), R[1:k] (k = 2..120), 50 random 30-mers, one of them with an N
    nested_non: the same without the 30-mer that holds the N: no N in the index
    nested300:  R = 300 bases nested the same way, 20 random 30-mers and the read "N": every occurrence of N ends its sequence"""

    def __init__(self, seed=SEED):
        rng = np.random.default_rng(seed)
        b = lambda n: rng.integers(1, 5, n).astype(np.uint8)
        R = b(120)
        mers = [b(30) for _ in range(50)]
        self.n_mer = 17
        mers[self.n_mer][11] = N
        nest = [R[:k] for k in range(1, 121)] + [R[1:k] for k in range(2, 121)]
        R3 = b(300)
        self.R, self.R3, self.mers = R, R3, mers
        self.reads = {
            "nested": nest + mers,
            "nested_non": nest + [m for i, m in enumerate(mers) if i != self.n_mer],
            "nested300": [R3[:k] for k in range(1, 301)] + [R3[1:k] for k in range(2, 301)] + [b(30) for _ in range(20)] + [np.array([N], dtype=np.uint8)],
        }
        junk = b(6)
        q2500 = np.concatenate([m[:25] for m in mers] + [m[3:28] for m in mers])
        last = np.concatenate([mers[0][:20], [mers[0][20] % 4 + 1]]).astype(np.uint8)
        rn = R[:40].copy()
        with_n = []
        for p in (0, 20, 39):
            v = rn.copy(); v[p] = N
            with_n.append(v)
        self.queries = {
            "nested": {"R": R, "junk_R": np.concatenate([junk, R]), "q2500": q2500, "len1": R[:1].copy(), "len0": np.zeros(0, dtype=np.uint8),
                       "last_base_start": last, "R_tail": R[60:].copy(), "mer_N": mers[self.n_mer].copy()},
            "nested_non": {"R_head": rn, "N_first": with_n[0], "N_middle": with_n[1], "N_last": with_n[2]},
            "nested300": {"R300": R3, "N_then_bases": np.concatenate([[N], R3[:12]]).astype(np.uint8), "bases_N_bases": np.concatenate([R3[:9], [N], R3[40:49]]).astype(np.uint8)},
        }
        # the undefined starts, by name: (index, query, x, self_match) -> marker.  Everything else goes to the oracle.
        self.undefined = {}
        for name, p in (("N_first", 0), ("N_middle", 20), ("N_last", 39)):
            for sm in (0, 1):
                self.undefined[("nested_non", name, p, sm)] = UNDEF_NO_BASE
        self.undefined[("nested300", "N_then_bases", 0, 1)] = UNDEF_EMPTY_FWD
        self.undefined[("nested300", "bases_N_bases", 9, 1)] = UNDEF_EMPTY_FWD
        # the long query of `exact`: more than 4096 bases around R300
        self.long_query = np.concatenate([b(2000), R3, b(1900)])

    @functools.lru_cache(maxsize=None)
    def bwt(self, index):
        return bwt_by_sorting_ragged(self.reads[index])

    @functools.lru_cache(maxsize=None)
    def ref(self, index):
        return RefIndex(self.bwt(index))

    @functools.lru_cache(maxsize=None)
    def single(self, index, name, sm):
        """smem1 at every start x of a query: list of (mem, ret, trace)"""
        q = self.queries[index][name]
        return [smem1(self.ref(index), q, x, sm) for x in range(len(q))]

    @functools.lru_cache(maxsize=None)
    def whole(self, index, name, sm):
        return chain(self.ref(index), self.queries[index][name], sm)

    def names(self):
        return [(ix, nm) for ix in self.queries for nm in self.queries[ix]]


@functools.lru_cache(maxsize=None)
def cases():
    return Cases()
