"""A periodic symbol string with exact counts in closed form: the reference of tests/test_gpu_layout_seams.py.

Rank, LF, fm6_extend and the backward-search recurrence are arithmetic on symbol counts, and the device layout is a way of storing those counts, so an index
can be checked at any size against a string whose counts need no index at all: s[p] = pat[p % P] for p < n has
    occ(k) = (k + 1) // P * comp + prefix[(k + 1) % P]
($, A, C, G, T, N in s[0..k]; comp = the counts of one period, prefix[i] = those of pat[:i]).  The string is not the BWT of any text -- none of the operations
checked here cares.  This generalises rank_closed of tools/huge_index_check.py (whose four bases alternate, so that their counts, and with them every packed
field of the layout, are equal) to arbitrary patterns: a heavy base, unequal shares, a base that does not occur.

Arithmetic is int64: every count is at most n < 2^40 (the layout's own limit) and no product occurs beyond (k + 1) // P * comp[c] <= k + 1.  occ_int is the same
formula in Python integers, for the test that says so (tests/test_periodic_ref.py).  No GPU, and torch only inside device_string."""
import numpy as np

P_DEFAULT = 1009   # prime: every phase of the period against the 32-, 64- and 96-position structures of the layout occurs
I64 = np.int64


def make_pattern(shares, seed, P=P_DEFAULT):
    """pat[0] = '$' (0), pat[1] = 'N' (5) -- exactly one of each per period unless `shares` adds Ns -- the rest drawn from default_rng(seed) with
    probabilities `shares` over the symbols 1..5 (A, C, G, T, N)."""
    shares = np.asarray(shares, dtype=np.float64)
    assert shares.shape == (5,) and abs(shares.sum() - 1.0) < 1e-9
    rng = np.random.default_rng(seed)
    pat = np.empty(P, dtype=np.uint8)
    pat[0], pat[1] = 0, 5
    pat[2:] = rng.choice(np.arange(1, 6, dtype=np.uint8), size=P - 2, p=shares)
    return pat


def heavy_shares(c, share):
    """`share` of symbol c (1..5), the rest in equal parts to the other bases A/C/G/T (N, unless it is the heavy one, stays at pat[1] alone)"""
    others = [b for b in (1, 2, 3, 4) if b != c]
    s = np.zeros(5)
    s[c - 1] = share
    for b in others:
        s[b - 1] = (1.0 - share) / len(others)
    return s


class Periodic:
    def __init__(self, pat, n):
        self.pat = np.ascontiguousarray(pat, dtype=np.uint8)
        assert self.pat.ndim == 1 and len(self.pat) > 0 and int(self.pat.max()) <= 5
        self.P = len(self.pat)
        self.n = int(n)
        assert 0 < self.n < (1 << 62)
        self.prefix = np.zeros((self.P + 1, 6), dtype=I64)       # prefix[i] = the counts of pat[:i]
        np.cumsum(self.pat[:, None] == np.arange(6)[None, :], axis=0, out=self.prefix[1:])
        self.comp = self.prefix[self.P].copy()
        self.mcnt = self.occ(self.n - 1)                         # the six marginal counts
        self.cnt = np.zeros(7, dtype=I64)                        # the C array: cnt[c] = symbols smaller than c (rld.c:282-284)
        np.cumsum(self.mcnt, out=self.cnt[1:])

    # ---- counts
    def occ(self, k):
        """the six counts of s[0..k] for every k of an integer array (any shape; -1 gives zeros): int64, shape k.shape + (6,)"""
        m = np.asarray(k, dtype=I64) + 1                         # symbols counted
        assert (m >= 0).all() and (m <= self.n).all()
        return (m // self.P)[..., None] * self.comp + self.prefix[m % self.P]

    def occ_int(self, k):
        """occ of ONE k in Python integers (no width to overflow): a list of six"""
        q, r = divmod(int(k) + 1, self.P)
        return [q * int(self.comp[c]) + int(self.prefix[r, c]) for c in range(6)]

    def occ1(self, k, c):
        """count of symbol c[i] in s[0..k[i]] (k, c of the same shape)"""
        m = np.asarray(k, dtype=I64) + 1
        c = np.asarray(c, dtype=np.intp)
        return m // self.P * self.comp[c] + self.prefix[m % self.P, c]

    def sym(self, p):
        return self.pat[np.asarray(p, dtype=I64) % self.P]

    def lf(self, p):
        """cnt[c] + occ(p)[c] - 1 with c = s[p]: the row one LF step on (exact.c:63-66)"""
        p = np.asarray(p, dtype=I64)
        c = self.sym(p).astype(np.intp)
        return self.cnt[c] + self.occ1(p, c) - 1

    def crossing(self, c, v):
        """the first position at which the count of c reaches v (v >= 1); None when it never does"""
        v = int(v)
        assert v >= 1
        if int(self.mcnt[c]) < v:
            return None
        lo, hi = 0, self.n - 1                                   # occ(hi)[c] >= v
        while lo < hi:
            mid = (lo + hi) // 2
            if int(self.occ(mid)[c]) >= v:
                hi = mid
            else:
                lo = mid + 1
        return lo

    # ---- fm_backward_search (exact.c:7-23) with occ in place of rld_rank21
    def backward_search(self, pats, lens, table_depth=0):
        """pats: (m, Lmax) symbols, row i = a pattern of lens[i] >= 1 symbols, searched from its last one.  Returns a dict:
            hit, k, l               per pattern: does it occur, and its interval where it does (zeros where not)
            step_pat, step_left, step_k, step_l, step_c1, step_c2
                                    one row per PAIR-ELIGIBLE step, i.e. per state of a search (interval [k, l] not empty, `left` symbols still to take) with
                                    left >= 2, left even and l - k < 64 -- the rule by which k_bsearch<1> hands a search to k_bsearch_pair (fmd_ops.hip), which then
                                    takes c1 = the next symbol and c2 = the one after it from the two-base block of k
        table_depth = D > 0: a pattern of at least D symbols whose last D are all A/C/G/T is D symbols in before its first state (the device starts such a search
        from its prefix table), so states inside those D symbols are not steps."""
        pats = np.asarray(pats, dtype=np.uint8)
        lens = np.asarray(lens, dtype=I64)
        m = len(lens)
        assert pats.shape[0] == m and (lens >= 1).all() and (lens <= pats.shape[1]).all()
        rows = np.arange(m)
        c = pats[rows, lens - 1].astype(np.intp)
        k = self.cnt[c].copy()
        l = self.cnt[c + 1] - 1
        left = lens - 1
        alive = k <= l
        first_state = lens - 1                                   # a state counts as a step when left <= first_state
        if table_depth > 0:
            idx = np.clip(lens[:, None] - 1 - np.arange(table_depth)[None, :], 0, None)
            tail = pats[rows[:, None], idx]
            acgt = (lens >= table_depth) & ((tail >= 1) & (tail <= 4)).all(axis=1)
            first_state = np.where(acgt, lens - table_depth, first_state)
        steps = {key: [] for key in ("pat", "left", "k", "l", "c1", "c2")}
        while True:
            go = alive & (left >= 1)
            if not go.any():
                break
            e = go & (left >= 2) & (left % 2 == 0) & (l - k < 64) & (left <= first_state)
            if e.any():
                i = np.nonzero(e)[0]
                steps["pat"].append(i); steps["left"].append(left[i]); steps["k"].append(k[i]); steps["l"].append(l[i])
                steps["c1"].append(pats[i, left[i] - 1]); steps["c2"].append(pats[i, left[i] - 2])
            i = np.nonzero(go)[0]
            c = pats[i, left[i] - 1].astype(np.intp)
            nk = self.cnt[c] + self.occ1(k[i] - 1, c)
            nl = self.cnt[c] + self.occ1(l[i], c) - 1
            k[i] = nk; l[i] = nl
            left[i] -= 1
            alive[i] = nk <= nl
        out = {"hit": alive, "k": np.where(alive, k, 0), "l": np.where(alive, l, 0)}
        for key, v in steps.items():
            out["step_" + key] = np.concatenate(v).astype(I64) if v else np.zeros(0, dtype=I64)
        return out

    # ---- fm6_extend (exact.c:72-88) with occ in place of rld_rank2a
    def extend(self, x, is_back):
        """x: (m, 3) bi-intervals {x[0], x[1], x[2]} (the layout of INTV_DT, fermi_amd/api.py), is_back: (m,).  Returns (m, 6, 3): the six intervals ok[c].x"""
        x = np.asarray(x, dtype=I64)
        b = np.asarray(is_back).astype(bool)
        m = len(x)
        rows = np.arange(m)
        o = np.where(b, 0, 1)                                    # x[!is_back] is the strand ranked
        a = x[rows, o]
        tk = self.occ(a - 1)
        tl = self.occ(a - 1 + x[:, 2]) - tk
        ok = np.zeros((m, 6, 3), dtype=I64)
        ranked = self.cnt[:6][None, :] + tk
        other = np.zeros((m, 6), dtype=I64)
        other[:, 0] = x[rows, 1 - o]                             # ok[0].x[is_back] = ik.x[is_back], then the running sum in the order $, T, G, C, A, N
        other[:, 4] = other[:, 0] + tl[:, 0]
        other[:, 3] = other[:, 4] + tl[:, 4]
        other[:, 2] = other[:, 3] + tl[:, 3]
        other[:, 1] = other[:, 2] + tl[:, 2]
        other[:, 5] = other[:, 1] + tl[:, 1]
        ok[:, :, 0] = np.where(b[:, None], ranked, other)
        ok[:, :, 1] = np.where(b[:, None], other, ranked)
        ok[:, :, 2] = tl
        return ok

    # ---- the string itself
    def materialise(self):
        """the string as a numpy array (small n only)"""
        return self.pat[np.arange(self.n, dtype=I64) % self.P]

    def device_string(self, torch_device):
        """the string as a uint8 tensor in HBM, made in chunks of at most 2^30 positions (as tools/huge_index_check.py makes its own)"""
        import torch
        pat_dev = torch.from_numpy(self.pat).to(torch_device)
        s = torch.empty(self.n, dtype=torch.uint8, device=torch_device)
        step = 1 << 30
        for o in range(0, self.n, step):
            c = min(step, self.n - o)
            p = torch.arange(o, o + c, dtype=torch.int64, device=torch_device)
            p %= self.P
            s[o:o + c] = pat_dev[p]
            del p
        torch.cuda.synchronize(torch_device)
        torch.cuda.empty_cache()
        return s


def draw_patterns(rng, m, shares4, max_len=48):
    """m search patterns: lengths uniform in 1..max_len, bases A/C/G/T with probability (shares4 + 1/4) / 2 each.  Returns (pats (m, max_len), lens)."""
    shares4 = np.asarray(shares4, dtype=np.float64)
    p = 0.5 * shares4 / shares4.sum() + 0.125
    lens = rng.integers(1, max_len + 1, m).astype(I64)
    pats = rng.choice(np.arange(1, 5, dtype=np.uint8), size=(m, max_len), p=p)
    return pats, lens
