"""The read sets of the kbubble tests (tests/test_kbubble_host.py on the CPU, tests/test_gpu_kbubble.py on the GPU), made once and never changed: the hand-made
negative controls, the indel, the planted variants with the check that the Python restatement (tests/kbubble_ref.py) recovers exactly them, and the
low-complexity fuzz.  Every case is (colours, k, min_occ): N lists of strings.  Nothing here calls the library."""
import random

import kgraph_ref as R
import kbubble_ref as BR

# flanks at k = 5 in which no 4-mer repeats, on either strand, within or between them (checked by test_the_flanks_are_clean)
L5, R5, Q5, X5, Y5 = "GACTTGCATAC", "TGGAGATCGTT", "CCGCTAAGGTG", "AAGAACC", "CAGTCAT"


def controls():
    """name -> (colours, k, min_occ): each gives NO bubble, for the reason its name says"""
    out = {}
    # s has three right arcs (the third path never comes back); t has two left arcs
    out["fork_of_three"] = ([[L5 + "A" + R5, L5 + "C" + R5, L5 + "G" + Q5]], 5, 1)
    # the mirror: a third path joins at t, which then has three left arcs
    out["join_of_three"] = ([[L5 + "A" + R5, L5 + "C" + R5, Q5 + "G" + R5]], 5, 1)
    # a dead end leaves the middle of allele A: one of its nodes has two right arcs
    a = L5 + "A" + R5
    out["tip_on_an_allele"] = ([[a, L5 + "C" + R5, a[9:15] + "CC"]], 5, 1)
    # A ends in T forward, B in T reversed; T has two left arcs on either side
    T = "GGTCTCA"
    out["opposite_target"] = ([[L5 + "A" + T, L5 + "C" + R.rc(T), X5 + T, Y5 + R.rc(T)]], 5, 1)
    # both branches of s end in s ^ 1: the read S W rc(S) beside its own reverse complement S rc(W) rc(S)
    S, W = "GACTTGC", "ATACCGA"
    out["s_and_t_on_one_node"] = ([[S + W + R.rc(S)]], 5, 1)
    return out


def indel(k, d):
    """one deletion of d bases between two colours: branches of k - 1 and k - 1 + d nodes"""
    rng = random.Random(1000 * k + d)
    while True:
        left, right, ins = ("".join(rng.choice("ACGT") for _ in range(m)) for m in (3 * k, 3 * k, d))
        both = left + ins + right
        words = [both[i:i + k - 1] for i in range(len(both) - k + 2)]
        words += [R.rc(w) for w in words]
        if len(set(words)) == len(words) and ins[0] != right[0] and ins[-1] != left[-1]:
            return [[left + right], [left + ins + right]], left, ins, right


def tiles(genome, length, step, flip):
    """error-free reads that tile the genome, every other one (from `flip` on) reverse-complemented"""
    starts = list(range(0, len(genome) - length, step)) + [len(genome) - length]
    return [R.rc(genome[a:a + length]) if (i + flip) % 2 else genome[a:a + length] for i, a in enumerate(starts)]


class Planted:
    """a random genome A and a copy B with n_sub substitutions and n_indel insertions / deletions of 1 to 4 bases, at least `apart` bases apart"""

    def __init__(self, seed, size=3000, n_sub=30, n_indel=10, k_max=31):
        rng = random.Random(seed)
        self.A = "".join(rng.choice("ACGT") for _ in range(size))
        apart, n = 2 * k_max + 2 + 4, n_sub + n_indel   # from position to position: 2 k + 2 bases and more between two sites for every k, whatever an indel takes
        slack = size - 240 - (n - 1) * apart
        assert slack >= 0
        cuts = sorted(rng.randrange(slack + 1) for _ in range(n))
        spots = [120 + x * apart + c for x, c in enumerate(cuts)]
        kinds = ["sub"] * n_sub + ["ins"] * (n_indel // 2) + ["del"] * (n_indel - n_indel // 2)
        rng.shuffle(kinds)
        self.sites, out, at = [], [], 0                 # a site: (kind, position in A, the bases changed: new base / inserted / deleted)
        for p, kind in zip(spots, kinds):
            out.append(self.A[at:p])
            if kind == "sub":
                new = rng.choice([c for c in "ACGT" if c != self.A[p]])
                out.append(new); at = p + 1
                self.sites.append((kind, p, self.A[p] + new))
            elif kind == "ins":
                s = "".join(rng.choice("ACGT") for _ in range(rng.randrange(1, 5)))
                out.append(s); at = p
                self.sites.append((kind, p, s))
            else:
                m = rng.randrange(1, 5)
                at = p + m
                self.sites.append((kind, p, self.A[p:p + m]))
        out.append(self.A[at:])
        self.B = "".join(out)
        # C: A with every other site of B -- every (k+1)-mer of C is one of A or of B, the sites being more than k + 1 apart
        out, at = [], 0
        for x, (kind, p, s) in enumerate(self.sites):
            if x % 2:
                continue
            out.append(self.A[at:p])
            if kind == "sub":
                out.append(s[1]); at = p + 1
            elif kind == "ins":
                out.append(s); at = p
            else:
                at = p + len(s)
        out.append(self.A[at:])
        self.C = "".join(out)

    def colours(self, n):
        """n read sets: A, B, then C, A, B .. with other strands; with n > 2 the last but one is an empty colour"""
        sets = [tiles(g, 100, 25, f) for g, f in ((self.A, 0), (self.B, 1), (self.C, 0), (self.A, 1), (self.B, 0), (self.C, 1), (self.A, 0))][:n if n <= 2 else n - 1]
        if n > 2:
            sets.insert(n - 2, [])
        return sets

    def check(self, G, recs):
        """the records are exactly the planted sites, each once, with the planted alleles up to where an indel in a repeat is put and to the strand"""
        assert len(recs) == len(self.sites), (len(recs), len(self.sites))
        seen = set()
        for rec in recs:
            kind, left, a0, a1, right = BR.alleles(G, rec)
            hap = [left + (a if a != "-" else "") + right for a in (a0, a1)]
            hit = None
            for flip in (0, 1):
                h = [R.rc(x) for x in hap] if flip else hap
                for in_a, in_b in ((0, 1), (1, 0)):
                    if self.A.count(h[in_a]) == 1 and self.B.count(h[in_b]) == 1 and h[in_a] not in self.B and h[in_b] not in self.A:
                        assert hit is None
                        hit = (self.A.index(h[in_a]), len(h[in_a]), [a0, a1][in_a], [a0, a1][in_b], flip)
            assert hit is not None, rec
            at, ln, al_a, al_b, flip = hit
            site = [x for x, (_, p, _) in enumerate(self.sites) if at <= p < at + ln]
            assert len(site) == 1 and site[0] not in seen, (rec, site)
            seen.add(site[0])
            skind, p, s = self.sites[site[0]]
            turn = (lambda x: R.rc(x)) if flip else (lambda x: x)
            if skind == "sub":
                assert kind == "SNP" and (turn(al_a), turn(al_b)) == (s[0], s[1]), (rec, self.sites[site[0]])
            else:
                gone, there = (al_a, al_b) if skind == "ins" else (al_b, al_a)
                assert kind == "INDEL" and gone == "-" and len(there) == len(s) and turn(there) in (s + s), (rec, self.sites[site[0]], there)
        assert len(seen) == len(self.sites)


PLANTED_SEED = 8     # a seed for which the restatement recovers exactly the planted sites at k = 11, 21 and 31 (a 3 kb genome repeats a few 11-mers)


def fuzz(seed):
    """low-complexity reads over three letters with short repeats: dense tangles in which most forks are no bubbles"""
    rng = random.Random(seed)
    units = ["".join(rng.choice("ACG") for _ in range(rng.randrange(2, 6))) for _ in range(4)]
    genome = "".join(rng.choice(units) if rng.random() < 0.6 else rng.choice("ACG") for _ in range(60))
    colours = [[], []]
    for _ in range(24):
        a = rng.randrange(max(1, len(genome) - 25))
        r = genome[a:a + rng.randrange(8, 26)]
        if rng.random() < 0.3 and len(r) > 2:
            p = rng.randrange(len(r))
            r = r[:p] + rng.choice("ACG") + r[p + 1:]
        r = R.rc(r) if rng.random() < 0.5 else r
        colours[rng.randrange(2)].append(r)
        if rng.random() < 0.3:
            colours[rng.randrange(2)].append(r)
    return colours


FUZZ_SEEDS = tuple(range(20))
