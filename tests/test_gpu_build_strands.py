"""GPU: fmd_build_bwt_strands (csrc/fmd_build.hip) -- the BWT of the forward strands, of the reverse complements, or of both, as `fermi ropebwt
[-F] [-R]` inserts them (ropebwt.c:22-45) -- against a restatement written here: lay the text out, sort its suffixes as (tail up to and
including the '$', sequence index), take the symbol in front of each.  Every case runs through the one-shot path in this process and again
through the bucketed path (FMD_BUILD_BUCKETED=1, at the depth the builder chooses and at depth 3) in ONE fresh child process, which is this
file run as a program."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FWD, REV, BOTH = 1, 2, 3
STRANDS = {"FWD": FWD, "REV": REV, "BOTH": BOTH}


def _cases():
    rng = np.random.default_rng(20261018)
    base = lambda n: rng.integers(1, 5, n).astype(np.uint8)
    genome = base(400)                       # reads that overlap: long common prefixes, ties between the strands of neighbours
    def draw(ln):
        a = int(rng.integers(0, len(genome) - ln + 1))
        return genome[a:a + ln].copy()
    c = {}
    c["one_base"] = [np.array([3], dtype=np.uint8)]
    c["uniform21"] = [draw(21) for _ in range(300)]          # a sequence is 22 symbols: the second key chunk holds the '$' alone
    c["uniform20"] = [draw(20) for _ in range(300)]          # the '$' is the last symbol of the first chunk
    ragged = [draw(int(rng.integers(1, 65))) for _ in range(300)]
    ragged[0] = draw(64); ragged[1] = draw(1); ragged[2] = draw(42); ragged[3] = draw(43)   # 63 = 3 * 21 symbols to the '$', and one more
    if sum(len(r) for r in ragged) % 2 == 0:
        ragged.append(draw(33))
    c["ragged"] = ragged                                      # an odd number of bases: the one-strand text is odd too, sequences start at any alignment
    with_n = [draw(int(rng.integers(5, 50))) for _ in range(120)]
    for r in with_n[::3]:
        r[rng.integers(0, len(r), 2)] = 5
    with_n.append(np.full(23, 5, dtype=np.uint8))
    c["with_N"] = with_n
    c["copies"] = [genome[17:17 + 30].copy() for _ in range(200)]     # ties decided by the sequence index alone
    empties = [draw(int(rng.integers(1, 30))) for _ in range(40)]
    for i in (0, 7, 8, 39):
        empties[i] = np.zeros(0, dtype=np.uint8)
    c["some_empty"] = empties                                 # a read of no bases is a '$' alone (bprope6.c:218-224)
    c["all_empty"] = [np.zeros(0, dtype=np.uint8)] * 5
    return c


CASES = _cases()
NO_EMPTY = [k for k in CASES if "empty" not in k]


def _comp(r):
    return np.where((r >= 1) & (r <= 4), 5 - r, r).astype(np.uint8)


def restate(reads, strands):
    """the text of the chosen strands, every sequence closed by its '$' (0); suffixes sorted by (tail up to the '$', sequence); the symbols in front"""
    seqs = []
    for r in reads:
        if strands & FWD:
            seqs.append(bytes(r))
        if strands & REV:
            seqs.append(bytes(_comp(r)[::-1]))
    text = b"".join(s + b"\0" for s in seqs)
    keys, t = [], 0
    for i, s in enumerate(seqs):
        whole = s + b"\0"
        keys += [(whole[j:], i, t + j) for j in range(len(whole))]
        t += len(whole)
    keys.sort()
    assert len(keys) == len(text)
    return np.array([text[p - 1] for _, _, p in keys], dtype=np.uint8)       # (p = 0: the last symbol, a '$')


_want = {}


def want(case, strands):
    if (case, strands) not in _want:
        _want[(case, strands)] = restate(CASES[case], strands)
    return _want[(case, strands)]


def build(api, reads, strands):
    """fmd_build_bwt_strands through ctypes -> (return code, BWT)"""
    flat, off = api.flatten_reads(reads)
    n = len(off) - 1
    bwt = np.full(2 * (int(off[n]) + n) + 8, 0xee, dtype=np.uint8)
    n_sym = C.c_uint64(0)
    rc = api.lib().fmd_build_bwt_strands(0, n, flat.ctypes.data, off.ctypes.data, strands, bwt.ctypes.data, C.byref(n_sym))
    assert rc != 0 or (bwt[n_sym.value:] == 0xee).all()        # nothing behind the n_sym symbols was touched
    return rc, bwt[:n_sym.value].copy()


@pytest.mark.parametrize("strands", sorted(STRANDS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_one_shot_path_equals_the_restatement(gpu, case, strands):
    reads = CASES[case]
    rc, bwt = build(gpu, reads, STRANDS[strands])
    assert rc == 0
    total = sum(len(r) for r in reads) + len(reads)
    assert len(bwt) == (2 * total if strands == "BOTH" else total)
    assert np.array_equal(bwt, want(case, STRANDS[strands]))


@pytest.fixture(scope="module")
def bucketed(gpu, tmp_path_factory):
    """every case and strand set through the bucketed path, in one fresh process (the switch is read through getenv)"""
    out = str(tmp_path_factory.mktemp("strands") / "bucketed.npz")
    env = dict(os.environ, FMD_BUILD_BUCKETED="1")
    env.pop("FMD_BUILD_DEPTH", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return dict(np.load(out))


@pytest.mark.parametrize("depth", ["auto", "3"])
@pytest.mark.parametrize("strands", sorted(STRANDS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_bucketed_path_equals_the_restatement(bucketed, case, strands, depth):
    assert np.array_equal(bucketed["%s.%s.%s" % (case, strands, depth)], want(case, STRANDS[strands]))


@pytest.mark.parametrize("case", NO_EMPTY)
def test_both_strands_is_fmd_build_bwt_byte_for_byte(gpu, case):
    rc, bwt = build(gpu, CASES[case], BOTH)
    assert rc == 0 and np.array_equal(bwt, gpu.build_bwt(CASES[case]))
    assert np.array_equal(gpu.build_bwt_strands(CASES[case], gpu.STRAND_BOTH), bwt)


def test_bad_strand_sets_and_arguments(gpu):
    reads = CASES["uniform20"][:4]
    for bad in (0, 4, 7, 0x11):
        assert build(gpu, reads, bad)[0] == gpu.FMD_E_ARG
    flat, off = gpu.flatten_reads(reads)
    d_bwt, n_sym = C.c_void_p(), C.c_uint64()
    L = gpu.lib()
    for bad in (0, 4):     # the device form looks at the strand set before it touches a pointer
        assert L.fmd_build_bwt_strands_dev(0, None, 4, flat.ctypes.data, off.ctypes.data, 80, 20, 1, bad, C.byref(d_bwt), C.byref(n_sym)) == gpu.FMD_E_ARG
    assert L.fmd_build_bwt_strands(0, 0, flat.ctypes.data, off.ctypes.data, FWD, flat.ctypes.data, C.byref(n_sym)) == gpu.FMD_E_ARG
    # fmd_build_bwt keeps refusing a read of no bases; the strand form takes it
    with pytest.raises(gpu.FmdError):
        gpu.build_bwt(CASES["some_empty"])


def test_sentinel_rows_follow_insertion_order(gpu):
    """the first n_seq rows of the BWT are the suffixes that are a '$' alone, in insertion order: row i holds the last base of sequence i"""
    reads = CASES["ragged"]
    for s, pick in ((FWD, lambda r: r[-1]), (REV, lambda r: _comp(r)[::-1][-1])):
        rc, bwt = build(gpu, reads, s)
        assert rc == 0 and list(bwt[:len(reads)]) == [pick(r) for r in reads]


def _child(out):
    sys.path.insert(0, ROOT)
    from fermi_amd import api
    assert os.environ.get("FMD_BUILD_BUCKETED") == "1"
    res = {}
    for depth in ("auto", "3"):
        if depth != "auto":
            os.environ["FMD_BUILD_DEPTH"] = depth
        for case, reads in CASES.items():
            for name, s in STRANDS.items():
                rc, bwt = build(api, reads, s)
                assert rc == 0, (case, name, depth, rc)
                res["%s.%s.%s" % (case, name, depth)] = bwt
    np.savez(out, **res)


if __name__ == "__main__":
    _child(sys.argv[1])
