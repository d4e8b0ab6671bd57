"""GPU: contrast assembly (fmd_contrast.hip, host/contrast_cmd.c) -- `fermi-amd contrast` and `sub` against the bytes the reference
writes (tests/golden/make_golden_contrast.py: two related samples ctA / ctB, their error-free twins cnA / cnB), the C ABI by hand on
ragged reads with Ns, the overflow / re-run path of the walk, a mid-size pair against the reference binary, the CLI's errors."""
import ctypes as C
import hashlib
import os
import subprocess
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "fermi")

# (pair, -k, -o) -> reads selected from the first / the second sample, of 3000 sequences each (`fermi contrast`)
CASES = {
    ("ct", 25, 2): (860, 904), ("ct", 55, 3): (510, 554), ("ct", 17, 1): (1080, 1146), ("ct", 31, 5): (334, 314), ("cn", 25, 2): (260, 298),
}
# `fermi sub` / `fermi sub -c` of ctA.fmd with contrast.<tag>.ctA-ctB.sub
SUB_MD5 = {
    "sub.k25o2.ctA": "9493c78e19e33b40f98247b3284543fb", "subc.k25o2.ctA": "9d61620366c1ef72535afb55e51bb826",
    "sub.k55o3.ctA": "e18b44dd3b12d24bf894744f7e9319c5", "subc.k55o3.ctA": "935698b0ed12745f4f66e2429f4499f9",
}
TINY_MD5 = "c6119facb2001a7abb624e33028e90d0"          # tiny.fmd = `fermi recode tiny.rle.fmd`
EMPTY_MD5 = "f6206ca009f1339b63551fec7f6a4233"         # sub.empty.fmd


def _g(name):
    return os.path.join(GOLD, name)


def _md5(b):
    return hashlib.md5(b).hexdigest()


def _run(args, timeout=120, **kw):
    return subprocess.run([AMD] + args, capture_output=True, timeout=timeout, **kw)


def _contrast(tmp_path, a, b, k, o, extra=(), tag="x"):
    oa, ob = str(tmp_path / ("%s.%s-%s.sub" % (tag, a, b))), str(tmp_path / ("%s.%s-%s.sub" % (tag, b, a)))
    p = _run(["contrast", "-k", str(k), "-o", str(o)] + list(extra) + [_g(a + ".fmd"), _g(a + ".rank"), oa, _g(b + ".fmd"), _g(b + ".rank"), ob])
    sel = [int(ln.split()[1]) for ln in p.stderr.decode().splitlines() if ln.startswith("[M::main_contrast]") and "reads selected from" in ln]
    return p, oa, ob, sel


def _conv(bits, rank_path, n):
    """fm6_sub_conv (cmp.c:128-144): bit i -> bit rank[i] >> 2"""
    rank = np.fromfile(rank_path, np.uint64)[:n]
    on = np.unpackbits(bits.view(np.uint8), bitorder="little")[:n].astype(bool)
    out = np.zeros((n + 63) // 64 * 64, np.uint8)
    out[(rank[on] >> np.uint64(2)).astype(np.int64)] = 1
    return np.packbits(out, bitorder="little").view(np.uint64)


def _fixture_bits(name):
    b = open(_g(name), "rb").read()
    return np.frombuffer(b[8:], np.uint64)


@pytest.mark.parametrize("pair,k,o", sorted(CASES))
def test_contrast_cli_writes_the_reference_bytes(gpu, tmp_path, pair, k, o):
    a, b = pair + "A", pair + "B"
    tag = "k%do%d" % (k, o)
    want_a, want_b = open(_g("contrast.%s.%s-%s.sub" % (tag, a, b)), "rb").read(), open(_g("contrast.%s.%s-%s.sub" % (tag, b, a)), "rb").read()
    p, oa, ob, sel = _contrast(tmp_path, a, b, k, o, extra=["-t", "1"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    print(pair, k, o, "selected", sel)
    assert open(oa, "rb").read() == want_a and open(ob, "rb").read() == want_b
    assert tuple(sel) == CASES[(pair, k, o)]
    assert "reads selected from %s" % _g(a + ".fmd") in p.stderr.decode()
    # the operands swapped, -t 16: the files swapped
    p, ob2, oa2, sel = _contrast(tmp_path, b, a, k, o, extra=["-t", "16"], tag="swap")
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert open(oa2, "rb").read() == want_a and open(ob2, "rb").read() == want_b
    assert tuple(sel) == CASES[(pair, k, o)][::-1]


def test_contrast_defaults_are_k55_o3(gpu, tmp_path):
    oa, ob = str(tmp_path / "a.sub"), str(tmp_path / "b.sub")
    p = _run(["contrast", _g("ctA.fmd"), _g("ctA.rank"), oa, _g("ctB.fmd"), _g("ctB.rank"), ob])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert open(oa, "rb").read() == open(_g("contrast.k55o3.ctA-ctB.sub"), "rb").read()
    assert open(ob, "rb").read() == open(_g("contrast.k55o3.ctB-ctA.sub"), "rb").read()


def test_contrast_with_itself_and_with_an_unrelated_index(gpu, tmp_path):
    """an index against itself: nothing is selected; tiny against repeat at k = 21: everything is (as the reference: 0 / 0, 4000 / 3000)"""
    p, oa, ob, sel = _contrast(tmp_path, "ctA", "ctA", 25, 2)
    assert p.returncode == 0 and sel == [0, 0], p.stderr.decode()[-2000:]
    zero = np.uint64(3000).tobytes() + np.zeros(47, np.uint64).tobytes()
    assert open(oa, "rb").read() == zero                                        # (oa == ob: the second write is the one that stays)
    p, oa, ob, sel = _contrast(tmp_path, "tiny", "repeat", 21, 3)
    assert p.returncode == 0 and sel == [4000, 3000], p.stderr.decode()[-2000:]
    for fn, n in ((oa, 4000), (ob, 3000)):
        raw = open(fn, "rb").read()
        assert int(np.frombuffer(raw[:8], np.uint64)[0]) == n
        w = np.frombuffer(raw[8:], np.uint64)
        assert len(w) == (n + 63) // 64 and int(np.unpackbits(w.view(np.uint8)).sum()) == n
        assert n % 64 == 0 or int(w[-1]) >> (n % 64) == 0                       # nothing beyond the last sequence


@pytest.mark.parametrize("name", sorted(SUB_MD5))
def test_sub_cli_writes_the_reference_bytes(gpu, name):
    kind, tag, _ = name.split(".")
    args = ["sub"] + (["-c"] if kind == "subc" else []) + ["-t", "4", _g("ctA.fmd"), _g("contrast.%s.ctA-ctB.sub" % tag)]
    p = _run(args)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert _md5(p.stdout) == SUB_MD5[name]
    assert p.stdout == open(_g(name + ".fmd"), "rb").read()


def test_sub_of_everything_nothing_and_an_rle6_input(gpu, tmp_path):
    n = 4000
    zero, ones = tmp_path / "zero.sub", tmp_path / "ones.sub"
    zero.write_bytes(np.uint64(n).tobytes() + np.zeros((n + 63) // 64, np.uint64).tobytes())
    w = np.full((n + 63) // 64, ~np.uint64(0), np.uint64)
    w[-1] = np.uint64((1 << (n % 64)) - 1)
    ones.write_bytes(np.uint64(n).tobytes() + w.tobytes())
    tiny = _g("tiny.rle.fmd")
    p = _run(["sub", tiny, str(ones)])
    assert p.returncode == 0 and _md5(p.stdout) == TINY_MD5 == _md5(open(_g("tiny.fmd"), "rb").read()), p.stderr.decode()[-2000:]
    p = _run(["sub", "-c", tiny, str(zero)])
    assert p.returncode == 0 and _md5(p.stdout) == TINY_MD5, p.stderr.decode()[-2000:]
    p = _run(["sub", tiny, str(zero)])                                         # nothing kept: the reference's 216-byte empty index, status 0
    assert p.returncode == 0 and len(p.stdout) == 216 and _md5(p.stdout) == EMPTY_MD5, p.stderr.decode()[-2000:]
    assert p.stdout == open(_g("sub.empty.fmd"), "rb").read()
    p = _run(["sub", "-c", tiny, str(ones)])
    assert p.returncode == 0 and p.stdout == open(_g("sub.empty.fmd"), "rb").read()


def _bwt_of(gpu, d):
    out = np.empty(d.n, dtype=np.uint8)
    gpu.check(gpu.lib().fmd_dev_export_bwt(d.h, 0, d.n, out.ctypes.data))
    return out


def _rank_ok(gpu, d):
    bad, first = C.c_uint64(), C.c_uint64()
    gpu.check(gpu.lib().fmd_dev_check_rank(d.h, C.byref(bad), C.byref(first)))
    return bad.value == 0


def test_api_sub_equals_the_build_of_the_selected_reads(gpu):
    """ragged reads with Ns, a random selection of reads (both strands of each): fmd_sub_mark_dev + fmd_sub_select_dev in two slices with
    the border anywhere, and DevIndex.sub with and without tables, are the BWT `build` makes of the selected reads alone; the complement
    is the build of the others"""
    from fermi_amd import synth
    rng = np.random.default_rng(11)
    gen = synth.genome(synth.DEFAULT_SEED + 6, 20000, 100, 10)
    L = gpu.lib()
    for trial in range(3):
        reads = synth.ragged_reads(synth.DEFAULT_SEED + 70 + trial, int(rng.integers(300, 3000)), gen, min_len=1, max_len=120, err=0.02)
        for r in reads[:: 7]:
            r[rng.integers(0, len(r), size=max(1, len(r) // 30))] = 5          # Ns
        pick = rng.random(len(reads)) < (0.05, 0.5, 0.9)[trial]
        pick[int(rng.integers(0, len(reads)))] = True
        pick[int(rng.integers(0, len(reads)))] = False
        n_seq = 2 * len(reads)
        on = np.zeros((n_seq + 63) // 64 * 64, np.uint8)
        on[: n_seq] = np.repeat(pick, 2)                                        # bit 2r, 2r + 1 <-> read r
        bits = np.packbits(on, bitorder="little").view(np.uint64)
        d = gpu.DevIndex.from_bwt(gpu.build_bwt(reads))
        assert int(d.mcnt[1]) == n_seq
        want = {0: gpu.build_bwt([r for r, p in zip(reads, pick) if p]), 1: gpu.build_bwt([r for r, p in zip(reads, pick) if not p])}
        nw = (d.n + 63) // 64
        wb = L.fmd_sub_work_bytes(d.n)
        d_sub, d_bits, d_work, d_out = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        gpu.check(L.fmd_dev_malloc(0, bits.nbytes, C.byref(d_sub))); gpu.check(L.fmd_dev_malloc(0, nw * 8 + 8, C.byref(d_bits)))
        gpu.check(L.fmd_dev_malloc(0, wb, C.byref(d_work))); gpu.check(L.fmd_dev_malloc(0, d.n, C.byref(d_out)))
        try:
            gpu.check(L.fmd_memcpy_h2d(d_sub, bits.ctypes.data, bits.nbytes, None))
            gpu.check(L.fmd_memset_dev(d_bits, 0, nw * 8 + 8, None))
            gpu.check(L.fmd_sub_mark_dev(d.h, None, d_sub, d_bits, d_work, wb, C.c_void_p(d_bits.value + nw * 8)))
            n_set = np.zeros(1, np.uint64)
            gpu.check(L.fmd_memcpy_d2h(n_set.ctypes.data, C.c_void_p(d_bits.value + nw * 8), 8, None))
            assert int(n_set[0]) == len(want[0]) and d.n - int(n_set[0]) == len(want[1]), trial
            for comp in (0, 1):
                n_out = len(want[comp])
                cut = int(rng.integers(1, n_out))
                got = np.full(n_out, 9, np.uint8)
                gpu.check(L.fmd_sub_select_dev(d.h, None, d_bits, d_work, comp, 0, cut, d_out))
                gpu.check(L.fmd_sub_select_dev(d.h, None, d_bits, d_work, comp, cut, n_out - cut, C.c_void_p(d_out.value + cut)))
                gpu.check(L.fmd_memcpy_d2h(got.ctypes.data, d_out, n_out, None))
                assert np.array_equal(got, want[comp]), (trial, comp, cut)
        finally:
            for p in (d_sub, d_bits, d_work, d_out):
                L.fmd_dev_free(p)
        for comp in (False, True):
            s = d.sub(bits, complement=comp, tables=(trial + comp) % 2 == 0)
            assert s.n == len(want[int(comp)]) and np.array_equal(_bwt_of(gpu, s), want[int(comp)]), (trial, comp)
            assert _rank_ok(gpu, s)
            s.close()
        d.close()


@pytest.mark.parametrize("rows", [4096, 4098])
def test_sub_of_a_parent_at_a_superblock_border(gpu, rows):
    """a parent index of exactly one 4096-row superblock of the row bit array, and of one with two rows in the next (an index of reads
    has 2 * sum(len + 1) rows, never 4097: 4098 takes the same 65 bit words in two superblocks); the first read only, the last read
    only and all but one: DevIndex.sub is the BWT `build` makes of the selected reads alone"""
    from fermi_amd import synth
    gen = synth.genome(synth.DEFAULT_SEED + 6, 20000, 100, 10)
    reads, left = [], rows // 2
    for r in synth.ragged_reads(synth.DEFAULT_SEED + 90 + rows % 7, 400, gen, min_len=5, max_len=60, err=0.02):
        if left == 0:
            break
        r = r[: min(len(r), left - 1)].copy()
        if left - (len(r) + 1) == 1:                                              # one row cannot hold a read: leave room for two
            r = r[:-1]
        r[3:: 11] = 5                                                             # Ns
        reads.append(r)
        left -= len(r) + 1
    d = gpu.DevIndex.from_bwt(gpu.build_bwt(reads))
    assert left == 0 and d.n == rows and int(d.mcnt[1]) == 2 * len(reads)
    for name, keep in (("first", [0]), ("last", [len(reads) - 1]), ("all but one", [i for i in range(len(reads)) if i != len(reads) // 2])):
        pick = np.zeros(len(reads), bool)
        pick[keep] = True
        on = np.zeros((2 * len(reads) + 63) // 64 * 64, np.uint8)
        on[: 2 * len(reads)] = np.repeat(pick, 2)                                # bit 2r, 2r + 1 <-> read r
        bits = np.packbits(on, bitorder="little").view(np.uint64)
        want = gpu.build_bwt([reads[i] for i in keep])
        s = d.sub(bits)
        assert s.n == len(want) and np.array_equal(_bwt_of(gpu, s), want), name
        assert _rank_ok(gpu, s), name
        s.close()
    d.close()


def test_contrast_overflow_is_reported_and_the_host_form_runs_again(gpu, monkeypatch):
    """fmd_contrast_dev with lists of 1024 entries: the overflow flag, no write outside the work area or the bit arrays, every bit it did
    set a right one; the host form started at that capacity, and in four parts, still returns the reference's bits"""
    L = gpu.lib()
    a, b = gpu.DevIndex.open_bare(_g("ctA.fmd")), gpu.DevIndex.open_bare(_g("ctB.fmd"))
    want = [_fixture_bits("contrast.k25o2.ctA-ctB.sub"), _fixture_bits("contrast.k25o2.ctB-ctA.sub")]
    n, nw, cap, guard = 3000, 47, 1024, 4096
    wb = L.fmd_contrast_work_bytes(cap)
    assert wb < 1 << 20
    d_sub, d_work, d_st = [C.c_void_p(), C.c_void_p()], C.c_void_p(), C.c_void_p()
    fill = np.full(wb + guard, 0xA5, np.uint8)
    subfill = np.zeros(nw + 8, np.uint64)
    subfill[nw:] = np.uint64(0xA5A5A5A5A5A5A5A5)
    try:
        for p in d_sub:
            gpu.check(L.fmd_dev_malloc(0, subfill.nbytes, C.byref(p)))
            gpu.check(L.fmd_memcpy_h2d(p, subfill.ctypes.data, subfill.nbytes, None))
        gpu.check(L.fmd_dev_malloc(0, wb + guard, C.byref(d_work))); gpu.check(L.fmd_dev_malloc(0, 32, C.byref(d_st)))
        gpu.check(L.fmd_memcpy_h2d(d_work, fill.ctypes.data, fill.nbytes, None))
        assert L.fmd_contrast_dev(a.h, b.h, None, 25, 2, 0xf, d_sub[0], d_sub[1], d_work, wb - 1, cap, d_st) == gpu.FMD_E_ARG
        assert L.fmd_contrast_dev(a.h, b.h, None, 25, 2, 0xf, d_sub[0], d_sub[1], d_work, wb, 1000, d_st) == gpu.FMD_E_ARG
        assert L.fmd_contrast_dev(a.h, b.h, None, 25, 2, 0, d_sub[0], d_sub[1], d_work, wb, cap, d_st) == gpu.FMD_E_ARG
        gpu.check(L.fmd_contrast_dev(a.h, b.h, None, 25, 2, 0xf, d_sub[0], d_sub[1], d_work, wb, cap, d_st))
        gpu.check(L.fmd_dev_sync(a.h, None))
        st = np.zeros(4, np.uint64)
        gpu.check(L.fmd_memcpy_d2h(st.ctypes.data, d_st, 32, None))
        print("cap 1024: status", st.tolist())
        assert st[1] != 0 and st[0] > 0
        back = np.empty_like(fill)
        gpu.check(L.fmd_memcpy_d2h(back.ctypes.data, d_work, back.nbytes, None))
        assert (back[wb:] == 0xA5).all()
        for i, (p, rk) in enumerate(zip(d_sub, ("ctA.rank", "ctB.rank"))):
            got = np.empty_like(subfill)
            gpu.check(L.fmd_memcpy_d2h(got.ctypes.data, p, got.nbytes, None))
            assert (got[nw:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
            conv = _conv(got[:nw].copy(), _g(rk), n)
            assert not (conv & ~want[i]).any()                                    # a subset of the right bits
    finally:
        for p in d_sub + [d_work, d_st]:
            L.fmd_dev_free(p)
    for env in ({"FMD_CONTRAST_CAP": "1024"}, {"FMD_CONTRAST_CAP": "2048", "FMD_CONTRAST_PARTS": "4"}, {}):
        for k_, v in env.items():
            monkeypatch.setenv(k_, v)
        b0, b1 = a.contrast(b, k=25, min_occ=2)
        assert np.array_equal(_conv(b0, _g("ctA.rank"), n), want[0]) and np.array_equal(_conv(b1, _g("ctB.rank"), n), want[1]), env
        for k_ in env:
            monkeypatch.delenv(k_)
    z0, z1 = a.contrast(a, k=25, min_occ=2)                                       # the same handle twice
    assert not z0.any() and not z1.any()
    out0, out1 = C.c_void_p(), C.c_void_p()
    assert L.fmd_contrast(a.h, b.h, 4, 3, C.byref(out0), C.byref(out1)) == gpu.FMD_E_ARG
    assert L.fmd_contrast(a.h, b.h, 25, 0, C.byref(out0), C.byref(out1)) == gpu.FMD_E_ARG
    assert L.fmd_contrast(a.h, None, 25, 3, C.byref(out0), C.byref(out1)) == gpu.FMD_E_ARG
    assert L.fmd_contrast(None, b.h, 25, 3, C.byref(out0), C.byref(out1)) == gpu.FMD_E_ARG
    a.close(); b.close()


# reads per sample (x 100 bp, both strands indexed).  Measured on the MI355X box at this size: `fermi contrast -t16` 1.7 s (40 042 / 41 246 of
# 4*10^5 sequences selected), `fermi sub -t16` 0.2 s, the whole test 4.9 s; at 2*10^6 reads the reference's contrast alone takes 46 s
MID_READS = 200_000


def test_mid_size_pair_against_the_reference_binary(gpu, tmp_path):
    """two related samples of MID_READS reads x 100 bp (a genome and a copy with 400 substitutions, 0.2 % errors), files written by
    `fermi-amd build` / `seqsort`: `fermi contrast -t16` and `fermi sub -t16` of the compiled reference write the same bytes"""
    if not os.path.exists(REF):
        pytest.skip("the reference binary is not built here (oracle/_ref/fermi)")
    from fermi_amd import synth
    g = synth.genome(synth.DEFAULT_SEED + 31, MID_READS, 100, 30)
    g2 = g.copy()
    pos = np.random.default_rng(3).choice(len(g), 400, replace=False)
    g2[pos] = 1 + g2[pos] % 4
    fmd, rank = {}, {}
    for name, gen, seed in (("s1", g, synth.DEFAULT_SEED + 32), ("s2", g2, synth.DEFAULT_SEED + 33)):
        fq = str(tmp_path / (name + ".fq"))
        rd = synth.reads(seed, MID_READS, 100, 30, err=0.002, gen=gen)
        tab = np.frombuffer(b"$ACGTN", dtype=np.uint8)
        rec = np.empty((MID_READS, 207), np.uint8)                             # "@r\n" SEQ "\n+\n" QUAL "\n" (names need not differ)
        rec[:, :3] = np.frombuffer(b"@r\n", np.uint8); rec[:, 3:103] = tab[rd]; rec[:, 103:106] = np.frombuffer(b"\n+\n", np.uint8)
        rec[:, 106:206] = ord("I"); rec[:, 206] = ord("\n")
        rec.tofile(fq)
        fmd[name], rank[name] = str(tmp_path / (name + ".fmd")), str(tmp_path / (name + ".rank"))
        p = _run(["build", "-fo", fmd[name], fq], timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        p = _run(["seqsort", fmd[name]], timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        open(rank[name], "wb").write(p.stdout)
        os.remove(fq)
    out = {w: [str(tmp_path / ("%s.%d.sub" % (w, i))) for i in (0, 1)] for w in ("ref", "amd")}
    t0 = time.time()
    p = subprocess.run([REF, "contrast", "-k55", "-o3", "-t16", fmd["s1"], rank["s1"], out["ref"][0], fmd["s2"], rank["s2"], out["ref"][1]], capture_output=True, timeout=600)
    t_ref = time.time() - t0
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    ref_lines = [ln.split()[1] for ln in p.stderr.decode().splitlines() if "reads selected from" in ln]
    t0 = time.time()
    p = _run(["contrast", fmd["s1"], rank["s1"], out["amd"][0], fmd["s2"], rank["s2"], out["amd"][1]], timeout=600)
    t_amd = time.time() - t0
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    amd_lines = [ln.split()[1] for ln in p.stderr.decode().splitlines() if "reads selected from" in ln]
    print("contrast: reference -t16 %.2f s, fermi-amd %.2f s; selected %s" % (t_ref, t_amd, ref_lines))
    assert ref_lines == amd_lines and 0 < int(ref_lines[0]) < 2 * MID_READS
    for i in (0, 1):
        assert open(out["ref"][i], "rb").read() == open(out["amd"][i], "rb").read(), i
    for flag in ([], ["-c"]):
        t0 = time.time()
        r = subprocess.run([REF, "sub", "-t16"] + flag + [fmd["s1"], out["ref"][0]], capture_output=True, timeout=600)
        t_ref = time.time() - t0
        t0 = time.time()
        p = _run(["sub"] + flag + [fmd["s1"], out["ref"][0]], timeout=600)
        t_amd = time.time() - t0
        print("sub %s: reference -t16 %.2f s, fermi-amd %.2f s, %d bytes" % (" ".join(flag), t_ref, t_amd, len(r.stdout)))
        assert r.returncode == 0 and p.returncode == 0, p.stderr.decode()[-2000:]
        assert _md5(p.stdout) == _md5(r.stdout) and len(r.stdout) > 1000


def test_cli_errors(gpu, tmp_path):
    oa, ob = tmp_path / "a.sub", tmp_path / "b.sub"
    six = [_g("ctA.fmd"), _g("ctA.rank"), str(oa), _g("ctB.fmd"), _g("ctB.rank"), str(ob)]
    p = _run(["contrast", "-k", "4"] + six)
    assert p.returncode == 1 and b"[E::main_contrast]" in p.stderr and not oa.exists() and not ob.exists()
    p = _run(["contrast", "-o", "0"] + six)
    assert p.returncode == 1 and b"[E::main_contrast]" in p.stderr and not oa.exists()
    p = _run(["contrast"] + six[:5])
    assert p.returncode == 1 and b"Usage:" in p.stderr
    p = _run(["contrast", _g("ctA.fmd"), str(tmp_path / "missing.rank"), str(oa), _g("ctB.fmd"), _g("ctB.rank"), str(ob)])
    assert p.returncode == 1 and b"[E::main_contrast]" in p.stderr and not oa.exists() and not ob.exists()
    # the reference's closing assert fires on special.fmd (it aborts): an error here, no abort, no output, no core
    for k in ("21", "55"):
        p = _run(["contrast", "-k", k, _g("tiny.fmd"), _g("tiny.rank"), str(oa), _g("special.fmd"), _g("special.rank"), str(ob)], cwd=str(tmp_path))
        assert p.returncode == 1 and b"[E::main_contrast]" in p.stderr, (p.returncode, p.stderr.decode()[-2000:])
        assert not oa.exists() and not ob.exists() and not [f for f in os.listdir(tmp_path) if f.startswith("core")]
    # sub: a bit array of another index
    p = _run(["sub", _g("tiny.fmd"), _g("contrast.k25o2.ctA-ctB.sub")])
    assert p.returncode == 1 and p.stdout == b"" and b"[E::main_sub] unmatched index and the bit array" in p.stderr
    p = _run(["sub", _g("ctA.fmd"), str(tmp_path / "missing.sub")])
    assert p.returncode == 1 and p.stdout == b"" and b"[E::main_sub]" in p.stderr
    p = _run(["sub", str(tmp_path / "missing.fmd"), _g("contrast.k25o2.ctA-ctB.sub")])
    assert p.returncode == 1 and p.stdout == b""
    p = _run(["sub", _g("ctA.fmd")])
    assert p.returncode == 1 and b"Usage:" in p.stderr
