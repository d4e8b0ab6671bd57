"""GPU: merging FMD indexes (fmd_merge.hip, host/merge_cmd.c) -- `fermi-amd merge`, `build -i`, `recode` against the bytes the reference
writes (md5s of tests/golden/make_golden_merge.py's files), the C ABI on ragged reads with Ns, a merge past 2^32 rows, the CLI's errors."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")

# `fermi merge` / `build -i` / `recode` of the reference (tests/golden/make_golden_merge.py)
REF_MD5 = {
    "tiny_special": "634b2f509cb3bb6d2b06777afdafb9c1",
    "special_palin": "97ef2d9ccee1ba7a1872912a24778583",
    "palin_special": "08ec58fd1c216e50c8a9cbea70fc4422",
    "tiny_tiny": "66047a90dc5b14555f491393828f311b",
    "tinyrle_special": "634b2f509cb3bb6d2b06777afdafb9c1",
    "dup32_palin": "a441e8fc71247a332d8d266950c9cb9e",
    "tiny_special_repeat": "b016de82566856f1e742dd1ca0d6c860",
    "build_i_tiny_special": "634b2f509cb3bb6d2b06777afdafb9c1",
    "recode_tiny_rle": "c6119facb2001a7abb624e33028e90d0",
}
MERGES = {"tiny_special": ["tiny", "special"], "special_palin": ["special", "palin"], "palin_special": ["palin", "special"],
          "tiny_tiny": ["tiny", "tiny"], "tinyrle_special": ["tiny.rle", "special"], "dup32_palin": ["dup32", "palin"],
          "tiny_special_repeat": ["tiny", "special", "repeat"]}


def _md5(b):
    return hashlib.md5(b).hexdigest()


def _run(args, **kw):
    return subprocess.run([AMD] + args, capture_output=True, timeout=120, **kw)


@pytest.mark.parametrize("name", sorted(MERGES))
def test_merge_cli_writes_the_reference_bytes(gpu, tmp_path, name):
    ins = [os.path.join(GOLD, p + ".fmd") for p in MERGES[name]]
    p = _run(["merge"] + ins)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert _md5(p.stdout) == REF_MD5[name]
    err = p.stderr.decode()                                                   # main_merge's messages (cmd.c:360-371), the last merge's included
    assert err.count("[M::main_merge] Loaded file") == len(ins) and err.count("[M::main_merge] Merged file") == len(ins) - 1
    out = str(tmp_path / "m.fmd")
    p = _run(["merge", "-t", "4", "-o", out] + ins)
    assert p.returncode == 0 and p.stdout == b"", p.stderr.decode()[-2000:]
    assert _md5(open(out, "rb").read()) == REF_MD5[name]
    assert open(os.path.join(GOLD, "merge.%s.fmd" % name), "rb").read() == open(out, "rb").read()


def test_measurement_switch_needs_its_gate(gpu):
    """FMD_MERGE_MARK=0 (the walk without its atomics: wrong output) is honoured only beside FMD_MERGE_TEST_HOOKS=1"""
    ins = [os.path.join(GOLD, p + ".fmd") for p in MERGES["tiny_special"]]
    p = _run(["merge"] + ins, env=dict(os.environ, FMD_MERGE_MARK="0"))
    assert p.returncode == 0 and _md5(p.stdout) == REF_MD5["tiny_special"]
    p = _run(["merge"] + ins, env=dict(os.environ, FMD_MERGE_MARK="0", FMD_MERGE_TEST_HOOKS="1"))
    assert p.returncode == 0 and _md5(p.stdout) != REF_MD5["tiny_special"]


def test_build_append_and_recode_write_the_reference_bytes(gpu):
    p = _run(["build", "-i", os.path.join(GOLD, "tiny.fmd"), os.path.join(GOLD, "special.fq.gz")])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert _md5(p.stdout) == REF_MD5["build_i_tiny_special"]
    p = _run(["recode", os.path.join(GOLD, "tiny.rle.fmd")])
    assert p.returncode == 0 and _md5(p.stdout) == REF_MD5["recode_tiny_rle"] == _md5(open(os.path.join(GOLD, "tiny.fmd"), "rb").read())
    p = _run(["recode", os.path.join(GOLD, "dup32.fmd")])
    assert p.returncode == 0 and p.stdout == open(os.path.join(GOLD, "dup32.fmd"), "rb").read()


def _bwt_of(gpu, d, first=0, n=None):
    n = d.n - first if n is None else n
    out = np.empty(n, dtype=np.uint8)
    gpu.check(gpu.lib().fmd_dev_export_bwt(d.h, first, n, out.ctypes.data))
    return out


def _rank_ok(gpu, d):
    bad, first = C.c_uint64(), C.c_uint64()
    gpu.check(gpu.lib().fmd_dev_check_rank(d.h, C.byref(bad), C.byref(first)))
    return bad.value == 0


def test_api_merge_of_parts_equals_the_build_of_the_whole(gpu):
    """ragged reads with Ns cut into 2-3 parts, each part built, the parts merged left to right (DevIndex.merge = fmd_dev_merge) and
    through the _dev pair by hand: the BWT of the whole, every rank consistent"""
    from fermi_amd import synth
    rng = np.random.default_rng(7)
    gen = synth.genome(synth.DEFAULT_SEED + 5, 20000, 100, 10)
    for trial in range(4):
        reads = synth.ragged_reads(synth.DEFAULT_SEED + 50 + trial, int(rng.integers(300, 3000)), gen, min_len=1, max_len=120, err=0.02)
        for r in reads[:: 7]:
            r[rng.integers(0, len(r), size=max(1, len(r) // 30))] = 5          # Ns
        k = 2 + trial % 2
        cuts = sorted(rng.choice(np.arange(1, len(reads)), size=k - 1, replace=False).tolist())
        parts = np.split(np.arange(len(reads)), cuts)
        idx = [gpu.DevIndex.from_bwt(gpu.build_bwt([reads[i] for i in p])) for p in parts]
        whole = gpu.build_bwt(reads)
        m = idx[0]
        for j, d in enumerate(idx[1:]):
            m2 = m.merge(d, tables=j % 2 == 1)                                    # with and without the prefix / tail tables
            if m is not idx[0]:
                m.close()
            m = m2
        assert m.n == len(whole) and np.array_equal(_bwt_of(gpu, m), whole), trial
        assert _rank_ok(gpu, m)
        m.close()
        if k == 2:   # the _dev pair: the bits say which rows come from the walked (smaller) index
            L, (a, b) = gpu.lib(), idx
            n_tot = a.n + b.n
            nw = (n_tot + 63) // 64
            wb = L.fmd_merge_work_bytes(n_tot)
            d_bits, d_work, d_out = C.c_void_p(), C.c_void_p(), C.c_void_p()
            gpu.check(L.fmd_dev_malloc(0, nw * 8, C.byref(d_bits))); gpu.check(L.fmd_dev_malloc(0, wb, C.byref(d_work))); gpu.check(L.fmd_dev_malloc(0, n_tot, C.byref(d_out)))
            try:
                gpu.check(L.fmd_memset_dev(d_bits, 0, nw * 8, None))
                walked = C.c_int(-1)
                gpu.check(L.fmd_merge_walk_dev(a.h, b.h, None, d_bits, d_work, wb, C.byref(walked)))
                assert walked.value == (1 if b.n <= a.n else 0)
                got = np.empty(n_tot, np.uint8)
                cut = int(rng.integers(1, n_tot))                                 # two slices, the border anywhere
                gpu.check(L.fmd_merge_interleave_dev(a.h, b.h, None, d_bits, d_work, 0, cut, d_out))
                gpu.check(L.fmd_merge_interleave_dev(a.h, b.h, None, d_bits, d_work, cut, n_tot - cut, C.c_void_p(d_out.value + cut)))
                gpu.check(L.fmd_memcpy_d2h(got.ctypes.data, d_out, n_tot, None))
                bits = np.empty(nw, np.uint64)
                gpu.check(L.fmd_memcpy_d2h(bits.ctypes.data, d_bits, nw * 8, None))
                assert np.array_equal(got, whole)
                assert int(np.unpackbits(bits.view(np.uint8)).sum()) == (b.n if walked.value else a.n)
            finally:
                for p in (d_bits, d_work, d_out):
                    L.fmd_dev_free(p)
        for d in idx:
            d.close()


def _reads_with_rows(rows):
    """ragged reads with Ns whose index has exactly `rows` rows: 2 * sum(len + 1), so an even number"""
    from fermi_amd import synth
    seed = synth.DEFAULT_SEED + 200 + rows % 97
    assert rows % 2 == 0
    gen = synth.genome(synth.DEFAULT_SEED + 5, 20000, 100, 10)
    out, left = [], rows // 2
    for r in synth.ragged_reads(seed, 400, gen, min_len=5, max_len=60, err=0.02):
        if left == 0:
            break
        r = r[: min(len(r), left - 1)].copy()
        if left - (len(r) + 1) == 1:                                              # one row cannot hold a read: leave room for two
            r = r[:-1]
        r[3:: 11] = 5                                                             # Ns
        out.append(r)
        left -= len(r) + 1
    assert left == 0
    return out


@pytest.mark.parametrize("rows", [4094, 4096, 4098, 2 * 4096 + 2])
def test_merge_at_a_superblock_border_equals_the_build_of_the_whole(gpu, rows):
    """two parts whose merged row count sits at the border of the 4096-row superblocks of the bit array's prefix counts (one superblock
    not full, exactly full, one and two full ones with two rows in the next): DevIndex.merge is the one-shot build of all reads, every
    rank consistent.  An index of reads holds both strands, 2 * sum(len + 1) rows -- never an odd number -- so the sizes are the even
    ones on either side of the border: 4094 / 4095 rows take 64 bit words in one superblock, 4097 / 4098 take 65 in two, 8193 / 8194 take
    129 in three, and the ranking sees a row count only through these two numbers."""
    reads = _reads_with_rows(rows)
    cut = len(reads) // 3
    a, b = (gpu.DevIndex.from_bwt(gpu.build_bwt(part)) for part in (reads[:cut], reads[cut:]))
    assert a.n + b.n == rows and a.n > 0 and b.n > 0
    whole = gpu.build_bwt(reads)
    m = a.merge(b)
    assert m.n == rows == len(whole) and np.array_equal(_bwt_of(gpu, m), whole)
    assert _rank_ok(gpu, m)
    for d in (a, b, m):
        d.close()


def test_merge_arguments(gpu):
    L = gpu.lib()
    a = gpu.DevIndex.open_bare(os.path.join(GOLD, "tiny.fmd"))
    out = C.c_void_p()
    assert L.fmd_dev_merge(a.h, None, C.byref(out)) == gpu.FMD_E_ARG
    assert L.fmd_dev_open_file_ex(0, os.path.join(GOLD, "tiny.fmd").encode(), 2, C.byref(out)) == gpu.FMD_E_ARG
    assert L.fmd_dev_merge_ex(a.h, a.h, 2, C.byref(out)) == gpu.FMD_E_ARG
    assert _rank_ok(gpu, a)
    b = gpu.DevIndex.open(os.path.join(GOLD, "special.fmd"))
    gpu.check(L.fmd_dev_merge(a.h, b.h, C.byref(out)))                        # the plain form: the same rows as the file the reference writes
    m = gpu.DevIndex(out)
    ref = gpu.DevIndex.open(os.path.join(GOLD, "merge.tiny_special.fmd"))
    assert np.array_equal(_bwt_of(gpu, m), _bwt_of(gpu, ref)) and _rank_ok(gpu, m)
    for d in (a, b, m, ref):
        d.close()


def test_merge_past_2_32_rows_equals_the_one_shot_build(gpu):
    """2.2*10^7 x 100 bp (4.4*10^9 symbols, in-place builder) merged with 10^5 reads in both orders: the one-shot build of the
    concatenation, slice by slice"""
    import torch
    from fermi_amd import synth
    n_big, n_small = 22_000_000, 100_000
    g = synth.genome_torch(synth.DEFAULT_SEED + 9, n_big + n_small, 100, 30)
    allr = synth.reads_torch(synth.DEFAULT_SEED + 9, n_big + n_small, 100, 30, gen=g).cpu().numpy()
    del g
    torch.cuda.empty_cache()
    big, small = allr[:n_big], allr[n_big:]
    for first, second in ((big, small), (small, big)):
        a, b = gpu.build_index_inplace(first), gpu.build_index_inplace(second)
        m = a.merge(b)
        a.close(); b.close()
        w = gpu.build_index_inplace(np.concatenate([first, second]))
        assert m.n == w.n > 1 << 32
        assert np.array_equal(m.mcnt, w.mcnt)
        S = 1 << 28
        for at in range(0, w.n, S):
            k = min(S, w.n - at)
            assert np.array_equal(_bwt_of(gpu, m, at, k), _bwt_of(gpu, w, at, k)), at
        m.close(); w.close()


def test_cli_errors(gpu, tmp_path):
    t, s = os.path.join(GOLD, "tiny.fmd"), os.path.join(GOLD, "special.fmd")
    out = tmp_path / "exists.fmd"
    out.write_bytes(b"keep")
    p = _run(["merge", "-o", str(out), t, s])
    assert p.returncode == 1 and b"exists. Please use `-f' to overwrite." in p.stderr and out.read_bytes() == b"keep"
    p = _run(["merge", "-f", "-o", str(out), t, s])
    assert p.returncode == 0 and _md5(out.read_bytes()) == REF_MD5["tiny_special"]
    p = _run(["merge", t])
    assert p.returncode == 1 and b"Usage:" in p.stderr
    missing, fresh = str(tmp_path / "missing.fmd"), tmp_path / "fresh.fmd"
    p = _run(["merge", "-o", str(fresh), t, missing])
    assert p.returncode == 1 and not fresh.exists()
    p = _run(["build", "-i", missing, "-o", str(fresh), os.path.join(GOLD, "special.fq.gz")])
    assert p.returncode == 1 and not fresh.exists()
