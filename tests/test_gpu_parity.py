"""GPU: the HIP path (through the C ABI) against the golden vectors and the oracle.
Integer/index work: the bar is bit-exact."""
import numpy as np
import pytest

import orcbind
from fermi_amd import synth

pytestmark = pytest.mark.gpu
U64 = np.uint64
NONE = U64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def tiny_dev(gpu, gold):
    d = gpu.DevIndex.open(gold.path("tiny.fmd"))
    yield d
    d.close()


@pytest.mark.parametrize("name", ["tiny", "special", "dup32"])
def test_open_rld_counts_and_rank1a_golden(gpu, gold, name):
    v = gold.npz(name + "_vectors.npz")
    d = gpu.DevIndex.open(gold.path(name + ".fmd"))
    ok, sym = d.rank1a(v["rank1a_k"])
    assert np.array_equal(ok, v["rank1a_ok"])
    assert np.array_equal(sym, v["rank1a_sym"])
    d.close()


def test_three_loaders_give_one_index(gpu, gold, oracle_lib):
    """RLD\\2 file, RLE\\6 file and the plain BWT string transcode to the same device index."""
    o = orcbind.OrcIndex(gold.path("tiny.fmd"))
    bwt = o.decode_all()
    ks = np.arange(o.n, dtype=U64)
    want, wsym = o.rank1a(ks)
    for d in (gpu.DevIndex.open(gold.path("tiny.fmd")), gpu.DevIndex.open(gold.path("tiny.rle.fmd")), gpu.DevIndex.from_bwt(bwt)):
        assert np.array_equal(d.cnt, o.cnt) and np.array_equal(d.mcnt, o.mcnt)
        ok, sym = d.rank1a(ks)  # chkbwt -r equivalent (cmd.c:90-105): every position
        assert np.array_equal(ok, want) and np.array_equal(sym, wsym)
        d.close()
    o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "special", "dup32"])
def test_fmd_file_uploaded_in_pieces_by_several_threads(gpu, gold, monkeypatch, name):
    """fmd_dev_open_file sends the payload of an RLD\\2 file to the device in pieces (32 MiB each, four threads with a pinned buffer and a stream each): with
    pieces of 4 KiB, 192 bytes and 64 bytes a fixture is hundreds of them, and the index is the one the single piece gives -- every position's rank."""
    ref = gpu.DevIndex.open(gold.path(name + ".fmd"))
    ks = np.arange(int(ref.mcnt[0]), dtype=U64)
    want, wsym = ref.rank1a(ks)
    for chunk in (4096, 192, 64):
        monkeypatch.setenv("FMD_LOAD_CHUNK", str(chunk))
        d = gpu.DevIndex.open(gold.path(name + ".fmd"))
        assert np.array_equal(d.cnt, ref.cnt) and np.array_equal(d.mcnt, ref.mcnt)
        ok, sym = d.rank1a(ks)
        assert np.array_equal(ok, want) and np.array_equal(sym, wsym)
        d.close()
    ref.close()


def test_rank2a_golden(tiny_dev, gold):
    v = gold.npz("tiny_vectors.npz")
    ok, ol = tiny_dev.rank2a(v["rank2a_k"], v["rank2a_l"])
    assert np.array_equal(ok, v["rank2a_ok"]) and np.array_equal(ol, v["rank2a_ol"])


def test_extend_golden(gpu, tiny_dev, gold):
    v = gold.npz("tiny_vectors.npz")
    ik = v["ext_ik"].copy().view(gpu.INTV_DT).reshape(-1)
    out = tiny_dev.extend(ik, v["ext_back"])
    assert np.array_equal(out.view(U64).reshape(-1, 24), v["ext_ok"])


def test_backward_search_golden(tiny_dev, gold):
    v = gold.npz("tiny_vectors.npz")
    cnt, beg, end = tiny_dev.backward_search(v["bs_reads"])
    assert np.array_equal(cnt, v["bs_cnt"])
    hit = cnt > 0
    assert np.array_equal(beg[hit], v["bs_beg"][hit]) and np.array_equal(end[hit], v["bs_end"][hit])
    assert not beg[~hit].any() and not end[~hit].any()
    short = [v["bs_short"][i, :v["bs_short_len"][i]] for i in range(len(v["bs_short_len"]))]
    cnt, beg, end = tiny_dev.backward_search(short)  # ragged, incl. length-1 queries
    assert np.array_equal(cnt, v["bs_short_cnt"])
    hit = cnt > 0
    assert np.array_equal(beg[hit], v["bs_short_beg"][hit]) and np.array_equal(end[hit], v["bs_short_end"][hit])


@pytest.mark.parametrize("name,stride", [("tiny", 128), ("special", 64)])
def test_retrieve_golden(gpu, gold, name, stride):
    v = gold.npz(name + "_vectors.npz")
    d = gpu.DevIndex.open(gold.path(name + ".fmd"))
    seqs, ln, rank = d.retrieve(v["ret_x"], stride=stride)
    assert np.array_equal(ln, v["ret_len"]) and np.array_equal(rank, v["ret_rank"])
    assert np.array_equal(seqs, v["ret_seq"])
    d.close()


def test_empty_and_edge_inputs(gpu, tiny_dev):
    ok, sym = tiny_dev.rank1a(np.zeros(0, dtype=U64))
    assert ok.shape == (0, 6)
    ok, sym = tiny_dev.rank1a(np.array([NONE, 0, tiny_dev.n - 1], dtype=U64))
    assert not ok[0].any() and sym[0] == -1
    assert ok[2].sum() == tiny_dev.n and np.array_equal(ok[2], tiny_dev.mcnt[1:])
    cnt, beg, end = tiny_dev.backward_search([np.array([], dtype=np.uint8), np.array([1], dtype=np.uint8)])
    assert cnt[0] == 0 and cnt[1] == tiny_dev.mcnt[2]
    # the newer entry points: nothing to do is not an error, impossible arguments are
    import ctypes as C
    L = gpu.lib()
    assert L.fmd_reach_batch(tiny_dev.h, 0, None, None) == 0
    assert L.fmd_smem_win_batch(tiny_dev.h, 0, None, 0, None, 0, 64, 8, None, None) == 0
    assert L.fmd_reach_batch(tiny_dev.h, 16, None, None) == gpu.FMD_E_ARG
    assert L.fmd_dev_export_bwt(tiny_dev.h, tiny_dev.n, 1, None) == gpu.FMD_E_ARG          # past the end
    buf = np.zeros(3, dtype=np.uint8)
    assert L.fmd_dev_export_bwt(tiny_dev.h, tiny_dev.n - 3, 3, buf.ctypes.data) == 0 and (buf < 6).all()
    r = tiny_dev.reach(np.array([0, 0, 5, 0, 1, 2, 0], dtype=np.uint8))                    # terminators, an N alone, a 2-mer
    assert r[0] == r[1] == r[3] == r[6] == 0 and r[2] == 0 and r[4] in (1, 2) and r[5] == 1
    bad, first = C.c_uint64(), C.c_uint64()
    assert L.fmd_dev_check_rank(tiny_dev.h, C.byref(bad), C.byref(first)) == 0 and bad.value == 0


def test_random_batches_vs_oracle(gpu, tiny_dev, tiny_oracle):
    """10^6 random rank2a / extend queries, oracle beside the GPU."""
    rng = np.random.default_rng(42)
    n = tiny_dev.n
    m = 1_000_000
    k = rng.integers(0, n, m).astype(U64)
    l = np.minimum(k + rng.integers(0, 1000, m).astype(U64), U64(n - 1))
    k[::1000] = NONE
    ok, ol = tiny_dev.rank2a(k, l)
    wk, wl = tiny_oracle.rank2a(k, l)
    assert np.array_equal(ok, wk) and np.array_equal(ol, wl)
    ik = np.zeros(m, dtype=gpu.INTV_DT)
    size = rng.integers(0, 300, m).astype(U64)
    x0 = rng.integers(0, n, m).astype(U64)
    x1 = rng.integers(0, n, m).astype(U64)
    ik["x"][:, 0] = np.minimum(x0, U64(n) - size); ik["x"][:, 1] = np.minimum(x1, U64(n) - size); ik["x"][:, 2] = size
    back = rng.integers(0, 2, m).astype(np.uint8)
    got = tiny_dev.extend(ik, back)
    want = tiny_oracle.extend(ik, back)
    assert np.array_equal(got.view(U64), want.view(U64))


def test_synthetic_index_properties(gpu, oracle_lib):
    """Size-independent properties on a bigger synthetic index (5k reads, BWT by brute-force suffix sorting
    encoder's input): every indexed read is found, with itself inside its interval; retrieve
    inverts; mutated reads agree with the oracle."""
    N = 5000
    reads = synth.reads(synth.DEFAULT_SEED, N)
    # BWT via sorting all suffixes on the host (small N): text = r $ revcomp(r) $ ...
    both = np.empty((2 * N, 101), dtype=np.uint8)
    both[0::2, :100] = reads
    both[1::2, :100] = (5 - reads)[:, ::-1]
    both[:, 100] = 0
    text = both.reshape(-1)
    # suffix keys: pad each suffix to its own sentinel, ties broken by sequence id
    from test_build_host import bwt_by_sorting
    bwt = bwt_by_sorting(both)
    d = gpu.DevIndex.from_bwt(bwt)
    o = orcbind.OrcIndex(bwt=bwt)
    assert np.array_equal(d.cnt, o.cnt)
    cnt, beg, end = d.backward_search(reads)
    assert (cnt >= 1).all()
    wc, wb, we = o.backward_search(reads[:2000])
    assert np.array_equal(cnt[:2000], wc) and np.array_equal(beg[:2000], wb) and np.array_equal(end[:2000], we)
    ids = np.arange(0, 2 * N, 7, dtype=U64)
    seqs, ln, rank = d.retrieve(ids, stride=128)
    assert (ln == 100).all()
    assert np.array_equal(seqs[:, :100], both[ids.astype(np.int64), :100])
    ws, wl, wr = o.retrieve(ids[:500], stride=128)
    assert np.array_equal(rank[:500], wr)
    miss = synth.reads(synth.DEFAULT_SEED, N, err=0.03)[:3000]
    c1, b1, e1 = d.backward_search(miss)
    c2, b2, e2 = o.backward_search(miss)
    assert np.array_equal(c1, c2)
    h = c1 > 0
    assert np.array_equal(b1[h], b2[h]) and np.array_equal(e1[h], e2[h])
    d.close(); o.close()


def test_gpu_build_equals_fermi_build(gpu, gold, oracle_lib, tmp_path):
    """GPU suffix-sort construction == `fermi build` BWT; the .fmd written from it is the same file."""
    from fermi_amd import hostlib
    import ctypes as C
    for name in ("tiny", "special"):
        reads = gold.fastq_nt6(name + ".fq.gz")
        reads = [r[:hostlib.trim_palindrome(r)] for r in reads]  # cmd.c:457-463
        bwt = gpu.build_bwt(reads)
        o = orcbind.OrcIndex(gold.path(name + ".fmd"))
        assert np.array_equal(bwt, o.decode_all()), name
        o.close()
        out = str(tmp_path / (name + ".fmd"))
        hostlib.write_rld_from_bwt(bwt, out)
        assert open(out, "rb").read() == open(gold.path(name + ".fmd"), "rb").read()
    # device BWT -> RLE\6 stream -> RLD file (the bench's path)
    reads = np.array(gold.fastq_nt6("tiny.fq.gz"), dtype=np.uint8)
    d = gpu.DevIndex.from_bwt(bwt_tiny := gpu.build_bwt(reads))
    dp = C.c_void_p()
    gpu.check(gpu.lib().fmd_dev_malloc(0, len(bwt_tiny), C.byref(dp)))
    gpu.check(gpu.lib().fmd_memcpy_h2d(dp, bwt_tiny.ctypes.data, len(bwt_tiny), None))
    p, nb = C.c_void_p(), C.c_uint64()
    gpu.check(gpu.lib().fmd_bwt_to_rle6(0, dp, len(bwt_tiny), C.byref(p), C.byref(nb)))
    gpu.lib().fmd_dev_free(dp)
    out = str(tmp_path / "viarle.fmd")
    hostlib.write_rld_from_rle6_ptr(p, nb.value, out)
    gpu.lib().fmd_host_free(p)
    assert open(out, "rb").read() == open(gold.path("tiny.fmd"), "rb").read()
    d.close()


def _check_overlap_records(gpu, gold, name, key, max_len):
    recs = gold.json_gz(name + "_overlap.json.gz")[key]
    mm = int(key[1:])
    d = gpu.DevIndex.open(gold.path(name + ".fmd"))
    ids = np.array([r["id"] for r in recs], dtype=U64)
    rec, nei, seq = d.overlap(ids, mm, max_len=max_len, max_nei=8)
    n_nei = n_fork = 0
    for i, want in enumerate(recs):
        g = rec[i]
        assert not (g["flags"] & gpu.OVLP_F_OVERFLOW), want
        assert g["rank"] == want["rank"] and g["len"] == want["len"], (i, g, want)
        if want.get("status") == -1:
            assert g["status"] == -1
            continue
        assert tuple(int(v) for v in g["k"]) == tuple(want["intv"]), (i, g, want)
        assert (g["status"] == -3) == (want["contained"] < 0)
        assert g["n_ovlp"] == want["n_ovlp"]
        if want["contained"] < 0 or want["n_ovlp"] == 0:
            assert g["n_nei"] == 0 and g["rbeg"] == -1
            continue
        assert g["rbeg"] == want["rbeg"], (i, g, want)
        assert g["n_nei"] == len(want["nei"]), (i, g, want)
        got_nei = [(int(e["x"][0]), int(e["x"][1]), int(e["x"][2]), int(e["info"])) for e in nei[i, :g["n_nei"]]]
        assert got_nei == [tuple(x) for x in want["nei"]], (i, got_nei, want)
        ext = bytes(seq[i, g["len"]:g["len"] + g["ext_len"]])
        assert ext.hex() == want["ext"], (i, ext.hex(), want)
        n_nei += g["n_nei"]; n_fork += int(bool(g["flags"] & gpu.OVLP_F_FORKED))
    assert n_nei > 0
    d.close()
    return n_fork


@pytest.mark.parametrize("name,key,max_len", [("tiny", "l50", 100), ("tiny", "l30", 100), ("special", "l20", 60),
                                              ("repeat", "l20", 80), ("repeat", "l35", 80)])
def test_overlap_records_golden(gpu, gold, name, key, max_len):
    """Per-read overlap records (fm_retrieve + fm6_is_contained + fm6_get_nei) vs the reference."""
    _check_overlap_records(gpu, gold, name, key, max_len)


@pytest.mark.parametrize("name,mm,max_len", [("tiny", 50, 100), ("special", 20, 60), ("repeat", 20, 80)])
def test_overlap_pack_equals_numpy_statement(gpu, gold, name, mm, max_len):
    """fmd_ovlp_pack_dev (what leaves the GPU: PCIe to the host walk, xGMI to rank 0) against tests/packref.py, incl.
    rows with Ns (4-bit form), contained/short rows (empty) and overflowed rows."""
    import packref
    d = gpu.DevIndex.open(gold.path(name + ".fmd"))
    ids = np.arange(int(d.mcnt[1]), dtype=U64)
    for ml in (max_len, max(8, max_len // 2)):   # the second pass overflows the longer reads
        rec, nei, seq = d.overlap(ids, mm, max_len=ml)
        prec, off, var = d.overlap_pack(rec, nei, seq)
        wp, wo, wv = packref.pack_rows(rec, nei, seq, nei.shape[1])
        assert prec.tobytes() == wp.tobytes() and np.array_equal(off, wo) and var.tobytes() == wv.tobytes()
    r0, n0, s0 = d.overlap(ids[:0], mm, max_len=max_len)
    p0, o0, v0 = d.overlap_pack(r0, n0, s0)
    assert len(p0) == 0 and list(o0) == [0] and len(v0) == 0
    d.close()


def test_overlap_sequences_and_capacity_flags(gpu, gold):
    d = gpu.DevIndex.open(gold.path("tiny.fmd"))
    ids = np.arange(0, 400, dtype=U64)
    rec, nei, seq = d.overlap(ids, 50, max_len=100)
    want, ln, _ = d.retrieve(ids, stride=128)
    for i in range(len(ids)):
        assert np.array_equal(seq[i, :100], want[i, :100])
    # a max_len smaller than the reads must raise the overflow flag, not corrupt anything
    rec2, _, _ = d.overlap(ids[:64], 50, max_len=64)
    assert ((rec2["flags"] & gpu.OVLP_F_OVERFLOW) != 0).all()
    d.close()


@pytest.mark.parametrize("w,mo", [(17, 3), (21, 3), (23, 2)])
def test_kmer_collect_golden(tiny_dev, gold, w, mo):
    """fm6_traverse + ec_collect (correct.c:35-87): sorted multiset of (bucket, key, val) and cnt[]."""
    v = gold.npz("tiny_solid.npz")
    tag = "w%d_o%d" % (w, mo)
    B, K, V, cnt = tiny_dev.kmer_collect(w, mo)
    o = np.lexsort([V, K, B])
    assert np.array_equal(B[o], v[tag + "_bucket"]) and np.array_equal(K[o], v[tag + "_key"]) and np.array_equal(V[o], v[tag + "_val"])
    assert cnt == list(v[tag + "_cnt"])


def test_kmer_collect_in_four_parts_equals_one_pass(tiny_dev, monkeypatch):
    """The harvest by last base (fmd_kmer_collect_part_dev: what carries indexes whose frontiers do not fit beside them)
    gives the triples of the one-pass harvest, and the same informative / ambiguous counts."""
    def pack(b, k, v):
        return np.sort(b.astype(np.uint64) << np.uint64(40) | k.astype(np.uint64) << np.uint64(8) | v.astype(np.uint64))
    for w, mo in ((17, 3), (23, 2)):
        monkeypatch.setenv("FMD_KMER_PARTS", "1")
        b1, k1, v1, c1 = tiny_dev.kmer_collect(w, mo)
        monkeypatch.setenv("FMD_KMER_PARTS", "4")
        b4, k4, v4, c4 = tiny_dev.kmer_collect(w, mo)
        assert len(b1) > 1000 and np.array_equal(pack(b1, k1, v1), pack(b4, k4, v4)) and list(c1) == list(c4)


@pytest.mark.parametrize("sm", [0, 1])
def test_smem_golden(tiny_dev, gold, sm):
    """fm6_smem (smem.c:397) on indexed and noisy reads, both self_match settings."""
    v = gold.npz("tiny_vectors.npz")
    off = v["smem%d_off" % sm]
    got = tiny_dev.smem(v["smem%d_reads" % sm], sm, max_mem=64)
    for i, m in enumerate(got):
        assert np.array_equal(m.view(U64).reshape(-1, 4), v["smem%d_mem" % sm][off[i]:off[i + 1]]), i


def test_smem_vs_oracle_ragged(gpu, tiny_dev, tiny_oracle):
    rng = np.random.default_rng(7)
    reads = synth.reads(synth.DEFAULT_SEED, 2000, coverage=20, err=0.02)
    qs = [r[int(rng.integers(0, 50)):][:int(rng.integers(1, 100))] for r in reads[:600]]
    got = tiny_dev.smem(qs, 0, max_mem=64)
    for q, m in zip(qs, got):
        assert m.tobytes() == tiny_oracle.smem(q, 0).tobytes()


@pytest.mark.parametrize("sm", [0, 1])
def test_smem_lists_and_refill_policies(gpu, oracle_lib, monkeypatch, sm):
    """k_smem's candidate lists (pairs of entries leave LDS as one burst; the last round of a backward sweep skips the entries that
    cannot matter and writes no list) and its three ways of taking new reads (whole waves in step for reads of one length, groups
    of 8 otherwise, one by one) give the oracle's SMEMs: 250-bp reads at 60x (lists of > 64 entries: beyond the per-entry bits),
    exact reads (one call, last round only), reads with errors (several calls, backward sweeps over many bases), queries that
    start in the middle of reads (x > 0 rounds), an N, and reads of mixed lengths."""
    rng = np.random.default_rng(31 + sm)
    reads = synth.reads(synth.DEFAULT_SEED + 77, 3000, 250, 60, 0.004)
    reads[7][100] = 5                                                              # (an N that is in the index: fm6_smem of a symbol the index lacks reads an empty list)
    bwt = gpu.build_bwt(reads)
    d = gpu.DevIndex.from_bwt(bwt)
    o = orcbind.OrcIndex(bwt=bwt)
    uni = [reads[i].copy() for i in range(400)]
    for r in uni[200:300]:
        for _ in range(3):
            r[rng.integers(0, len(r))] = rng.integers(1, 5)                        # errors: the forward sweep stops, more calls follow
    mixed = [r[int(rng.integers(0, 120)):][: int(rng.integers(20, 250))] for r in uni]
    want_u = [o.smem(q, sm).tobytes() for q in uni]
    want_m = [o.smem(q, sm).tobytes() for q in mixed]
    assert max(len(w) for w in want_u) >= 2 * 32
    for env in ({}, {"FMD_SMEM_REFILL": "64"}, {"FMD_SMEM_REFILL": "1"}, {"FMD_SMEM_PATIENCE": "2"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        assert [m.tobytes() for m in d.smem(uni, sm, max_mem=256)] == want_u, env
        assert [m.tobytes() for m in d.smem(mixed, sm, max_mem=256)] == want_m, env
        for k in env:
            monkeypatch.delenv(k)
    d.close(); o.close()


@pytest.mark.parametrize("name,mm", [("tiny", 50), ("repeat", 20), ("palin", 40)])
def test_unitig_cli_equals_fermi_unitig_t1(gpu, gold, tmp_path, name, mm):
    """`fermi-amd unitig -l mm x.fmd` (GPU overlap table + host walk) == `fermi unitig -t1` bytes."""
    import subprocess, os
    from fermi_amd import hostlib
    out = str(tmp_path / "o.mag")
    hostlib.unitig(gold.path(name + ".fmd"), mm, out)
    assert open(out, "rb").read() == gold.text_gz(name + ".mag.gz")
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fermi_amd", "bin", "fermi-amd")
    if os.path.exists(exe):
        got = subprocess.run([exe, "unitig", "-l%d" % mm, "-t4", gold.path(name + ".fmd")], stdout=subprocess.PIPE, check=True).stdout
        assert got == gold.text_gz(name + ".mag.gz")


@pytest.mark.parametrize("name,mm", [("tiny", 50), ("repeat", 20), ("special", 20), ("palin", 40)])
@pytest.mark.parametrize("n_rep", [2, 3])
def test_unitig_sharded_over_replicas_equals_one_gpu(gpu, gold, tmp_path, name, mm, n_rep):
    """`fermi-amd unitig -g a,b[,c]`: the index replicated n_rep times, replica g computing the rows of the ids
    i = g (mod n_rep) on its own host thread (unitig.c:333, 398-399), one walk over the shards: the MAG must be the
    single-GPU one, i.e. `fermi unitig -t1`'s.  Distinct GPUs when the box has them, else replicas on GPU 0."""
    import subprocess, os
    from fermi_amd import hostlib
    n_gpu = gpu.device_count()
    devs = tuple(g % n_gpu for g in range(n_rep))
    out = str(tmp_path / "o.mag")
    hostlib.unitig(gold.path(name + ".fmd"), mm, out, devices=devs)
    assert open(out, "rb").read() == gold.text_gz(name + ".mag.gz")
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fermi_amd", "bin", "fermi-amd")
    if os.path.exists(exe):
        got = subprocess.run([exe, "unitig", "-l%d" % mm, "-g", ",".join(map(str, devs)), gold.path(name + ".fmd")], stdout=subprocess.PIPE, check=True).stdout
        assert got == gold.text_gz(name + ".mag.gz")


def test_packed_batch_equals_fixed_stride_batch(gpu, gold):
    """fmd_ovlp_packed_batch (pipelined chunks, ids by first/step or explicit) == pack(fmd_ovlp_batch) row for row."""
    import ctypes as C
    import packref
    d = gpu.DevIndex.open(gold.path("tiny.fmd"))
    L = gpu.lib()
    n_seq = int(d.mcnt[1])
    for first, step, shift in ((0, 1, 10), (1, 3, 11), (2, 3, 20)):
        ids = np.arange(first, n_seq, step, dtype=U64)
        n = len(ids)
        rec, nei, seq = d.overlap(ids, 50, max_len=128, max_nei=4)
        wp, wo, wv = packref.pack_rows(rec, nei, seq, 4)
        for explicit in (False, True):
            prec = np.zeros(n, dtype=gpu.OVLP_DT); off = np.zeros(n, dtype=U64)
            nc = (n + (1 << shift) - 1) >> shift
            chunks = (C.c_void_p * nc)()
            gpu.check(L.fmd_ovlp_packed_batch(d.h, ids.ctypes.data if explicit else None, first, step, n, 50, 128, 4, 1,
                                              prec.ctypes.data, off.ctypes.data, shift, chunks))
            assert prec.tobytes() == wp.tobytes()
            for i in (list(range(0, n, 97)) + [n - 1]):
                c = i >> shift
                ln = int(wo[i + 1] - wo[i])
                got = C.string_at(chunks[c] + int(off[i]), ln) if ln else b""
                assert got == wv[int(wo[i]):int(wo[i + 1])].tobytes()
                # offsets restart in every chunk
                assert int(off[i]) == int(wo[i] - wo[c << shift])
            L.fmd_ovlp_packed_free(chunks, nc)
    d.close()


def _lfork_decide(lf, rbeg):
    R, D = int(lf) & 0x7fff, int(lf) >> 15
    if rbeg <= R or R == 0x7fff:
        return 0
    return -1 if D else 1


@pytest.mark.parametrize("name,mm,ml", [("tiny", 50, 100), ("tiny", 30, 100), ("repeat", 20, 80), ("special", 20, 60)])
def test_lfork_never_claims_more_than_the_truth_and_decides_check_left(gpu, gold, oracle_lib, name, mm, ml):
    """rec.lfork (include/fmd_hip.h): what fm6_get_nei's rounds on strand X already tell about check_left_simple on
    any edge whose neighbour is revcomp(X).  (1) the GPU's claim is implied by the oracle's exact value; (2) for every
    edge of the fixture, deciding check_left_simple from the lfork of the neighbour's reverse strand gives what the
    oracle's check_left_simple (unitig.c:186-204) returns -- or says `undecided`, never the wrong answer."""
    d = gpu.DevIndex.open(gold.path(name + ".fmd")); o = orcbind.OrcIndex(gold.path(name + ".fmd"))
    n = int(o.mcnt[1])
    ids = np.arange(n, dtype=U64)
    g_rec, g_nei, _ = d.overlap(ids, mm, max_len=ml, max_nei=8, check_left=True)
    w_rec, w_nei, _ = o.overlap_batch(ids, mm, max_len=ml, max_nei=8)
    Rg, Dg = g_rec["lfork"] & 0x7fff, g_rec["lfork"] >> 15
    Ro, Do = w_rec["lfork"] & 0x7fff, w_rec["lfork"] >> 15
    assert np.array_equal(Rg[Dg == 1], Ro[Dg == 1]) and (Do[Dg == 1] == 1).all()   # a fork the GPU reports is the first one
    assert (Rg[Dg == 0] <= Ro[Dg == 0]).all()                                        # rounds it vouches for really pass (0x7fff = all)
    assert (g_rec["lfork"][g_rec["status"] != 0] == 0).all()
    row_of = {}
    for i in range(n - 1, -1, -1):
        if g_rec[i]["status"] == 0:
            row_of[int(g_rec[i]["k"][0])] = i
    edges = undecided = 0
    for i in range(n):
        r = w_rec[i]
        if r["status"] == 0 and r["n_nei"] == 1 and r["rbeg"] >= 0 and r["reserved"] != 2:
            row2 = row_of[int(w_nei[i, 0]["x"][1])]
            dec = _lfork_decide(g_rec[row2]["lfork"], int(r["rbeg"]))
            edges += 1
            if dec == 1:
                undecided += 1
            else:
                assert dec == (-1 if r["reserved"] == 1 else 0), (name, i)
            assert _lfork_decide(w_rec[row2]["lfork"], int(r["rbeg"])) == (-1 if r["reserved"] == 1 else 0)   # the exact value decides every edge
    # what is left goes to fmd_ovlp_check_left_dev: few on ordinary reads, more where the read set forks or holds contained reads
    assert edges > 100 and undecided <= (0.05 if name == "tiny" else 0.3) * edges, (edges, undecided)
    d.close(); o.close()


def _ecfix_gpu(gpu, w, bucket, key, val, seqs_nt6, quals, step=5):
    import ctypes as C
    L = gpu.lib()
    bucket = np.ascontiguousarray(bucket, dtype=np.uint32); key = np.ascontiguousarray(key, dtype=np.uint32); val = np.ascontiguousarray(val, dtype=np.uint8)
    t = C.c_void_p()
    gpu.check(L.fmd_ectab_build(0, w, w - 15 if w > 15 else 1, len(key), bucket.ctypes.data, key.ctypes.data, val.ctypes.data, C.byref(t)))
    n = len(seqs_nt6)
    off = np.zeros(n + 1, dtype=U64)
    np.cumsum([len(x) for x in seqs_nt6], out=off[1:])
    s = np.concatenate([np.asarray(x, dtype=np.uint8) for x in seqs_nt6] + [np.zeros(8, np.uint8)])
    q = np.concatenate([np.asarray(x, dtype=np.uint8) for x in quals] + [np.zeros(8, np.uint8)])
    info = np.zeros(n, dtype=np.int32)
    gpu.check(L.fmd_ecfix_batch(t, n, s.ctypes.data, q.ctypes.data, off.ctypes.data, step, info.ctypes.data))
    L.fmd_ectab_free(t)
    return s[: int(off[n])], q[: int(off[n])], off, info


@pytest.mark.parametrize("step", [5, 0, 2])
def test_ecfix_kernel_equals_oracle_and_fermi_correct(gpu, gold, oracle_lib, step):
    """fmd_ecfix_batch (ec_fix1 / ec_fix on the GPU: one lane per read, device hash table, its own queue) == the oracle's
    statement of correct.c:121-246 on corrected bases, qualities and info words of every read of tiny.fq; with the
    default step the marked and filtered FASTQ is `fermi correct -t1`'s."""
    from test_oracle_golden import _fastq_records, finish_correct
    v = gold.npz("tiny_solid.npz")
    recs = _fastq_records(gold.text_gz("tiny.fq.gz"))
    nt6 = gold.fastq_nt6("tiny.fq.gz")
    quals = [np.frombuffer(r[2], dtype=np.uint8) for r in recs]
    g = _ecfix_gpu(gpu, 17, v["w17_o3_bucket"], v["w17_o3_key"], v["w17_o3_val"], nt6, quals, step)
    w = orcbind.ec_fix(17, v["w17_o3_bucket"], v["w17_o3_key"], v["w17_o3_val"], nt6, quals, step)
    assert np.array_equal(g[3], w[3]) and np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])
    if step == 5:
        assert finish_correct([r[1] for r in recs], *g) == gold.text_gz("tiny.ec.fq.gz")


def _odd_reads(base):
    """600 reads made of the reads `base` that the fixture does not hold: shorter than k, all N, Ns near either end (a strand without a
    clean k-mer), very low and very high qualities, reads of other genomes, reads of 300 bases -> (reads, qualities)"""
    rng = np.random.default_rng(7)
    seqs, quals = [], []
    for i in range(600):
        r = base[i % len(base)].copy()
        kind = i % 12
        if kind == 0: r = r[: int(rng.integers(0, 18))]
        elif kind == 1: r[:] = 5
        elif kind == 2: r[-int(rng.integers(1, 30)):] = 5
        elif kind == 3: r[: int(rng.integers(1, 30))] = 5
        elif kind == 4: r = rng.integers(1, 5, size=len(r)).astype(np.uint8)
        elif kind == 5: r[rng.integers(0, len(r), size=8)] = rng.integers(1, 5, size=8)
        elif kind == 6: r[rng.integers(0, len(r), size=3)] = 5
        elif kind == 7: r = np.concatenate([r, r[::-1], r])            # 300 bases
        q = rng.integers(33, 33 + 45, size=len(r)).astype(np.uint8) if kind % 2 else np.full(len(r), 33 + (2 if kind == 8 else 30), dtype=np.uint8)
        seqs.append(r); quals.append(q)
    return seqs, quals


def test_ecfix_kernel_odd_reads_vs_oracle(gpu, gold, oracle_lib):
    """Reads the fixture does not hold: shorter than k, all N, Ns near either end (a strand without a clean k-mer), very
    low and very high qualities, reads of other genomes (every look-up misses: the longest searches, trace re-runs)."""
    v = gold.npz("tiny_solid.npz")
    seqs, quals = _odd_reads(gold.fastq_nt6("tiny.fq.gz"))
    for step in (5, 0):
        g = _ecfix_gpu(gpu, 17, v["w17_o3_bucket"], v["w17_o3_key"], v["w17_o3_val"], seqs, quals, step)
        w = orcbind.ec_fix(17, v["w17_o3_bucket"], v["w17_o3_key"], v["w17_o3_val"], seqs, quals, step)
        assert np.array_equal(g[3], w[3]) and np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])


def test_correct_phase2_on_the_golden_table(gpu, gold, tmp_path):
    """fmdh_correct_reads (GPU correction pass + host marking, filter, printing) over the golden solid table ==
    `fermi correct -t1` output, byte for byte, with any number of host threads."""
    from fermi_amd import hostlib
    v = gold.npz("tiny_solid.npz")
    for threads in (1, 5):
        out = str(tmp_path / ("ec%d.fq" % threads))
        hostlib.lib().fmdh_correct_set_threads(threads)
        try:
            hostlib.correct_reads(17, 3, v["w17_o3_bucket"], v["w17_o3_key"], v["w17_o3_val"], gold.path("tiny.fq.gz"), out)
        finally:
            hostlib.lib().fmdh_correct_set_threads(1)
        assert open(out, "rb").read() == gold.text_gz("tiny.ec.fq.gz")


def test_check_left_flags_vs_oracle(gpu, gold, oracle_lib):
    for name, mm, ml in (("tiny", 50, 100), ("repeat", 20, 80), ("special", 20, 60)):
        d = gpu.DevIndex.open(gold.path(name + ".fmd")); o = orcbind.OrcIndex(gold.path(name + ".fmd"))
        ids = np.arange(int(o.mcnt[1]), dtype=U64)
        g = d.overlap(ids, mm, max_len=ml, max_nei=8); w = o.overlap_batch(ids, mm, max_len=ml, max_nei=8)
        assert np.array_equal(g[0]["reserved"], w[0]["reserved"]), name
        for f in ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei"):  # flags are GPU-side diagnostics
            assert np.array_equal(g[0][f], w[0][f]), (name, f)
        assert g[1].tobytes() == w[1].tobytes(), name
        d.close(); o.close()


def _cli(*args):
    import subprocess, os
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fermi_amd", "bin", "fermi-amd")
    assert os.path.exists(exe), "fermi-amd is not built (make cli)"
    return subprocess.run([exe] + list(args), stdout=subprocess.PIPE, check=True).stdout


def test_exact_cli_equals_fermi_exact(gpu, gold, tmp_path):
    """`fermi-amd exact [-s]` == `fermi exact [-s]` bytes (SMEMs on the GPU, printing on the host)."""
    fq = str(tmp_path / "tiny.fq")
    open(fq, "wb").write(gold.text_gz("tiny.fq.gz"))
    assert _cli("exact", gold.path("tiny.fmd"), fq) == gold.text_gz("tiny.exact.gz")
    assert _cli("exact", "-s", gold.path("tiny.fmd"), gold.path("tiny.fq.gz")) == gold.text_gz("tiny.exact_s.gz")


def test_correct_cli_equals_fermi_correct(gpu, gold):
    """`fermi-amd correct` == `fermi correct -t1` bytes: GPU k-mer harvest + host ec_fix."""
    assert _cli("correct", "-t4", gold.path("tiny.fmd"), gold.path("tiny.fq.gz")) == gold.text_gz("tiny.ec.fq.gz")


@pytest.mark.parametrize("n_rep", [2, 3, 5])
def test_correct_and_exact_sharded_over_replicas(gpu, gold, n_rep):
    """`correct -g a,b,..`: the harvest sharded by the k-mer's last base (whole trees of the trie, at most four GPUs), the table on
    every GPU, each batch of reads split over the GPUs; `exact -g a,b,..`: the index on every GPU, each batch of queries split.
    Replicas on GPU 0 where the box has one GPU (distinct GPUs where it has more): the bytes are the single-GPU ones, i.e. the
    reference's."""
    n_gpu = gpu.device_count()
    devs = ",".join(str(g % n_gpu) for g in range(n_rep))
    assert _cli("correct", "-t4", "-g", devs, gold.path("tiny.fmd"), gold.path("tiny.fq.gz")) == gold.text_gz("tiny.ec.fq.gz")
    assert _cli("exact", "-g", devs, gold.path("tiny.fmd"), gold.path("tiny.fq.gz")) == gold.text_gz("tiny.exact.gz")
    assert _cli("exact", "-s", "-g", devs, gold.path("tiny.fmd"), gold.path("tiny.fq.gz")) == gold.text_gz("tiny.exact_s.gz")


@pytest.mark.parametrize("name", ["tiny", "special", "repeat"])
def test_build_cli_equals_fermi_build(gpu, gold, tmp_path, name):
    """`fermi-amd build -fo x.fmd reads.fq` writes the file `fermi build` wrote, byte for byte."""
    out = str(tmp_path / "x.fmd")
    _cli("build", "-fo", out, gold.path(name + ".fq.gz"))
    assert open(out, "rb").read() == open(gold.path(name + ".fmd"), "rb").read()


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_bucketed_builder_equals_one_shot(gpu, gold, oracle_lib, monkeypatch, depth):
    """The >= 2^32-symbol construction path (buckets by the first `depth` symbols, 64-bit positions), forced on
    small inputs, gives the same BWT as `fermi build` -- ragged reads, Ns and sequences shorter than the prefix included."""
    from fermi_amd import hostlib
    monkeypatch.setenv("FMD_BUILD_BUCKETED", "1")
    monkeypatch.setenv("FMD_BUILD_DEPTH", str(depth))
    tiny_reads = [np.array(x, dtype=np.uint8) for x in ([1], [2, 2], [4, 5, 1], [3], [1, 2], [1])]   # tails shorter than any prefix
    monkeypatch.delenv("FMD_BUILD_BUCKETED")
    want_small = gpu.build_bwt(tiny_reads)                      # the one-shot builder (equal to `fermi build` on every fixture)
    monkeypatch.setenv("FMD_BUILD_BUCKETED", "1")
    assert np.array_equal(gpu.build_bwt(tiny_reads), want_small)
    for name in ("tiny", "special", "repeat"):
        reads = gold.fastq_nt6(name + ".fq.gz")
        reads = [r[:hostlib.trim_palindrome(r)] for r in reads]
        bwt = gpu.build_bwt(reads)
        o = orcbind.OrcIndex(gold.path(name + ".fmd"))
        assert np.array_equal(bwt, o.decode_all()), name
        o.close()


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_inplace_builder_gives_the_same_index(gpu, monkeypatch, depth):
    """fmd_builder_* (text 4 bits per symbol, no byte BWT: every bucket's slice goes straight into the planes of the device
    index, reads appended in pieces) == fmd_build_bwt + fmd_dev_open_bwt: the decoded BWT, the counts, the rank self-check
    and a backward search of every read."""
    import ctypes as C
    monkeypatch.setenv("FMD_BUILD_DEPTH", str(depth))
    for n, ln, err, seed in ((3000, 37, 0.02, 1), (501, 5, 0.0, 2), (2000, 100, 0.01, 3)):
        reads = synth.reads(synth.DEFAULT_SEED + seed, n, ln, 20, err)
        if seed == 1:
            reads[::17, 3] = 5                                  # some Ns
        a = gpu.build_index_inplace(reads, pieces=3)
        want = gpu.build_bwt(reads)
        got = np.zeros(a.n, dtype=np.uint8)
        gpu.check(gpu.lib().fmd_dev_export_bwt(a.h, 0, a.n, got.ctypes.data))
        assert a.n == len(want) and np.array_equal(got, want)
        b = gpu.DevIndex.from_bwt(want)
        assert np.array_equal(a.cnt, b.cnt) and np.array_equal(a.mcnt, b.mcnt)
        bad, first = C.c_uint64(), C.c_uint64()
        gpu.check(gpu.lib().fmd_dev_check_rank(a.h, C.byref(bad), C.byref(first)))
        assert bad.value == 0
        ca, cb = a.backward_search(reads), b.backward_search(reads)
        assert all(np.array_equal(x, y) for x, y in zip(ca, cb)) and (ca[0] >= 1).all()
        a.close(); b.close()


@pytest.mark.parametrize("depth", [1, 3])
def test_builders_with_the_ended_suffixes_set_aside(gpu, gold, oracle_lib, monkeypatch, depth):
    """FMD_BUILD_PARTITION=1 (off by default): before a chunk is sorted, the suffixes that ended in front of it keep their order at the head of
    the bucket by two stable selections and only the rest gets keys and a sort.  The bucketed byte-BWT builder on the fixtures (uniform, ragged,
    Ns) == `fermi build`; the in-place builder on reads of 100 bp (five chunks, buckets of several selection tiles) and 37 bp == the one-shot builder."""
    from fermi_amd import hostlib
    monkeypatch.setenv("FMD_BUILD_DEPTH", str(depth))
    monkeypatch.setenv("FMD_BUILD_PARTITION", "1")
    monkeypatch.setenv("FMD_BUILD_BUCKETED", "1")
    for name in ("tiny", "special", "repeat"):
        reads = gold.fastq_nt6(name + ".fq.gz")
        reads = [r[:hostlib.trim_palindrome(r)] for r in reads]
        o = orcbind.OrcIndex(gold.path(name + ".fmd"))
        assert np.array_equal(gpu.build_bwt(reads), o.decode_all()), name
        o.close()
    monkeypatch.delenv("FMD_BUILD_BUCKETED")
    for n, ln, err, seed in ((6000, 100, 0.01, 3), (3000, 37, 0.02, 1)):
        reads = synth.reads(synth.DEFAULT_SEED + seed, n, ln, 20, err)
        monkeypatch.setenv("FMD_BUILD_PARTITION", "1")
        a = gpu.build_index_inplace(reads, pieces=3)
        monkeypatch.setenv("FMD_BUILD_PARTITION", "0")
        want = gpu.build_bwt(reads)
        got = np.zeros(a.n, dtype=np.uint8)
        gpu.check(gpu.lib().fmd_dev_export_bwt(a.h, 0, a.n, got.ctypes.data))
        assert a.n == len(want) and np.array_equal(got, want), (n, ln)
        a.close()


@pytest.mark.parametrize("name,mm", [("tiny", 50), ("repeat", 20), ("special", 20)])
def test_seqsort_and_unitig_r_cli(gpu, gold, tmp_path, name, mm):
    """`fermi-amd seqsort` == `fermi seqsort` bytes; `fermi-amd unitig -r` == `fermi unitig -t1 -r` bytes."""
    rank = _cli("seqsort", gold.path(name + ".fmd"))
    assert rank == open(gold.path(name + ".rank"), "rb").read()
    rf = str(tmp_path / "x.rank")
    open(rf, "wb").write(rank)
    assert _cli("unitig", "-l%d" % mm, "-r", rf, gold.path(name + ".fmd")) == gold.text_gz(name + ".r.mag.gz")
    assert _cli("unitig", "-l%d" % mm, gold.path(name + ".fmd")) == gold.text_gz(name + ".mag.gz")


def _contigs_nt6(path):
    import gzip
    lines = gzip.open(path, "rt").read().split("\n")
    nt6 = {c: i for i, c in enumerate("$ACGTN")}
    return [np.array([nt6[c] for c in s], dtype=np.uint8) for s in lines[1::4] if s]


@pytest.mark.gpu
def test_smem_chain_of_contigs_vs_oracle(gpu, gold, oracle_lib):
    """fm6_smem over long sequences the way `fermi remap` walks them (fm6_miter_next, smem.c:96-102):
    forward reach of every position -> chain of start positions -> one fm6_smem1_core work item per
    position == the sequential chain of the oracle, for unitigs, the genome, a chimera, a reverse strand."""
    from fermi_amd import api
    d = api.DevIndex.open(gold.path("pairs.fmd"))
    o = orcbind.OrcIndex(gold.path("pairs.fmd"))
    for s in _contigs_nt6(gold.path("pairs_contigs.fq.gz")):
        want = o.smem(s, 0)
        got = d.smem_chain(s, max_len=64)
        assert got.tobytes() == want.tobytes(), (len(s), len(got), len(want))
        full = d.smem_chain(s, max_len=64, full_only=True)
        keep = ((want["info"] >> np.uint64(63)) != 0) & (want["x"][:, 1] < o.mcnt[1])
        assert full.tobytes() == want[keep].tobytes()
    o.close(); d.close()


def test_reach_vs_oracle_backward_search(gpu, gold, oracle_lib):
    """fmd_reach: longest indexed prefix at every position == the longest hit of fm_backward_search on
    the reverse complement (checked position by position on a chimera with a foreign insert)."""
    from fermi_amd import api
    d = api.DevIndex.open(gold.path("pairs.fmd"))
    o = orcbind.OrcIndex(gold.path("pairs.fmd"))
    s = _contigs_nt6(gold.path("pairs_contigs.fq.gz"))[3][:700].copy()
    s[300:310] = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 1], dtype=np.uint8)
    buf = np.concatenate([s, [0], s[:50], [0, 0, 0]]).astype(np.uint8)
    got = d.reach(buf)
    for p in range(len(buf)):
        if buf[p] == 0:
            assert got[p] == 0
            continue
        e = p
        while buf[e] != 0:
            e += 1
        want = 0
        for m in range(1, min(e - p, 70) + 1):       # matches are monotone: stop at the first miss
            q = (5 - buf[p:p + m])[::-1].copy()
            cnt, _, _ = o.backward_search(q[None, :])
            if cnt[0] == 0:
                break
            want = m
        assert got[p] == want, (p, got[p], want)
    o.close(); d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,args", [("u", []), ("p", ["-l", "20", "-D", "600", "-r", "RANK"]),
                                       ("c", ["-l", "20", "-D", "600", "-c", "2", "-r", "RANK"]), ("d", ["-D", "310", "-c", "1", "-t", "3", "-r", "RANK"])])
def test_remap_cli_equals_fermi_remap(gpu, gold, mode, args):
    """`fermi-amd remap` == `fermi remap -t1` bytes (stdout) and its insert-size line (stderr)."""
    import json, os, subprocess
    args = [gold.path("pairs.rank") if a == "RANK" else a for a in args]
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fermi_amd", "bin", "fermi-amd")
    p = subprocess.run([exe, "remap"] + args + [gold.path("pairs.fmd"), gold.path("pairs_contigs.fq.gz")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    assert p.stdout == gold.text_gz("pairs.remap_%s.gz" % mode)
    assert [l for l in p.stderr.decode().split("\n") if "fm6_remap" in l] == json.load(open(gold.path("pairs.remap_stderr.json")))[mode]


def test_unpack_cli_equals_fermi_unpack(gpu, gold):
    """`fermi-amd unpack` == `fermi unpack` bytes (every sequence + its rank), and the -i selection."""
    want = gold.text_gz("tiny.unpack.gz")
    assert _cli("unpack", gold.path("tiny.fmd")) == want
    lines = want.split(b"\n")
    assert _cli("unpack", "-i", "5", "-i", "99999999", "-i", "0", "-i", "3999", gold.path("tiny.fmd")) == b"\n".join([lines[5], lines[0], lines[3999]]) + b"\n"


@pytest.mark.parametrize("name", ["tiny", "special", "dup32", "pairs"])
def test_chkbwt_cli(gpu, gold, oracle_lib, name):
    """`fermi-amd chkbwt -p` prints the BWT `fermi chkbwt -p` prints (decoded back from the device
    planes), and -r (rank self-check on the GPU) passes."""
    import hashlib, json
    e = orcbind.OrcIndex(gold.path(name + ".fmd"))
    want = np.frombuffer(b"$ACGTN", dtype=np.uint8)[e.decode_all()].tobytes() + b"\n"
    e.close()
    got = _cli("chkbwt", "-r", "-p", gold.path(name + ".fmd"))
    assert got == want
    if name == "tiny":
        assert hashlib.md5(got).hexdigest() == json.load(open(gold.path("MANIFEST.json")))["tiny_bwt_md5"]


@pytest.mark.parametrize("flag,name", [([], "pairs.exact_contigs.gz"), (["-s"], "pairs.exact_s_contigs.gz")])
def test_exact_cli_long_queries(gpu, gold, flag, name):
    """`fermi-amd exact [-s]` with queries longer than the per-read path handles (contigs against a read
    index): reach + chain work items (or, with -s, one chain-walking item) == `fermi exact` bytes."""
    assert _cli("exact", *flag, gold.path("pairs.fmd"), gold.path("pairs_contigs.fq.gz")) == gold.text_gz(name)


@pytest.mark.parametrize("name", ["tiny", "special"])
def test_backward_search_around_the_prefix_table(gpu, gold, oracle_lib, name):
    """Queries shorter than, equal to and longer than the prefix-table depth, with ambiguous bases and
    sentinels' neighbours in every position of the table window, hits and misses: == the oracle."""
    from fermi_amd import api
    d = api.DevIndex.open(gold.path(name + ".fmd"))
    o = orcbind.OrcIndex(gold.path(name + ".fmd"))
    rng = np.random.default_rng(5)
    seqs, _, _ = o.retrieve(np.arange(0, 400, dtype=np.uint64), 128)
    base = [s[:40][::-1].copy() for s in seqs if (s[:40] != 0).all()][:200]
    for L in [1, 2, 3, 5, 7, 8, 9, 11, 12, 13, 16, 25, 40]:
        qs = []
        for b in base:
            q = b[len(b) - L:].copy()
            r = rng.integers(0, 4)
            if r == 1: q[rng.integers(0, L)] = 5                                  # an N somewhere
            elif r == 2: q[rng.integers(0, L)] = 1 + (q[rng.integers(0, L)] % 4)  # a (possible) mismatch
            qs.append(q)
        qs = np.array(qs, dtype=np.uint8)
        cnt, beg, end = d.backward_search(qs)
        wc, wb, we = o.backward_search(qs)
        hit = wc > 0
        assert np.array_equal(cnt, wc), L
        assert np.array_equal(beg[hit], wb[hit]) and np.array_equal(end[hit], we[hit]), L
    o.close(); d.close()


def test_large_index_properties(gpu):
    """Size-independent properties at a size the oracle would not finish in seconds (300 k reads, 6*10^7
    symbols, index built on the GPU; the prefix table is 12 deep here like at the bench size):
      * every read is found by backward search;
      * fm_retrieve inverts the index: sequence id 2i is read i, 2i+1 its reverse complement, the ranks are a
        permutation of the sentinels;
      * overlap records: rank/len agree with retrieve, the `$read$` interval of a strand and of its
        reverse strand mirror each other (x[0] <-> x[1]), and unique irreducible overlaps are mutual:
        if b is the only right neighbour of a with overlap o, then a^1 follows b^1 with the same o;
      * an indexed read is its own single, sentinel-closed SMEM with the multiplicity backward search reports."""
    import os
    N, L = 300_000, 100
    reads = synth.reads(synth.DEFAULT_SEED, N)
    bwt = gpu.build_bwt(reads)
    d = gpu.DevIndex.from_bwt(bwt)
    assert d.n == 2 * N * (L + 1)
    cnt, beg, end = d.backward_search(reads)
    assert (cnt >= 1).all()
    ids = np.arange(2 * N, dtype=U64)
    seqs, ln, rank = d.retrieve(ids, stride=128)
    assert (ln == L).all()
    assert np.array_equal(seqs[0::2, :L], reads)
    assert np.array_equal(seqs[1::2, :L], (5 - reads)[:, ::-1])
    assert np.array_equal(np.sort(rank), np.arange(2 * N, dtype=U64))
    assert (end - beg + 1 == cnt).all()
    rec, nei, seq = d.overlap(ids, 50, L, 4, check_left=False)
    assert np.array_equal(rec["rank"], rank) and (rec["len"] == L).all()
    ok = rec["status"] == 0
    a = np.where(ok)[0]
    assert np.array_equal(rec["k"][a, 0], rec["k"][a ^ 1, 1]) and np.array_equal(rec["k"][a, 2], rec["k"][a ^ 1, 2])
    # mutual unique overlaps: map `$read$` interval starts back to sequence ids
    row_of = np.full(2 * N, -1, dtype=np.int64)
    row_of[rec["k"][a, 0].astype(np.int64)] = a
    u = np.where(ok & (rec["n_nei"] == 1))[0]
    b = row_of[nei["x"][u, 0, 0].astype(np.int64)]
    good = b >= 0
    u, b = u[good], b[good]
    back = (rec["n_nei"][b ^ 1] == 1) & ok[b ^ 1] & (rec["k"][u, 2] == 1) & (rec["k"][b, 2] == 1)   # duplicated reads share a row
    u, b = u[back], b[back]
    assert len(u) > N // 2
    assert np.array_equal(row_of[nei["x"][b ^ 1, 0, 0].astype(np.int64)], u ^ 1)
    assert np.array_equal(nei["info"][b ^ 1, 0], nei["info"][u, 0])
    # an indexed, error-free read is its own single SMEM, closed by sentinels on both sides, as often as it occurs
    mems = d.smem(reads[:50_000], 0, max_mem=8)
    assert all(len(m) == 1 for m in mems)
    m0 = np.concatenate(mems)
    assert (m0["info"] == np.uint64(1 << 63 | L)).all() and (m0["x"][:, 1] < np.uint64(2 * N)).all()
    assert np.array_equal(m0["x"][:, 2], cnt[:50_000])
    d.close()


def test_kmer_harvest_cross_checked_by_backward_search(gpu):
    """Two independent kernels must agree at a size beyond the oracle: every (k+1)-mer the harvest calls
    solid occurs at least min_occ times according to backward search, its k-mer prefix at least as often,
    and no k-mer is reported twice (100 k reads with 1 % errors, index built on the GPU)."""
    N, L, w, min_occ = 100_000, 100, 19, 3
    reads = synth.reads(synth.DEFAULT_SEED, N, err=0.01)
    d = gpu.DevIndex.from_bwt(gpu.build_bwt(reads))
    suf = w - 15
    b, k, v, cnt = d.kmer_collect(w, min_occ, suf)
    assert len(b) == cnt[0] and len(b) > N
    K = (k.astype(np.uint64) >> np.uint64(2)) << np.uint64(2 * suf) | b.astype(np.uint64)
    assert len(np.unique(K)) == len(K)
    sel = np.random.default_rng(1).choice(len(K), 200_000, replace=False)
    Ks, best = K[sel], (k[sel] & 3).astype(np.uint8)
    kmer = np.empty((len(sel), w + 1), dtype=np.uint8)
    kmer[:, 0] = best + 1                                                        # the base the table predicts, to the left
    for dd in range(w):
        kmer[:, w - dd] = ((Ks >> np.uint64(2 * dd)) & np.uint64(3)).astype(np.uint8) + 1   # base_0 = rightmost
    c1, _, _ = d.backward_search(kmer)
    c0, _, _ = d.backward_search(np.ascontiguousarray(kmer[:, 1:]))
    assert (c1 >= min_occ).all() and (c0 >= c1).all()
    # the stored ratio code: max / rest, capped at 31, rounded (correct.c:67-75) -- rest = k-mer count - best - '$' - N >= 0
    assert ((v[sel] >> 3) >= 1).all()
    d.close()


@pytest.mark.parametrize("L,cov,mm,err", [(300, 40, 100, 0.0), (251, 60, 60, 0.003), (150, 25, 31, 0.01)])
def test_overlap_longer_reads_vs_oracle(gpu, oracle_lib, L, cov, mm, err):
    """Reads longer than the bench's 100 bp, deep coverage: candidate lists beyond 32 entries (the
    lane-per-strand kernel), list capacities in the hundreds, intervals wider than the 64-position window
    late into the walk -- every record, neighbour and sequence equals the oracle's."""
    N = 3000
    reads = synth.reads(synth.DEFAULT_SEED + L, N, L, cov, err)
    bwt = gpu.build_bwt(reads)
    d = gpu.DevIndex.from_bwt(bwt)
    o = orcbind.OrcIndex(bwt=bwt)
    ids = np.arange(2 * N, dtype=U64)

    def compare(idl, max_len, max_nei):
        rec, nei, seq = d.overlap(idl, mm, max_len, max_nei, check_left=True)
        wrec, wnei, wseq = o.overlap_batch(idl, mm, max_len, max_nei, 4, check_left=True)
        over = (rec["flags"] & gpu.OVLP_F_OVERFLOW) != 0       # capacity exceeded: the caller runs these again, larger
        g = ~over
        for f in ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei", "reserved"):
            assert np.array_equal(rec[f][g], wrec[f][g]), f
        for j in range(max_nei):
            m = g & (wrec["n_nei"] > j)
            assert nei[m, j].tobytes() == wnei[m, j].tobytes(), j
        used = (wrec["len"] + np.maximum(wrec["ext_len"], 0)).astype(np.int64)
        for i in np.where(g & (wrec["status"] == 0))[0][::7]:
            assert np.array_equal(seq[i, :used[i]], wseq[i, :used[i]]), i
        return rec, over
    rec, over = compare(ids, L, 8)
    if over.any():
        assert over.sum() < len(ids) // 4
        rec2, over2 = compare(ids[over], 2 * L, 64)
        assert not over2.any()
    assert (rec["n_ovlp"] > 32).sum() > 0 or cov < 40
    d.close(); o.close()


def _same_overlap(a, b, max_nei):
    rec0, nei0, seq0 = a; rec1, nei1, seq1 = b
    assert rec1.tobytes() == rec0.tobytes()
    for j in range(max_nei):
        mj = rec0["n_nei"] > j
        assert nei1[mj, j].tobytes() == nei0[mj, j].tobytes(), j
    used = (rec0["len"] + np.maximum(rec0["ext_len"], 0)).astype(np.int64)
    for i in np.where(rec0["status"] == 0)[0]:
        assert np.array_equal(seq1[i, :used[i]], seq0[i, :used[i]]), i


@pytest.mark.parametrize("L,cov,mm,err,N", [(100, 30, 50, 0.0, 20000), (100, 30, 50, 0.01, 20000), (100, 60, 40, 0.003, 8000), (151, 12, 31, 0.02, 6000),
                                            (100, 80, 45, 0.0, 6000), (100, 80, 45, 0.005, 6000)])   # the last two: widest candidates of 32..63 occurrences, the 64-bit masks
def test_unforked_fast_path_equals_general_group_kernels(gpu, oracle_lib, monkeypatch, capfd, L, cov, mm, err, N):
    """The unforked path (k_ovl_nei_lane / k_ovl_nei_fast: candidates in the narrow form, no x[0]-side fetch, one shared window per strand and round; hands a strand
    on to k_ovl_nei_grp the moment its reads show a second base) against the general group kernels alone (FMD_OVLP_FAST=0) and the
    oracle: records incl. lfork, neighbours, appended bases.  Also: the fast path really ran, and with errors in the reads really
    handed strands on."""
    import re
    reads = synth.reads(synth.DEFAULT_SEED + 5 * L + cov, N, L, cov, err)
    bwt = gpu.build_bwt(reads)
    d = gpu.DevIndex.from_bwt(bwt)
    ids = np.arange(2 * N, dtype=U64)
    monkeypatch.setenv("FMD_OVLP_STATS", "1")
    capfd.readouterr()
    fast = d.overlap(ids, mm, L, 8, check_left=True)
    msg = capfd.readouterr().err
    monkeypatch.delenv("FMD_OVLP_STATS")
    monkeypatch.setenv("FMD_OVLP_FAST", "0")
    general = d.overlap(ids, mm, L, 8, check_left=True)
    monkeypatch.delenv("FMD_OVLP_FAST")
    _same_overlap(general, fast, 8)
    # the two forms of the unforked path: one lane per STRAND (k_ovl_nei_lane, what ran above for the classes up to 16 candidates: quiet rounds inline, full rounds
    # and admissions in batches -- also with a batch of one lane and of a whole wave) and one lane per CANDIDATE (k_ovl_nei_fast, FMD_NEI_LANE=0)
    for env in ({"FMD_NEI_LANE": "0"}, {"FMD_LANE_BATCH": "1"}, {"FMD_LANE_BATCH": "64", "FMD_LANE_TICKETS": "16"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        other = d.overlap(ids, mm, L, 8, check_left=True)
        for k in env:
            monkeypatch.delenv(k)
        _same_overlap(other, fast, 8)
        for f in ("lfork", "flags"):
            assert np.array_equal(other[0][f], fast[0][f]), (env, f)
    took = [(int(a), int(b)) for a, b in re.findall(r"(\d+) to the unforked path \((\d+) of them handed on\)", msg)]
    assert took and sum(a for a, _ in took) > N // 2, msg
    if err > 0:
        assert sum(b for _, b in took) > 0, msg
    o = orcbind.OrcIndex(bwt=bwt)
    sub = ids[:4000]
    wrec, wnei, wseq = o.overlap_batch(sub, mm, L, 8, 4, check_left=True)
    ok = (fast[0]["flags"][:4000] & gpu.OVLP_F_OVERFLOW) == 0     # (more than max_nei neighbours: the caller runs those again, larger)
    assert ok.sum() > 3900
    for f in ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei", "reserved"):   # (lfork: the oracle's is exact, the product's may say less)
        assert np.array_equal(fast[0][f][:4000][ok], wrec[f][ok]), f
    for j in range(8):
        mj = ok & (wrec["n_nei"] > j)
        assert fast[1][:4000][mj, j].tobytes() == wnei[mj, j].tobytes(), j
    d.close(); o.close()


@pytest.mark.parametrize("L,cov,mm,err,N", [(100, 30, 50, 0.01, 400000), (100, 30, 50, 0.0, 30000), (151, 12, 31, 0.02, 6000)])
def test_dealt_out_work_lists_equal_the_round_robin_deal(gpu, oracle_lib, monkeypatch, L, cov, mm, err, N):
    """The get_nei kernels take their strands from chunks of the work list handed out as the groups ask (fmd_deal_next) -- against the
    round-robin shares of rounds 1-3 (FMD_NEI_DYN=0, read at every launch) and the oracle: records, neighbours, appended bases.  The
    first set has more strands in its lists than the first chunks of the grid hold (8 * 10^5 strands: ~10^5 in the general list of the groups
    of 8 against 32 768 first positions), so waves come back for chunks; the others fit the first chunks (one strand per group: the old deal)."""
    reads = synth.reads(synth.DEFAULT_SEED + 11 * L + cov, N, L, cov, err)
    bwt = gpu.build_bwt(reads)
    d = gpu.DevIndex.from_bwt(bwt)
    ids = np.arange(2 * N, dtype=U64)
    dealt = d.overlap(ids, mm, L, 8, check_left=True)
    monkeypatch.setenv("FMD_NEI_DYN", "0")
    fixed = d.overlap(ids, mm, L, 8, check_left=True)
    monkeypatch.delenv("FMD_NEI_DYN")
    _same_overlap(fixed, dealt, 8)
    o = orcbind.OrcIndex(bwt=bwt)
    sub = ids[:3000]
    wrec, wnei, wseq = o.overlap_batch(sub, mm, L, 8, 4, check_left=True)
    ok = (dealt[0]["flags"][:3000] & gpu.OVLP_F_OVERFLOW) == 0
    assert ok.sum() > 2900
    for f in ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei", "reserved"):
        assert np.array_equal(dealt[0][f][:3000][ok], wrec[f][ok]), f
    for j in range(8):
        mj = ok & (wrec["n_nei"] > j)
        assert dealt[1][:3000][mj, j].tobytes() == wnei[mj, j].tobytes(), j
    d.close(); o.close()


@pytest.mark.parametrize("pipe", ["3,9,7", "8,2,2", "5,16,16"])
def test_overlap_pipelined_parts_equal_serial(gpu, oracle_lib, monkeypatch, pipe):
    """fmd_ovlp_dev cuts a large batch into parts and runs get_nei of one part on a second stream beside
    the walk of the next (FMD_OVLP_PIPE = parts, waves per CU of either phase; the default engages above
    2^21 strands).  Forced here on a small batch with ragged part sizes: records, neighbours and
    sequences equal the serial order byte for byte, and the oracle on a sample."""
    N = 20000
    reads = synth.reads(synth.DEFAULT_SEED + 77, N, 100, 30, 0.005)
    bwt = gpu.build_bwt(reads)
    d = gpu.DevIndex.from_bwt(bwt)
    ids = np.arange(2 * N - 37, dtype=U64)
    monkeypatch.setenv("FMD_OVLP_PIPE", "1")
    rec0, nei0, seq0 = d.overlap(ids, 50, 100, 8, check_left=True)
    monkeypatch.setenv("FMD_OVLP_PIPE", pipe)
    for _ in range(2):   # twice: the second call reuses the stream and the events
        rec1, nei1, seq1 = d.overlap(ids, 50, 100, 8, check_left=True)
        assert rec1.tobytes() == rec0.tobytes()
        m = rec0["n_nei"] > 0
        for j in range(8):
            mj = rec0["n_nei"] > j
            assert nei1[mj, j].tobytes() == nei0[mj, j].tobytes()
        used = (rec0["len"] + np.maximum(rec0["ext_len"], 0)).astype(np.int64)
        for i in np.where(rec0["status"] == 0)[0][::11]:
            assert np.array_equal(seq1[i, :used[i]], seq0[i, :used[i]]), i
        assert m.sum() > N
    o = orcbind.OrcIndex(bwt=bwt)
    sub = ids[:3000]
    wrec, wnei, wseq = o.overlap_batch(sub, 50, 100, 8, 4, check_left=True)
    for f in ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei", "reserved"):
        assert np.array_equal(rec1[f][:3000], wrec[f]), f
    d.close(); o.close()


@pytest.mark.parametrize("seed", list(range(40)))
def test_fuzz_small_read_sets(gpu, oracle_lib, tmp_path, seed):
    """Differential fuzzing over small, nasty read sets -- ragged lengths from 3 bases up (shorter than the
    prefix table is deep), Ns, exact duplicates, reverse-complement palindromes, both strands: GPU
    construction against `fermi build` (when the compiled reference travelled), then rank, backward search,
    overlap discovery, check_left, SMEM (both modes), the k-mer harvest and the SMEM chain of a long
    chimeric query, all against the oracle on the same index."""
    import os, subprocess
    from fermi_amd import hostlib
    rng = np.random.default_rng(1000 + seed)
    G = int(rng.integers(300, 1500))
    genome = rng.integers(1, 5, G).astype(np.uint8)
    reads = []
    for _ in range(int(rng.integers(150, 500))):
        L = int(rng.integers(3, 81)) if rng.random() < 0.8 else int(rng.integers(3, 14))
        p = int(rng.integers(0, G - L))
        r = genome[p:p + L].copy()
        if rng.random() < 0.5:
            r = (5 - r)[::-1].copy()
        if rng.random() < 0.05:
            r[int(rng.integers(0, L))] = 5
        reads.append(r)
    for _ in range(6):                                    # duplicates and palindromes
        reads.append(reads[int(rng.integers(0, len(reads)))].copy())
        x = genome[int(rng.integers(0, G - 12)):][:int(rng.integers(2, 12))]
        reads.append(np.concatenate([x, (5 - x)[::-1]]))
    tab = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    fq = str(tmp_path / "f.fq")
    with open(fq, "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, tab[r].tobytes().decode(), "I" * len(r)))
    trimmed = [r[:hostlib.trim_palindrome(r)] for r in reads]   # cmd.c:457-463
    bwt = gpu.build_bwt(trimmed)
    ref = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "fermi")
    if os.path.exists(ref):
        fmd = str(tmp_path / "f.fmd")
        subprocess.run([ref, "build", "-fo", fmd, fq], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        e = orcbind.OrcIndex(fmd)
        assert np.array_equal(bwt, e.decode_all())
        e.close()
    d = gpu.DevIndex.from_bwt(bwt)
    o = orcbind.OrcIndex(bwt=bwt)
    n, n_seq = d.n, int(o.mcnt[1])
    k = rng.integers(0, n, 20000).astype(U64); l = np.minimum(k + rng.integers(0, 200, 20000).astype(U64), U64(n - 1))
    k[::97] = NONE
    gk, gl = d.rank2a(k, l); wk, wl = o.rank2a(k, l)
    assert np.array_equal(gk, wk) and np.array_equal(gl, wl)
    # backward search: the reads, mutated copies, by length
    qs = [r.copy() for r in trimmed] + [r.copy() for r in trimmed[:200]]
    for q in qs[len(trimmed):]:
        q[int(rng.integers(0, len(q)))] = int(rng.integers(1, 6))
    cnt, beg, end = d.backward_search(qs)
    for Lq in sorted({len(q) for q in qs}):
        idx = [i for i, q in enumerate(qs) if len(q) == Lq]
        wc, wb, we = o.backward_search(np.array([qs[i] for i in idx], dtype=np.uint8))
        assert np.array_equal(cnt[idx], wc), Lq
        h = wc > 0
        assert np.array_equal(beg[idx][h], wb[h]) and np.array_equal(end[idx][h], we[h]), Lq
    # overlap discovery + check_left, short minimum so that short reads overlap too
    ids = np.arange(n_seq, dtype=U64)
    for mm in (5, 13):
        rec, nei, seq = d.overlap(ids, mm, 80, 16, check_left=True)
        wrec, wnei, wseq = o.overlap_batch(ids, mm, 80, 16, 2, check_left=True)
        g = (rec["flags"] & gpu.OVLP_F_OVERFLOW) == 0
        assert g.sum() > n_seq // 2
        for f in ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei", "reserved"):
            assert np.array_equal(rec[f][g], wrec[f][g]), (mm, f)
        for j in range(16):
            m = g & (wrec["n_nei"] > j)
            assert nei[m, j].tobytes() == wnei[m, j].tobytes(), (mm, j)
    # SMEM, both modes, reads and mutated reads
    for sm in (0, 1):
        got = d.smem(qs[:300] + qs[len(trimmed):], sm, max_mem=128)
        for q, m in zip(qs[:300] + qs[len(trimmed):], got):
            assert m.tobytes() == o.smem(q, sm).tobytes(), sm
    # k-mer harvest
    for (w, mo) in ((7, 2), (11, 1)):
        B, K, V, c2 = d.kmer_collect(w, mo, 1)
        per_bucket, wc2 = o.ec_collect(w, mo, 1)
        wB = np.concatenate([np.full(len(kv[0]), b, dtype=np.uint32) for b, kv in enumerate(per_bucket)])
        wK = np.concatenate([kv[0] for kv in per_bucket]); wV = np.concatenate([kv[1] for kv in per_bucket])
        a, b_ = np.lexsort([V, K, B]), np.lexsort([wV, wK, wB])
        assert np.array_equal(B[a], wB[b_]) and np.array_equal(K[a], wK[b_]) and np.array_equal(V[a], wV[b_]) and list(c2) == list(wc2), (w, mo)
    # the chain over a long chimeric query
    long_q = np.concatenate([t for t in trimmed[:40] if (t <= 4).all()] + [genome[:200]])
    assert d.smem_chain(long_q, max_len=128).tobytes() == o.smem(long_q, 0).tobytes()
    d.close(); o.close()


@pytest.mark.parametrize("seed", list(range(12)))
def test_fuzz_cli_against_reference_binary(gpu, tmp_path, seed):
    """Whole commands on random small read sets against the compiled reference (when it travelled):
    build, seqsort, unitig (with and without -r), exact (-s too), correct, remap (three option sets).
    A command the reference itself cannot finish on an input (abort, time-out) is skipped for that input."""
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ref, amd = os.path.join(root, "oracle", "_ref", "fermi"), os.path.join(root, "fermi_amd", "bin", "fermi-amd")
    if not os.path.exists(ref):
        pytest.skip("oracle/_ref/fermi is not here")
    rng = np.random.default_rng(7000 + seed)
    G = int(rng.integers(800, 4000))
    genome = rng.integers(1, 5, G).astype(np.uint8)
    if seed % 3 == 0:                                   # a repeat, so that forks and bubbles appear
        genome[G // 2:G // 2 + 150] = genome[50:200]
    tab = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    Lmax = int(rng.integers(36, 90))
    fq = str(tmp_path / "r.fq")
    with open(fq, "w") as f:
        for i in range(int(G * rng.integers(15, 40) / Lmax)):
            L = Lmax if rng.random() < 0.7 else int(rng.integers(25, Lmax + 1))
            p = int(rng.integers(0, G - L))
            r = genome[p:p + L].copy()
            if rng.random() < 0.5:
                r = (5 - r)[::-1].copy()
            if rng.random() < 0.3:
                j = int(rng.integers(0, L)); r[j] = 1 + (r[j] + int(rng.integers(0, 3))) % 4
            bases, quals = tab[r].tobytes().decode(), "".join(chr(33 + int(q)) for q in rng.integers(5, 41, L))
            odd = int(rng.integers(0, 12)) if seed % 4 == 1 else 99    # records the reader's corner cases decide (kseq.h:171-210)
            if odd == 0: f.write("@r%d\r\n%s\r\n+\r\n%s\r\n" % (i, bases, quals))                               # CR LF
            elif odd == 1: f.write("@r%d\tlane 3\n%s\n%s\n+r%d\n%s\n%s\n" % (i, bases[:L // 2], bases[L // 2:], i, quals[:L // 3], quals[L // 3:]))  # wrapped lines, a comment
            elif odd == 2: f.write(">r%d some text\n%s\n" % (i, bases))                                           # FASTA among FASTQ
            elif odd == 3: f.write("@r%d\v1\n%s\n+\n%s\n" % (i, bases, quals))                                   # the name ends at ANY white space
            else: f.write("@r%d\n%s\n+\n%s\n" % (i, bases, quals))

    def run(exe, args, out):
        try:
            with open(out, "wb") as fo:
                p = subprocess.run([exe] + args, stdout=fo, stderr=subprocess.DEVNULL, timeout=60)
            return p.returncode == 0
        except subprocess.TimeoutExpired:
            return False
    T = str(tmp_path)
    assert run(ref, ["build", "-fo", T + "/b.fmd", fq], T + "/b.log") and run(amd, ["build", "-fo", T + "/a.fmd", fq], T + "/a.log")
    assert open(T + "/a.fmd", "rb").read() == open(T + "/b.fmd", "rb").read()
    mm = str(int(rng.integers(12, 24)))
    cmds = [("seqsort", ["seqsort", T + "/b.fmd"], None),
            ("unitig", ["unitig", "-l", mm, T + "/b.fmd"], ["unitig", "-l", mm, "-t1", T + "/b.fmd"]),
            ("unitig-r", ["unitig", "-l", mm, "-r", T + "/b.seqsort", T + "/b.fmd"], ["unitig", "-l", mm, "-t1", "-r", T + "/b.seqsort", T + "/b.fmd"]),
            ("exact", ["exact", T + "/b.fmd", fq], None), ("exact-s", ["exact", "-s", T + "/b.fmd", fq], None),
            ("correct", ["correct", "-k", "13", "-t", "3", T + "/b.fmd", fq], ["correct", "-k", "13", "-t1", T + "/b.fmd", fq]),
            ("remap-u", ["remap", T + "/b.fmd", T + "/b.unitig"], None),
            ("remap-p", ["remap", "-l", "10", "-D", "400", "-r", T + "/b.seqsort", T + "/b.fmd", T + "/b.unitig"], None),
            ("remap-c", ["remap", "-l", "10", "-D", "400", "-c", "1", "-r", T + "/b.seqsort", T + "/b.fmd", T + "/b.unitig"], None)]
    compared, skipped = 0, []
    for name, a_args, r_args in cmds:
        if not run(ref, r_args or a_args, T + "/b." + name):
            skipped.append(name)                        # the reference itself gives up on this input
            continue
        assert run(amd, a_args, T + "/a." + name), name
        assert open(T + "/a." + name, "rb").read() == open(T + "/b." + name, "rb").read(), name
        compared += 1
    print("compared %d commands, reference gave up on %s" % (compared, skipped or "none"))
    assert compared >= 5


def _long_read_set(path, G, L, cov, seed):
    rng = np.random.default_rng(seed)
    genome = rng.integers(1, 5, G).astype(np.uint8)
    tab = np.frombuffer(b"$ACGTN", dtype=np.uint8)
    with open(path, "w") as f:
        for i in range(G * cov // L):
            p = int(rng.integers(0, G - L))
            r = genome[p:p + L].copy()
            if rng.random() < 0.5:
                r = (5 - r)[::-1].copy()
            f.write("@r%d\n%s\n+\n%s\n" % (i, tab[r].tobytes().decode(), "I" * L))


def test_the_tested_ceiling_of_sequence_length(gpu, tmp_path):
    """The reference's vectors grow without bound (kvec.h:76-82); here a candidate list holds at most 4095 entries, which caps a sequence at
    4000 + min_match bases (host/ovlp_table.c: the capacity ladder stops there).  Pinned on both sides of the limit:
      * reads of 3900 bases (lists of 3850 entries, the ladder's largest class): `unitig -l50` == the reference's bytes, through the re-run of the flagged rows;
      * reads of 5000 bases: the reference assembles them; `fermi-amd unitig` REFUSES -- exit status 1, nothing on stdout, and a message that names the limit --
        rather than truncating a list.  A hard edge the reference does not have, stated here so that it cannot move unnoticed."""
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ref, amd = os.path.join(root, "oracle", "_ref", "fermi"), os.path.join(root, "fermi_amd", "bin", "fermi-amd")
    have_ref = os.path.exists(ref)
    for L, ok in ((3900, True), (5000, False)):
        fq, fmd = str(tmp_path / ("l%d.fq" % L)), str(tmp_path / ("l%d.fmd" % L))
        _long_read_set(fq, 40000, L, 12, 1000 + L)
        subprocess.check_call([amd, "build", "-fo", fmd, fq], stderr=subprocess.DEVNULL)
        p = subprocess.run([amd, "unitig", "-l50", fmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        want = subprocess.run([ref, "unitig", "-l50", "-t1", fmd], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600) if have_ref else None
        if want is not None:
            assert want.returncode == 0 and len(want.stdout) > 30000                 # the reference has no such limit
        if ok:
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            if want is not None:
                assert p.stdout == want.stdout
        else:
            assert p.returncode == 1 and p.stdout == b"", (p.returncode, len(p.stdout))
            err = p.stderr.decode()
            assert "rows still overflow at max_len 4050" in err and "not supported" in err, err[-2000:]
