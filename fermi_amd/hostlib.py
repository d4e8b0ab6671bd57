"""ctypes view of libfmdhost.so (fermi_amd/host/*.c): file-format helpers in plain C."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfmdhost.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libfmdhost.so is not built; run `make host`")
        L = C.CDLL(LIB_PATH)
        L.fmdh_write_rld_from_rle6.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p]
        L.fmdh_write_rle6.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p]
        L.fmdh_write_rld_from_bwt.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p]
        L.fmdh_trim_palindrome.restype = C.c_uint32
        L.fmdh_trim_palindrome.argtypes = [C.c_void_p, C.c_uint32]
        class Shard(C.Structure):
            _fields_ = [("n", C.c_uint64), ("rec", C.c_void_p), ("off", C.c_void_p), ("chunk", C.POINTER(C.c_void_p)),
                        ("chunk_shift", C.c_uint32), ("max_nei", C.c_uint32), ("seq_stride", C.c_uint32)]
        class Table(C.Structure):
            _fields_ = [("n", C.c_uint64), ("n_shards", C.c_int), ("shard", C.POINTER(Shard)), ("side_of", C.c_void_p), ("side", Shard),
                        ("row_of", C.c_void_p), ("link", C.c_void_p)]
        L.fmdh_ovlp_table_link.argtypes = [C.POINTER(Table), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.Shard = Shard
        L.Table = Table
        L.fmdh_unitig_walk.argtypes = [C.POINTER(Table), C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
        L.fmdh_slim_stats.argtypes = [C.POINTER(Table), C.POINTER(C.c_uint64)]
        L.fmdh_unitig.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_void_p]
        class EcOpt(C.Structure):
            _fields_ = [("w", C.c_int), ("min_occ", C.c_int), ("keep_bad", C.c_int), ("is_paired", C.c_int), ("trim_l", C.c_int),
                        ("step", C.c_int), ("max_corr", C.c_float)]
        L.EcOpt = EcOpt
        L.fmdh_correct_reads.argtypes = [C.POINTER(EcOpt), C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p]
        L.fmdh_correct_kmer.argtypes = [C.c_uint64]
        class RemapOpt(C.Structure):
            _fields_ = [("skip", C.c_int), ("min_pcv", C.c_int), ("max_dist", C.c_int)]
        L.RemapOpt = RemapOpt
        L.fmdh_remap_new.restype = C.c_void_p
        L.fmdh_remap_new.argtypes = [C.POINTER(RemapOpt), C.c_void_p, C.c_uint64]
        L.fmdh_remap_contig.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.fmdh_remap_finish.argtypes = [C.c_void_p, C.c_void_p]
        L.fmdh_remap.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(RemapOpt), C.c_char_p, C.c_void_p]
        class PPart(C.Structure):
            _fields_ = [("seq", C.c_void_p), ("qual", C.c_void_p), ("len", C.c_void_p), ("n", C.c_size_t), ("bytes", C.c_size_t), ("has_qual", C.c_int), ("bad", C.c_int),
                        ("m_bytes", C.c_size_t), ("m_n", C.c_size_t)]
        L.PPart = PPart
        L.fmdh_seq_open.restype = C.c_void_p; L.fmdh_seq_open.argtypes = [C.c_char_p]
        L.fmdh_seq_read.argtypes = [C.c_void_p]
        L.fmdh_seq_bases.restype = C.c_void_p; L.fmdh_seq_bases.argtypes = [C.c_void_p]
        L.fmdh_seq_qual.restype = C.c_void_p; L.fmdh_seq_qual.argtypes = [C.c_void_p]
        L.fmdh_seq_close.restype = None; L.fmdh_seq_close.argtypes = [C.c_void_p]
        L.fmdh_pseq_open.restype = C.c_void_p; L.fmdh_pseq_open.argtypes = [C.c_char_p, C.c_int, C.c_size_t]
        L.fmdh_pseq_next.argtypes = [C.c_void_p, C.POINTER(C.POINTER(PPart)), C.POINTER(C.c_int)]
        L.fmdh_pseq_close.restype = None; L.fmdh_pseq_close.argtypes = [C.c_void_p]
        L.fmdh_api_unitig.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
        L.fmdh_api_correct.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
        L.fmdh_api_seqlen.argtypes = [C.c_int64, C.c_void_p, C.c_double]
        L.fmdh_sw_score.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_char_p]
        class SwAln(C.Structure):
            _fields_ = [(n, C.c_int) for n in ("score", "te", "qe", "tb", "qb")]
        L.SwAln = SwAln
        L.fmdh_sw_align.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.POINTER(SwAln)]
        for f, n in (("fmdh_kf_lgamma", 1), ("fmdh_kf_betai", 3), ("fmdh_scaf_correct_mean", 3)):
            getattr(L, f).restype = C.c_double; getattr(L, f).argtypes = [C.c_double] * n
        L.fmdh_scaf_pvalue.restype = C.c_double; L.fmdh_scaf_pvalue.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_double]
        vp = C.c_void_p
        L.fmdh_scaf_read.restype = vp; L.fmdh_scaf_read.argtypes = [C.c_char_p]
        L.fmdh_scaf_count.restype = C.c_size_t; L.fmdh_scaf_count.argtypes = [vp]
        L.fmdh_scaf_unitig_info.restype = None; L.fmdh_scaf_unitig_info.argtypes = [vp, C.c_size_t, vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.fmdh_scaf_entries.restype = C.c_uint64; L.fmdh_scaf_entries.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]
        L.fmdh_scaf_set_links.argtypes = [vp, vp, vp]
        L.fmdh_scaf_exclude.restype = None; L.fmdh_scaf_exclude.argtypes = [vp, C.c_double]
        L.fmdh_scaf_choose.argtypes = [vp, C.c_uint64, vp, vp, vp]
        L.fmdh_scaf_resolve_contained.restype = None; L.fmdh_scaf_resolve_contained.argtypes = [vp, C.c_uint32, C.c_double, C.c_double, C.c_int, vp]
        L.fmdh_scaf_print_links.restype = None; L.fmdh_scaf_print_links.argtypes = [vp, vp]
        L.fmdh_scaf_free.restype = None; L.fmdh_scaf_free.argtypes = [vp]
        L.fmdh_scaf_cal_rdist.restype = C.c_double; L.fmdh_scaf_cal_rdist.argtypes = [vp]
        L.fmdh_locate_hits.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.POINTER(vp), C.POINTER(C.c_uint64)]
        L.fmdh_kmer_text.restype = vp; L.fmdh_kmer_text.argtypes = [C.c_uint64, C.c_int, vp]
        L.fmdh_kcount_print_hist.restype = None; L.fmdh_kcount_print_hist.argtypes = [vp, vp, C.c_uint32]
        L.fmdh_kcmp_print_hist.restype = None; L.fmdh_kcmp_print_hist.argtypes = [vp, vp, C.c_uint32]
        L.fmdh_kmat_parse_sel.argtypes = [C.c_char_p, C.c_int, vp]
        L.fmdh_kmat_print_pt.restype = None; L.fmdh_kmat_print_pt.argtypes = [vp, vp, C.c_int]
        L.fmdh_kmat_print_sm.restype = None; L.fmdh_kmat_print_sm.argtypes = [vp, C.c_int, vp]
        L.fmdh_kprofile_print_kp.restype = None; L.fmdh_kprofile_print_kp.argtypes = [vp, C.c_int, vp, C.c_uint64]
        L.fmdh_kprofile_print_ks.argtypes = [vp, C.c_int, vp, C.c_uint64, C.c_int, vp]
        L.fmdh_kprofile_qual.argtypes = [vp, C.c_uint64, C.c_int, vp]
        L.fmdh_kprofile_run.argtypes = [vp, C.c_char_p, C.c_int, vp, C.c_int, C.c_int, C.c_size_t]
        L.fmdh_kgraph_compact_host.argtypes = [C.c_int, C.c_uint64, vp, vp, vp]
        L.fmdh_kgraph_print_gfa.argtypes = [vp, C.c_int, vp]
        L.fmdh_kgraph_print_fasta.argtypes = [vp, C.c_int, vp]
        L.fmdh_kgraph_print_arcs.restype = None; L.fmdh_kgraph_print_arcs.argtypes = [vp, C.c_int, C.c_uint64, vp, vp, vp]
        L.fmdh_kgraph_free.restype = None; L.fmdh_kgraph_free.argtypes = [vp]
        L.fmdh_kcgraph_compact_host.argtypes = [C.c_int, C.c_int, C.c_uint64, vp, vp, vp, vp, C.c_uint, vp]
        L.fmdh_kcgraph_print_gfa.argtypes = [vp, C.c_int, vp, C.c_int, C.c_uint]
        L.fmdh_kcgraph_print_fasta.argtypes = [vp, C.c_int, vp, C.c_int, C.c_uint]
        L.fmdh_kcgraph_print_arcs.restype = None; L.fmdh_kcgraph_print_arcs.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, vp, vp, vp, vp]
        L.fmdh_kcgraph_free.restype = None; L.fmdh_kcgraph_free.argtypes = [vp]
        L.fmdh_kcbubble_host.argtypes = [C.c_int, vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(vp)]
        L.fmdh_kbubble_print.argtypes = [vp, C.c_int, vp, C.c_uint64, vp, C.c_int]
        L.fmdh_asearch_pattern.argtypes = [vp, C.c_uint32, vp, vp]
        L.fmdh_esearch_cigar.restype = vp; L.fmdh_esearch_cigar.argtypes = [vp, C.c_uint32, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.fmdh_esearch_rankmap.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
        L.fmdh_esearch_patterns.argtypes = [vp, vp, C.c_uint64, C.c_size_t, vp, vp, vp]
        _lib = L
    return _lib


def _chk(rc, what):
    if rc != 0:
        raise OSError(-rc, "%s failed: %s" % (what, os.strerror(-rc)))


def write_rld_from_rle6(runs, path):
    runs = np.ascontiguousarray(runs, dtype=np.uint8)
    _chk(lib().fmdh_write_rld_from_rle6(runs.ctypes.data, len(runs), path.encode()), "write_rld_from_rle6")


def write_rld_from_rle6_ptr(ptr, n, path):
    _chk(lib().fmdh_write_rld_from_rle6(ptr, n, path.encode()), "write_rld_from_rle6")


def write_rle6(runs, path):
    runs = np.ascontiguousarray(runs, dtype=np.uint8)
    _chk(lib().fmdh_write_rle6(runs.ctypes.data, len(runs), path.encode()), "write_rle6")


def write_rld_from_bwt(bwt, path):
    bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
    _chk(lib().fmdh_write_rld_from_bwt(bwt.ctypes.data, len(bwt), path.encode()), "write_rld_from_bwt")


def trim_palindrome(seq):
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    return int(lib().fmdh_trim_palindrome(seq.ctypes.data, len(seq)))


LOCATE_RUN_DT = np.dtype([("rank", "<u8"), ("n", "<u4"), ("off", "<u4"), ("query", "<u4"), ("reserved", "<u4")])   # fmd_locate_run_t (include/fmd_hip.h)
LOCATE_HIT_DT = np.dtype([("id", "<u8"), ("query", "<u4"), ("off", "<u4")])                                       # fmdh_locate_hit_t (fmd_host.h)


def locate_hits(runs, n_seq, sorted_map=None):
    """fmdh_locate_hits: the runs of a locate expanded into hits (LOCATE_HIT_DT) sorted by (query, id, off); id = sorted_map[rank] >> 2 with seqsort's
    map, the sentinel rank itself without one.  ValueError when a run reaches a rank >= n_seq."""
    runs = np.ascontiguousarray(runs, dtype=LOCATE_RUN_DT)
    m = None if sorted_map is None else np.ascontiguousarray(sorted_map, dtype=np.uint64)
    if m is not None and len(m) < n_seq:
        raise ValueError("locate_hits: a map of %d entries for %d sequences" % (len(m), n_seq))
    p, n = C.c_void_p(), C.c_uint64()
    if lib().fmdh_locate_hits(runs.ctypes.data, len(runs), None if m is None else m.ctypes.data, n_seq, C.byref(p), C.byref(n)) != 0:
        raise ValueError("locate_hits: a run reaches beyond the %d sequences" % n_seq)
    hits = np.zeros(n.value, dtype=LOCATE_HIT_DT)
    if n.value:
        C.memmove(hits.ctypes.data, p.value, n.value * LOCATE_HIT_DT.itemsize)
    _libc.free(p)
    return hits


def kmer_text(kmer, k):
    """fmdh_kmer_text: the k bases of a packed k-mer (2 bits per base, A=0 C=1 G=2 T=3, the first base highest) as str; ValueError for k outside 1..32."""
    buf = C.create_string_buffer(40)
    if not lib().fmdh_kmer_text(int(kmer), int(k), buf):
        raise ValueError("kmer_text: k = %d is outside 1..32" % k)
    return buf.value.decode()


ASEARCH_HIT_DT = np.dtype([("beg", "<u8"), ("cnt", "<u8"), ("query", "<u4"), ("n_sub", "<u4"), ("sub", "<u2", 4)])   # fmd_asearch_hit_t (include/fmd_hip.h)


def asearch_pattern(query, hit):
    """fmdh_asearch_pattern: the pattern of an asearch hit -- `query` (nt6) with the hit's substitutions applied -- as a uint8 array; ValueError when a
    substitution lies outside the query or the list is not 0xffff-padded and in descending order of position."""
    q = np.ascontiguousarray(query, dtype=np.uint8)
    h = np.zeros(1, dtype=ASEARCH_HIT_DT)
    h[0] = hit
    out = np.zeros(max(len(q), 1), dtype=np.uint8)
    if lib().fmdh_asearch_pattern(q.ctypes.data, len(q), h.ctypes.data, out.ctypes.data) != 0:
        raise ValueError("asearch_pattern: a substitution list that does not fit a query of %d bases" % len(q))
    return out[:len(q)]


ESEARCH_HIT_DT = np.dtype([("beg", "<u8"), ("cnt", "<u8"), ("query", "<u4"), ("n_edit", "<u4"), ("len", "<u4"), ("reserved", "<u4")])   # fmd_esearch_hit_t (include/fmd_hip.h)


def esearch_cigar(query, pattern):
    """fmdh_esearch_cigar: (cigar, n_edit) of one optimal alignment of `pattern` to `query` (both nt6; a base outside A/C/G/T equals none): run lengths
    and '=' equal, 'X' substituted, 'I' a query base absent from the pattern, 'D' a pattern base absent from the query, from the start of both; n_edit
    = the edit distance = the operations that are not '='.  Traced back from the end, preferring the diagonal to 'I' and 'I' to 'D'."""
    q = np.ascontiguousarray(query, dtype=np.uint8); p = np.ascontiguousarray(pattern, dtype=np.uint8)
    ne = C.c_uint32()
    s = lib().fmdh_esearch_cigar(q.ctypes.data, len(q), p.ctypes.data, len(p), C.byref(ne))
    if not s:
        raise MemoryError("fmdh_esearch_cigar")
    try:
        return C.string_at(s).decode(), int(ne.value)
    finally:
        _libc.free(s)


def esearch_rankmap(dev_handle):
    """fmdh_esearch_rankmap (GPU): row_of[r] = the row whose LF-walk ends on sentinel rank r, for the index behind dev_handle (an api.DevIndex.h)."""
    p, n = C.c_void_p(), C.c_uint64()
    if lib().fmdh_esearch_rankmap(dev_handle, C.byref(p), C.byref(n)) != 0:
        raise RuntimeError("fmdh_esearch_rankmap failed")
    out = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), (max(n.value, 1),))[:n.value].copy()
    _libc.free(p)
    return out


def esearch_patterns(dev_handle, row_of, hits):
    """fmdh_esearch_patterns (GPU): the patterns of esearch hits (ESEARCH_HIT_DT), read back from the index: a list of uint8 arrays (nt6)."""
    hits = np.ascontiguousarray(hits, dtype=ESEARCH_HIT_DT)
    row_of = np.ascontiguousarray(row_of, dtype=np.uint64)
    off = np.zeros(len(hits) + 1, dtype=np.uint64)
    np.cumsum(hits["len"], out=off[1:])
    pats = np.zeros(int(off[-1]) + 1, dtype=np.uint8)
    if len(hits) and lib().fmdh_esearch_patterns(dev_handle, row_of.ctypes.data, len(row_of), len(hits), hits.ctypes.data, off.ctypes.data, pats.ctypes.data) != 0:
        raise RuntimeError("fmdh_esearch_patterns: hits that do not fit the index")
    return [pats[int(off[j]):int(off[j + 1])].copy() for j in range(len(hits))]


def kcount_hist_text(hist):
    """fmdh_kcount_print_hist: the lines `fermi-amd kcount` prints for a histogram (count <tab> n_kmers per non-empty bin), as one str."""
    import tempfile
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    with tempfile.NamedTemporaryFile() as tf:
        fp = _libc.fopen(tf.name.encode(), b"wb")
        lib().fmdh_kcount_print_hist(fp, hist.ctypes.data, len(hist))
        _libc.fclose(fp)
        return open(tf.name).read()


def kcmp_hist_text(hist2d):
    """fmdh_kcmp_print_hist: the lines `fermi-amd kcmp` prints for a square 2-D histogram (c0 <tab> c1 <tab> n_kmers per non-empty cell, row-major), as one str."""
    import tempfile
    hist2d = np.ascontiguousarray(hist2d, dtype=np.uint64)
    if hist2d.ndim != 2 or hist2d.shape[0] != hist2d.shape[1]:
        raise ValueError("kcmp_hist_text: the histogram is not square")
    with tempfile.NamedTemporaryFile() as tf:
        fp = _libc.fopen(tf.name.encode(), b"wb")
        lib().fmdh_kcmp_print_hist(fp, hist2d.ctypes.data, hist2d.shape[0])
        _libc.fclose(fp)
        return open(tf.name).read()


def _printed(call):
    """what call(FILE *) writes, as one str"""
    import tempfile
    with tempfile.NamedTemporaryFile() as tf:
        fp = _libc.fopen(tf.name.encode(), b"wb")
        try:
            call(fp)
        finally:
            _libc.fclose(fp)
        return open(tf.name).read()


def kmat_parse_sel(text, n_idx):
    """fmdh_kmat_parse_sel: the argument of `fermi-amd kmat -s` (None = not given) for n_idx indexes -> [(min, max)] * n_idx, max = None for no upper bound;
    ValueError where the command prints its usage (an entry without a colon, anything but digits, min > max, more entries than indexes)."""
    sel = np.zeros(18, dtype=np.uint32)               # fmd_kmat_sel_t: min[8], max[8], present, reserved
    if lib().fmdh_kmat_parse_sel(None if text is None else text.encode(), int(n_idx), sel.ctypes.data) != 0:
        raise ValueError("kmat_parse_sel: %r for %d indexes" % (text, n_idx))
    return [(int(sel[i]), None if sel[8 + i] == 0xFFFFFFFF else int(sel[8 + i])) for i in range(int(n_idx))]


def kmat_pt_text(hist):
    """fmdh_kmat_print_pt: the PT lines `fermi-amd kmat` prints for a pattern spectrum of 2^n cells (PT <tab> bits <tab> n_kmers per non-empty pattern, ascending
    by pattern; bits = n characters, index 0 first), as one str."""
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    n = len(hist).bit_length() - 1
    if hist.ndim != 1 or n < 1 or n > 8 or len(hist) != 1 << n:
        raise ValueError("kmat_pt_text: not the spectrum of 1 to 8 indexes")
    return _printed(lambda fp: lib().fmdh_kmat_print_pt(fp, hist.ctypes.data, n))


def kmat_sm_text(n_present, n_total):
    """fmdh_kmat_print_sm: the SM lines `fermi-amd kmat` prints (SM <tab> i <tab> n_present <tab> n_total per index), as one str."""
    if len(n_present) != len(n_total) or not 1 <= len(n_total) <= 8:
        raise ValueError("kmat_sm_text: one n_present and one n_total for each of 1 to 8 indexes")
    st = np.zeros(22, dtype=np.uint64)                # fmd_kmat_stat_t: n_kmers, n_total[8], n_present[8], ..
    st[1:1 + len(n_total)] = n_total; st[9:9 + len(n_present)] = n_present
    return _printed(lambda fp: lib().fmdh_kmat_print_sm(fp, len(n_total), st.ctypes.data))


def kprofile_kp_text(idx, counts):
    """fmdh_kprofile_print_kp: the line `fermi-amd kprofile` prints for one sequence's counts in index idx (KP <tab> idx <tab> c_0,c_1,..; * for no window)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    return _printed(lambda fp: lib().fmdh_kprofile_print_kp(fp, int(idx), counts.ctypes.data if len(counts) else None, len(counts)))


def kprofile_ks_text(idx, seq, k, counts):
    """fmdh_kprofile_print_ks: the line `kprofile -s` prints for one sequence (nt6) and its len - k + 1 counts in index idx: KS <tab> idx <tab> n_valid
    <tab> n_zero <tab> min <tab> median <tab> max <tab> mean over the windows without an N; median = the lower one, the last four * when n_valid = 0."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8); counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if len(counts) != max(0, len(seq) - int(k) + 1):
        raise ValueError("kprofile_ks_text: %d counts for %d bases and k = %d" % (len(counts), len(seq), k))
    def call(fp):
        if lib().fmdh_kprofile_print_ks(fp, int(idx), seq.ctypes.data if len(seq) else None, len(seq), int(k), counts.ctypes.data if len(counts) else None) != 0:
            raise MemoryError("fmdh_kprofile_print_ks")
    return _printed(call)


def kprofile_qual_text(length, k, counts):
    """fmdh_kprofile_qual: the quality line `kprofile -q` prints for a sequence of `length` bases and its length - k + 1 counts: per base the character
    33 + min(93, the largest count among the windows that cover it), 33 where no window does."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if len(counts) != max(0, int(length) - int(k) + 1):
        raise ValueError("kprofile_qual_text: %d counts for %d bases and k = %d" % (len(counts), length, k))
    buf = C.create_string_buffer(int(length) + 1)
    if lib().fmdh_kprofile_qual(counts.ctypes.data if len(counts) else None, int(length), int(k), buf) != 0:
        raise MemoryError("fmdh_kprofile_qual")
    return buf.value.decode()


def kprofile_run(query_path, dev_handles, k, mode="", batch_bases=0):
    """fmdh_kprofile_run (GPU): what `fermi-amd kprofile` prints for the queries of query_path against the open indexes (api.DevIndex.h each), as one str;
    mode "" = KP lines, "s" = KS lines, "q" = FASTQ (one index); batch_bases = the bases of a batch of queries (0 = the command's 64 MB)."""
    hs = (C.c_void_p * len(dev_handles))(*dev_handles)
    def call(fp):
        if lib().fmdh_kprofile_run(fp, query_path.encode(), len(dev_handles), hs, int(k), ord(mode) if mode else 0, int(batch_bases)) != 0:
            raise RuntimeError("fmdh_kprofile_run failed")
    return _printed(call)


def kgraph_compact_host(k, kmers, arcs, counts=None):
    """fmdh_kgraph_compact_host: the unitigs of the de Bruijn graph given by its ascending canonical k-mers and their arc bytes (include/fmd_hip.h, kgraph),
    walked by one thread on the host -> an api.KUnitigs whose stat has n_nodes, n_arcs, n_links, n_unitigs and n_cycles.  counts: carried along (default 0)."""
    from . import api
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64); arcs = np.ascontiguousarray(arcs, dtype=np.uint8)
    if len(arcs) != len(kmers):
        raise ValueError("kgraph_compact_host: %d k-mers and %d arc bytes" % (len(kmers), len(arcs)))
    g = api.KUnitigC()
    rc = lib().fmdh_kgraph_compact_host(int(k), len(kmers), kmers.ctypes.data if len(kmers) else None, arcs.ctypes.data if len(arcs) else None, C.addressof(g))
    if rc == 1:
        raise MemoryError("fmdh_kgraph_compact_host")
    if rc:
        raise ValueError("kgraph_compact_host: k = %d with %d nodes" % (k, len(kmers)))
    try:
        arrays = dict(kmers=kmers, arcs=arcs, counts=np.zeros(len(kmers), np.uint32) if counts is None else counts)
        for name, field, dt in api.KUnitigs.NODE[3:] + api.KUnitigs.UNITIG:
            n = int(g.n_nodes if field in ("unitig", "offset", "orient") else g.n_unitigs)
            a = np.zeros(n, dtype=dt)
            if n:
                C.memmove(a.ctypes.data, getattr(g, field), a.nbytes)
            arrays[name] = a
        out = api.KUnitigs(k, **arrays)
        out.stat = {f: getattr(g.stat, f) for f in ("n_nodes", "n_arcs", "n_links", "n_unitigs", "n_cycles")}
    finally:
        lib().fmdh_kgraph_free(C.addressof(g))
    return out


def kgraph_gfa_text(g):
    """fmdh_kgraph_print_gfa: what `fermi-amd kgraph` prints for an api.KUnitigs (H, S and L lines), as one str."""
    def call(fp):
        c = g.as_c()
        if lib().fmdh_kgraph_print_gfa(fp, g.k, C.addressof(c)) != 0:
            raise RuntimeError("fmdh_kgraph_print_gfa failed")
    return _printed(call)


def kgraph_fasta_text(g):
    """fmdh_kgraph_print_fasta: what `fermi-amd kgraph -f` prints for an api.KUnitigs, as one str."""
    def call(fp):
        c = g.as_c()
        if lib().fmdh_kgraph_print_fasta(fp, g.k, C.addressof(c)) != 0:
            raise RuntimeError("fmdh_kgraph_print_fasta failed")
    return _printed(call)


def kgraph_arcs_text(k, kmers, counts, arcs):
    """fmdh_kgraph_print_arcs: the lines `fermi-amd kgraph -a` prints (KMER <tab> count <tab> right <tab> left), as one str."""
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64); counts = np.ascontiguousarray(counts, dtype=np.uint32); arcs = np.ascontiguousarray(arcs, dtype=np.uint8)
    if not len(kmers) == len(counts) == len(arcs):
        raise ValueError("kgraph_arcs_text: arrays of different lengths")
    return _printed(lambda fp: lib().fmdh_kgraph_print_arcs(fp, int(k), len(kmers), kmers.ctypes.data if len(kmers) else None,
                                                           counts.ctypes.data if len(kmers) else None, arcs.ctypes.data if len(kmers) else None))


def kcgraph_compact_host(k, kmers, counts, uarcs, pattern, split=False, arcs=None):
    """fmdh_kcgraph_compact_host: the unitigs of the coloured de Bruijn graph given by its ascending canonical k-mers, their counts (n x N), union arc bytes and
    patterns (include/fmd_hip.h, kcgraph), walked by one thread on the host, with the per-unitig sums -> an api.KCUnitigs whose stat has n_nodes, n_arcs,
    n_links, n_unitigs, n_cycles and n_nodes_in.  split: FMD_KCGRAPH_SPLIT.  arcs (n x N): carried along (default 0)."""
    from . import api
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64); uarcs = np.ascontiguousarray(uarcs, dtype=np.uint8); pattern = np.ascontiguousarray(pattern, dtype=np.uint8)
    counts = np.asfortranarray(np.asarray(counts, dtype=np.uint32))
    if counts.ndim != 2:
        raise ValueError("kcgraph_compact_host: counts is not n x N")
    n, n_idx = counts.shape
    if not len(kmers) == len(uarcs) == len(pattern) == n:
        raise ValueError("kcgraph_compact_host: arrays of different lengths")
    g = api.KCUnitigC()
    d = lambda a: a.ctypes.data if a.size else None
    rc = lib().fmdh_kcgraph_compact_host(int(k), n_idx, n, d(kmers), d(counts), d(uarcs), d(pattern), api.KCGRAPH_SPLIT if split else 0, C.addressof(g))
    if rc == 1:
        raise MemoryError("fmdh_kcgraph_compact_host")
    if rc:
        raise ValueError("kcgraph_compact_host: k = %d with %d nodes of %d indexes" % (k, n, n_idx))
    try:
        arrays = dict(kmers=kmers, counts=counts, uarcs=uarcs, pattern=pattern, arcs=np.zeros((n, n_idx), np.uint8) if arcs is None else arcs)
        for name, field, dt in api.KCUnitigs.NODE[5:] + api.KCUnitigs.UNITIG:
            m = int(g.n_nodes if field in ("unitig", "offset", "orient") else g.n_unitigs)
            a = np.zeros(m * n_idx if field in ("u_count", "u_present") else m, dtype=dt)
            if m:
                C.memmove(a.ctypes.data, getattr(g, field), a.nbytes)
            arrays[name] = a
        out = api.KCUnitigs(k, n_idx, **arrays)
        out.stat = {f: getattr(g.stat.g, f) for f in ("n_nodes", "n_arcs", "n_links", "n_unitigs", "n_cycles")}
        out.stat["n_nodes_in"] = [int(v) for v in g.stat.n_nodes_in[:n_idx]]
    finally:
        lib().fmdh_kcgraph_free(C.addressof(g))
    return out


def _kcgraph_text(fn, name, g, pattern):
    want = 0
    if pattern is not None:
        if len(pattern) != g.n_idx or set(pattern) - set("01"):
            raise ValueError("%s: pattern %r for %d indexes" % (name, pattern, g.n_idx))
        want = sum(1 << i for i, c in enumerate(pattern) if c == "1")

    def call(fp):
        c = g.as_c()
        if fn(fp, g.k, C.addressof(c), int(pattern is not None), want) != 0:
            raise RuntimeError(name + " failed")
    return _printed(call)


def kcgraph_gfa_text(g, pattern=None):
    """fmdh_kcgraph_print_gfa: what `fermi-amd kcgraph [-p pattern]` prints for an api.KCUnitigs (H, S and L lines), as one str; pattern = the bits of -p."""
    return _kcgraph_text(lib().fmdh_kcgraph_print_gfa, "fmdh_kcgraph_print_gfa", g, pattern)


def kcgraph_fasta_text(g, pattern=None):
    """fmdh_kcgraph_print_fasta: what `fermi-amd kcgraph -f [-p pattern]` prints for an api.KCUnitigs, as one str."""
    return _kcgraph_text(lib().fmdh_kcgraph_print_fasta, "fmdh_kcgraph_print_fasta", g, pattern)


def kcgraph_arcs_text(k, min_occ, kmers, counts, arcs, uarcs):
    """fmdh_kcgraph_print_arcs: the lines `fermi-amd kcgraph -a` prints (KMER, the counts, the pattern, right and left of the union, right/left per index), as
    one str; counts and arcs are n x N."""
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64); uarcs = np.ascontiguousarray(uarcs, dtype=np.uint8)
    n = len(kmers)
    counts = np.asfortranarray(np.asarray(counts, dtype=np.uint32).reshape(n, -1)) if n else np.zeros((0, 1), np.uint32)
    arcs = np.asfortranarray(np.asarray(arcs, dtype=np.uint8).reshape(n, -1)) if n else np.zeros((0, 1), np.uint8)
    if counts.shape != arcs.shape or len(uarcs) != n:
        raise ValueError("kcgraph_arcs_text: arrays of different shapes")
    d = lambda a: a.ctypes.data if a.size else None
    return _printed(lambda fp: lib().fmdh_kcgraph_print_arcs(fp, int(k), counts.shape[1], int(min_occ), n, n, d(kmers), d(counts), d(arcs), d(uarcs)))


def kcbubble_host(g, max_len=0):
    """fmdh_kcbubble_host: (n_forks, bubbles) of the graph of an api.KCUnitigs -- its k-mers and union arc bytes alone, none of its labels --, every branch walked
    node by node by one thread on the host; bubbles is an api.KBUBBLE_DT array ascending by src (include/fmd_hip.h, kbubble)."""
    from . import api
    c = g.as_c()
    nf, n, ptr = C.c_uint64(), C.c_uint64(), C.c_void_p()
    rc = lib().fmdh_kcbubble_host(int(g.k), C.addressof(c), int(max_len), C.byref(nf), C.byref(n), C.byref(ptr))
    if rc == 1:
        raise MemoryError("fmdh_kcbubble_host")
    if rc:
        raise ValueError("kcbubble_host: k = %d with %d nodes" % (g.k, len(g.kmers)))
    try:
        out = np.zeros(n.value, dtype=api.KBUBBLE_DT)
        if n.value:
            C.memmove(out.ctypes.data, ptr, out.nbytes)
    finally:
        _libc.free(ptr)
    return int(nf.value), out


def kbubble_text(g, bubbles, differing_only=False):
    """fmdh_kbubble_print: the BB lines `fermi-amd kbubble [-d]` prints for the records `bubbles` (api.KBUBBLE_DT) over an api.KCUnitigs, as one str."""
    from . import api
    bubbles = np.ascontiguousarray(bubbles, dtype=api.KBUBBLE_DT)

    def call(fp):
        c = g.as_c()
        rc = lib().fmdh_kbubble_print(fp, g.k, C.addressof(c), len(bubbles), bubbles.ctypes.data if len(bubbles) else None, int(bool(differing_only)))
        if rc == 1:
            raise MemoryError("fmdh_kbubble_print")
        if rc:
            raise ValueError("kbubble_text: the records are not bubbles of this graph")
    return _printed(call)


def kbubble_sm_text(g, n_forks, n_bubbles):
    """the SM line of `fermi-amd kbubble`"""
    return "SM\t%d\t%d\t%d\t%d\n" % (len(g.kmers), len(g.u_nodes), n_forks, n_bubbles)


_libc = C.CDLL(None)
_libc.fopen.restype = C.c_void_p
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fclose.argtypes = [C.c_void_p]
_libc.free.argtypes = [C.c_void_p]
_libc.free.restype = None


def unitig_walk(shards, n_seq, min_match, out_path, sorted_map=None, max_nei=4, seq_stride=256, link=0, resolve=None, stats=None):
    """Replay the `fermi unitig -t1` walk over a packed per-id overlap table kept in len(shards) shards -- id i = row
    i // N of shard i % N; each shard = (prec[OVLP_DT], off[u64, n+1], var[u8]) as fmd_ovlp_pack_dev writes them.
    Writes MAG records to out_path."""
    L = lib()
    keep = []
    arr = (L.Shard * len(shards))()
    n_total = 0
    for k, (prec, off, var) in enumerate(shards):
        prec = np.ascontiguousarray(prec); off = np.ascontiguousarray(off, dtype=np.uint64)
        var = np.ascontiguousarray(var, dtype=np.uint8) if len(var) else np.zeros(8, np.uint8)
        chunk = (C.c_void_p * 1)(var.ctypes.data)
        keep += [prec, off, var, chunk]
        arr[k] = L.Shard(len(prec), prec.ctypes.data, off.ctypes.data, chunk, 40, max_nei, seq_stride)   # one chunk: shift beyond any row count
        n_total += len(prec)
    t = L.Table(n_total, len(shards), arr, None, L.Shard(), None, None)
    undecided = None
    if link:   # the parallel link pass of the product path (rec.reserved of decided edges is written in place)
        und, n_und = C.c_void_p(), C.c_uint64()
        _chk(L.fmdh_ovlp_table_link(C.byref(t), link, C.byref(und), C.byref(n_und)), "table_link")
        undecided = np.ctypeslib.as_array(C.cast(und, C.POINTER(C.c_uint64)), (n_und.value,)).copy() if n_und.value else np.zeros(0, np.uint64)
        _libc.free(und)
        if resolve is not None and len(undecided):   # the product runs fmd_ovlp_check_left on these ids (ovlp_table.c)
            vals = resolve(undecided)
            n_sh = len(shards)
            for i, v in zip(undecided, vals):
                keep[4 * int(i % n_sh)]["reserved"][int(i // n_sh)] = v
    if stats is not None:   # what the walk's own table (host/slim_table.c) makes of these rows
        st = (C.c_uint64 * 6)()
        _chk(L.fmdh_slim_stats(C.byref(t), st), "slim_stats")
        stats.update(bytes=st[0], big=st[1], ext_in_var=st[2], plain=st[3], own_seq=st[4], undecided=st[5])
    fp = _libc.fopen(out_path.encode(), b"wb")
    try:
        sm = None if sorted_map is None else np.ascontiguousarray(sorted_map, dtype=np.uint64)
        _chk(L.fmdh_unitig_walk(C.byref(t), n_seq, min_match, None if sm is None else sm.ctypes.data, fp), "unitig_walk")
    finally:
        _libc.fclose(fp)
        _libc.free(t.row_of); _libc.free(t.link)
    return undecided


class DistRoot:
    """fmdh_dist_root_t: the root of an N-process overlap job (fermi_amd.dist.DistJob with host_table = 2) keeps no packed table -- every piece is folded into
    the rows `unitig` walks as it arrives.  sink / ctx go into the job (row_sink, sink_ctx); feed() is the same entry for callers that hold pieces themselves."""

    def __init__(self, n_seq, max_len=128):
        L = lib()
        L.fmdh_dist_root_new.restype = C.c_void_p
        L.fmdh_dist_root_new.argtypes = [C.c_uint64, C.c_uint32]
        L.fmdh_dist_root_sink.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.fmdh_dist_root_rows.restype = C.c_uint64
        L.fmdh_dist_root_rows.argtypes = [C.c_void_p]
        L.fmdh_dist_root_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.fmdh_dist_root_free.argtypes = [C.c_void_p]
        L.fmdh_dist_root_free.restype = None
        L.fmdh_slim_free.argtypes = [C.c_void_p]
        L.fmdh_slim_bytes.restype = C.c_uint64
        L.fmdh_slim_bytes.argtypes = [C.c_void_p]
        L.fmdh_unitig_walk_slim.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        self.L, self.n_seq = L, n_seq
        self.ctx = L.fmdh_dist_root_new(n_seq, max_len)
        if not self.ctx:
            raise MemoryError("fmdh_dist_root_new")
        self.sink = C.cast(L.fmdh_dist_root_sink, C.c_void_p).value
        self.slim = None

    def feed(self, ids, prec, off, var, max_nei):
        ids = np.ascontiguousarray(ids, dtype=np.uint32); prec = np.ascontiguousarray(prec); off = np.ascontiguousarray(off, dtype=np.uint64)
        var = np.ascontiguousarray(var, dtype=np.uint8) if len(var) else np.zeros(8, np.uint8)
        _chk(self.L.fmdh_dist_root_sink(self.ctx, len(ids), ids.ctypes.data, prec.ctypes.data, off.ctypes.data, var.ctypes.data, max_nei), "dist_root_sink")

    def rows(self):
        return int(self.L.fmdh_dist_root_rows(self.ctx))

    def finish(self, min_match, dev_handle=None):
        """-> bytes of the table; the rows that exceeded a capacity and the edges lfork leaves open go through the GPU behind dev_handle (an api.DevIndex.h)"""
        slim = C.c_void_p()
        ctx, self.ctx = self.ctx, None
        if self.L.fmdh_dist_root_finish(ctx, dev_handle, min_match, C.byref(slim)):
            raise RuntimeError("fmdh_dist_root_finish failed")
        self.slim = slim
        return int(self.L.fmdh_slim_bytes(slim))

    def walk(self, min_match, out_path):
        fp = _libc.fopen(out_path.encode(), b"wb")
        try:
            _chk(self.L.fmdh_unitig_walk_slim(self.slim, self.n_seq, min_match, None, fp, 0), "unitig_walk_slim")
        finally:
            _libc.fclose(fp)

    def close(self):
        if self.ctx:
            self.L.fmdh_dist_root_free(self.ctx); self.ctx = None
        if self.slim:
            self.L.fmdh_slim_free(self.slim); self.slim = None


def unitig(fmd_path, min_match, out_path, devices=(0,)):
    """`fermi-amd unitig -l min_match -g d0,d1,.. fmd_path > out_path` (GPU)."""
    L = lib()
    dev = (C.c_int * len(devices))(*devices)
    fp = _libc.fopen(out_path.encode(), b"wb")
    try:
        rc = L.fmdh_unitig(fmd_path.encode(), len(devices), dev, min_match, None, fp)
    finally:
        _libc.fclose(fp)
    if rc:
        raise RuntimeError("fmdh_unitig failed")


def slim_build(fmd_path, min_match, devices=(0,)):
    """The table `fermi-amd unitig -l min_match -g d0,d1,..` walks, built and freed again: one index replica + one host thread per GPU, rows of ids
    i = g (mod G) streamed over each GPU's own PCIe link into the slim table, host threads link them.  -> dict of seconds / bytes (fmdh_slim_last_build)."""
    L = lib()
    dev = (C.c_int * len(devices))(*devices)
    slim, n_seq = C.c_void_p(), C.c_uint64()
    L.fmdh_slim_build.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.fmdh_slim_free.argtypes = [C.c_void_p]
    rc = L.fmdh_slim_build(fmd_path.encode(), len(devices), dev, min_match, C.byref(slim), C.byref(n_seq))
    if rc:
        raise RuntimeError("fmdh_slim_build failed")
    t = (C.c_double * 4)()
    L.fmdh_slim_last_build(t)
    L.fmdh_slim_free(slim)
    return {"n_seq": int(n_seq.value), "index_load_s": t[0], "rows_s": t[1], "build_s": t[2], "table_bytes": t[3]}


def correct_reads(w, min_occ, bucket, key, val, fq_path, out_path, step=5, max_corr=0.3, device=0):
    """ec_fix phase of `fermi correct` against a harvested solid-k-mer table (GPU correction pass + host marking/printing)."""
    L = lib()
    opt = L.EcOpt(w, min_occ, 0, 0, 0, step, max_corr)
    bucket = np.ascontiguousarray(bucket, dtype=np.uint32); key = np.ascontiguousarray(key, dtype=np.uint32)
    val = np.ascontiguousarray(val, dtype=np.uint8)
    fp = _libc.fopen(out_path.encode(), b"wb")
    try:
        rc = L.fmdh_correct_reads(C.byref(opt), device, w - 15 if w > 15 else 1, len(key), bucket.ctypes.data, key.ctypes.data, val.ctypes.data,
                                  fq_path.encode(), fp)
    finally:
        _libc.fclose(fp)
    if rc:
        raise RuntimeError("fmdh_correct_reads failed")


def remap_contigs(contigs, mems, n_seq, out_path, err_path, skip=50, min_pcv=0, max_dist=1000, sorted_map=None):
    """The host part of `fermi remap` (paircov + printing) over precomputed SMEM lists.
    contigs: list of (name, comment or None, nt6 array); mems: one INTV_DT array per contig, sorted by start."""
    L = lib()
    opt = L.RemapOpt(skip, min_pcv, max_dist)
    sm = None if sorted_map is None else np.ascontiguousarray(sorted_map, dtype=np.uint64)
    st = L.fmdh_remap_new(C.byref(opt), None if sm is None else sm.ctypes.data, n_seq)
    fp = _libc.fopen(out_path.encode(), b"wb"); fe = _libc.fopen(err_path.encode(), b"wb")
    try:
        for (name, comment, seq), m in zip(contigs, mems):
            buf = np.zeros(len(seq) + 1, dtype=np.uint8); buf[:len(seq)] = seq
            m = np.ascontiguousarray(m)
            L.fmdh_remap_contig(st, name.encode(), None if comment is None else comment.encode(), len(seq), buf.ctypes.data,
                                m.ctypes.data, len(m), fp)
        L.fmdh_remap_finish(st, fe)
    finally:
        _libc.fclose(fp); _libc.fclose(fe)


BIN_PATH = os.path.join(_HERE, "bin", "fermi-amd")


def clean(in_path, out_path, args=()):
    """`fermi-amd clean <args> in_path > out_path` (host/clean_cmd.c; no GPU): the graph cleaned as `fermi clean` cleans it."""
    import subprocess
    if not os.path.exists(BIN_PATH):
        raise RuntimeError("fermi-amd is not built; run `make cli`")
    with open(out_path, "wb") as out:
        p = subprocess.run([BIN_PATH, "clean"] + list(args) + [in_path], stdout=out, stderr=subprocess.PIPE)
    if p.returncode:
        raise RuntimeError("fermi-amd clean failed: " + p.stderr.decode(errors="replace").strip())


_NT4 = bytes.maketrans(b"ACGTacgt", bytes([0, 1, 2, 3, 0, 1, 2, 3]))


def sw_score(a, b):
    """fmdh_sw_score (host/swscore.c) of two sequences given as ACGT byte strings: the score of the local alignment the bubble poppers ask for."""
    a, b = bytes(a).translate(_NT4), bytes(b).translate(_NT4)
    return int(lib().fmdh_sw_score(len(a), a, len(b), b))


_NT6 = bytes.maketrans(b"ACGTNacgtn", bytes([1, 2, 3, 4, 5, 1, 2, 3, 4, 5]))


def sw_align(query, target):
    """fmdh_sw_align (host/scaf_stat.c) of two ACGT byte strings, handed over as nt6 codes the way `scaf` does: (score, te, qe, tb, qb) as
    ksw_align returns them with KSW_XSTART (match 1, mismatch -3, gap 5 + 2k)."""
    L = lib()
    q, t = bytes(query).translate(_NT6), bytes(target).translate(_NT6)
    r = L.SwAln()
    if L.fmdh_sw_align(len(q), q, len(t), t, C.byref(r)) != 0:
        raise MemoryError("fmdh_sw_align")
    return r.score, r.te, r.qe, r.tb, r.qb


def scaf_betai(a, b, x):
    return lib().fmdh_kf_betai(a, b, x)


def scaf_correct_mean(l, mu, sigma):
    return lib().fmdh_scaf_correct_mean(l, mu, sigma)


def _scaf_unitig_list(L, s):
    out = []
    for i in range(L.fmdh_scaf_count(s)):
        k, ilm, A, nr = (C.c_uint64 * 2)(), (C.c_int32 * 3)(), C.c_double(0), C.c_uint64(0)
        L.fmdh_scaf_unitig_info(s, i, k, ilm, C.byref(A), C.byref(nr))
        out.append(dict(k=(k[0], k[1]), len=ilm[0], nsr=ilm[1], maxo=ilm[2], A=A.value, n_reads=nr.value))
    return out


def scaf_unitigs(mag_path):
    """The reader and the statistics of `scaf` (host/scaf_core.c; no GPU) over a remapped MAG: (rdist, [dict per unitig with a UR:Z: tag])."""
    L = lib()
    s = L.fmdh_scaf_read(os.fsencode(mag_path))
    if not s:
        raise IOError("cannot read " + str(mag_path))
    try:
        rdist = L.fmdh_scaf_cal_rdist(s)
        return rdist, _scaf_unitig_list(L, s)
    finally:
        L.fmdh_scaf_free(s)


def scaf_link_lines(mag_path, links, max_dist, a_thres=20., details=False, avg=None, std=None):
    """The LK lines of `scaf -P` before any gap is patched, on the host: reader, rdist and A, then `links(x, span, utig, length, excluded,
    max_dist)` -- the link stage, as api.scaf_links or a restatement of it: (self, mate, gkey, gval, n_nei) -- and the choice of the best two
    neighbours of every end (fmdh_scaf_choose: the replay of the reference's small table).  Returns the lines; with details, also a dict of
    the unitigs, the entries' unitig and the two words per entry.
    With avg and std the contained unitigs are resolved as under -P (their CT lines come first)."""
    import tempfile
    L = lib()
    s = L.fmdh_scaf_read(os.fsencode(mag_path))
    if not s:
        raise IOError("cannot read " + str(mag_path))
    try:
        L.fmdh_scaf_cal_rdist(s)
        L.fmdh_scaf_exclude(s, a_thres)
        us = _scaf_unitig_list(L, s)
        exc = np.zeros(max(len(us), 1), dtype=np.uint8)
        px, ps, pu = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = L.fmdh_scaf_entries(s, C.byref(px), C.byref(ps), C.byref(pu), exc.ctypes.data)
        arr = lambda p, t, dt: np.frombuffer((t * n).from_address(p.value), dtype=dt).copy() if n else np.zeros(0, dtype=dt)
        x, span, utig = arr(px, C.c_uint64, np.uint64), arr(ps, C.c_uint64, np.uint64), arr(pu, C.c_uint32, np.uint32)
        own, mate, gkey, gval, n_nei = links(x, span, utig, np.array([u["len"] for u in us], dtype=np.int32), exc[:len(us)], max_dist)
        own, mate, gkey, gval = (np.ascontiguousarray(a, dtype=np.uint64) for a in (own, mate, gkey, gval))
        n_nei = np.ascontiguousarray(n_nei, dtype=np.uint32)
        if L.fmdh_scaf_set_links(s, own.ctypes.data, mate.ctypes.data) or L.fmdh_scaf_choose(s, len(gkey), gkey.ctypes.data, gval.ctypes.data, n_nei.ctypes.data):
            raise RuntimeError("fmdh_scaf_choose failed")
        with tempfile.NamedTemporaryFile() as tf:
            fp = _libc.fopen(tf.name.encode(), b"wb")
            if avg is not None:
                for i in range(len(us)):
                    L.fmdh_scaf_resolve_contained(s, i, float(avg), float(std), 1, fp)
            L.fmdh_scaf_print_links(s, fp)
            _libc.fclose(fp)
            lines = open(tf.name).read().split("\n")[:-1]
        return (lines, dict(unitigs=us, utig=utig, own=own, mate=mate)) if details else lines
    finally:
        L.fmdh_scaf_free(s)


def scaf(fmd_path, mag_path, avg, std, out_path, args=(), device=0):
    """`fermi-amd scaf <args> -g device fmd mag avg std > out_path` (host/scaf_cmd.c): scaftigs as `fermi scaf` writes them; returns stderr
    (with -P in args: the LK / CT / SW lines among it)."""
    import subprocess
    if not os.path.exists(BIN_PATH):
        raise RuntimeError("fermi-amd is not built; run `make cli`")
    with open(out_path, "wb") as out:
        p = subprocess.run([BIN_PATH, "scaf"] + list(args) + ["-g", str(device), fmd_path, mag_path, str(avg), str(std)], stdout=out, stderr=subprocess.PIPE)
    if p.returncode:
        raise RuntimeError("fermi-amd scaf failed: " + p.stderr.decode(errors="replace").strip())
    return p.stderr.decode(errors="replace")


def ropebwt(in_path, out_path, args=("-a", "bcr", "-bN"), device=0):
    """`fermi-amd ropebwt <args> -g device -o out_path in_path` (host/ropebwt_cmd.c over api.build_bwt_strands' entry, fmd_build_bwt_strands): the BWT
    of one strand or both as text, or with -b as RLE\\6 runs; returns stderr (the reference's warnings, and with -v3 the phase lines)."""
    import subprocess
    if not os.path.exists(BIN_PATH):
        raise RuntimeError("fermi-amd is not built; run `make cli`")
    p = subprocess.run([BIN_PATH, "ropebwt"] + list(args) + ["-g", str(device), "-o", out_path, in_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode:
        raise RuntimeError("fermi-amd ropebwt failed: " + p.stderr.decode(errors="replace").strip())
    return p.stderr.decode(errors="replace")


def _read_buffer(reads):
    """list of byte strings -> one buffer with a NUL after every read (what fm6_api_readseq returns, seq.c:385-408)"""
    return np.frombuffer(b"".join(r + b"\0" for r in reads), dtype=np.uint8).copy()


def api_unitig(reads, min_match, out_path, device=0):
    """fm6_api_unitig (unitig.c:413-434) over reads held in memory: list of ASCII byte strings -> MAG text in out_path."""
    L = lib()
    buf = _read_buffer(reads)
    fp = _libc.fopen(out_path.encode(), b"wb")
    try:
        if L.fmdh_api_unitig(device, min_match, len(buf), buf.ctypes.data, fp) != 0:
            raise RuntimeError("fmdh_api_unitig failed")
    finally:
        _libc.fclose(fp)


def api_correct(reads, quals, kmer, step=5, device=0):
    """fm6_api_correct (correct.c:464-511): -> (corrected reads, qualities) as lists of byte strings (upper case = kept, lower = corrected)."""
    L = lib()
    s, q = _read_buffer(reads), _read_buffer(quals)
    if L.fmdh_api_correct(device, kmer, step, len(s), s.ctypes.data, q.ctypes.data) != 0:
        raise RuntimeError("fmdh_api_correct failed")
    return s.tobytes().split(b"\0")[:-1], q.tobytes().split(b"\0")[:-1]


def read_records_serial(path):
    """[(bases, qualities or None)] as fmdh_seq_read gives them (seqio.c: the reader `build`, `correct`, `remap` use)."""
    L = lib()
    io = L.fmdh_seq_open(path.encode())
    out = []
    while True:
        n = L.fmdh_seq_read(io)
        if n < 0:
            break
        q = L.fmdh_seq_qual(io)
        out.append((C.string_at(L.fmdh_seq_bases(io), n), C.string_at(q, n) if q else None))
    L.fmdh_seq_close(io)
    return out, n


def read_records_parallel(path, threads, span):
    """the same records through fmdh_pseq_* (seqpar.c); None if the input cannot be mapped (gzip, stdin)."""
    L = lib()
    r = L.fmdh_pseq_open(path.encode(), threads, span)
    if not r:
        return None
    out = []
    parts, n_parts = C.POINTER(L.PPart)(), C.c_int()
    while L.fmdh_pseq_next(r, C.byref(parts), C.byref(n_parts)) == 1:
        for k in range(n_parts.value):
            p = parts[k]
            if p.n == 0:   # a cut guess that ran into the end of its span: no records, len never allocated
                continue
            lens = np.ctypeslib.as_array(C.cast(p.len, C.POINTER(C.c_uint32)), (max(p.n, 1),))[: p.n]
            seq = C.string_at(p.seq, p.bytes) if p.bytes else b""
            qual = C.string_at(p.qual, p.bytes) if p.bytes else b""
            o = 0
            for ln in lens:
                ln = int(ln)
                q = qual[o:o + ln]
                out.append((seq[o:o + ln], q if p.has_qual and (ln == 0 or any(q)) else None))
                o += ln
    L.fmdh_pseq_close(r)
    return out
