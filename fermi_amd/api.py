"""ctypes view of the C ABI in include/fmd_hip.h (libfmdhip.so) -- the product path.

Names mirror the reference's C API (rld.h:45-58, fermi.h:61-103): `rld_restore` -> DevIndex.open,
`rld_rank1a` -> rank1a, `rld_rank2a` -> rank2a, `fm6_extend` -> extend, `fm_backward_search` ->
backward_search, `fm_retrieve` -> retrieve.  Everything here runs on the GPU; there is no CPU
fallback -- if the library or a device is missing the calls raise FmdError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMD_HIP_LIB") or os.path.join(_HERE, "lib", "libfmdhip.so")  # FMD_HIP_LIB: A/B builds
INTV_DT = np.dtype([("x", "<u8", 3), ("info", "<u8")])  # fmd_intv_t == fmintv_t (fermi.h:13-16)
NONE64 = np.uint64(0xFFFFFFFFFFFFFFFF)
OVLP_DT = np.dtype([("rank", "<u8"), ("k", "<u8", 3), ("len", "<i4"), ("status", "<i4"), ("n_ovlp", "<i4"),
                    ("rbeg", "<i4"), ("ext_len", "<i4"), ("n_nei", "<i4"), ("flags", "<u4"), ("reserved", "<u2"), ("lfork", "<u2")])
OVLP_F_FORKED, OVLP_F_OVERFLOW, OVLP_F_FIXED = 1, 2, 4
LOCATE_RUN_DT = np.dtype([("rank", "<u8"), ("n", "<u4"), ("off", "<u4"), ("query", "<u4"), ("reserved", "<u4")])  # fmd_locate_run_t
LOCATE_STAT_DT = np.dtype([(f, "<u8") for f in ("n_runs", "n_rows", "n_skipped", "n_unfinished", "overflow", "n_ext")])  # fmd_locate_stat_t
KCOUNT_STAT_DT = np.dtype([(f, "<u8") for f in ("n_kmers", "n_total", "n_ext", "overflow", "widest_level", "n_parts", "n_retries")])  # fmd_kcount_stat_t
KCOUNT_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32))  # fmd_kcount_sink_fn
KCOUNT_MIN_CAP, KCOUNT_MAX_CAP = 4096, 1 << 30   # FMD_KCOUNT_MIN_CAP, FMD_KCOUNT_MAX_CAP
KCMP_STAT_DT = np.dtype([(f, "<u8") for f in ("n_kmers", "n_total0", "n_total1", "n_only0", "n_only1", "n_shared", "n_ext", "overflow", "widest_level", "n_parts", "n_retries")])  # fmd_kcmp_stat_t
KCMP_NODE_DT = np.dtype([("x0", "<u8", 2), ("size", "<u8", 2), ("kmer", "<u8"), ("reserved", "<u8")])  # fmd_kcmp_node_t
KCMP_SEL_DT = np.dtype([(f, "<u4") for f in ("min0", "max0", "min1", "max1")])  # fmd_kcmp_sel_t
KCMP_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))  # fmd_kcmp_sink_fn
KCMP_MIN_CAP, KCMP_MAX_CAP, KCMP_NO_MAX = 4096, 1 << 30, 0xFFFFFFFF   # FMD_KCMP_MIN_CAP, FMD_KCMP_MAX_CAP, FMD_KCMP_NO_MAX
KMAT_MAX_IDX, KMAT_MIN_CAP, KMAT_MAX_CAP, KMAT_NO_MAX = 8, 4096, 1 << 30, 0xFFFFFFFF   # FMD_KMAT_MAX_IDX, FMD_KMAT_MIN_CAP, FMD_KMAT_MAX_CAP, FMD_KMAT_NO_MAX
KMAT_SEL_DT = np.dtype([("min", "<u4", 8), ("max", "<u4", 8), ("present", "<u4"), ("reserved", "<u4")])  # fmd_kmat_sel_t
KMAT_STAT_DT = np.dtype([("n_kmers", "<u8"), ("n_total", "<u8", 8), ("n_present", "<u8", 8), ("n_ext", "<u8"), ("overflow", "<u8"), ("widest_level", "<u8"), ("n_parts", "<u8"),
                         ("n_retries", "<u8")])  # fmd_kmat_stat_t
KMAT_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.POINTER(C.c_uint32)))  # fmd_kmat_sink_fn
KPROFILE_STAT_DT = np.dtype([(f, "<u8") for f in ("n_windows", "n_valid", "n_hit", "n_ext", "n_table")])  # fmd_kprofile_stat_t
KPROFILE_MAX_K, KPROFILE_PLAIN = 255, 1   # FMD_KPROFILE_MAX_K, FMD_KPROFILE_PLAIN
KGRAPH_STAT_DT = np.dtype([(f, "<u8") for f in ("n_nodes", "n_arcs", "n_links", "n_unitigs", "n_cycles", "n_ext", "n_rounds")] +
                          [(f, "<f8") for f in ("ms_arcs", "ms_links", "ms_label")])  # fmd_kgraph_stat_t
KARCS_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8))  # fmd_karcs_sink_fn
KGRAPH_MAX_NODES, KGRAPH_CYCLE = 0x7FFFFFFE, 1   # FMD_KGRAPH_MAX_NODES, FMD_KGRAPH_CYCLE
KCGRAPH_SPLIT = 1   # FMD_KCGRAPH_SPLIT
KCGRAPH_STAT_DT = np.dtype(KGRAPH_STAT_DT.descr + [("n_nodes_in", "<u8", 8), ("n_arcs_in", "<u8", 8)])  # fmd_kcgraph_stat_t
KCARCS_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint8)),
                          C.POINTER(C.c_uint8))  # fmd_kcarcs_sink_fn
KBUBBLE_DT = np.dtype([("src", "<u4"), ("dst", "<u4"), ("first", "<u4", 2), ("len", "<u4", 2)])  # fmd_kbubble_t
ASEARCH_HIT_DT = np.dtype([("beg", "<u8"), ("cnt", "<u8"), ("query", "<u4"), ("n_sub", "<u4"), ("sub", "<u2", 4)])  # fmd_asearch_hit_t
ASEARCH_STAT_DT = np.dtype([(f, "<u8") for f in ("n_hits", "n_occ", "n_skipped", "n_truncated", "n_unfinished", "overflow", "n_ext", "widest_level")])  # fmd_asearch_stat_t
ASEARCH_MAX_SUB, ASEARCH_MAX_LEN, ASEARCH_MIN_CAP, ASEARCH_MAX_CAP = 4, 16383, 4096, 1 << 28   # FMD_ASEARCH_*
ASEARCH_NO_PRUNE, ASEARCH_BEST = 1, 2
ESEARCH_HIT_DT = np.dtype([("beg", "<u8"), ("cnt", "<u8"), ("query", "<u4"), ("n_edit", "<u4"), ("len", "<u4"), ("reserved", "<u4")])  # fmd_esearch_hit_t
ESEARCH_STAT_DT = ASEARCH_STAT_DT                                                                           # fmd_esearch_stat_t: the same fields
ESEARCH_MAX_EDIT, ESEARCH_MAX_LEN, ESEARCH_MIN_CAP, ESEARCH_MAX_CAP = 4, 16383, 4096, 1 << 28   # FMD_ESEARCH_*
ESEARCH_NO_PRUNE, ESEARCH_BEST = 1, 2

# every symbol include/fmd_hip.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "fmd_strerror", "fmd_last_hip_error", "fmd_device_count",
    "fmd_dev_open_file", "fmd_dev_open_rld", "fmd_dev_open_rle6", "fmd_dev_open_bwt", "fmd_dev_open_bwt_dev",
    "fmd_dev_close", "fmd_dev_trim", "fmd_dev_info", "fmd_dev_sync", "fmd_dev_line_count",
    "fmd_rank1a_dev", "fmd_rank2a_dev", "fmd_rank1a_batch", "fmd_rank2a_batch",
    "fmd_extend_dev", "fmd_extend_batch", "fmd_bsearch_dev", "fmd_bsearch_batch",
    "fmd_retrieve_dev", "fmd_retrieve_batch", "fmd_probe_gather",
    "fmd_build_bwt", "fmd_build_bwt_dev", "fmd_build_bwt_strands", "fmd_build_bwt_strands_dev", "fmd_dev_free", "fmd_builder_new", "fmd_builder_add_dev", "fmd_builder_finish", "fmd_builder_free", "fmd_bwt_to_rle6", "fmd_host_free",
    "fmd_dev_malloc", "fmd_memcpy_h2d", "fmd_memcpy_d2h",
    "fmd_smem_work_bytes", "fmd_smem_dev", "fmd_smem_batch", "fmd_smem_win_dev", "fmd_smem_win_batch", "fmd_reach_dev", "fmd_reach_batch", "fmd_dev_export_bwt", "fmd_dev_check_rank", "fmd_dev_build_pairs", "fmd_dev_check_pairs", "fmd_dev_line_count3",
    "fmd_kmer_work_bytes", "fmd_kmer_collect_dev", "fmd_kmer_collect_part_dev", "fmd_kmer_collect", "fmd_kmer_collect_seeds",
    "fmd_ectab_build_dev", "fmd_ectab_build", "fmd_ectab_free", "fmd_ecfix_work_bytes", "fmd_ecfix_dev", "fmd_ecfix_batch", "fmd_ectab_line_count",
    "fmd_ovlp_work_bytes", "fmd_ovlp_dev", "fmd_ovlp_sorted_work_bytes", "fmd_ovlp_sorted_dev", "fmd_ovlp_batch", "fmd_ovlp_check_left_dev", "fmd_seqinfo_dev", "fmd_seqinfo_batch",
    "fmd_ovlp_pack_max_bytes", "fmd_ovlp_pack_work_bytes", "fmd_ovlp_pack_dev", "fmd_ovlp_packed_batch", "fmd_ovlp_packed_free", "fmd_table_alloc", "fmd_table_free", "fmd_ovlp_link_dev", "fmd_ovlp_packed_table",
    "fmd_ovlp_packed_stream", "fmd_ovlp_tabjob_rows", "fmd_ovlp_tabjob_patch", "fmd_ovlp_tabjob_link", "fmd_ovlp_tabjob_free",
    "fmd_ovlp_two_pass_ok", "fmd_ovlp_head_work_bytes", "fmd_ovlp_head_dev", "fmd_ovlp_tail_dev", "fmd_ovlp_pack_rows_dev",
    "fmd_comm_rccl_unique_id", "fmd_comm_rccl_init", "fmd_comm_rccl_version", "fmd_comm_rccl_count", "fmd_comm_free",
    "fmd_ovlp_side_work_bytes", "fmd_ovlp_rerun_overflow_dev",
    "fmd_ovlp_dist_new", "fmd_ovlp_dist_step", "fmd_ovlp_dist_table", "fmd_ovlp_dist_local", "fmd_ovlp_dist_free",
    "fmd_dev_open_file_ex", "fmd_dev_open_bwt_ex", "fmd_merge_work_bytes", "fmd_merge_walk_dev", "fmd_merge_interleave_dev", "fmd_dev_merge", "fmd_dev_merge_ex", "fmd_memset_dev",
    "fmd_contrast_work_bytes", "fmd_contrast_dev", "fmd_contrast", "fmd_sub_work_bytes", "fmd_sub_mark_dev", "fmd_sub_select_dev", "fmd_dev_sub",
    "fmd_fltuniq_table_bytes", "fmd_fltuniq_count_dev", "fmd_fltuniq_test_dev", "fmd_fltuniq", "fmd_fltuniq_table",
    "fmd_fltuniq_open", "fmd_fltuniq_slot", "fmd_fltuniq_count", "fmd_fltuniq_test", "fmd_fltuniq_sync", "fmd_fltuniq_export", "fmd_fltuniq_close",
    "fmd_fltuniq_batch_limits",
    "fmd_scaf_links_work_bytes", "fmd_scaf_links_dev", "fmd_scaf_links",
    "fmd_multi_bsearch_work_bytes", "fmd_multi_bsearch_dev", "fmd_multi_bsearch_batch",
    "fmd_locate_work_bytes", "fmd_locate_dev", "fmd_locate_batch",
    "fmd_kcount_work_bytes", "fmd_kcount_part_dev", "fmd_kcount",
    "fmd_kcmp_work_bytes", "fmd_kcmp_part_dev", "fmd_kcmp",
    "fmd_kmat_node_bytes", "fmd_kmat_work_bytes", "fmd_kmat_part_dev", "fmd_kmat",
    "fmd_kprofile_dev", "fmd_kprofile_batch",
    "fmd_karcs", "fmd_kunitig",
    "fmd_kcarcs", "fmd_kcunitig",
    "fmd_kcbubble", "fmd_kcbubble_dev",
    "fmd_asearch_work_bytes", "fmd_asearch_bound_dev", "fmd_asearch_dev", "fmd_asearch_batch",
    "fmd_esearch_work_bytes", "fmd_esearch_dev", "fmd_esearch_batch",
]


class FmdError(RuntimeError):
    pass


# status codes of include/fmd_hip.h
FMD_OK, FMD_E_NODEV, FMD_E_ARG, FMD_E_FORMAT, FMD_E_IO, FMD_E_NOMEM, FMD_E_HIP, FMD_E_OVERFLOW = 0, -1, -2, -3, -4, -5, -6, -7


class Info(C.Structure):
    _fields_ = [("cnt", C.c_uint64 * 7), ("mcnt", C.c_uint64 * 7), ("n_blocks", C.c_uint64),
                ("hbm_bytes", C.c_uint64), ("device", C.c_int)]


class KGraphStatC(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_nodes", "n_arcs", "n_links", "n_unitigs", "n_cycles", "n_ext", "n_rounds")] + \
               [(f, C.c_double) for f in ("ms_arcs", "ms_links", "ms_label")]


class KUnitigC(C.Structure):
    """fmd_kunitig_t"""
    _fields_ = [("n_nodes", C.c_uint64), ("n_unitigs", C.c_uint64)] + \
               [(f, C.c_void_p) for f in ("kmer", "count", "arcs", "unitig", "offset", "orient", "u_nodes", "u_first", "u_flags")] + [("stat", KGraphStatC)]


class KCGraphStatC(C.Structure):
    """fmd_kcgraph_stat_t"""
    _fields_ = [("g", KGraphStatC), ("n_nodes_in", C.c_uint64 * 8), ("n_arcs_in", C.c_uint64 * 8)]


class KCUnitigC(C.Structure):
    """fmd_kcunitig_t"""
    _fields_ = [("n_nodes", C.c_uint64), ("n_unitigs", C.c_uint64), ("n_idx", C.c_int32), ("reserved", C.c_int32)] + \
               [(f, C.c_void_p) for f in ("kmer", "count", "arcs", "uarcs", "pattern", "unitig", "offset", "orient", "u_nodes", "u_first", "u_flags", "u_count",
                                          "u_present", "u_pattern")] + [("stat", KCGraphStatC)]


class KCBubbleC(C.Structure):
    """fmd_kcbubble_t"""
    _fields_ = [("g", KCUnitigC), ("n_forks", C.c_uint64), ("n_bubbles", C.c_uint64), ("bubble", C.c_void_p), ("ms_bubble", C.c_double)]


def _kcgraph_stat(st, n_idx):
    """a KCGraphStatC as a dict: kgraph's fields on the union graph, n_nodes_in and n_arcs_in as lists of n_idx"""
    out = {f: getattr(st.g, f) for f in KGRAPH_STAT_DT.names}
    out["n_nodes_in"] = [int(v) for v in st.n_nodes_in[:n_idx]]; out["n_arcs_in"] = [int(v) for v in st.n_arcs_in[:n_idx]]
    return out


class KUnitigs:
    """The compacted de Bruijn graph of DevIndex.kmer_unitigs (fmd_kunitig_t as numpy arrays).  Per node, ascending by k-mer: kmers uint64, counts uint32,
    arcs uint8, unitig uint32, offset uint32, orient uint8 (1 = the node reads reversed in the printed unitig); per unitig: u_nodes uint32, u_first uint32
    (the node at offset 0), u_flags uint8 (KGRAPH_CYCLE); stat = the fields of KGRAPH_STAT_DT as a dict (None when not asked for)."""
    NODE = (("kmers", "kmer", np.uint64), ("counts", "count", np.uint32), ("arcs", "arcs", np.uint8), ("unitig", "unitig", np.uint32),
            ("offset", "offset", np.uint32), ("orient", "orient", np.uint8))
    UNITIG = (("u_nodes", "u_nodes", np.uint32), ("u_first", "u_first", np.uint32), ("u_flags", "u_flags", np.uint8))

    def __init__(self, k, **arrays):
        self.k, self.stat = int(k), None
        for name, _, dt in self.NODE + self.UNITIG:
            setattr(self, name, np.ascontiguousarray(arrays[name], dtype=dt))

    def as_c(self):
        """a KUnitigC over these arrays (they must outlive it)"""
        g = KUnitigC()
        g.n_nodes, g.n_unitigs = len(self.kmers), len(self.u_nodes)
        for name, field, _ in self.NODE + self.UNITIG:
            a = getattr(self, name)
            setattr(g, field, a.ctypes.data if len(a) else None)
        return g

    def strings(self):
        """the unitigs as printed: one str per unitig, u_nodes + k - 1 bases"""
        k = self.k
        first = np.zeros(len(self.u_nodes) + 1, dtype=np.int64)
        np.cumsum(self.u_nodes, out=first[1:])
        order = np.zeros(len(self.kmers), dtype=np.int64)
        order[first[self.unitig.astype(np.int64)] + self.offset.astype(np.int64)] = np.arange(len(self.kmers))
        sh = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
        base = ((self.kmers[:, None] >> sh) & np.uint64(3)).astype(np.int64)          # the bases of every node, forward
        rev = self.orient.astype(bool)
        base[rev] = 3 - base[rev][:, ::-1]
        out = []
        for u in range(len(self.u_nodes)):
            nodes = order[first[u]:first[u + 1]]
            s = np.concatenate([base[nodes[0]], base[nodes[1:], k - 1]])
            out.append("".join("ACGT"[c] for c in s))
        return out


_lib = None
_count_lib = None
COUNT_LIB_PATH = os.path.join(_HERE, "lib", "libfmdhip_count.so")  # same sources, gathers instrumented (-DFMD_COUNT_LINES=1)


def _configure(L):
    """Prototypes of include/fmd_hip.h on a loaded library."""
    vp, sz, u64p = C.c_void_p, C.c_size_t, C.c_void_p
    L.fmd_strerror.restype = C.c_char_p; L.fmd_strerror.argtypes = [C.c_int]
    L.fmd_last_hip_error.restype = C.c_char_p
    L.fmd_device_count.restype = C.c_int
    L.fmd_dev_open_file.argtypes = [C.c_int, C.c_char_p, C.POINTER(vp)]
    L.fmd_dev_open_rld.argtypes = [C.c_int, vp, C.c_uint64, vp, C.POINTER(vp)]
    L.fmd_dev_open_rle6.argtypes = [C.c_int, vp, C.c_uint64, C.POINTER(vp)]
    L.fmd_dev_open_bwt.argtypes = [C.c_int, vp, C.c_uint64, C.POINTER(vp)]
    L.fmd_dev_open_bwt_dev.argtypes = [C.c_int, vp, C.c_uint64, C.POINTER(vp)]
    L.fmd_dev_open_file_ex.argtypes = [C.c_int, C.c_char_p, C.c_uint, C.POINTER(vp)]
    L.fmd_dev_open_bwt_ex.argtypes = [C.c_int, vp, C.c_uint64, C.c_uint, C.POINTER(vp)]
    L.fmd_merge_work_bytes.restype = sz; L.fmd_merge_work_bytes.argtypes = [C.c_uint64]
    L.fmd_merge_walk_dev.argtypes = [vp, vp, vp, vp, vp, sz, C.POINTER(C.c_int)]
    L.fmd_merge_interleave_dev.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, C.c_uint64, vp]
    L.fmd_dev_merge.argtypes = [vp, vp, C.POINTER(vp)]
    L.fmd_dev_merge_ex.argtypes = [vp, vp, C.c_uint, C.POINTER(vp)]
    L.fmd_memset_dev.argtypes = [vp, C.c_int, sz, vp]
    L.fmd_contrast_work_bytes.restype = sz; L.fmd_contrast_work_bytes.argtypes = [C.c_uint64]
    L.fmd_contrast_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, sz, C.c_uint64, vp]
    L.fmd_contrast.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp)]
    L.fmd_sub_work_bytes.restype = sz; L.fmd_sub_work_bytes.argtypes = [C.c_uint64]
    L.fmd_sub_mark_dev.argtypes = [vp, vp, vp, vp, vp, sz, vp]
    L.fmd_sub_select_dev.argtypes = [vp, vp, vp, vp, C.c_int, C.c_uint64, C.c_uint64, vp]
    L.fmd_dev_sub.argtypes = [vp, vp, C.c_int, C.c_uint, C.POINTER(vp)]
    L.fmd_fltuniq_table_bytes.restype = sz; L.fmd_fltuniq_table_bytes.argtypes = [C.c_int]
    L.fmd_fltuniq_count_dev.argtypes = [C.c_int, vp, C.c_int, vp, u64p, C.c_uint64, u64p]
    L.fmd_fltuniq_test_dev.argtypes = [C.c_int, vp, C.c_int, vp, u64p, C.c_uint64, u64p, vp]
    L.fmd_fltuniq.argtypes = [C.c_int, C.c_int, vp, u64p, C.c_uint64, vp]
    L.fmd_fltuniq_table.argtypes = [C.c_int, C.c_int, vp, u64p, C.c_uint64, u64p]
    L.fmd_fltuniq_open.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.fmd_fltuniq_slot.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.fmd_fltuniq_count.argtypes = [vp, C.c_uint64]
    L.fmd_fltuniq_test.argtypes = [vp, C.c_uint64, vp]
    L.fmd_fltuniq_sync.argtypes = [vp, vp]
    L.fmd_fltuniq_export.argtypes = [vp, C.c_uint64, C.c_uint64, u64p]
    L.fmd_fltuniq_close.restype = None; L.fmd_fltuniq_close.argtypes = [vp]
    L.fmd_fltuniq_batch_limits.restype = None; L.fmd_fltuniq_batch_limits.argtypes = [u64p, u64p]
    L.fmd_scaf_links_work_bytes.restype = sz; L.fmd_scaf_links_work_bytes.argtypes = [C.c_uint64]
    L.fmd_scaf_links_dev.argtypes = [C.c_int, vp, C.c_uint64, u64p, u64p, vp, C.c_uint64, vp, vp, C.c_int, u64p, u64p, u64p, u64p, vp, u64p, vp, sz]
    L.fmd_scaf_links.argtypes = [C.c_int, C.c_uint64, u64p, u64p, vp, C.c_uint64, vp, vp, C.c_int, u64p, u64p, u64p, u64p, vp, u64p]
    L.fmd_dev_close.restype = None; L.fmd_dev_close.argtypes = [vp]
    L.fmd_dev_trim.restype = C.c_uint64; L.fmd_dev_trim.argtypes = [vp]
    L.fmd_dev_info.argtypes = [vp, C.POINTER(Info)]
    L.fmd_dev_sync.argtypes = [vp, vp]
    L.fmd_rank1a_dev.argtypes = [vp, vp, sz, u64p, u64p, vp]
    L.fmd_rank2a_dev.argtypes = [vp, vp, sz, u64p, u64p, u64p, u64p]
    L.fmd_rank1a_batch.argtypes = [vp, sz, u64p, u64p, vp]
    L.fmd_rank2a_batch.argtypes = [vp, sz, u64p, u64p, u64p, u64p]
    L.fmd_extend_dev.argtypes = [vp, vp, sz, vp, vp, vp]
    L.fmd_extend_batch.argtypes = [vp, sz, vp, vp, vp]
    L.fmd_bsearch_dev.argtypes = [vp, vp, sz, vp, u64p, u64p, u64p, u64p]
    L.fmd_bsearch_batch.argtypes = [vp, sz, vp, u64p, u64p, u64p, u64p]
    L.fmd_multi_bsearch_work_bytes.restype = sz; L.fmd_multi_bsearch_work_bytes.argtypes = [C.c_int, sz]
    L.fmd_multi_bsearch_dev.argtypes = [C.c_int, vp, vp, sz, vp, u64p, u64p, u64p, u64p, vp, sz]
    L.fmd_multi_bsearch_batch.argtypes = [C.c_int, vp, sz, vp, u64p, u64p, u64p, u64p]
    L.fmd_retrieve_dev.argtypes = [vp, vp, sz, u64p, vp, C.c_uint32, vp, u64p]
    L.fmd_locate_work_bytes.restype = sz; L.fmd_locate_work_bytes.argtypes = [sz, C.c_uint64]
    L.fmd_locate_dev.argtypes = [vp, vp, sz, u64p, u64p, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, vp, sz]
    L.fmd_locate_batch.argtypes = [vp, sz, u64p, u64p, C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint64), vp]
    L.fmd_kcount_work_bytes.restype = sz; L.fmd_kcount_work_bytes.argtypes = [C.c_uint64]
    L.fmd_kcount_part_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, sz, vp, C.c_uint64, C.c_uint32, u64p, u64p, vp, C.c_uint64, vp, vp, sz]
    L.fmd_kcount.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, u64p, C.c_uint64, vp, vp, vp]
    L.fmd_kcmp_work_bytes.restype = sz; L.fmd_kcmp_work_bytes.argtypes = [C.c_uint64]
    L.fmd_kcmp_part_dev.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, sz, vp, C.c_uint64, C.c_uint32, u64p, u64p, u64p, C.c_uint64, vp, vp, sz]
    L.fmd_kcmp.argtypes = [vp, vp, C.c_int, vp, C.c_uint32, u64p, C.c_uint64, vp, vp, vp]
    L.fmd_kmat_node_bytes.restype = sz; L.fmd_kmat_node_bytes.argtypes = [C.c_int]
    L.fmd_kmat_work_bytes.restype = sz; L.fmd_kmat_work_bytes.argtypes = [C.c_int, C.c_uint64]
    L.fmd_kmat_part_dev.argtypes = [C.c_int, vp, vp, C.c_int, vp, C.c_int, sz, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, vp, sz]
    L.fmd_kmat.argtypes = [C.c_int, vp, C.c_int, vp, vp, C.c_uint64, vp, vp, vp]
    L.fmd_kprofile_dev.argtypes = [vp, vp, sz, vp, u64p, u64p, C.c_int, C.c_uint, vp, vp]
    L.fmd_kprofile_batch.argtypes = [vp, sz, vp, u64p, C.c_int, C.c_uint, u64p, C.POINTER(vp), vp]
    L.fmd_karcs.argtypes = [vp, C.c_int, C.c_int, C.c_uint64, vp, vp, vp]
    L.fmd_kunitig.argtypes = [vp, C.c_int, C.c_int, C.c_uint64, C.POINTER(KUnitigC)]
    L.fmd_kcarcs.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_uint64, vp, vp, C.POINTER(KCGraphStatC)]
    L.fmd_kcunitig.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_uint, C.c_uint64, C.POINTER(KCUnitigC)]
    L.fmd_kcbubble.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.POINTER(KCBubbleC)]
    L.fmd_kcbubble_dev.argtypes = [vp, C.c_int, C.c_uint64, vp, vp, C.c_uint32, C.c_int, u64p, u64p, C.POINTER(vp)]
    L.fmd_asearch_work_bytes.restype = sz; L.fmd_asearch_work_bytes.argtypes = [sz, C.c_uint64]
    L.fmd_asearch_bound_dev.argtypes = [vp, vp, sz, vp, u64p, vp]
    L.fmd_asearch_dev.argtypes = [vp, vp, sz, vp, u64p, vp, C.c_int, C.c_uint32, C.c_uint32, vp, C.c_uint64, u64p, vp, vp, sz]
    L.fmd_asearch_batch.argtypes = [vp, sz, vp, u64p, C.c_int, C.c_uint32, C.c_uint, C.c_uint64, C.POINTER(vp), C.POINTER(C.c_uint64), u64p, vp]
    L.fmd_esearch_work_bytes.restype = sz; L.fmd_esearch_work_bytes.argtypes = [sz, C.c_uint64]
    L.fmd_esearch_dev.argtypes = [vp, vp, sz, vp, u64p, vp, C.c_int, C.c_uint32, C.c_uint32, vp, C.c_uint64, u64p, vp, vp, sz]
    L.fmd_esearch_batch.argtypes = [vp, sz, vp, u64p, C.c_int, C.c_uint32, C.c_uint, C.c_uint64, C.POINTER(vp), C.POINTER(C.c_uint64), u64p, vp]
    L.fmd_retrieve_batch.argtypes = [vp, sz, u64p, vp, C.c_uint32, vp, u64p]
    L.fmd_build_bwt.argtypes = [C.c_int, sz, vp, u64p, vp, C.POINTER(C.c_uint64)]
    L.fmd_build_bwt_dev.argtypes = [C.c_int, vp, sz, vp, u64p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.fmd_build_bwt_strands.argtypes = [C.c_int, sz, vp, u64p, C.c_uint, vp, C.POINTER(C.c_uint64)]
    L.fmd_build_bwt_strands_dev.argtypes = [C.c_int, vp, sz, vp, u64p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.fmd_dev_free.restype = None; L.fmd_dev_free.argtypes = [vp]
    L.fmd_builder_new.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.POINTER(vp)]
    L.fmd_builder_add_dev.argtypes = [vp, vp, C.c_uint64, vp]
    L.fmd_builder_finish.argtypes = [vp, C.POINTER(vp)]
    L.fmd_builder_free.restype = None; L.fmd_builder_free.argtypes = [vp]
    L.fmd_bwt_to_rle6.argtypes = [C.c_int, vp, C.c_uint64, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.fmd_host_free.restype = None; L.fmd_host_free.argtypes = [vp]
    L.fmd_dev_malloc.argtypes = [C.c_int, sz, C.POINTER(vp)]
    L.fmd_memcpy_h2d.argtypes = [vp, vp, sz, vp]
    L.fmd_memcpy_d2h.argtypes = [vp, vp, sz, vp]
    L.fmd_ovlp_work_bytes.restype = sz; L.fmd_ovlp_work_bytes.argtypes = [sz, C.c_uint32, C.c_int]
    L.fmd_ovlp_sorted_work_bytes.restype = sz; L.fmd_ovlp_sorted_work_bytes.argtypes = [sz, sz, C.c_uint32, C.c_int]
    L.fmd_ovlp_sorted_dev.argtypes = [vp, vp, sz, u64p, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, vp, sz, sz]
    L.fmd_ovlp_dev.argtypes = [vp, vp, sz, u64p, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, vp, sz]
    L.fmd_ovlp_batch.argtypes = [vp, sz, u64p, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_int]
    L.fmd_ovlp_check_left_dev.argtypes = [vp, vp, sz, C.c_int, C.c_uint32, vp, vp, C.c_uint32, vp, sz]
    L.fmd_kmer_work_bytes.restype = sz; L.fmd_kmer_work_bytes.argtypes = [C.c_uint64]
    L.fmd_kmer_collect_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, sz, C.c_uint64, vp, vp, vp, vp]
    L.fmd_kmer_collect_part_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, sz, C.c_uint64, vp, vp, vp, vp]
    L.fmd_kmer_collect.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64), vp]
    L.fmd_kmer_collect_seeds.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64), vp]
    L.fmd_smem_work_bytes.restype = sz; L.fmd_smem_work_bytes.argtypes = [sz, C.c_uint32]
    L.fmd_smem_dev.argtypes = [vp, vp, sz, vp, u64p, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, sz]
    L.fmd_smem_batch.argtypes = [vp, sz, vp, u64p, C.c_int, C.c_uint32, C.c_uint32, vp, vp]
    L.fmd_dev_export_bwt.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    L.fmd_dev_check_rank.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.fmd_dev_build_pairs.argtypes = [vp, C.POINTER(C.c_int)]
    L.fmd_dev_check_pairs.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.fmd_reach_dev.argtypes = [vp, vp, sz, vp, vp]
    L.fmd_reach_batch.argtypes = [vp, sz, vp, vp]
    L.fmd_smem_win_dev.argtypes = [vp, vp, sz, vp, vp, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, sz]
    L.fmd_smem_win_batch.argtypes = [vp, sz, vp, C.c_uint64, vp, C.c_int, C.c_uint32, C.c_uint32, vp, vp]
    L.fmd_seqinfo_dev.argtypes = [vp, vp, sz, u64p, C.c_uint32, vp, vp, C.c_uint32, vp, sz]
    L.fmd_seqinfo_batch.argtypes = [vp, sz, u64p, C.c_uint32, vp]
    L.fmd_probe_gather.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_float)]
    L.fmd_dev_line_count.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.fmd_dev_line_count3.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.fmd_ovlp_pack_max_bytes.restype = sz; L.fmd_ovlp_pack_max_bytes.argtypes = [sz, C.c_uint32, C.c_uint32]
    L.fmd_ovlp_pack_work_bytes.restype = sz; L.fmd_ovlp_pack_work_bytes.argtypes = [sz]
    L.fmd_ectab_build_dev.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_uint64, vp, vp, vp, C.POINTER(vp)]
    L.fmd_ectab_build.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, vp, vp, vp, C.POINTER(vp)]
    L.fmd_ectab_free.restype = None; L.fmd_ectab_free.argtypes = [vp]
    L.fmd_ecfix_work_bytes.restype = sz; L.fmd_ecfix_work_bytes.argtypes = [vp, sz, C.c_uint32]
    L.fmd_ecfix_dev.argtypes = [vp, vp, sz, vp, vp, u64p, C.c_int, C.c_uint32, vp, vp, sz]
    L.fmd_ecfix_batch.argtypes = [vp, sz, vp, vp, u64p, C.c_int, vp]
    L.fmd_ectab_line_count.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.fmd_ovlp_packed_batch.argtypes = [vp, vp, C.c_uint64, C.c_uint64, sz, C.c_int, C.c_uint32, C.c_uint32, C.c_int, vp, vp, C.c_uint32, vp]
    L.fmd_ovlp_link_dev.argtypes = [vp, vp, sz, vp, vp, C.c_uint32, vp, vp, vp, vp]
    L.fmd_ovlp_packed_table.argtypes = [vp, sz, C.c_int, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.fmd_ovlp_packed_free.restype = None; L.fmd_ovlp_packed_free.argtypes = [vp, sz]
    L.fmd_table_alloc.restype = vp; L.fmd_table_alloc.argtypes = [sz]
    L.fmd_table_free.restype = None; L.fmd_table_free.argtypes = [vp]
    L.fmd_ovlp_pack_dev.argtypes = [vp, vp, sz, vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, sz]
    L.fmd_ovlp_two_pass_ok.argtypes = [vp, sz, C.c_int, C.c_uint32]
    L.fmd_ovlp_head_work_bytes.restype = sz; L.fmd_ovlp_head_work_bytes.argtypes = [sz]
    L.fmd_ovlp_head_dev.argtypes = [vp, vp, sz, u64p, C.c_int, C.c_uint32, vp, vp, vp, vp, vp, sz]
    L.fmd_ovlp_tail_dev.argtypes = [vp, vp, sz, vp, vp, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, vp, sz]
    L.fmd_ovlp_pack_rows_dev.argtypes = [vp, vp, sz, vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint64, vp, sz]
    L.fmd_ovlp_side_work_bytes.restype = sz; L.fmd_ovlp_side_work_bytes.argtypes = [sz, C.c_uint32, C.c_int]
    L.fmd_ovlp_rerun_overflow_dev.argtypes = [vp, vp, sz, vp, vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, vp, vp, C.c_uint32, vp, sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.fmd_comm_rccl_unique_id.argtypes = [vp]
    L.fmd_comm_rccl_init.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.fmd_comm_rccl_version.restype = C.c_int
    L.fmd_comm_free.restype = None; L.fmd_comm_free.argtypes = [vp]
    L.fmd_ovlp_dist_new.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.fmd_ovlp_dist_step.argtypes = [vp, vp, vp]
    L.fmd_ovlp_dist_table.argtypes = [vp, vp]
    L.fmd_ovlp_dist_local.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint32)]
    L.fmd_ovlp_dist_free.restype = None; L.fmd_ovlp_dist_free.argtypes = [vp]
    return L


def _load(path):
    try:  # one process, one HIP runtime: if torch is going to be used, its bundled
        import torch  # noqa: F401  libamdhip64 must be the copy that gets loaded (same soname)
    except Exception:
        pass
    return _configure(C.CDLL(path))


def lib():
    """Load libfmdhip.so; raises FmdError (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FmdError("libfmdhip.so is not built (%s); run `make` or __graft_entry__.build()" % LIB_PATH)
        _lib = _load(LIB_PATH)
    return _lib


def count_lib():
    """The instrumented build (measurement only: bench.py's device-byte model); None when it has not been built."""
    global _count_lib
    if _count_lib is None and os.path.exists(COUNT_LIB_PATH):
        _count_lib = _load(COUNT_LIB_PATH)
    return _count_lib


def check(rc):
    if rc != 0:
        L = lib()
        msg = L.fmd_strerror(rc).decode()
        if rc == -6:
            msg += ": " + L.fmd_last_hip_error().decode()
        raise FmdError("libfmdhip: %s (%d)" % (msg, rc))


def device_count():
    return lib().fmd_device_count()


def _ptr(a):
    return a.ctypes.data


def flatten_reads(seqs):
    """list/2-D array of nt6 reads -> (uint8 concatenation padded to 8 bytes, uint64 offsets[n+1])"""
    if isinstance(seqs, np.ndarray) and seqs.ndim == 2:
        n, ln = seqs.shape
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(ln)
        flat = np.ascontiguousarray(seqs, dtype=np.uint8).reshape(-1)
    else:
        lens = np.array([len(s) for s in seqs], dtype=np.uint64)
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum(lens, out=off[1:])
        flat = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs]) if len(seqs) else np.zeros(0, np.uint8)
    pad = (-len(flat)) % 8 + 8
    return np.concatenate([flat, np.zeros(pad, dtype=np.uint8)]), off


class DevIndex:
    """An FMD index resident in one GPU's HBM (fmd_dev_t)."""

    def __init__(self, handle):
        self.h = handle
        info = Info()
        check(lib().fmd_dev_info(self.h, C.byref(info)))
        self.cnt = np.array(info.cnt[:], dtype=np.uint64)
        self.mcnt = np.array(info.mcnt[:], dtype=np.uint64)
        self.n_blocks = int(info.n_blocks)
        self.hbm_bytes = int(info.hbm_bytes)
        self.device = int(info.device)
        self.n = int(self.mcnt[0])

    # ---- rld_restore (rld.c:288) and friends
    @classmethod
    def open(cls, fn, device=0, empty_ok=False):
        """empty_ok: a file of no symbols opens as an index of no rows (FMD_OPEN_EMPTY_OK), a part for multi_backward_search"""
        h = C.c_void_p()
        if empty_ok:
            check(lib().fmd_dev_open_file_ex(device, fn.encode(), FMD_OPEN_EMPTY_OK, C.byref(h)))
        else:
            check(lib().fmd_dev_open_file(device, fn.encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def from_bwt(cls, bwt, device=0):
        bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
        h = C.c_void_p()
        check(lib().fmd_dev_open_bwt(device, _ptr(bwt), len(bwt), C.byref(h)))
        return cls(h)

    @classmethod
    def from_bwt_dev(cls, d_ptr, n, device=0):
        h = C.c_void_p()
        check(lib().fmd_dev_open_bwt_dev(device, d_ptr, n, C.byref(h)))
        return cls(h)

    @classmethod
    def from_rle6(cls, runs, device=0):
        runs = np.ascontiguousarray(runs, dtype=np.uint8)
        h = C.c_void_p()
        check(lib().fmd_dev_open_rle6(device, _ptr(runs), len(runs), C.byref(h)))
        return cls(h)

    @classmethod
    def open_bare(cls, fn, device=0):
        """rld_restore without the prefix and tail tables (fmd_dev_open_file_ex, FMD_OPEN_NO_TABLES): enough to rank, decode, merge"""
        h = C.c_void_p()
        check(lib().fmd_dev_open_file_ex(device, fn.encode(), 1, C.byref(h)))
        return cls(h)

    def merge(self, other, tables=True):
        """fm_merge (merge.c:100): a new resident index of this index's sequences followed by other's; both stay as they are
        (tables=False: without the prefix and tail tables, fmd_dev_merge_ex(.., FMD_OPEN_NO_TABLES))"""
        h = C.c_void_p()
        check(lib().fmd_dev_merge_ex(self.h, other.h, 0 if tables else 1, C.byref(h)))
        return DevIndex(h)

    def contrast(self, other, k=55, min_occ=3):
        """fm6_contrast (cmp.c:94): (bits0, bits1), np.uint64 words with one bit per sequence of this index / of other in SORTED order
        (bit i = the i-th '$' of the BWT; fm6_sub_conv with the `seqsort` ranks turns it into sequence numbers): set where the sequence runs through a string of up to k bases that the other index lacks"""
        a, b = C.c_void_p(), C.c_void_p()
        check(lib().fmd_contrast(self.h, other.h, k, min_occ, C.byref(a), C.byref(b)))
        out = []
        for p, d in ((a, self), (b, other)):
            nw = (int(d.mcnt[1]) + 63) // 64
            out.append(np.ctypeslib.as_array((C.c_uint64 * max(nw, 1)).from_address(p.value))[:nw].astype(np.uint64, copy=True))
            lib().fmd_host_free(p)
        return out[0], out[1]

    def sub(self, bits, complement=False, tables=True):
        """fm_sub (sub.c:71): a new resident index of the sequences whose bit (by sequence number = sentinel row) is set in `bits` -- complement=True: of
        the others, `fermi sub -c` -- (tables=False: without the prefix and tail tables)"""
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        if len(bits) != (int(self.mcnt[1]) + 63) // 64:
            raise FmdError("sub: the bit array has %d words, the index %d sequences" % (len(bits), int(self.mcnt[1])))
        h = C.c_void_p()
        check(lib().fmd_dev_sub(self.h, _ptr(bits), int(bool(complement)), 0 if tables else 1, C.byref(h)))
        return DevIndex(h)

    def refresh_info(self):
        """cnt / mcnt / bytes again (the handle may have grown: fmd_dev_build_pairs)"""
        info = Info()
        check(lib().fmd_dev_info(self.h, C.byref(info)))
        self.hbm_bytes = int(info.hbm_bytes)

    def build_pairs(self):
        """the two-base blocks now (fmd_dev_build_pairs) -> True when the handle has them"""
        b = C.c_int(0)
        check(lib().fmd_dev_build_pairs(self.h, C.byref(b)))
        return bool(b.value)

    def check_pairs(self):
        """every row's pair step against two single LF steps -> (number of bad rows, the first one)"""
        bad, first = C.c_uint64(), C.c_uint64()
        check(lib().fmd_dev_check_pairs(self.h, C.byref(bad), C.byref(first)))
        return int(bad.value), int(first.value)

    def close(self):  # rld_destroy (rld.c:81)
        if self.h:
            lib().fmd_dev_close(self.h)
            self.h = None

    def sync(self, stream=None):
        check(lib().fmd_dev_sync(self.h, stream))

    # ---- host-array forms
    def rank1a(self, ks):
        ks = np.ascontiguousarray(ks, dtype=np.uint64)
        ok = np.zeros((len(ks), 6), dtype=np.uint64); sym = np.zeros(len(ks), dtype=np.int8)
        check(lib().fmd_rank1a_batch(self.h, len(ks), _ptr(ks), _ptr(ok), _ptr(sym)))
        return ok, sym

    def rank2a(self, ks, ls):
        ks = np.ascontiguousarray(ks, dtype=np.uint64); ls = np.ascontiguousarray(ls, dtype=np.uint64)
        ok = np.zeros((len(ks), 6), dtype=np.uint64); ol = np.zeros((len(ks), 6), dtype=np.uint64)
        check(lib().fmd_rank2a_batch(self.h, len(ks), _ptr(ks), _ptr(ls), _ptr(ok), _ptr(ol)))
        return ok, ol

    def extend(self, iks, is_back):
        iks = np.ascontiguousarray(iks, dtype=INTV_DT); is_back = np.ascontiguousarray(is_back, dtype=np.uint8)
        out = np.zeros((len(iks), 6), dtype=INTV_DT)
        check(lib().fmd_extend_batch(self.h, len(iks), _ptr(iks), _ptr(is_back), _ptr(out)))
        return out

    def backward_search(self, seqs):
        flat, off = flatten_reads(seqs)
        n = len(off) - 1
        cnt = np.zeros(n, dtype=np.uint64); beg = np.zeros(n, dtype=np.uint64); end = np.zeros(n, dtype=np.uint64)
        check(lib().fmd_bsearch_batch(self.h, n, _ptr(flat), _ptr(off), _ptr(cnt), _ptr(beg), _ptr(end)))
        return cnt, beg, end

    def retrieve(self, xs, stride=256):
        """fm_retrieve for each x, returned in READ order (the C ABI returns it reversed, as
        exact.c:59 does; this wrapper applies the callers' seq_reverse, unitig.c:285)."""
        xs = np.ascontiguousarray(xs, dtype=np.uint64)
        seqs = np.zeros((len(xs), stride), dtype=np.uint8); ln = np.zeros(len(xs), dtype=np.uint32)
        rank = np.zeros(len(xs), dtype=np.uint64)
        check(lib().fmd_retrieve_batch(self.h, len(xs), _ptr(xs), _ptr(seqs), stride, _ptr(ln), _ptr(rank)))
        out = np.zeros_like(seqs)
        for i in range(len(xs)):
            l = min(int(ln[i]), stride)
            out[i, :l] = seqs[i, :l][::-1]
        return out, ln.astype(np.int32), rank

    def locate_rows(self, beg, cnt, max_occ=1000, max_len=0):
        """fmd_locate_batch: the sequences that hold the rows [beg[i], beg[i] + cnt[i]) and the offsets of those rows in them, as runs
        (LOCATE_RUN_DT: sentinel ranks rank .. rank + n - 1 of query `query`, all at offset `off`), sorted by (query, off, rank), and the
        statistics as a dict.  Intervals above max_occ are left out whole (n_skipped); max_len = 0: walk until every row has ended."""
        beg = np.ascontiguousarray(beg, dtype=np.uint64); cnt = np.ascontiguousarray(cnt, dtype=np.uint64)
        if len(beg) != len(cnt):
            raise FmdError("locate_rows: %d starts, %d counts" % (len(beg), len(cnt)))
        p, m = C.c_void_p(), C.c_uint64()
        stat = np.zeros(1, dtype=LOCATE_STAT_DT)
        check(lib().fmd_locate_batch(self.h, len(beg), _ptr(beg), _ptr(cnt), int(max_occ), int(max_len), C.byref(p), C.byref(m), _ptr(stat)))
        runs = np.zeros(m.value, dtype=LOCATE_RUN_DT)
        if m.value:
            C.memmove(_ptr(runs), p.value, m.value * LOCATE_RUN_DT.itemsize)
        lib().fmd_host_free(p)
        return runs, {f: int(stat[0][f]) for f in LOCATE_STAT_DT.names}

    def locate(self, seqs, max_occ=1000, sorted_map=None):
        """Backward search of every query, then locate: (cnt, located, hit_off, hit_id, hit_pos).  cnt[i] = occurrences; located[i] = its hits
        are listed (cnt[i] <= max_occ; trivially so for a miss); the hits of query i are hit_id / hit_pos[hit_off[i] : hit_off[i + 1]], sorted
        by (id, pos): id = the sequence's sentinel rank, or sorted_map[rank] >> 2 with seqsort's map (read = id >> 1, strand = id & 1), pos =
        the 0-based offset of the match in that strand's sequence as indexed."""
        cnt, beg, _ = self.backward_search(seqs)
        runs, _ = self.locate_rows(beg, cnt, max_occ=max_occ)
        n = len(cnt)
        located = cnt <= np.uint64(max_occ)
        q = np.repeat(runs["query"].astype(np.int64), runs["n"])
        pos = np.repeat(runs["off"].astype(np.int64), runs["n"])
        first = np.cumsum(runs["n"].astype(np.int64)) - runs["n"].astype(np.int64)
        ids = np.repeat(runs["rank"].astype(np.int64) - first, runs["n"]) + np.arange(len(q), dtype=np.int64)
        if sorted_map is not None:
            ids = (np.asarray(sorted_map, dtype=np.uint64)[ids] >> np.uint64(2)).astype(np.int64)
        order = np.lexsort((pos, ids, q))
        hit_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(q, minlength=n), out=hit_off[1:])
        return cnt, located, hit_off, ids[order], pos[order]

    def _kcount(self, k, min_occ, n_bins, cap, sink):
        hist = np.zeros(max(int(n_bins), 0), dtype=np.uint64)
        stat = np.zeros(1, dtype=KCOUNT_STAT_DT)
        cb = KCOUNT_SINK(sink) if sink is not None else None
        check(lib().fmd_kcount(self.h, int(k), int(min_occ), int(n_bins), _ptr(hist) if len(hist) else None, int(cap),
                               C.cast(cb, C.c_void_p) if cb is not None else None, None, _ptr(stat)))
        return hist, {f: int(stat[0][f]) for f in KCOUNT_STAT_DT.names}

    def kmer_spectrum(self, k, min_occ=1, n_bins=1024, cap=0):
        """fmd_kcount without a sink: (hist, stat).  hist[i] = the canonical k-mers (1 <= k <= 32) with count i, hist[n_bins - 1] = those with
        count >= n_bins - 1, hist[0] = 0; only k-mers with count >= min_occ are in it.  stat: the fields of KCOUNT_STAT_DT (n_kmers, n_total,
        n_ext, widest_level, n_parts, n_retries, ..).  cap: the frontier capacity of a part in entries (KCOUNT_MIN_CAP ..; 0 = sized from
        the index and the free device memory); the result does not depend on it.  An index of one strand only raises FmdError."""
        return self._kcount(k, min_occ, n_bins, cap, None)

    def kmer_counts(self, k, min_occ=1, cap=0, slices=None):
        """fmd_kcount with a sink: (kmers uint64[], counts uint32[], stat), the canonical k-mers with count >= min_occ, ascending.  A k-mer is
        packed 2 bits per base (A=0 C=1 G=2 T=3), the first base in the highest of the low 2k bits; a count saturates at 2^32 - 1.  slices:
        a list that receives the length of every slice the sink was handed."""
        ks, cs = [], []

        def sink(ctx, n, kmer, count):
            ks.append(np.ctypeslib.as_array(kmer, (n,)).astype(np.uint64, copy=True))
            cs.append(np.ctypeslib.as_array(count, (n,)).astype(np.uint32, copy=True))
            if slices is not None:
                slices.append(int(n))
            return 0

        _, stat = self._kcount(k, min_occ, 2, cap, sink)
        return (np.concatenate(ks) if ks else np.zeros(0, np.uint64)), (np.concatenate(cs) if cs else np.zeros(0, np.uint32)), stat

    def _kcmp(self, other, k, sel, n_bins, cap, sink):
        hist = np.zeros(max(int(n_bins), 0) ** 2, dtype=np.uint64)
        stat = np.zeros(1, dtype=KCMP_STAT_DT)
        s = np.zeros(1, dtype=KCMP_SEL_DT)
        s[0] = tuple(KCMP_NO_MAX if v is None else int(v) for v in sel)
        cb = KCMP_SINK(sink) if sink is not None else None
        check(lib().fmd_kcmp(self.h, other.h, int(k), _ptr(s), int(n_bins), _ptr(hist) if len(hist) else None, int(cap),
                             C.cast(cb, C.c_void_p) if cb is not None else None, None, _ptr(stat)))
        return hist.reshape(max(int(n_bins), 0), -1), {f: int(stat[0][f]) for f in KCMP_STAT_DT.names}

    def kmer_compare_spectrum(self, other, k, sel=(0, None, 0, None), n_bins=256, cap=0):
        """fmd_kcmp without a sink: (hist2d, stat), the joint counts of the canonical k-mers (1 <= k <= 32) of this index (c0) and `other` (c1), both of
        both strands.  sel = (min0, max0, min1, max1), None or KCMP_NO_MAX = no upper bound: a k-mer is reported iff c0 + c1 >= 1, min0 <= c0 <= max0 and
        min1 <= c1 <= max1.  hist2d[min(c0, n_bins - 1), min(c1, n_bins - 1)] = the reported k-mers there (2 <= n_bins <= 1024), hist2d[0, 0] = 0.  stat:
        the fields of KCMP_STAT_DT (n_kmers, n_total0, n_total1, n_only0, n_only1, n_shared, n_ext, widest_level, n_parts, n_retries, ..).  cap: the
        frontier capacity of a part in entries (KCMP_MIN_CAP ..; 0 = sized from the indexes and the free device memory); the result does not depend on it."""
        return self._kcmp(other, k, sel, n_bins, cap, None)

    def kmer_compare(self, other, k, sel=(0, None, 0, None), cap=0, slices=None):
        """fmd_kcmp with a sink: (kmers uint64[], c0 uint32[], c1 uint32[], stat), the reported canonical k-mers (kmer_compare_spectrum) ascending with
        their counts in this index and in `other`; a count saturates at 2^32 - 1.  slices: a list that receives the length of every slice the sink was handed."""
        ks, a0, a1 = [], [], []

        def sink(ctx, n, kmer, c0, c1):
            ks.append(np.ctypeslib.as_array(kmer, (n,)).astype(np.uint64, copy=True))
            a0.append(np.ctypeslib.as_array(c0, (n,)).astype(np.uint32, copy=True))
            a1.append(np.ctypeslib.as_array(c1, (n,)).astype(np.uint32, copy=True))
            if slices is not None:
                slices.append(int(n))
            return 0

        _, stat = self._kcmp(other, k, sel, 2, cap, sink)
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
        return cat(ks, np.uint64), cat(a0, np.uint32), cat(a1, np.uint32), stat

    def kmer_profile(self, seqs, k, flags=0, with_stat=False):
        """fmd_kprofile_batch: (counts uint32[], woff uint64[n + 1][, stat]).  Window j of sequence i -- its bases [j, j + k), 1 <= k <= KPROFILE_MAX_K --
        has counts[woff[i] + j] = kcount's COUNT of its k-mer: occ on the index of both strands, halved for a k-mer that is its own reverse complement,
        saturated at 2^32 - 1, and 0 for a window with a base outside A/C/G/T.  flags: 0 = the library chooses the path, KPROFILE_PLAIN = the plain
        path (the only one there is).  stat: the fields of KPROFILE_STAT_DT as a dict.  An index of one strand only raises FmdError."""
        flat, off = flatten_reads(seqs)
        n = len(off) - 1
        woff = np.zeros(n + 1, dtype=np.uint64)
        stat = np.zeros(1, dtype=KPROFILE_STAT_DT)
        p = C.c_void_p()
        check(lib().fmd_kprofile_batch(self.h, n, _ptr(flat), _ptr(off), int(k), int(flags), _ptr(woff), C.byref(p), _ptr(stat)))
        counts = np.zeros(int(woff[n]), dtype=np.uint32)
        if p.value:
            C.memmove(_ptr(counts), p.value, counts.nbytes)
        lib().fmd_host_free(p)
        if with_stat:
            return counts, woff, {f: int(stat[0][f]) for f in KPROFILE_STAT_DT.names}
        return counts, woff

    def kmer_arcs(self, k, min_occ=1, cap=0, with_stat=False, slices=None):
        """fmd_karcs: (kmers uint64[], counts uint32[], arcs uint8[][, stat]): the canonical k-mers (k odd, 3..31) with count >= min_occ, ascending -- the list of
        kmer_counts(k, min_occ) -- and per k-mer x its arc byte: bit c (A, C, G, T = 0..3) set iff the (k+1)-mer x.c has count >= min_occ, bit 4 + c iff c.x
        has.  cap: the most nodes (0 = no limit); more raise FmdError (-5).  slices: a list that receives the length of every slice the sink was handed."""
        ks, cs, As = [], [], []

        def sink(ctx, n, kmer, count, arcs):
            ks.append(np.ctypeslib.as_array(kmer, (n,)).astype(np.uint64, copy=True))
            cs.append(np.ctypeslib.as_array(count, (n,)).astype(np.uint32, copy=True))
            As.append(np.ctypeslib.as_array(arcs, (n,)).astype(np.uint8, copy=True))
            if slices is not None:
                slices.append(int(n))
            return 0

        cb = KARCS_SINK(sink)
        stat = np.zeros(1, dtype=KGRAPH_STAT_DT)
        check(lib().fmd_karcs(self.h, int(k), int(min_occ), int(cap), C.cast(cb, C.c_void_p), None, _ptr(stat)))
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
        out = (cat(ks, np.uint64), cat(cs, np.uint32), cat(As, np.uint8))
        return out + ({f: stat[0][f].item() for f in KGRAPH_STAT_DT.names},) if with_stat else out

    def kmer_unitigs(self, k, min_occ=1, cap=0, with_stat=False):
        """fmd_kunitig: the de Bruijn graph of kmer_arcs compacted to unitigs, as a KUnitigs (its strings() are the unitigs as `fermi-amd kgraph` prints
        them); with_stat: its .stat is filled in (n_nodes, n_arcs, n_links, n_unitigs, n_cycles, n_ext, n_rounds, ms_arcs, ms_links, ms_label)."""
        g = KUnitigC()
        try:
            check(lib().fmd_kunitig(self.h, int(k), int(min_occ), int(cap), C.byref(g)))
            arrays = {}
            for name, field, dt in KUnitigs.NODE + KUnitigs.UNITIG:
                n = int(g.n_nodes if (name, field, dt) in KUnitigs.NODE else g.n_unitigs)
                a = np.zeros(n, dtype=dt)
                if n:
                    C.memmove(_ptr(a), getattr(g, field), a.nbytes)
                arrays[name] = a
        finally:
            for _, field, _ in KUnitigs.NODE + KUnitigs.UNITIG:
                lib().fmd_host_free(getattr(g, field))
        out = KUnitigs(k, **arrays)
        if with_stat:
            out.stat = {f: getattr(g.stat, f) for f in KGRAPH_STAT_DT.names}
        return out

    def approx_search(self, seqs, max_sub=1, max_hits=1000, best=False, prune=True, cap=0, count_only=False, with_stat=False):
        """fmd_asearch_batch: the patterns within max_sub substitutions (0 .. ASEARCH_MAX_SUB; no insertions or deletions) of every query that occur
        -> (strata[n, max_sub + 1, 2], hits).  strata[i, j] = (the hits of query i with j substitutions, the sum of their counts), exact whether or
        not the hits are listed; hits = a structured array (ASEARCH_HIT_DT: beg, cnt = the SA interval of the pattern, query, n_sub, sub[4] =
        pos << 2 | base - 1 by descending pos, 0xffff = unused; approx_pattern gives the pattern) sorted by (query, n_sub, beg), without those of
        the queries that have more than max_hits.  An N in a query costs one substitution.  best: only the lowest stratum of every query that
        has a hit.  prune=False: without the lower bound (approx_bound) -- the same result, more extensions.  cap: the frontier capacity in entries
        (ASEARCH_MIN_CAP ..; 0 = sized from the batch); the result does not depend on it.  count_only: hits is empty, nothing is listed.
        with_stat: a third element, the fields of ASEARCH_STAT_DT as a dict."""
        flat, off = flatten_reads(seqs)
        n = len(off) - 1
        if not 0 <= int(max_sub) <= ASEARCH_MAX_SUB:
            raise FmdError("approx_search: max_sub = %d is outside 0..%d" % (max_sub, ASEARCH_MAX_SUB))
        strata = np.zeros((n, int(max_sub) + 1, 2), dtype=np.uint64)
        stat = np.zeros(1, dtype=ASEARCH_STAT_DT)
        p, m = C.c_void_p(), C.c_uint64()
        flags = (0 if prune else ASEARCH_NO_PRUNE) | (ASEARCH_BEST if best else 0)
        check(lib().fmd_asearch_batch(self.h, n, _ptr(flat), _ptr(off), int(max_sub), int(max_hits), flags, int(cap),
                                      None if count_only else C.byref(p), None if count_only else C.byref(m), _ptr(strata) if n else None, _ptr(stat)))
        hits = np.zeros(m.value, dtype=ASEARCH_HIT_DT)
        if m.value:
            C.memmove(_ptr(hits), p.value, m.value * ASEARCH_HIT_DT.itemsize)
        if p.value:
            lib().fmd_host_free(p)
        if with_stat:
            return strata, hits, {f: int(stat[0][f]) for f in ASEARCH_STAT_DT.names}
        return strata, hits

    def edit_search(self, seqs, max_edit=1, max_hits=1000, best=False, prune=True, cap=0, count_only=False, with_stat=False):
        """fmd_esearch_batch: the patterns within max_edit edits (0 .. ESEARCH_MAX_EDIT; substitutions, insertions and deletions, 1 each) of every query
        that occur -> (strata[n, max_edit + 1, 2], hits).  strata[i, j] = (the hits of query i at edit distance j, the sum of their counts), exact whether
        or not the hits are listed; hits = a structured array (ESEARCH_HIT_DT: beg, cnt = the SA interval of the pattern, query, n_edit = its exact
        distance, len = its length, max(1, L - max_edit) .. L + max_edit; edit_patterns reads the patterns back) sorted by (query, n_edit, beg, len),
        without those of the queries that have more than max_hits.  Every distinct pattern is one hit.  An N in a query costs one.  best: only the
        lowest stratum of every query that has a hit.  prune=False: without the lower bound (approx_bound) -- the same result, more extensions.  cap:
        the frontier capacity in entries (ESEARCH_MIN_CAP ..; 0 = sized from the batch); the result does not depend on it.  count_only: hits is empty,
        nothing is listed.  with_stat: a third element, the fields of ESEARCH_STAT_DT as a dict."""
        flat, off = flatten_reads(seqs)
        n = len(off) - 1
        if not 0 <= int(max_edit) <= ESEARCH_MAX_EDIT:
            raise FmdError("edit_search: max_edit = %d is outside 0..%d" % (max_edit, ESEARCH_MAX_EDIT))
        strata = np.zeros((n, int(max_edit) + 1, 2), dtype=np.uint64)
        stat = np.zeros(1, dtype=ESEARCH_STAT_DT)
        p, m = C.c_void_p(), C.c_uint64()
        flags = (0 if prune else ESEARCH_NO_PRUNE) | (ESEARCH_BEST if best else 0)
        check(lib().fmd_esearch_batch(self.h, n, _ptr(flat), _ptr(off), int(max_edit), int(max_hits), flags, int(cap),
                                      None if count_only else C.byref(p), None if count_only else C.byref(m), _ptr(strata) if n else None, _ptr(stat)))
        hits = np.zeros(m.value, dtype=ESEARCH_HIT_DT)
        if m.value:
            C.memmove(_ptr(hits), p.value, m.value * ESEARCH_HIT_DT.itemsize)
        if p.value:
            lib().fmd_host_free(p)
        if with_stat:
            return strata, hits, {f: int(stat[0][f]) for f in ESEARCH_STAT_DT.names}
        return strata, hits

    def edit_patterns(self, hits):
        """hostlib.esearch_patterns for the hits of edit_search on this index: a list of uint8 arrays (nt6), the pattern of every hit.  The map from
        sentinel ranks to rows (hostlib.esearch_rankmap: one walk over every sequence) is made at the first call and kept."""
        from . import hostlib
        if getattr(self, "_esearch_row_of", None) is None:
            self._esearch_row_of = hostlib.esearch_rankmap(self.h)
        return hostlib.esearch_patterns(self.h, self._esearch_row_of, hits)

    def approx_bound(self, seqs):
        """fmd_asearch_bound_dev: per query a uint8 array, lb[p] = min(255, the disjoint substrings of q[0 .. p], taken greedily from the left, that
        do not occur) -- a lower bound of the substitutions a hit spends in q[0 .. p]; an N costs one.  All zero on an index that is not of
        both strands; zero for a query longer than ASEARCH_MAX_LEN."""
        flat, off = flatten_reads(seqs)
        n = len(off) - 1
        if n == 0:
            return []
        L = lib()
        bufs = []
        try:
            for a in (flat, off, np.zeros(len(flat), dtype=np.uint8)):
                p = C.c_void_p()
                check(L.fmd_dev_malloc(self.device, max(a.nbytes, 16), C.byref(p)))
                bufs.append(p)
                check(L.fmd_memcpy_h2d(p, _ptr(a), a.nbytes, None))
            check(L.fmd_asearch_bound_dev(self.h, None, n, bufs[0], bufs[1], bufs[2]))
            self.sync()
            lb = np.zeros(len(flat), dtype=np.uint8)
            check(L.fmd_memcpy_d2h(_ptr(lb), bufs[2], lb.nbytes, None))
        finally:
            for p in bufs:
                L.fmd_dev_free(p)
        return [lb[int(off[i]):int(off[i + 1])].copy() for i in range(n)]


def approx_pattern(query, hit):
    """The pattern of a hit of approx_search: `query` (nt6) with the hit's substitutions applied, as a uint8 array."""
    out = np.array(query, dtype=np.uint8)
    for v in hit["sub"][:int(hit["n_sub"])]:
        out[int(v) >> 2] = 1 + (int(v) & 3)
    return out


FMD_MULTI_MAX = 16   # include/fmd_hip.h
FMD_OPEN_EMPTY_OK = 4


def multi_backward_search(indexes, seqs):
    """fm_multi_backward_search (exact.c:25-57) for each read: (cnt, beg, end) in the MERGED index of `indexes` (DevIndex objects on one GPU, in
    merge order; the same one may appear twice), computed from the parts -- nothing is merged.  A miss is cnt = beg = end = 0."""
    flat, off = flatten_reads(seqs)
    n = len(off) - 1
    hs = (C.c_void_p * max(len(indexes), 1))(*[d.h for d in indexes])
    cnt = np.zeros(n, dtype=np.uint64); beg = np.zeros(n, dtype=np.uint64); end = np.zeros(n, dtype=np.uint64)
    check(lib().fmd_multi_bsearch_batch(len(indexes), hs, n, _ptr(flat), _ptr(off), _ptr(cnt), _ptr(beg), _ptr(end)))
    return cnt, beg, end


class KCUnitigs(KUnitigs):
    """The compacted coloured de Bruijn graph of kmer_joint_unitigs (fmd_kcunitig_t as numpy arrays) of N indexes.  Per node, ascending by k-mer: kmers uint64,
    counts uint32[n, N] and arcs uint8[n, N] (held column by column), uarcs uint8 (the union byte), pattern uint8, unitig, offset, orient as in KUnitigs; per
    unitig: u_nodes, u_first, u_flags, u_count uint64[nu, N], u_present uint32[nu, N], u_pattern uint8.  strings() are the unitigs as `fermi-amd kcgraph`
    prints them."""
    NODE = (("kmers", "kmer", np.uint64), ("counts", "count", np.uint32), ("arcs", "arcs", np.uint8), ("uarcs", "uarcs", np.uint8), ("pattern", "pattern", np.uint8),
            ("unitig", "unitig", np.uint32), ("offset", "offset", np.uint32), ("orient", "orient", np.uint8))
    UNITIG = (("u_nodes", "u_nodes", np.uint32), ("u_first", "u_first", np.uint32), ("u_flags", "u_flags", np.uint8), ("u_count", "u_count", np.uint64),
              ("u_present", "u_present", np.uint32), ("u_pattern", "u_pattern", np.uint8))

    def __init__(self, k, n_idx, **arrays):
        self.k, self.n_idx, self.stat = int(k), int(n_idx), None
        for name, _, dt in self.NODE + self.UNITIG:
            a = np.asarray(arrays[name], dtype=dt)
            if name in ("counts", "arcs"):
                a = np.asfortranarray(a.reshape(-1, self.n_idx))
            elif name in ("u_count", "u_present"):
                a = np.ascontiguousarray(a.reshape(-1, self.n_idx))
            else:
                a = np.ascontiguousarray(a)
            setattr(self, name, a)

    def as_c(self):
        """a KCUnitigC over these arrays (they must outlive it)"""
        g = KCUnitigC()
        g.n_nodes, g.n_unitigs, g.n_idx = len(self.kmers), len(self.u_nodes), self.n_idx
        for name, field, _ in self.NODE + self.UNITIG:
            a = getattr(self, name)
            setattr(g, field, a.ctypes.data if len(a) else None)
        return g


def _handles(indexes):
    return (C.c_void_p * max(len(indexes), 1))(*[None if d is None else d.h for d in indexes])


def kmer_joint_arcs(indexes, k, min_occ=1, cap=0, with_stat=False, slices=None):
    """fmd_kcarcs: (kmers uint64[n], counts uint32[n, N], arcs uint8[n, N], uarcs uint8[n][, stat]): the coloured de Bruijn graph of 1 to KMAT_MAX_IDX indexes
    of both strands (DevIndex objects on one GPU; the same one may appear several times), k odd, 3..31.  A canonical k-mer is a node iff its count in SOME
    index is >= min_occ; counts[:, i] is its exact count in indexes[i]; arcs[:, i] is kmer_arcs' byte within index i, uarcs the OR over the indexes.  The node's
    pattern is counts >= min_occ.  counts and arcs are held column by column.  cap: the most nodes (0 = no limit); more raise FmdError (-5).  slices: a list
    that receives the length of every slice the sink was handed.  stat: kgraph's fields on the union graph, n_nodes_in and n_arcs_in per index."""
    n_idx = len(indexes)
    ks, us, cs, As = [], [], [[] for _ in range(n_idx)], [[] for _ in range(n_idx)]

    def sink(ctx, n, kmer, count, arcs, uarcs):
        ks.append(np.ctypeslib.as_array(kmer, (n,)).astype(np.uint64, copy=True))
        us.append(np.ctypeslib.as_array(uarcs, (n,)).astype(np.uint8, copy=True))
        for i in range(n_idx):
            cs[i].append(np.ctypeslib.as_array(count[i], (n,)).astype(np.uint32, copy=True))
            As[i].append(np.ctypeslib.as_array(arcs[i], (n,)).astype(np.uint8, copy=True))
        if slices is not None:
            slices.append(int(n))
        return 0

    cb = KCARCS_SINK(sink)
    st = KCGraphStatC()
    check(lib().fmd_kcarcs(n_idx, _handles(indexes), int(k), int(min_occ), int(cap), C.cast(cb, C.c_void_p), None, C.byref(st)))
    kmers = np.concatenate(ks) if ks else np.zeros(0, np.uint64)
    uarcs = np.concatenate(us) if us else np.zeros(0, np.uint8)
    counts = np.zeros((len(kmers), max(n_idx, 0)), dtype=np.uint32, order="F"); arcs = np.zeros((len(kmers), max(n_idx, 0)), dtype=np.uint8, order="F")
    for i in range(n_idx):
        if cs[i]:
            np.concatenate(cs[i], out=counts[:, i]); np.concatenate(As[i], out=arcs[:, i])
    out = (kmers, counts, arcs, uarcs)
    return out + (_kcgraph_stat(st, n_idx),) if with_stat else out


def kmer_joint_unitigs(indexes, k, min_occ=1, split=False, cap=0, with_stat=False):
    """fmd_kcunitig: the coloured de Bruijn graph of kmer_joint_arcs compacted to unitigs on its union bytes, as a KCUnitigs.  split (KCGRAPH_SPLIT): a unitig
    ends where the pattern changes, so every unitig has one pattern.  with_stat: its .stat is filled in."""
    n_idx = len(indexes)
    g = KCUnitigC()
    try:
        check(lib().fmd_kcunitig(n_idx, _handles(indexes), int(k), int(min_occ), KCGRAPH_SPLIT if split else 0, int(cap), C.byref(g)))
        out = _kcunitigs_copied(g, k, n_idx)
    finally:
        _kcunitig_free(g)
    if with_stat:
        out.stat = _kcgraph_stat(g.stat, n_idx)
    return out


def _kcunitigs_copied(g, k, n_idx):
    """the arrays of a KCUnitigC the library filled, copied into a KCUnitigs"""
    arrays = {}
    for name, field, dt in KCUnitigs.NODE + KCUnitigs.UNITIG:
        n = int(g.n_nodes if (name, field, dt) in KCUnitigs.NODE else g.n_unitigs)
        wide = name in ("counts", "arcs", "u_count", "u_present")
        a = np.zeros(n * n_idx if wide else n, dtype=dt)
        if n:
            C.memmove(_ptr(a), getattr(g, field), a.nbytes)
        if name in ("counts", "arcs"):
            a = a.reshape(n_idx, n).T               # columns n_nodes apart
        arrays[name] = a
    return KCUnitigs(k, n_idx, **arrays)


def _kcunitig_free(g):
    for _, field, _ in KCUnitigs.NODE + KCUnitigs.UNITIG:
        lib().fmd_host_free(getattr(g, field))


def _bubbles_copied(ptr, n):
    out = np.zeros(int(n), dtype=KBUBBLE_DT)
    if n:
        C.memmove(_ptr(out), ptr, out.nbytes)
    return out


def kmer_joint_bubbles(indexes, k, min_occ=1, max_len=0, cap=0, with_stat=False):
    """fmd_kcbubble: (KCUnitigs, bubbles): the unsplit compaction of kmer_joint_unitigs and the simple variant bubbles of its graph (include/fmd_hip.h, kbubble)
    as a KBUBBLE_DT array ascending by src -- src, dst, first[2], len[2], nodes oriented as 2 * id + o.  max_len: only bubbles whose branches have at most
    that many nodes (0 = any).  The graph's n_forks is the number of ports with exactly two right arcs; with_stat fills its .stat, ms_bubble included."""
    n_idx = len(indexes)
    o = KCBubbleC()
    try:
        check(lib().fmd_kcbubble(n_idx, _handles(indexes), int(k), int(min_occ), int(max_len), int(cap), C.byref(o)))
        g = _kcunitigs_copied(o.g, k, n_idx)
        bubbles = _bubbles_copied(o.bubble, o.n_bubbles)
    finally:
        _kcunitig_free(o.g)
        lib().fmd_host_free(o.bubble)
    g.n_forks = int(o.n_forks)
    if with_stat:
        g.stat = _kcgraph_stat(o.g.stat, n_idx)
        g.stat["n_forks"] = int(o.n_forks); g.stat["n_bubbles"] = int(o.n_bubbles); g.stat["ms_bubble"] = float(o.ms_bubble)
    return g, bubbles


def kmer_bubbles_dev(index, k, kmers, uarcs, max_len=0, grid=0):
    """fmd_kcbubble_dev: (n_forks, bubbles) of the graph given by its ascending canonical k-mers and arc bytes, uploaded to index's GPU; the bubble kernels run
    on `grid` blocks of 256 threads (0 = the library's choice)."""
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64); uarcs = np.ascontiguousarray(uarcs, dtype=np.uint8)
    if len(kmers) != len(uarcs):
        raise ValueError("kmer_bubbles_dev: %d k-mers and %d arc bytes" % (len(kmers), len(uarcs)))
    L = lib()
    bufs = []
    nf, nb, ptr = C.c_uint64(), C.c_uint64(), C.c_void_p()
    try:
        for a in (kmers, uarcs):
            p = C.c_void_p()
            check(L.fmd_dev_malloc(index.device, max(a.nbytes, 16), C.byref(p)))
            bufs.append(p)
            check(L.fmd_memcpy_h2d(p, _ptr(a), a.nbytes, None))
        check(L.fmd_kcbubble_dev(index.h, int(k), len(kmers), bufs[0], bufs[1], int(max_len), int(grid), C.byref(nf), C.byref(nb), C.byref(ptr)))
        out = _bubbles_copied(ptr, nb.value)
    finally:
        L.fmd_host_free(ptr)
        for p in bufs:
            L.fmd_dev_free(p)
    return int(nf.value), out


def bubble_alleles(g, bubbles):
    """Per record of kmer_joint_bubbles over the KCUnitigs g: (type, left flank, allele_0, allele_1, right flank) as `fermi-amd kbubble` prints them.  P_b =
    text(src) + the last base of every node of branch b + the last base of text(dst); the longest common prefix of P_0 and P_1 is stripped, then the longest
    common suffix of the rest; an empty allele is "-".  SNP: both 1 base; MNP: equal lengths above 1; INDEL: exactly one empty; COMPLEX: anything else."""
    k, mask = g.k, (1 << (2 * g.k)) - 1

    def comp(w):                                        # the reverse complement of a packed k-mer
        r = 0
        for _ in range(k):
            r, w = r << 2 | (3 - (w & 3)), w >> 2
        return r

    def word(u):
        x = int(g.kmers[u >> 1])
        return comp(x) if u & 1 else x

    def right(u):
        a = int(g.uarcs[u >> 1])
        return [c for c in range(4) if (a >> (4 + 3 - c) & 1 if u & 1 else a >> c & 1)]

    def follow(u, c):
        v = (word(u) << 2 | c) & mask
        r = comp(v)
        j = int(np.searchsorted(g.kmers, np.uint64(min(v, r))))
        return 2 * j + (0 if v < r else 1)

    out = []
    for b in bubbles:
        P = []
        for br in (0, 1):
            s = "".join("ACGT"[word(int(b["src"])) >> (2 * (k - 1 - i)) & 3] for i in range(k))
            v = int(b["first"][br])
            for _ in range(int(b["len"][br])):
                s += "ACGT"[word(v) & 3]
                v = follow(v, right(v)[0])
            P.append(s + "ACGT"[word(v) & 3])
        pre = 0
        while pre < min(len(P[0]), len(P[1])) and P[0][pre] == P[1][pre]:
            pre += 1
        R = [P[0][pre:], P[1][pre:]]
        suf = 0
        while suf < min(len(R[0]), len(R[1])) and R[0][len(R[0]) - 1 - suf] == R[1][len(R[1]) - 1 - suf]:
            suf += 1
        a = [r[:len(r) - suf] for r in R]
        kind = "SNP" if len(a[0]) == len(a[1]) == 1 else "MNP" if len(a[0]) == len(a[1]) else "INDEL" if (not a[0]) != (not a[1]) else "COMPLEX"
        out.append((kind, P[0][pre - k:pre], a[0] or "-", a[1] or "-", R[0][len(R[0]) - suf:][:k]))
    return out


def kmat_sel(n_idx, sel=None, present=1):
    """The fmd_kmat_sel_t (a KMAT_SEL_DT array of one) of a selection given as up to n_idx pairs (min, max), max None or KMAT_NO_MAX = no upper bound;
    missing trailing pairs are (0, None)."""
    s = np.zeros(1, dtype=KMAT_SEL_DT)
    s["max"] = KMAT_NO_MAX
    s["present"] = int(present)
    sel = list(sel) if sel is not None else []
    if len(sel) > n_idx:
        raise ValueError("kmat_sel: %d bounds for %d indexes" % (len(sel), n_idx))
    for i, (lo, hi) in enumerate(sel):
        s["min"][0, i] = int(lo); s["max"][0, i] = KMAT_NO_MAX if hi is None else int(hi)
    return s


def _kmat(indexes, k, sel, present, cap, sink):
    n = len(indexes)
    hist = np.zeros(1 << n if 1 <= n <= KMAT_MAX_IDX else 0, dtype=np.uint64)
    stat = np.zeros(1, dtype=KMAT_STAT_DT)
    s = kmat_sel(max(n, 0) if n <= KMAT_MAX_IDX else KMAT_MAX_IDX, sel, present)
    hs = (C.c_void_p * max(n, 1))(*[d.h for d in indexes])
    cb = KMAT_SINK(sink) if sink is not None else None
    check(lib().fmd_kmat(n, hs, int(k), _ptr(s), _ptr(hist) if len(hist) else None, int(cap), C.cast(cb, C.c_void_p) if cb is not None else None, None, _ptr(stat)))
    st = {f: int(stat[0][f]) for f in KMAT_STAT_DT.names if f not in ("n_total", "n_present")}
    st["n_total"] = [int(v) for v in stat[0]["n_total"][:n]]; st["n_present"] = [int(v) for v in stat[0]["n_present"][:n]]
    return hist, st


def kmer_matrix_spectrum(indexes, k, sel=None, present=1, cap=0):
    """fmd_kmat without a sink: (hist, stat), the presence patterns of the canonical k-mers (1 <= k <= 32) of 1 to KMAT_MAX_IDX indexes of both strands (DevIndex
    objects on one GPU; the same one may appear several times), unmerged.  c_i = kcount's count of a k-mer in indexes[i].  sel = up to one (min, max) per index,
    max None = no upper bound, missing ones (0, None): a k-mer is reported iff some c_i >= 1 and min_i <= c_i <= max_i for every i.  hist[pattern] = the reported
    k-mers with bit i of pattern set iff c_i >= present (2^N words).  stat: the fields of KMAT_STAT_DT as a dict, n_total and n_present as lists of N.  cap: the
    frontier capacity of a part in entries (KMAT_MIN_CAP ..; 0 = sized from the indexes and the free device memory); the result does not depend on it."""
    return _kmat(indexes, k, sel, present, cap, None)


def kmer_matrix(indexes, k, sel=None, present=1, cap=0, slices=None):
    """fmd_kmat with a sink: (kmers uint64[n], counts uint32[n, N], stat), the reported canonical k-mers (kmer_matrix_spectrum) ascending with their count in every
    index; a count saturates at 2^32 - 1.  counts is held column by column (Fortran order), as the sink hands the columns over.  slices: a list that receives
    the length of every slice the sink was handed."""
    n_idx = len(indexes)
    ks, cs = [], [[] for _ in range(n_idx)]

    def sink(ctx, n, kmer, count):
        ks.append(np.ctypeslib.as_array(kmer, (n,)).astype(np.uint64, copy=True))
        for i in range(n_idx):
            cs[i].append(np.ctypeslib.as_array(count[i], (n,)).astype(np.uint32, copy=True))
        if slices is not None:
            slices.append(int(n))
        return 0

    _, stat = _kmat(indexes, k, sel, present, cap, sink)
    kmers = np.concatenate(ks) if ks else np.zeros(0, np.uint64)
    counts = np.empty((len(kmers), n_idx), dtype=np.uint32, order="F")
    for i in range(n_idx):
        if cs[i]:
            np.concatenate(cs[i], out=counts[:, i])
    return kmers, counts, stat


def _ovlp(self, ids, min_match, max_len=100, max_nei=4, check_left=True):
    """Per-id overlap records (see include/fmd_hip.h): (rec[OVLP_DT], nei[n, max_nei, INTV_DT], seq[n, 2*max_len])."""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    n = len(ids)
    stride = 2 * ((max_len + 3) // 4 * 4)
    rec = np.zeros(n, dtype=OVLP_DT); nei = np.zeros((n, max_nei), dtype=INTV_DT); seq = np.zeros((n, stride), dtype=np.uint8)
    check(lib().fmd_ovlp_batch(self.h, n, _ptr(ids), min_match, max_len, max_nei, _ptr(rec), _ptr(nei), _ptr(seq), stride, int(check_left)))
    return rec, nei, seq


DevIndex.overlap = _ovlp


def _ovlp_sorted(self, ids, min_match, max_len=100, max_nei=4, batch=0, check_left=False):
    """fmd_ovlp_sorted_dev over device copies: the records of ALL ids from one job (every strand 32 bases in, the strands sorted by
    the minimizer of those bases, the rest in that order, `batch` strands at a time).  Same arrays as overlap()."""
    L = lib()
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    n = len(ids)
    stride = 2 * ((max_len + 3) // 4 * 4)
    rec = np.zeros(n, dtype=OVLP_DT); nei = np.zeros((n, max_nei), dtype=INTV_DT); seq = np.zeros((n, stride), dtype=np.uint8)
    if n == 0:
        return rec, nei, seq
    wb = L.fmd_ovlp_sorted_work_bytes(n, batch, max_len, min_match)
    ptrs = []
    try:
        for b in (ids.nbytes, rec.nbytes, nei.nbytes, seq.nbytes, wb):
            p = C.c_void_p()
            check(L.fmd_dev_malloc(self.device, max(b, 16), C.byref(p)))
            ptrs.append(p)
        d_ids, d_rec, d_nei, d_seq, d_work = ptrs
        check(L.fmd_memcpy_h2d(d_ids, _ptr(ids), ids.nbytes, None))
        for d, a in ((d_rec, rec), (d_nei, nei), (d_seq, seq)):   # zeroes: rows of short / contained strands are not written
            check(L.fmd_memcpy_h2d(d, _ptr(a), a.nbytes, None))
        check(L.fmd_ovlp_sorted_dev(self.h, None, n, d_ids, min_match, max_len, max_nei, d_rec, d_nei, d_seq, stride, d_work, wb, batch))
        if check_left:
            m = batch if 0 < batch < n else n
            for o in range(0, n, m):
                c = min(m, n - o)
                check(L.fmd_ovlp_check_left_dev(self.h, None, c, min_match, max_len, C.c_void_p(d_rec.value + 64 * o), C.c_void_p(d_seq.value + stride * o), stride, d_work, wb))
        check(L.fmd_dev_sync(self.h, None))
        for d, a in ((d_rec, rec), (d_nei, nei), (d_seq, seq)):
            check(L.fmd_memcpy_d2h(_ptr(a), d, a.nbytes, None))
        return rec, nei, seq
    finally:
        for p in ptrs:
            L.fmd_dev_free(p)


DevIndex.overlap_sorted = _ovlp_sorted


def _ovlp_pack(self, rec, nei, seq):
    """fmd_ovlp_pack_dev over host copies of a finished batch: (prec[OVLP_DT], off[u64, n+1], var[u8])."""
    L = lib()
    n = len(rec)
    max_nei, stride = nei.shape[1], seq.shape[1]
    rec = np.ascontiguousarray(rec); nei = np.ascontiguousarray(nei); seq = np.ascontiguousarray(seq)
    cap = L.fmd_ovlp_pack_max_bytes(n, max_nei, stride)
    wb = L.fmd_ovlp_pack_work_bytes(n)
    sizes = [max(rec.nbytes, 16), max(nei.nbytes, 16), max(seq.nbytes, 16), max(rec.nbytes, 16), (n + 1) * 8, max(cap, 16), wb]
    ptrs = []
    try:
        for b in sizes:
            p = C.c_void_p()
            check(L.fmd_dev_malloc(self.device, b, C.byref(p)))
            ptrs.append(p)
        d_rec, d_nei, d_seq, d_prec, d_off, d_var, d_work = ptrs
        for d, a in ((d_rec, rec), (d_nei, nei), (d_seq, seq)):
            if a.nbytes:
                check(L.fmd_memcpy_h2d(d, _ptr(a), a.nbytes, None))
        check(L.fmd_ovlp_pack_dev(self.h, None, n, d_rec, d_nei, max_nei, d_seq, stride, d_prec, d_off, d_var, cap, d_work, wb))
        prec = np.zeros(n, dtype=OVLP_DT); off = np.zeros(n + 1, dtype=np.uint64)
        if n:
            check(L.fmd_memcpy_d2h(_ptr(prec), d_prec, prec.nbytes, None))
        check(L.fmd_memcpy_d2h(_ptr(off), d_off, off.nbytes, None))
        var = np.zeros(int(off[n]), dtype=np.uint8)
        if len(var):
            check(L.fmd_memcpy_d2h(_ptr(var), d_var, var.nbytes, None))
        return prec, off, var
    finally:
        for p in ptrs:
            L.fmd_dev_free(p)


DevIndex.overlap_pack = _ovlp_pack


def _kmer_collect(self, w, min_occ, suf_len=None, seed_mask=None):
    """fm6_traverse + ec_collect over all buckets: (bucket u32[], key u32[], val u8[], cnt[2]).  seed_mask: fmd_kmer_collect_seeds instead, the
    k-mers that end in a base of the mask (bit c-1 = nt6 base c)."""
    if suf_len is None:
        suf_len = w - 15 if w > 15 else 1   # compute_SUF (correct.c:319)
    b, k, v, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    cnt = (C.c_int64 * 2)()
    if seed_mask is None:
        check(lib().fmd_kmer_collect(self.h, w, min_occ, suf_len, C.byref(b), C.byref(k), C.byref(v), C.byref(n), cnt))
    else:
        check(lib().fmd_kmer_collect_seeds(self.h, w, min_occ, suf_len, seed_mask, C.byref(b), C.byref(k), C.byref(v), C.byref(n), cnt))
    m = n.value

    def take(p, ct, dt):   # (ctypes.string_at stops at 2^31 bytes; a 5*10^10-symbol index has 1.7*10^9 solid k-mers)
        return np.ctypeslib.as_array((ct * max(m, 1)).from_address(p.value))[:m].astype(dt, copy=True) if m else np.zeros(0, dtype=dt)
    out = (take(b, C.c_uint32, np.uint32), take(k, C.c_uint32, np.uint32), take(v, C.c_uint8, np.uint8), [cnt[0], cnt[1]])
    for p in (b, k, v):
        lib().fmd_host_free(p)
    return out


DevIndex.kmer_collect = _kmer_collect
DevIndex.kmer_collect_seeds = lambda self, w, min_occ, suf_len, seed_mask: _kmer_collect(self, w, min_occ, suf_len, seed_mask)   # one GPU's shard of `correct -g`


def _smem(self, seqs, self_match=0, max_mem=32):
    """fm6_smem for each read: list of INTV_DT arrays (one per read)."""
    flat, off = flatten_reads(seqs)
    n = len(off) - 1
    max_len = int(np.max(np.diff(off))) if n else 1
    mem = np.zeros((n, max_mem), dtype=INTV_DT); n_mem = np.zeros(n, dtype=np.uint32)
    check(lib().fmd_smem_batch(self.h, n, _ptr(flat), _ptr(off), self_match, max(max_len, 1), max_mem, _ptr(mem), _ptr(n_mem)))
    if (n_mem >> 31).any():
        raise FmdError("smem: capacity exceeded for %d reads (raise max_mem)" % int((n_mem >> 31).sum()))
    return [mem[i, :n_mem[i]].copy() for i in range(n)]


DevIndex.smem = _smem

SMEM_WIN_DT = np.dtype([("seq_off", "<u8"), ("seq_len", "<u4"), ("start", "<u4"), ("stop", "<u4"), ("reserved", "<u4")])


def _reach(self, seqs_zero_terminated):
    """len[p] = longest prefix of buffer[p..] (up to the next 0 byte) that occurs in the index."""
    buf = np.ascontiguousarray(seqs_zero_terminated, dtype=np.uint8)
    out = np.zeros(len(buf), dtype=np.uint32)
    check(lib().fmd_reach_batch(self.h, len(buf), _ptr(buf), _ptr(out)))
    return out


DevIndex.reach = _reach


def _smem_chain(self, seq, max_len=256, self_match=0, full_only=False):
    """fm6_smem of one long sequence, exactly as the reference walks it.  self_match=0: reach -> chain positions -> one
    fm6_smem1_core item per position, results concatenated in chain order.  With self_match the chain's step is not the plain
    reach (the forward sweep stops where fewer than two occurrences are left), so the sequence is one window [0, len) that walks
    the chain inside the kernel, as `exact -s` does on a long query.  max_len bounds the length of a match."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    L = len(seq)
    if L == 0:
        return np.zeros(0, dtype=INTV_DT)
    flat = np.zeros(L + 8, dtype=np.uint8); flat[:L] = seq
    if self_match:
        pos, stop = [0], [L]
    else:
        reach = self.reach(flat[:L + 1])
        pos = []
        x = 0
        while x < L:
            pos.append(x)
            x += int(reach[x]) if reach[x] else 1
        stop = np.array(pos) + 1
    n = len(pos)
    wins = np.zeros(n, dtype=SMEM_WIN_DT)
    wins["seq_len"] = L; wins["start"] = pos; wins["stop"] = stop; wins["reserved"] = 1 if full_only else 0
    max_mem = 2 * max_len + 2
    for _ in range(2):
        mem = np.zeros((n, max_mem), dtype=INTV_DT); n_mem = np.zeros(n, dtype=np.uint32)
        check(lib().fmd_smem_win_batch(self.h, n, _ptr(flat), L, _ptr(wins), self_match, max_len, max_mem, _ptr(mem), _ptr(n_mem)))
        need = int((n_mem & 0x7fffffff).max())
        if not (n_mem >> 31).any() or need <= max_mem:
            break
        max_mem = need   # rows that were too short: the low bits are the true counts (a whole chain in one window has no bound known up front)
    if (n_mem >> 31).any():
        raise FmdError("smem_chain: capacity exceeded in %d calls (raise max_len)" % int((n_mem >> 31).sum()))
    return np.concatenate([mem[i, :n_mem[i]] for i in range(n)])


DevIndex.smem_chain = _smem_chain


def build_index_inplace(reads_2d, device=0, pieces=3):
    """The index of equal-length reads through the in-place builder (fmd_builder_*: packed text, BWT slices written
    straight into the device layout, reads appended in `pieces` calls) -> DevIndex."""
    L = lib()
    reads_2d = np.ascontiguousarray(reads_2d, dtype=np.uint8)
    n, ln = reads_2d.shape
    b = C.c_void_p()
    check(L.fmd_builder_new(device, n, ln, C.byref(b)))
    try:
        step = max(1, (n + pieces - 1) // pieces)
        for s in range(0, n, step):
            part = reads_2d[s:s + step]
            d = C.c_void_p()
            check(L.fmd_dev_malloc(device, part.nbytes + 16, C.byref(d)))
            try:
                check(L.fmd_memcpy_h2d(d, _ptr(part), part.nbytes, None))
                check(L.fmd_builder_add_dev(b, None, len(part), d))
                check(L.fmd_memcpy_d2h(_ptr(np.zeros(1, np.uint8)), d, 1, None))   # the add kernel has read the piece before it is freed
            finally:
                L.fmd_dev_free(d)
        h = C.c_void_p()
        check(L.fmd_builder_finish(b, C.byref(h)))
        b = None
        return DevIndex(h)
    finally:
        if b:
            L.fmd_builder_free(b)


def build_bwt(seqs, device=0):
    """`fermi build` BWT of a read collection (list or 2-D array of nt6 reads), computed on the GPU."""
    flat, off = flatten_reads(seqs)
    n = len(off) - 1
    bwt = np.zeros(2 * (int(off[n]) + n), dtype=np.uint8)
    n_sym = C.c_uint64(0)
    check(lib().fmd_build_bwt(device, n, _ptr(flat), _ptr(off), _ptr(bwt), C.byref(n_sym)))
    assert n_sym.value == len(bwt)
    return bwt


STRAND_FWD, STRAND_REV, STRAND_BOTH = 1, 2, 3   # FMD_STRAND_*: the flags of ropebwt.c:14-15


def build_bwt_strands(seqs, strands=STRAND_BOTH, device=0):
    """`fermi ropebwt [-F] [-R]` BWT of a read collection (ropebwt.c:22-45): the forward strand, the reverse complement, or both per read."""
    flat, off = flatten_reads(seqs)
    n = len(off) - 1
    bwt = np.zeros((2 if strands == STRAND_BOTH else 1) * (int(off[n]) + n), dtype=np.uint8)
    n_sym = C.c_uint64(0)
    check(lib().fmd_build_bwt_strands(device, n, _ptr(flat), _ptr(off), int(strands), _ptr(bwt), C.byref(n_sym)))
    assert n_sym.value == len(bwt)
    return bwt


def fltuniq_table_words(k):
    """64-bit words of the k-mer state table of `fltuniq` (seq.c:161); raises for a k outside the range"""
    nb = lib().fmd_fltuniq_table_bytes(int(k))
    if nb == 0:
        check(FMD_E_ARG)
    return nb // 8


def fltuniq_pass(seqs, k, device=0):
    """main_fltuniq's verdict per read (seq.c:192-199) over nt6 reads: numpy bool, True = no non-base and no k-mer seen only once"""
    flat, off = flatten_reads(seqs)
    ok = np.zeros(max(len(off) - 1, 1), dtype=np.uint8)
    check(lib().fmd_fltuniq(device, int(k), _ptr(flat), _ptr(off), len(off) - 1, _ptr(ok)))
    return ok[:len(off) - 1].astype(bool)


def fltuniq_table(seqs, k, device=0):
    """the 2-bit k-mer states after pass 1 (seq.c:164-175) as the reference's flags[]: uint64 words"""
    flat, off = flatten_reads(seqs)
    tab = np.zeros(fltuniq_table_words(k), dtype=np.uint64)
    check(lib().fmd_fltuniq_table(device, int(k), _ptr(flat), _ptr(off), len(off) - 1, _ptr(tab)))
    return tab


SCAF_NONE = NONE64


def scaf_links(x, span, utig, length, excluded, max_dist, device=0):
    """The link stage of `scaf` (collect_nei, scaf.c:189-254) over the UR entries of all unitigs: x = read id << 1 | strand, span = b << 32 | e,
    utig = unitig of each entry; length / excluded per unitig.  Returns (self, mate, gkey, gval, n_nei) as include/fmd_hip.h describes them."""
    x = np.ascontiguousarray(x, dtype=np.uint64); span = np.ascontiguousarray(span, dtype=np.uint64); utig = np.ascontiguousarray(utig, dtype=np.uint32)
    length = np.ascontiguousarray(length, dtype=np.int32); excluded = np.ascontiguousarray(excluded, dtype=np.uint8)
    n, nu = len(x), len(length)
    assert len(span) == n and len(utig) == n and len(excluded) == nu
    own, mate, gkey, gval = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(4))
    n_nei = np.zeros(max(2 * nu, 1), dtype=np.uint32)
    ng = C.c_uint64(0)
    check(lib().fmd_scaf_links(device, n, _ptr(x), _ptr(span), _ptr(utig), nu, _ptr(length), _ptr(excluded), int(max_dist), _ptr(own), _ptr(mate),
                               _ptr(gkey), _ptr(gval), _ptr(n_nei), C.byref(ng)))
    return own[:n], mate[:n], gkey[:ng.value], gval[:ng.value], n_nei[:2 * nu]


def probe_gather(ws_bytes, line_bytes, n_access, iters=3, device=0):
    ms = C.c_float(0)
    check(lib().fmd_probe_gather(device, ws_bytes, line_bytes, n_access, iters, C.byref(ms)))
    return ms.value
