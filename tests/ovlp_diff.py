"""Helper (no tests): what differs between two sets of overlap records, as text -- the message of every assert of test_gpu_ovlp_padded.py."""
import numpy as np

FIELDS = ("rank", "k", "len", "status", "n_ovlp", "rbeg", "ext_len", "n_nei", "flags", "reserved", "lfork")
F_OVERFLOW = 2


def _words(row):
    return " ".join("%016x" % w for w in np.frombuffer(row.tobytes(), dtype="<u8"))


def differing(rec_gpu, nei_gpu, rec_ref, nei_ref, fields=FIELDS, rows=None, first_nei_only=False):
    """per field (and "nei[j]") the mask of rows that differ, among `rows` (all by default); neighbour j is compared where the reference has more than j"""
    n = len(rec_ref)
    rows = np.ones(n, dtype=bool) if rows is None else np.asarray(rows, dtype=bool)
    out = {}
    for f in fields:
        d = rec_gpu[f] != rec_ref[f]
        out[f] = rows & (d.any(axis=1) if d.ndim > 1 else d)
    m = min(nei_gpu.shape[1], nei_ref.shape[1], 1 if first_nei_only else 1 << 30)
    for j in range(m):
        d = (nei_gpu["x"][:, j] != nei_ref["x"][:, j]).any(axis=1) | (nei_gpu["info"][:, j] != nei_ref["info"][:, j])
        out["nei[%d]" % j] = rows & (rec_ref["n_nei"] > j) & d
    return out


def explain(rec_gpu, nei_gpu, rec_ref, nei_ref, ids, fields=FIELDS, rows=None, first_nei_only=False, what=""):
    """text: the number of differing rows per field; the first ten differing ids with both records in full (words in hex), their candidate count
    and flags, and the neighbours of both.  `rows`: the rows that are compared at all (others are counted as left out)."""
    n = len(rec_ref)
    diff = differing(rec_gpu, nei_gpu, rec_ref, nei_ref, fields, rows, first_nei_only)
    any_d = np.zeros(n, dtype=bool)
    for d in diff.values():
        any_d |= d
    left_out = 0 if rows is None else int((~np.asarray(rows, dtype=bool)).sum())
    lines = ["%s: %d of %d rows differ (%d rows left out of the comparison)" % (what or "overlap records", int(any_d.sum()), n, left_out),
             "differing rows per field: " + ", ".join("%s %d" % (f, int(d.sum())) for f, d in diff.items())]
    for i in np.nonzero(any_d)[0][:10]:
        g, r = rec_gpu[i], rec_ref[i]
        lines.append("id %d (row %d): differs in %s" % (int(ids[i]), i, ", ".join(f for f, d in diff.items() if d[i])))
        for tag, rec, nei in (("got ", g, nei_gpu), ("want", r, nei_ref)):
            lines.append("  %s candidates %d, flags %#x (overflow %d), status %d, len %d, rbeg %d, ext_len %d, n_nei %d, reserved %d, lfork %#x"
                         % (tag, rec["n_ovlp"], rec["flags"], int((rec["flags"] & F_OVERFLOW) != 0), rec["status"], rec["len"], rec["rbeg"], rec["ext_len"],
                            rec["n_nei"], rec["reserved"], rec["lfork"]))
            lines.append("  %s record %s" % (tag, _words(rec)))
            for j in range(min(max(int(rec["n_nei"]), 0), nei.shape[1])):
                lines.append("  %s nei[%d] %s" % (tag, j, _words(nei[i, j])))
    return "\n".join(lines)


def same(rec_gpu, nei_gpu, rec_ref, nei_ref, fields=FIELDS, rows=None, first_nei_only=False):
    return not any(d.any() for d in differing(rec_gpu, nei_gpu, rec_ref, nei_ref, fields, rows, first_nei_only).values())
