"""The link stage of `scaf` (collect_nei, scaf.c:189-254; include/fmd_hip.h: fmd_scaf_links) restated with Python dictionaries: the dictionary of
reads that occur once, the join of every entry with itself and its mate, the groups per (own end, mate's end).  Test infrastructure: what
tests/test_gpu_scaf_links.py holds the GPU against, and what tests/test_scaf_host.py feeds the host's choice of links with."""
import numpy as np

NONE = 0xFFFFFFFFFFFFFFFF


def restate(x, span, utig, length, excluded, max_dist):
    n = len(x)
    seen, val_of = {}, {}
    for i in range(n):
        u = int(utig[i])
        if excluded[u]:
            continue
        xi, sp = int(x[i]), int(span[i])
        dist = (sp & 0xffffffff) if xi & 1 else int(length[u]) - (sp >> 32)
        if dist > max_dist:
            continue
        r = xi >> 1
        seen[r] = seen.get(r, 0) + 1
        val_of[r] = (u << 1 | ((xi & 1) ^ 1)) << 32 | dist
    d = {r: v for r, v in val_of.items() if seen[r] == 1 and v != 0}
    own = np.full(n, NONE, dtype=np.uint64)
    mate = np.full(n, NONE, dtype=np.uint64)
    groups = {}
    for i in range(n):
        r, u = int(x[i]) >> 1, int(utig[i])
        s, m = d.get(r), d.get(r ^ 1)
        if s is not None:
            own[i] = s
        if m is not None:
            mate[i] = m
        if s is None or m is None or (m >> 33) == u:
            continue
        key = (u << 1 | (s >> 32 & 1)) << 32 | (m >> 32)
        groups[key] = groups.get(key, 0) + (1 << 40 | ((s & 0xffffffff) + (m & 0xffffffff)))
    keys = sorted(groups)
    n_nei = np.zeros(2 * len(length), dtype=np.uint32)
    for k in keys:
        n_nei[k >> 32] += 1
    return own, mate, np.array(keys, dtype=np.uint64), np.array([groups[k] for k in keys], dtype=np.uint64), n_nei
