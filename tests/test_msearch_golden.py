"""CPU: the fixture of the multi-index backward search (tests/golden/msearch.npz, made by tests/golden/make_golden_msearch.py from the
reference's fm_multi_backward_search and fm_backward_search), the three C-ABI entries, the `msearch` usage error -- and the kernel's
formulation of the search (no `done` flag: a part is done when its interval is empty; the search ends when every part's is) worked by hand
over the oracle's rank against the recorded results."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from fermi_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
ENTRIES = ["fmd_multi_bsearch_work_bytes", "fmd_multi_bsearch_dev", "fmd_multi_bsearch_batch"]


@pytest.fixture(scope="module")
def npz():
    d = dict(np.load(os.path.join(GOLD, "msearch.npz")))
    return d, json.loads(bytes(d["sets"]).decode())


def test_fixture_holds_what_its_maker_asserted(npz):
    d, sets = npz
    assert sorted(sets) == sorted(["tiny_special", "tiny_special_repeat", "special_palin", "dup32_palin", "tiny_tiny", "tiny_empty_special"])
    for name, (parts, merged) in sets.items():
        n = len(d[name + ".off"]) - 1
        assert n >= 3000 and d[name + ".part_cnt"].shape == (len(parts), n)
        for f in ("cnt", "beg", "end"):                                       # multi over the parts == single on the merged file
            assert np.array_equal(d[name + ".multi_" + f], d[name + ".single_" + f]), (name, f)
        miss = d[name + ".multi_cnt"] == 0
        assert not d[name + ".multi_beg"][miss].any() and not d[name + ".multi_end"][miss].any()
        hit = d[name + ".part_cnt"] > 0
        assert np.array_equal(hit.any(0), ~miss)
        assert np.array_equal(d[name + ".part_cnt"].sum(0), d[name + ".multi_cnt"])      # the merged count is the sum of the parts'
        if len(set(parts)) > 1:
            partial = hit.any(0) & ~hit.all(0)
            assert partial.mean() >= 0.2 and miss.mean() >= 0.2, (name, partial.mean(), miss.mean())
        ln = np.diff(d[name + ".off"].astype(np.int64))
        assert ln.min() >= 1 and set(np.unique(d[name + ".kind"])) == {0, 1, 2}
        assert d[name + ".seqs"].min() >= 1 and d[name + ".seqs"].max() == 5


def test_header_declares_and_library_exports_the_entries():
    hdr = open(os.path.join(ROOT, "include", "fmd_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fmd_[a-z0-9_]+)\s*\(", hdr))
    L = api.lib()
    for s in ENTRIES:
        assert s in declared and s in api.ABI_SYMBOLS and hasattr(L, s), s
    m = re.search(r"#define\s+FMD_MULTI_MAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == api.FMD_MULTI_MAX >= 16
    # the argument checks come before anything touches a device
    assert L.fmd_multi_bsearch_batch(0, None, 1, None, None, None, None, None) == api.FMD_E_ARG
    assert L.fmd_multi_bsearch_batch(api.FMD_MULTI_MAX + 1, None, 1, None, None, None, None, None) == api.FMD_E_ARG
    assert L.fmd_multi_bsearch_work_bytes(0, 10) == 0 and L.fmd_multi_bsearch_work_bytes(api.FMD_MULTI_MAX + 1, 10) == 0
    assert 0 < L.fmd_multi_bsearch_work_bytes(1, 10) <= L.fmd_multi_bsearch_work_bytes(api.FMD_MULTI_MAX, 10)


def test_msearch_usage_and_unreadable_files(tmp_path):
    q = os.path.join(GOLD, "tiny.fq.gz")
    for args in ([], [q]):                                                    # no index argument
        p = subprocess.run([AMD, "msearch"] + args, capture_output=True, timeout=60)
        assert p.returncode == 1 and b"Usage:" in p.stderr and b"msearch" in p.stderr and p.stdout == b""
    p = subprocess.run([AMD, "msearch", q, os.path.join(GOLD, "tiny.fmd"), str(tmp_path / "missing.fmd")], capture_output=True, timeout=60)
    assert p.returncode == 1 and b"missing.fmd" in p.stderr and b"no usable HIP device" not in p.stderr
    p = subprocess.run([AMD, "msearch", q] + [os.path.join(GOLD, "tiny.fmd")] * (api.FMD_MULTI_MAX + 1), capture_output=True, timeout=60)
    assert p.returncode == 1 and b"at most" in p.stderr
    p = subprocess.run([AMD], capture_output=True, timeout=60)
    assert b"msearch" in p.stderr


def test_search_without_a_done_flag_gives_the_recorded_results(npz, oracle_lib):
    """fmd_multi.hip keeps no `done` flag (exact.c:29): part j takes rank11 when k_j == l_j and rank21 otherwise, a k_j - 1 of 2^64 - 1 ranks
    to zero, and the search is a miss as soon as every part's interval is empty.  The same rule over the oracle's rank1a, every 9th query."""
    import orcbind
    d, sets = npz
    NONE = 0xFFFFFFFFFFFFFFFF
    idx = {}
    for name, (parts, merged) in sets.items():
        for p in parts:
            if p not in idx:
                idx[p] = orcbind.OrcIndex(os.path.join(GOLD, p + ".fmd"))
        os_ = [idx[p] for p in parts]
        cnt = [[int(x) for x in o.cnt] for o in os_]

        def rank(o, k, c):
            return 0 if k == NONE else int(o.rank1a(np.array([k], np.uint64))[0][0, c])
        seqs, off = d[name + ".seqs"], d[name + ".off"]
        for i in range(0, len(off) - 1, 9):
            q = seqs[int(off[i]):int(off[i + 1])]
            c = int(q[-1])
            k, l = [cn[c] for cn in cnt], [cn[c + 1] for cn in cnt]
            pos, res = len(q) - 2, None
            while res is None:
                if k == l:
                    res = (0, 0, 0)
                elif pos < 0:
                    res = (sum(l) - sum(k), sum(k), sum(l) - 1)
                else:
                    c = int(q[pos])
                    for j, o in enumerate(os_):
                        ok = rank(o, (k[j] - 1) & NONE, c)
                        ol = rank(o, l[j] - 1, c) if k[j] != l[j] else ok
                        k[j], l[j] = cnt[j][c] + ok, cnt[j][c] + ol
                    pos -= 1
            assert res == (int(d[name + ".multi_cnt"][i]), int(d[name + ".multi_beg"][i]), int(d[name + ".multi_end"][i])), (name, i)
    for o in idx.values():
        o.close()
