"""CPU: `fermi-amd clean` (host/mag.c, mag_bubble.c, swscore.c, clean_cmd.c) against what `fermi clean` printed for the same graphs
(tests/golden/make_golden_clean.py): every byte of every output, from a plain file, a gzip file and stdin; the usage text; malformed
input; the alignment score against ksw_align's; and, where the reference is compiled here, the single operations one after the other
with the parameters the reference's local assembler gives them (scaf.c:418-428).  No GPU is asked for: HIP_VISIBLE_DEVICES is empty."""
import ctypes as C
import gzip
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")
REFLIB = os.path.join(ROOT, "oracle", "_ref", "libfermi_ref.so")
sys.path.insert(0, GOLD)
import make_golden_clean as mk  # noqa: E402  (the option sets live in one place: the script that made the fixtures)

MANIFEST = json.load(open(os.path.join(GOLD, "clean.manifest.json")))
HAND = json.load(gzip.open(os.path.join(GOLD, "clean.hand.json.gz"), "rt"))
SW = json.load(open(os.path.join(GOLD, "clean.sw.json")))
ENV = dict(os.environ, HIP_VISIBLE_DEVICES="")


def _run(args, **kw):
    assert os.path.exists(AMD), "fermi-amd is not built"
    return subprocess.run([AMD] + args, capture_output=True, timeout=120, env=ENV, **kw)


def _gold(name):
    data = gzip.open(os.path.join(GOLD, name)).read()
    assert hashlib.md5(data).hexdigest() == MANIFEST["md5"][name], name
    return data


def _clean(args, path=None, data=None):
    p = _run(["clean"] + args + [path or "-"], input=data)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout


@pytest.fixture(scope="module")
def clean3_plain(tmp_path_factory):
    p = tmp_path_factory.mktemp("clean3") / "clean3.mag"
    p.write_bytes(_gold("clean3.mag.gz"))
    return str(p)


def test_no_device_is_needed():
    code = "from fermi_amd import api; print(api.device_count())"
    n = subprocess.run([sys.executable, "-c", code], capture_output=True, env=ENV, cwd=ROOT)
    assert n.returncode == 0 and int(n.stdout) == 0                     # fmd_device_count() == 0 under this environment ...
    assert _clean(["-C"], os.path.join(GOLD, "tiny.mag.gz")) == _gold("tiny.clean_C.mag.gz")   # ... and clean runs


@pytest.mark.parametrize("tag,args", mk.RUNS, ids=[t for t, _ in mk.RUNS])
def test_clean3_every_option_set(clean3_plain, tag, args):
    want = _gold("clean3.%s.mag.gz" % tag)
    assert want.count(b"\n+\n") == MANIFEST["unitigs"][tag]
    assert _clean(args, clean3_plain) == want                                                  # a plain file
    assert _clean(args, os.path.join(GOLD, "clean3.mag.gz")) == want                           # gzip
    assert _clean(args, data=open(clean3_plain, "rb").read()) == want                          # stdin
    assert _clean(args, data=open(os.path.join(GOLD, "clean3.mag.gz"), "rb").read()) == want   # gzip on stdin


def test_clean3_outputs_differ_from_each_other():
    """every option set does something of its own on this input: no golden is another one's copy"""
    md5 = [MANIFEST["md5"]["clean3.%s.mag.gz" % t] for t, _ in mk.RUNS] + [MANIFEST["md5"]["clean3.%s.mag.gz" % mk.CHAIN[0]], MANIFEST["md5"]["clean3.mag.gz"]]
    assert len(set(md5)) == len(md5)
    n = MANIFEST["unitigs"]
    assert n["unitig"] == n["clean_O"] > n["clean"] > n["clean_CS"] > n["clean_C"] > n[mk.CHAIN[0]] >= n["clean_CA"] > 0


def test_the_chain_of_the_driver_script(clean3_plain):
    """run-fermi.pl:91-94: clean, then clean -CAOFo <k> over its output"""
    first = _clean([], clean3_plain)
    assert first == _gold("clean3.clean.mag.gz")
    assert _clean(mk.CHAIN[1], data=first) == _gold("clean3.%s.mag.gz" % mk.CHAIN[0])
    sh = "set -o pipefail; '%s' clean '%s' | '%s' clean -CAOFo 33 -" % (AMD, clean3_plain, AMD)
    p = subprocess.run(["bash", "-c", sh], capture_output=True, timeout=120, env=ENV)
    assert p.returncode == 0 and p.stdout == _gold("clean3.%s.mag.gz" % mk.CHAIN[0])


@pytest.mark.parametrize("tag,args", mk.RUNS[:2], ids=[t for t, _ in mk.RUNS[:2]])
@pytest.mark.parametrize("name", mk.SMALL)
def test_small_graphs(name, tag, args):
    got = _clean(args, os.path.join(GOLD, name + ".mag.gz"))
    assert got == _gold("%s.%s.mag.gz" % (name, tag))
    if name == "special":
        assert got == b""                                   # every unitig of it is a one-read tip


@pytest.mark.parametrize("tag,args", mk.RUNS[:2], ids=[t for t, _ in mk.RUNS[:2]])
def test_records_without_qualities(tag, args):
    """FASTA records: coverage '"' everywhere; arcs into the part of the graph that is not in the file are amended away"""
    src = _gold("clean3.first100.fa.gz")
    assert src.count(b">") == 100 and b"+" not in src
    got = _clean(args, os.path.join(GOLD, "clean3.first100.fa.gz"))
    assert got == _gold("clean3.first100.%s.mag.gz" % tag) and b'\n+\n"' in got


def test_empty_input(tmp_path):
    p = tmp_path / "empty.mag"
    p.write_bytes(b"")
    for args in ([], ["-C"], ["-CA"]):
        assert _clean(args, str(p)) == b""
    assert _clean(["-C"], data=b"") == b""


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_graphs(name, tmp_path):
    case = HAND[name]
    p = tmp_path / "h.mag"
    p.write_text(case["mag"])
    assert 2 <= case["mag"].count("\n+\n") <= 6 and sorted(case["out"]) == sorted(" ".join(a) for a in mk.HAND_RUNS)
    for args, want in case["out"].items():
        assert _clean(args.split(), str(p)).decode("ascii") == want, args


def test_hand_written_graphs_show_what_they_are_for():
    n = lambda name, args: HAND[name]["out"][args].count("\n+\n")
    assert n("tip", "") == 3 and n("tip", "-C") == 1                                    # the tip goes, the rest merges
    assert n("bubble_weak_arm", "") == 4 and n("bubble_weak_arm", "-C") == 3 and n("bubble_equal_arms", "-CA") == 4      # the weak arm goes, of two equal ones neither
    assert n("arm_shorter_than_overlaps", "-C") == 3
    assert n("flip_on_merge", "") == 1 and n("neighbour_missing", "") == 1
    assert n("low_count_internal", "") == 5 and n("low_count_internal", "-C") == 4
    assert "," not in HAND["neighbour_missing"]["out"][""].split("\n")[0]               # both arcs to nowhere are gone


def test_usage():
    p = _run(["clean"])
    assert p.returncode == 1 and p.stdout == b""
    want = ("\nUsage:   fermi-amd clean [options] <in.mog>\n\n"
            "Options: -N INT      read maximum INT neighbors per node [512]\n"
            "         -d FLOAT    drop a neighbor if relative overlap ratio below FLOAT [0.70]\n\n"
            "         -C          clean the graph\n"
            "         -l INT      minimum tip length [300]\n"
            "         -e INT      minimum tip read count [4]\n"
            "         -i INT      minimum internal unitig read count [3]\n"
            "         -o INT      minimum overlap [60]\n"
            "         -R FLOAT    minimum relative overlap ratio [0.80]\n"
            "         -n INT      number of iterations [3]\n"
            "         -A          aggressive bubble popping\n"
            "         -S          skip bubble simplification\n"
            "         -w FLOAT    minimum coverage to keep a bubble [10.00]\n"
            "         -r FLOAT    minimum fraction to keep a bubble [0.15]\n\n")
    assert p.stderr.decode() == want
    p = _run(["clean", "-l", "77", "-d", "0.5"])
    assert p.returncode == 1 and "[77]" in p.stderr.decode() and "[0.50]" in p.stderr.decode()
    top = _run([]).stderr.decode()
    for cmd in ("clean ", "example ", "seqrank "):
        assert "         " + cmd in top


def _bad_inputs():
    good = gzip.open(os.path.join(GOLD, "clean3.mag.gz")).read()
    recs = good.split(b"\n")
    at = next(i for i in range(4, len(recs), 4) if b"," in recs[i])
    cut = b"\n".join(recs[:at]) + b"\n" + recs[at][:recs[at].rindex(b",")]   # the file ends inside a header, in the middle of an arc
    hdr = good.replace(b"@", b"@x", 1)                                      # a name that is no number
    nsr = b"@1:2\tmany\t.\t.\nACGT\n+\n5555\n"
    arc = b"@1:2\t3\t7,x;\t.\nACGT\n+\n5555\n"
    nohdr = b"@1:2\nACGT\n+\n5555\n"
    dangling = HAND["tip"]["mag"].replace("\t.\t", "\t424242,50;\t", 1).encode()   # -OF: taken as it is, an arc to an end nobody has
    twin = HAND["tip"]["mag"].encode().replace(b",50;", b",51;", 1)          # -OF: the arc back says another overlap
    return [("truncated", [], cut), ("name", [], hdr), ("nsr", [], nsr), ("arc", [], arc), ("no_header_fields", [], nohdr),
            ("dangling_arc", ["-COF"], dangling), ("twin_differs", ["-OF"], twin)]


@pytest.mark.parametrize("tag,args,data", _bad_inputs(), ids=[b[0] for b in _bad_inputs()])
def test_malformed_input_is_an_error_not_a_crash(tag, args, data):
    p = _run(["clean"] + args + ["-"], input=data)
    assert p.returncode == 1, (p.returncode, p.stderr.decode()[-500:])      # not a signal, not 0
    assert p.stdout == b"" and b"[E::" in p.stderr


def test_sw_score_is_ksw_aligns():
    from fermi_amd import hostlib
    assert len(SW) > 150
    seen = set()
    for c in SW:
        a, b = c["a"], c.get("b", c["a"])
        seen.add(c["score"])
        assert hostlib.sw_score(a.encode(), b.encode()) == c["score"], (a[:50], b[:50])
        assert hostlib.sw_score(b.encode(), a.encode()) == c["score"]
    assert {0, 5, 10, 32765, 32767} <= seen                                 # nothing in common, lengths 1 and 2, below and at the 16-bit ceiling
    assert [(len(c["a"]), c["score"]) for c in SW if "b" not in c] == [(6553, 32765), (6554, 32767), (7000, 32767)]
    assert hostlib.sw_score(b"", b"ACGT") == 0 and hostlib.sw_score(b"ACGNNT", b"ACGNNT") == 15   # an N matches nothing, itself included


def test_a_quality_string_of_the_wrong_length_ends_the_graph(tmp_path):
    """as in the reference (mag.c:205 reads while the reader returns a length); special.mag.gz is such a file from its first record on, and its
    golden -- nothing -- says what the reference does.  Here: the records before the bad one are the graph, and stderr says so."""
    recs = gzip.open(os.path.join(GOLD, "clean3.mag.gz")).read().split(b"\n")
    whole = b"\n".join(recs[:40]) + b"\n"
    p = _run(["clean", "-O", "-"], input=whole + b"\n".join(recs[40:43]) + b"\n" + recs[43][:10] + b"\n" + b"\n".join(recs[44:60]) + b"\n")
    assert p.returncode == 0 and b"[W::fmdh_mag_read] record 11:" in p.stderr
    assert p.stdout == _clean(["-O"], data=whole) and p.stdout.count(b"\n+\n") == 10
    assert b"[W::fmdh_mag_read] record 1:" in _run(["clean", os.path.join(GOLD, "special.mag.gz")]).stderr


# ---- the single operations against the reference's, where it is compiled here ----
class _Arc(C.Structure):
    _fields_ = [("x", C.c_uint64), ("y", C.c_uint64)]


class _ArcV(C.Structure):    # ku128_v
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.POINTER(_Arc))]


class _RefV(C.Structure):    # magv_t, mag.h:29-36
    _fields_ = [("len", C.c_int), ("nsr", C.c_int), ("max_len", C.c_uint32), ("k", C.c_uint64 * 2), ("nei", _ArcV * 2),
                ("seq", C.POINTER(C.c_char)), ("cov", C.POINTER(C.c_char)), ("ptr", C.c_void_p)]

    def ends(self):          # per end: its id, the number of slots of its list, the live arcs in order
        out = []
        for j in range(2):
            arcs = [(self.nei[j].a[k].x, self.nei[j].a[k].y) for k in range(self.nei[j].n)]
            out.append((self.k[j], len(arcs), tuple(a for a in arcs if a[0] != 2 ** 64 - 2 and a[1] != 0)))
        return tuple(out)


class _OurArcs(C.Structure):  # fmdh_arcs_t, host/mag.h: the live arcs, and how many went since the list was compacted
    _fields_ = [("a", C.POINTER(_Arc)), ("n", C.c_uint32), ("room", C.c_uint32), ("n_gone", C.c_uint32)]


class _OurEnd(C.Structure):
    _fields_ = [("id", C.c_uint64), ("arcs", _OurArcs)]


class _OurV(C.Structure):    # fmdh_magv_t
    _fields_ = [("len", C.c_int), ("nsr", C.c_int), ("cap", C.c_uint32), ("aux", C.c_int32), ("end", _OurEnd * 2),
                ("seq", C.POINTER(C.c_char)), ("cov", C.POINTER(C.c_char))]

    def ends(self):
        return tuple((e.id, e.arcs.n + e.arcs.n_gone, tuple((e.arcs.a[k].x, e.arcs.a[k].y) for k in range(e.arcs.n))) for e in self.end)


def _graph_struct(vtype):
    class G(C.Structure):
        _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("v", C.POINTER(vtype)), ("rdist", C.c_float), ("min_ovlp", C.c_int)]
    return G


class _Opt(C.Structure):     # magopt_t = fmdh_magopt_t
    _fields_ = [(n, C.c_int) for n in ("flag", "max_arc", "n_iter", "min_ovlp", "min_elen", "min_ensr", "min_insr", "max_bdist", "max_bvtx")] + \
               [(n, C.c_float) for n in ("min_dratio0", "min_dratio1", "max_bcov", "max_bfrac")]


def _dump(g):
    """every slot: reads, both ends (id, slots of the arc list -- deleted arcs count until a list is compacted --, live arcs in order),
    bases and coverage"""
    out = []
    for i in range(g.n):
        v = g.v[i]
        out.append(None if v.len < 0 else (v.nsr, v.ends(), C.string_at(v.seq, v.len), C.string_at(v.cov, v.len)))
    return out


def test_single_operations_against_the_reference(clean3_plain):
    if not os.path.exists(REFLIB):
        pytest.skip("the reference is not compiled here (oracle/_ref)")
    from fermi_amd import hostlib
    ours, ref = hostlib.lib(), C.CDLL(REFLIB)
    opt = _Opt()
    ours.fmdh_mag_init_opt(C.byref(opt))
    opt.flag = 0x1 | 0x40                                # as it is in the file, nothing amended, nothing merged: fm6_api_unitig's graph
    ours.fmdh_mag_read.restype = C.POINTER(_graph_struct(_OurV))
    ref.mag_g_read.restype = C.POINTER(_graph_struct(_RefV))
    a, b = ours.fmdh_mag_read(clean3_plain.encode(), C.byref(opt)), ref.mag_g_read(clean3_plain.encode(), C.byref(opt))
    assert a and b
    for lib_, names in ((ours, ("fmdh_mag_merge", "fmdh_mag_rm_vext", "fmdh_mag_rm_edge", "fmdh_mag_simplify_bubble", "fmdh_mag_pop_simple", "fmdh_mag_pop_open", "fmdh_mag_rm_vint")),
                        (ref, ("mag_g_merge", "mag_g_rm_vext", "mag_g_rm_edge", "mag_g_simplify_bubble", "mag_g_pop_simple", "mag_g_pop_open", "mag_g_rm_vint"))):
        for n, at in zip(names, ([C.c_void_p, C.c_int], [C.c_void_p, C.c_int, C.c_int], [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int],
                                 [C.c_void_p, C.c_int, C.c_int], [C.c_void_p, C.c_float, C.c_float, C.c_int], [C.c_void_p, C.c_int], [C.c_void_p, C.c_int, C.c_int, C.c_int])):
            getattr(lib_, n).argtypes = at
            getattr(lib_, n).restype = None
    ours.fmdh_mag_destroy.argtypes = [C.c_void_p]
    max_len = 100
    steps = [("merge", (1,)), ("rm_vext", (int(max_len * 1.1), 4)), ("simplify_bubble", (25, max_len * 2)), ("pop_simple", (10., 0.15, 1)),
             ("rm_edge", (0, 0.8, int(max_len * 1.1), 5)), ("merge", (1,)), ("rm_vext", (int(max_len * 1.1), 100)), ("merge", (0,)),
             ("simplify_bubble", (25, max_len * 2)), ("pop_simple", (10., 0.15, 1)),
             ("pop_open", (300,)), ("rm_vint", (300, 3, 60)), ("merge", (1,))]          # (the last three: not in scaf.c, so that every operation is stepped once)
    assert _dump(a.contents) == _dump(b.contents)
    alive = []
    for i, (op, args) in enumerate(steps):
        getattr(ours, "fmdh_mag_" + op)(a, *args)
        getattr(ref, "mag_g_" + op)(b, *args)
        da, db = _dump(a.contents), _dump(b.contents)
        assert da == db, "step %d: %s%r" % (i, op, args)
        alive.append(sum(1 for v in da if v is not None))
    assert alive[0] <= MANIFEST["unitigs"]["unitig"] and alive[-1] < alive[0] and len(set(alive)) > 4   # the steps do change the graph
    # the graph as `clean` reads it (arcs filtered, tips cut, amended, merged) and the read distance estimated on the way
    ours.fmdh_mag_init_opt(C.byref(opt))
    c, d = ours.fmdh_mag_read(clean3_plain.encode(), C.byref(opt)), ref.mag_g_read(clean3_plain.encode(), C.byref(opt))
    assert _dump(c.contents) == _dump(d.contents) and c.contents.min_ovlp == d.contents.min_ovlp
    ours.fmdh_mag_destroy(c)
    ours.fmdh_mag_cal_rdist.restype = ref.mag_cal_rdist.restype = C.c_double
    ours.fmdh_mag_cal_rdist.argtypes = ref.mag_cal_rdist.argtypes = [C.c_void_p]
    big = os.path.join(GOLD, "gen_rule_20k.mag.gz").encode()         # unitigs long enough to pass the A-statistic: a finite estimate
    e, f = ours.fmdh_mag_read(big, C.byref(opt)), ref.mag_g_read(big, C.byref(opt))
    assert e.contents.rdist == f.contents.rdist and 1 < e.contents.rdist < 100      # estimated before the merge that ends the reading ...
    assert ours.fmdh_mag_cal_rdist(e) == ref.mag_cal_rdist(f) > 1                    # ... and again on the merged graph
    ours.fmdh_mag_destroy(e)
    ours.fmdh_mag_destroy(a)
