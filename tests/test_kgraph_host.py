"""CPU: the host side of kgraph -- fmdh_kgraph_compact_host (the one-thread walk that labels the unitigs from the k-mers and their arc bytes) and the
three formatters of `fermi-amd kgraph` -- against the definitions restated in Python (tests/kgraph_ref.py), on hand-made graphs: a path, a bubble, a
tip, an isolated cycle that the reads enter away from its smallest node, a homopolymer loop, a hairpin through a (k+1)-mer that is its own reverse
complement (and one whose halved count falls below the threshold), two nodes joined in opposite orientations, no node, one node."""
import os
import random
import subprocess

import numpy as np
import pytest

from fermi_amd import api, hostlib
import kgraph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMD = os.path.join(ROOT, "fermi_amd", "bin", "fermi-amd")


def as_arrays(nodes, counts, arcs):
    return (np.array([R.pack(x) for x in nodes], dtype=np.uint64), np.array(counts, dtype=np.uint32), np.array(arcs, dtype=np.uint8))


def same_labelling(got, want):
    """an api.KUnitigs against the restated Compacted, every array"""
    assert got.unitig.tolist() == want.unitig and got.offset.tolist() == want.offset and got.orient.tolist() == want.orient
    assert got.u_nodes.tolist() == want.u_nodes and got.u_first.tolist() == want.u_first and got.u_flags.tolist() == want.u_flags
    assert got.strings() == want.strings


def run(reads, k, min_occ):
    nodes, counts, arcs = R.graph_from_strings(reads, k, min_occ)
    want = R.compact(nodes, arcs, k, counts)
    km, ct, ar = as_arrays(nodes, counts, arcs)
    got = hostlib.kgraph_compact_host(k, km, ar, ct)
    same_labelling(got, want)
    assert got.stat == dict(n_nodes=len(nodes), n_arcs=want.n_arcs, n_links=want.n_links, n_unitigs=want.n_unitigs, n_cycles=want.n_cycles)
    assert want.n_arcs == sum(1 for c in R.count_dict(reads, k + 1).values() if c >= min_occ)
    assert hostlib.kgraph_gfa_text(got) == R.gfa_text(want, k)
    assert hostlib.kgraph_fasta_text(got) == R.fasta_text(want)
    assert hostlib.kgraph_arcs_text(k, km, ct, ar) == R.arcs_text(nodes, counts, arcs)
    return nodes, counts, arcs, want, got


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_shapes(name):
    k, min_occ, reads = R.SHAPES[name]
    nodes, counts, arcs, want, got = run(reads, k, min_occ)
    R.check_shape(name, nodes, counts, arcs, want)
    for x, a in zip(nodes, arcs):                      # arcs are symmetric: x.c is an arc of x iff it is a left arc of its last k bases
        for c in range(4):
            if a >> c & 1:
                v = x[1:] + "ACGT"[c]
                j, b = (nodes.index(v), 16 << R.CODE[x[0]]) if v < R.rc(v) else (nodes.index(R.rc(v)), 1 << 3 - R.CODE[x[0]])
                assert arcs[j] & b


def test_gfa_of_the_cycle_and_the_loops():
    k, min_occ, reads = R.SHAPES["cycle"]
    got = run(reads, k, min_occ)[4]
    assert hostlib.kgraph_gfa_text(got).endswith("L\t0\t+\t0\t+\t4M\n") and hostlib.kgraph_gfa_text(got).count("\nL\t") == 1
    k, min_occ, reads = R.SHAPES["homopolymer"]
    nodes, _, _, want, got = run(reads, k, min_occ)
    u = want.unitig[nodes.index("AAAAA")]
    assert "L\t%d\t+\t%d\t+\t4M\n" % (u, u) in hostlib.kgraph_gfa_text(got)          # the loop, once: its twin leaves (u, -)
    assert "L\t%d\t-\t%d\t-\t4M\n" % (u, u) not in hostlib.kgraph_gfa_text(got)
    k, min_occ, reads = R.SHAPES["hairpin"]
    nodes, _, _, want, got = run(reads, k, min_occ)
    u = want.unitig[nodes.index("ACGCG")]
    assert "L\t%d\t+\t%d\t-\t4M\n" % (u, u) in hostlib.kgraph_gfa_text(got)          # its own twin


@pytest.mark.parametrize("k,min_occ", [(3, 1), (5, 1), (5, 2), (7, 2), (11, 1)])
def test_random_reads(k, min_occ):
    """reads off a short random genome with a repeat, both strands, some with a substitution: branches, tips and bubbles of every kind"""
    rng = random.Random(k * 10 + min_occ)
    genome = "".join(rng.choice("ACGT") for _ in range(150))
    genome += genome[20:60] + "".join(rng.choice("ACGT") for _ in range(60))
    reads = []
    for _ in range(120):
        a = rng.randrange(len(genome) - 30)
        r = genome[a:a + 30]
        if rng.random() < 0.15:
            p = rng.randrange(30)
            r = r[:p] + rng.choice("ACGT") + r[p + 1:]
        reads.append(R.rc(r) if rng.random() < 0.5 else r)
    reads.append("ACGTNNACGTACGGTNACGTTGCA")
    nodes, counts, arcs, want, got = run(reads, k, min_occ)
    assert want.n_unitigs > 3 and (k == 3 or max(want.u_nodes) > 3)    # (at k = 3 nearly every 4-mer occurs: nothing compacts)


def test_long_chain_and_long_cycle():
    """5000 nodes in one chain, and the same sequence closed into a circle"""
    rng = random.Random(7)
    k = 15
    s = "".join(rng.choice("ACGT") for _ in range(5000 + k - 1))
    nodes, _, _, want, _ = run([s], k, 1)
    assert want.n_unitigs == 1 and want.u_nodes == [5000] and want.strings[0] in (s, R.rc(s))
    circ = s[:5000]
    nodes, _, _, want, _ = run([circ + circ[:k]], k, 1)
    assert want.n_unitigs == 1 and want.n_cycles == 1 and want.u_nodes == [5000] and want.u_first == [0]
    assert want.strings[0][:k] == nodes[0] and want.strings[0][:5000] in ((circ + circ)[j:j + 5000] for j in range(5000)) or \
        R.rc(want.strings[0])[k - 1:] in ((circ + circ)[j:j + 5000] for j in range(5000))


def test_refused_arguments():
    km = np.array([R.pack("ACCGT")], dtype=np.uint64)
    for k in (4, 1, 2, 32, 33, 0, -1):
        with pytest.raises(ValueError):
            hostlib.kgraph_compact_host(k, km, np.zeros(1, np.uint8))
    with pytest.raises(ValueError):
        hostlib.kgraph_compact_host(5, km, np.zeros(2, np.uint8))
    fmd = os.path.join(ROOT, "tests", "golden", "tiny.fmd")
    for args in (["-k", "20"], ["-k", "33"], ["-k", "1"], ["-o", "0"], ["-f", "-a"], []):   # refused before a device is looked for
        a = subprocess.run([AMD, "kgraph"] + args + ([fmd] if args else []), capture_output=True, timeout=60)
        assert a.returncode == 1 and b"Usage:   fermi-amd kgraph" in a.stderr and a.stdout == b"", args
    a = subprocess.run([AMD, "kgraph", "/nonexistent.fmd"], capture_output=True, timeout=60)
    assert a.returncode == 1 and b"fail to open file" in a.stderr
    a = subprocess.run([AMD], capture_output=True, timeout=60)
    assert b"kgraph" in a.stderr


def test_symbols_are_declared():
    assert "fmd_karcs" in api.ABI_SYMBOLS and "fmd_kunitig" in api.ABI_SYMBOLS
    assert api.KGRAPH_STAT_DT.itemsize == 80
