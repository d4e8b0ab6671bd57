"""bench.py without --full: the headline alone (set-up, warm-up, the timed steps, the JSON line), and --dump-outputs: a fixed sample of
what the last timed step computed, the same from run to run.  CPU: what the sample keeps of a job's arrays, the argument check;
GPU: two plain runs at 10^6 reads."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
DUMPED = ("ids.npy", "records.npy", "neighbours.npy", "sequences.npy")


def test_dump_outputs_keeps_what_a_caller_receives(tmp_path):
    """records whole, neighbours up to n_nei, sequence rows up to len + ext_len; every 32-bit word exact in float64"""
    import torch
    from benchlegs.overlap import dump_outputs
    from fermi_amd import api

    class Job:
        pass
    n, rng = 1000, np.random.default_rng(0)
    j = Job()
    j.n, j.max_nei, j.stride, j.dev = n, 4, 200, torch.device("cpu")
    j.ids = torch.arange(0, 2 * n, 2, dtype=torch.int64)
    rec = np.zeros(n, dtype=api.OVLP_DT)
    rec["rank"] = (1 << 40) + np.arange(n)
    rec["k"] = rng.integers(0, 1 << 62, size=(n, 3), dtype=np.uint64)
    rec["len"] = 100
    rec["ext_len"] = np.arange(n) % 7 - 1
    rec["n_nei"] = np.arange(n) % 6
    rec["flags"] = 0xfffffff0
    j.rec = torch.from_numpy(rec.view(np.uint8).copy())
    j.nei = torch.from_numpy(rng.integers(0, 256, n * 4 * 32, dtype=np.uint8))
    j.seq = torch.from_numpy(rng.integers(1, 6, n * 200, dtype=np.uint8))
    dump_outputs(torch, j, str(tmp_path), rows=64)
    got = {f: np.load(str(tmp_path / f)) for f in DUMPED}
    assert got["sequences.npy"].dtype == np.float32 and all(got[f].dtype == np.float64 for f in DUMPED[:3])
    rows = got["ids.npy"].astype(np.int64) // 2
    assert len(rows) == 64 and np.array_equal(got["ids.npy"], 2 * rows) and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["records.npy"].astype(np.uint32).view(api.OVLP_DT).reshape(-1), rec[rows])
    nei, seq = j.nei.numpy().reshape(n, 128), j.seq.numpy().reshape(n, 200)
    for i, r in enumerate(rows):
        k, u = min(rec["n_nei"][r], 4), 100 + max(rec["ext_len"][r], 0)
        assert np.array_equal(got["neighbours.npy"][i].astype(np.uint32).view(np.uint8).reshape(-1), np.where(np.arange(128) < 32 * k, nei[r], 0))
        assert np.array_equal(got["sequences.npy"][i], np.where(np.arange(200) < u, seq[r], 0))
    dump_outputs(torch, j, str(tmp_path / "again"), rows=64)
    assert all(np.array_equal(got[f], np.load(str(tmp_path / "again" / f))) for f in DUMPED)


def test_dump_outputs_is_for_one_gpu(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 2 and b"--gpus 1" in p.stderr


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_the_same_outputs_twice(gpu, tmp_path):
    env = dict(os.environ, FMD_BENCH_READS="1000000")
    for k in ("FMD_BENCH_LEGS", "RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    runs = []
    for r in range(2):
        d = str(tmp_path / str(r))
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", d],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        line = json.loads([x for x in p.stdout.decode().splitlines() if x.startswith("{")][-1])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "reads/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
        assert line["metric"].startswith("reads/sec") and abs(line["value"] * line["ms_per_step"] * 1e-3 / 1e6 - 1) < 1e-9
        assert line["overlap_discovery"]["strands_this_rank"] == 2_000_000 and line["overlap_discovery"]["overflow_records"] == 0
        for moved in ("roofline", "cpu_baseline", "parity_vs_cpu_on_sample", "check_left", "backward_search", "smem", "kmer_harvest", "ec_fix",
                      "overlap_discovery_on_raw_reads", "pmc_in_run", "product_path_unitig_g"):
            assert moved not in line, moved
        assert "id_order_one_pass_walk" not in line["overlap_discovery"] and "without_two_base_blocks" not in line["overlap_discovery"]
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
        got = {f: np.load(os.path.join(d, f)) for f in DUMPED}
        assert got["records.npy"].shape == (1 << 15, 16) and got["neighbours.npy"].shape == (1 << 15, 4, 8) and got["sequences.npy"].shape == (1 << 15, 200)
        assert (got["records.npy"][:, 13] > 0).mean() > 0.9                 # error-free reads at 30x: nearly every strand has a neighbour
        runs.append(got)
    for f in DUMPED:
        assert np.array_equal(runs[0][f], runs[1][f]), f
